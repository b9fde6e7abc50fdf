// Stand-alone program for the 32-bit packed 4:4:4 frames (melf_process_packed32*: AYUV / VUYA, Y410, X2RGB10 ..), on the CPU.
// Three parts:
//   1. check_packed32 (meterelf_amd/csrc/melf_frame_checks.h, the function the entry points call) over accepted and rejected
//      descriptors: the extent of every accepted one is the header's formula, both colours are accepted, every rejected one names
//      its condition -- every message of the check's table is produced (counted) --, and pitches and strides at the ends of 32 and
//      64 bits overflow nothing (the sanitizers watch the arithmetic).
//   2. The dial source DialWord32<true | false> of meterelf_amd/csrc/melf_frame_src.h, the header the kernels compile, driven the way
//      k_dials_body.inc drives it (px for the colour core, col_px for the exact path, window / request / unpack for the window
//      fetch) on frames malloc'd to exactly (n - 1) * frame_stride + extent as the check leaves them: under -fsanitize=address the
//      allocation's red zones are the bounds check.  Every pixel that leaves the source equals this program's plain indexing of the
//      layout through yuv_bgr / yuv_chroma of melf_device.h (YUV) or the three reads as they are (RGB).  Swept: base phases 0, 4, 8
//      and 12 modulo 16; any W, odd ones too; the crop's right edge on the frame's last pixel -- of the last row of the last frame
//      as well: the buffer's last word -- and one pixel short of it; windows flush with the crop's last column and windows that
//      leave the crop (quads false); padded and tight rows; several sets of positions.
//   3. The prep arm's addresses, through the functions of meterelf_amd/csrc/melf_prep_addr.h it calls (PX 28 / 29 of
//      prep_lplane_body.inc: packed_rows_safe, packed_x_off and packed_lane_ok with 4-byte pixels and the 128-byte window): every load
//      of every live lane lies inside the buffer and holds the lane's pixels.
// Built and run by tests/test_packed32_frames.py (test_checks_and_load_bounds), plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

// the device intrinsics of the header, as host functions (the source run here uses none of them: the other sources' text names them)
[[maybe_unused]] static inline uint32_t host_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 255u;
        uint32_t b;
        if (s < 8) b = (uint32_t)(src >> (8 * s)) & 255u;
        else if (s < 12) b = ((src >> (16 * (s - 8) + 15)) & 1u) ? 255u : 0u;
        else if (s == 12) b = 0u;
        else b = 255u;
        out |= b << (8 * i);
    }
    return out;
}
[[maybe_unused]] static inline uint32_t host_alignbyte(uint32_t hi, uint32_t lo, uint32_t n) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (n & 3u))); }
[[maybe_unused]] static inline uint32_t host_alignbit(uint32_t hi, uint32_t lo, uint32_t n) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (n & 31u)); }
[[maybe_unused]] static inline int host_readfirstlane(int v) { return v; }
#ifndef __builtin_amdgcn_perm
#define __builtin_amdgcn_perm host_perm
#define __builtin_amdgcn_alignbyte host_alignbyte
#define __builtin_amdgcn_alignbit host_alignbit
#define __builtin_amdgcn_readfirstlane host_readfirstlane
#endif

// (HIP declares min of ints for device code; the plain C++ compile has none: the header's calls find this one)
namespace melf {
static inline int min(int a, int b) { return a < b ? a : b; }
}  // namespace melf

#include "../meterelf_amd/csrc/melf_frame_src.h"
#include "../meterelf_amd/csrc/melf_frame_checks.h"
#include "../meterelf_amd/csrc/melf_prep_addr.h"

using namespace melf;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

static long long g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                                                 \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(cond)) { if (g_fail++ < 20) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } \
    } while (0)

// ---- 1. the check ----------------------------------------------------------------------------------------------------------------
static const int POSITIONS[][3] = {{16, 8, 0}, {8, 16, 24}, {8, 0, 16}, {12, 2, 22}, {14, 4, 24}, {22, 12, 2}, {2, 12, 22}, {0, 9, 24}, {24, 16, 7}};
constexpr int NPOS = sizeof(POSITIONS) / sizeof(POSITIONS[0]);

static melf_packed32_frames desc_of(int colour, int n, int H, int W, int64_t pad, int64_t spad, const int* pos = POSITIONS[3])
{
    melf_packed32_frames d = {};
    d.colour = colour; d.matrix = colour == MELF_P32_YUV ? MELF_YUV_BT709_LIMITED : 0; d.n = n; d.H = H; d.W = W;
    d.pos[0] = pos[0]; d.pos[1] = pos[1]; d.pos[2] = pos[2];
    d.row_pitch = (int64_t)W * 4 + pad;
    d.frame_stride = (int64_t)(H - 1) * d.row_pitch + (int64_t)W * 4 + spad;
    return d;
}
static const void* base_at(size_t phase) { return (const void*)(uintptr_t)(4096 + phase); }   // never read: NULL and alignment only

static long long g_msg[P32_MESSAGES] = {0};   // how often each message of the check's table was produced
static void expect(const melf_packed32_frames* d, const void* base, int want, const char* what)
{
    FrameBatch b = {};
    const char* msg = check_packed32(base, d, &b);
    int k = -1;
    if (msg) {
        k = 0;
        while (k < P32_MESSAGES && msg != PACKED32_MESSAGES[k]) ++k;
        CHECK(k < P32_MESSAGES, "check: \"%s\" is not a message of the table", msg);
        if (k < P32_MESSAGES) ++g_msg[k];
    }
    CHECK(k == want, "check: %s gives \"%s\", expected %s", what, msg ? msg : "(taken)", want < 0 ? "(taken)" : PACKED32_MESSAGES[want]);
}

static long long g_accepted[2] = {0, 0}, g_rejected = 0;
static void check_sweep()
{
    for (int colour = 0; colour < 2; ++colour) {
        for (int W = 1; W <= 21; ++W)
            for (int H = 1; H <= 5; H += 2)
                for (int n = 0; n <= 3; ++n)
                    for (int pi = 0; pi < 3; ++pi)
                        for (int si = 0; si < 2; ++si) {
                            const int* pos = POSITIONS[(W + H + n) % NPOS];
                            const melf_packed32_frames d = desc_of(colour, n, H, W, pi * 4, si * 12, pos);
                            FrameBatch b = {};
                            const char* msg = check_packed32(n ? base_at(4 * (size_t)((W + pi) % 4)) : nullptr, &d, &b);
                            ++g_accepted[colour];
                            CHECK(msg == nullptr, "check: a descriptor of the sweep is not taken: %s (colour %d n %d H %d W %d)", msg ? msg : "", colour, n, H, W);
                            if (msg) continue;
                            const int64_t row = (int64_t)4 * W;
                            CHECK((int64_t)b.lay.extent == (int64_t)(H - 1) * d.row_pitch + row, "check: extent %zu (H %d W %d)", b.lay.extent, H, W);
                            CHECK(b.n == n && b.H == H && b.W == W && b.row_stride == d.row_pitch && b.frame_stride == (size_t)d.frame_stride &&
                                      b.lay.pix == (colour ? PIX_P32_RGB : PIX_P32_YUV) && b.lay.mx == (colour ? nullptr : yuv_matrix(d.matrix)) &&
                                      b.lay.p32.pos[0] == (uint32_t)pos[0] && b.lay.p32.pos[1] == (uint32_t)pos[1] && b.lay.p32.pos[2] == (uint32_t)pos[2],
                                  "check: the batch is not the descriptor's");
                            // every rejected neighbour names its condition
                            melf_packed32_frames e;
                            const void* const base = base_at(0);
                            ++g_rejected;
                            e = d; e.colour = 2; expect(&e, base, P32_COLOUR, "colour 2");
                            e = d; e.colour = -1; expect(&e, base, P32_COLOUR, "colour -1");
                            if (colour == MELF_P32_YUV) {
                                e = d; e.matrix = 1; expect(&e, base, P32_MATRIX_YUV, "matrix 1");
                                e = d; e.matrix = 5; expect(&e, base, P32_MATRIX_YUV, "matrix 5");
                                e = d; e.matrix = -1; expect(&e, base, P32_MATRIX_YUV, "matrix -1");
                                for (int m : {0, 2, 3, 4}) { e = d; e.matrix = m; expect(&e, base, -1, "a matrix code"); }
                            } else {
                                e = d; e.matrix = 3; expect(&e, base, P32_MATRIX_RGB, "a matrix for RGB");
                                e = d; e.matrix = -1; expect(&e, base, P32_MATRIX_RGB, "a matrix for RGB");
                            }
                            e = d; e.reserved = 1; expect(&e, base, P32_RESERVED, "reserved 1");
                            e = d; e.reserved2 = -1; expect(&e, base, P32_RESERVED, "reserved2 -1");
                            for (int k = 0; k < 3; ++k) {
                                e = d; e.pos[k] = 25; expect(&e, base, P32_POS_RANGE, "pos 25");
                                e = d; e.pos[k] = -1; expect(&e, base, P32_POS_RANGE, "pos -1");
                                e = d; e.pos[k] = 32; expect(&e, base, P32_POS_RANGE, "pos 32");
                                e = d; e.pos[k] = e.pos[(k + 1) % 3]; expect(&e, base, P32_POS_OVERLAP, "two equal positions");
                                e = d; e.pos[k] = e.pos[(k + 1) % 3] >= 7 ? e.pos[(k + 1) % 3] - 7 : e.pos[(k + 1) % 3] + 7; expect(&e, base, P32_POS_OVERLAP, "positions 7 apart");
                            }
                            e = d; e.H = 0; expect(&e, base, P32_SHAPE, "H 0");
                            e = d; e.W = 0; expect(&e, base, P32_SHAPE, "W 0");
                            e = d; e.W = -2; expect(&e, base, P32_SHAPE, "W -2");
                            e = d; e.n = -1; expect(&e, base, P32_SHAPE, "n -1");
                            e = d; e.row_pitch = row - 4; expect(&e, base, P32_PITCH_SMALL, "a short pitch");
                            e = d; e.row_pitch = row - 1; expect(&e, base, P32_PITCH_SMALL, "a short pitch");
                            e = d; e.row_pitch = -4; expect(&e, base, P32_PITCH_SMALL, "a negative pitch");
                            e = d; e.row_pitch = (int64_t)INT32_MAX + 1; e.frame_stride = INT64_MAX & ~(int64_t)3; expect(&e, base, P32_PITCH_LARGE, "pitch 2^31");
                            e = d; e.frame_stride = (int64_t)b.lay.extent - 4; expect(&e, base, P32_STRIDE_SMALL, "a short stride");
                            e = d; e.frame_stride = 0; expect(&e, base, P32_STRIDE_SMALL, "stride 0");
                            e = d; e.frame_stride = -4; expect(&e, base, P32_STRIDE_SMALL, "a negative stride");
                            e = d; e.row_pitch += 2; e.frame_stride = (int64_t)(H - 1) * e.row_pitch + row + 32; e.frame_stride -= e.frame_stride % 4;
                            expect(&e, base, P32_STRIDES, "a misaligned pitch");
                            e = d; e.frame_stride += 2; expect(&e, base, P32_STRIDES, "a misaligned stride");
                            e = d; e.frame_stride += 1; expect(&e, base, P32_STRIDES, "a misaligned stride");
                            if (n) {
                                expect(&d, nullptr, P32_FRAMES_NULL, "NULL frames");
                                for (size_t ph : {1, 2, 3, 6}) expect(&d, base_at(ph), P32_BASE, "a misaligned base");
                                for (size_t ph : {0, 4, 8, 12}) expect(&d, base_at(ph), -1, "a 4-byte aligned base");
                            } else {
                                expect(&d, nullptr, -1, "n == 0 with NULL frames");
                                expect(&d, base_at(1), -1, "n == 0 with any pointer");
                            }
                        }
        expect(nullptr, base_at(0), P32_DESC_NULL, "a NULL descriptor");
        // the ends of 32 and 64 bits: nothing may overflow (the sanitizers watch), and what is taken has the formula's extent
        const int64_t values[] = {INT32_MAX, (int64_t)INT32_MAX + 1, (int64_t)INT32_MAX - 1, (int64_t)INT32_MAX - 3, (int64_t)INT32_MAX - 7, (int64_t)1 << 32,
                                  INT64_MAX, INT64_MAX - 1, INT64_MAX - 3, INT64_MAX - 7, -1, -4, -8, INT32_MIN, INT64_MIN, INT64_MIN + 4, 0, 4, 8};
        const int dims[] = {1, 2, 3, INT32_MAX - 1, INT32_MAX, INT32_MIN, -1, 0};
        for (int64_t pitch : values)
            for (int64_t stride : values)
                for (int W : dims)
                    for (int H : dims)
                        for (int n : {0, 1, 3, INT32_MAX}) {
                            melf_packed32_frames d = desc_of(colour, n, 2, 2, 0, 0);
                            d.H = H; d.W = W; d.row_pitch = pitch; d.frame_stride = stride;
                            FrameBatch b = {};
                            const char* msg = check_packed32(base_at(0), &d, &b);
                            ++g_checks;
                            if (msg) continue;
                            const bool fine = W > 0 && H > 0 && pitch >= (int64_t)W * 4 && pitch <= INT32_MAX && pitch % 4 == 0 && stride % 4 == 0 &&
                                              (__int128)stride >= (__int128)(H - 1) * pitch + (int64_t)W * 4;
                            CHECK(fine && (__int128)b.lay.extent == (__int128)(H - 1) * pitch + (int64_t)W * 4,
                                  "check: an edge descriptor is taken (n %d H %d W %d pitch %lld stride %lld)", n, H, W, (long long)pitch, (long long)stride);
                        }
    }
}

// ---- the layout by plain indexing ---------------------------------------------------------------------------------------------------
static uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

struct Buf {
    uint8_t *alloc = nullptr, *mem = nullptr;   // mem: the frames' base; the allocation ends where the frames end
    int colour = 0, n = 0, H = 0, W = 0, row_stride = 0;
    size_t frame_stride = 0, extent = 0;
    const YuvMatrix* mx = nullptr;
    Packed32Fields fields = {};
    size_t readable() const { return (size_t)(n - 1) * frame_stride + extent; }
    void release() { free(alloc); alloc = mem = nullptr; }
    // the B G R dword of frame pixel (fx, fy)
    uint32_t bgr(int f, int fx, int fy) const
    {
        const uint32_t w = le32(mem + (size_t)f * frame_stride + (size_t)fy * row_stride + (size_t)fx * 4);
        const uint32_t r0 = (w >> fields.pos[0]) & 255u, r1 = (w >> fields.pos[1]) & 255u, r2 = (w >> fields.pos[2]) & 255u;
        if (colour == MELF_P32_YUV) return yuv_bgr((int)r0, yuv_chroma<false>((int)r1, (int)r2, *mx), *mx) & 0xffffffu;
        return r2 | r1 << 8 | r0 << 16;   // R, G, B -> B in byte 0
    }
};
// the frames of a descriptor as its check leaves them, malloc'd to exactly what it says is readable, random bytes, the base at
// `phase` (0, 4, 8, 12) modulo 16
static Buf make_buf(int colour, int n, int H, int W, int64_t pad, int64_t spad, const int* pos, size_t phase)
{
    const melf_packed32_frames d = desc_of(colour, n, H, W, pad, spad, pos);
    FrameBatch fb = {};
    const char* msg = check_packed32(base_at(phase), &d, &fb);
    if (msg) { fprintf(stderr, "a descriptor of the sweep is not taken: %s (n %d H %d W %d)\nfailures 1\n", msg, n, H, W); exit(1); }
    Buf b;
    b.colour = colour; b.n = fb.n; b.H = fb.H; b.W = fb.W; b.row_stride = fb.row_stride; b.frame_stride = fb.frame_stride; b.extent = fb.lay.extent;
    b.mx = fb.lay.mx; b.fields = fb.lay.p32;
    // exactly the readable bytes, ending where the allocation ends; the bytes in front of the base (up to 15 + 12) belong to the
    // allocation too, which a load before the base would need more than: no source computes an address below its first pixel's
    b.alloc = (uint8_t*)malloc(b.readable() + 32);
    if (!b.alloc) { fprintf(stderr, "out of memory\n"); exit(2); }
    const size_t slack = ((size_t)(-(uintptr_t)b.alloc & 15) + phase) % 16;
    uint8_t* const fitted = (uint8_t*)realloc(b.alloc, b.readable() + slack);
    if (fitted != b.alloc && ((uintptr_t)fitted & 15) != ((uintptr_t)b.alloc & 15)) { fprintf(stderr, "realloc moved the block to another phase\n"); exit(2); }
    b.alloc = fitted;
    b.mem = b.alloc + slack;
    if (((uintptr_t)b.mem & 15) != phase) { fprintf(stderr, "the base is not at phase %zu\n", phase); exit(2); }
    for (size_t i = 0; i < b.readable(); ++i) b.mem[i] = (uint8_t)rnd();
    return b;
}

// ---- 2. the dial source -------------------------------------------------------------------------------------------------------------
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static long long g_quads[2] = {0, 0}, g_exact[2] = {0, 0}, g_phase[4] = {0, 0, 0, 0}, g_flush = 0, g_last_word = 0;

template <class Src>
static void dial_case(const Buf& b, const DialsSrc& ds, const melf_params& P, int f, int mx, int my, int wx0, int wy0, int ws)
{
    const char* const name = b.colour ? "DialWord32<false>" : "DialWord32<true>";
    const uint8_t* const frame = ds.base + (size_t)f * ds.frame_stride;
    const YuvMatrix none = {};
    const typename Src::Args sargs{b.fields, b.mx ? *b.mx : none};
    const Src FS(ds, sargs, P, frame, mx, my);
    const int tw = P.tw, th1 = P.th - 1, ylast = ws - 1, rs_u = (int)FS.rstride;
    const int ox = ds.x0 + mx, oy = ds.y0 + my;
    // the colour core, at clamped coordinates
    const int xs[5] = {-1, 0, tw / 2, tw - 1, tw}, ys[4] = {-1, 1, th1 - 1, th1 + 1};
    for (int a = 0; a < 5; ++a)
        for (int c = 0; c < 4; ++c) {
            const int X = clampi(xs[a], 0, tw - 1), Y = clampi(ys[c], 0, th1);
            const uint32_t got = FS.px(X, Y) & 0xffffffu, want = b.bgr(f, ox + X, oy + Y);
            CHECK(got == want, "%s: px(%d, %d) = %06x, plain indexing gives %06x (frame %d, match %d %d)", name, X, Y, got, want, f, mx, my);
        }
    // the exact path: a lane's column at clamped rows
    for (int lane = 0, prevX = -1; lane < 64; ++lane) {
        const int Xc = clampi(wx0 + (lane < ws - 1 ? lane : ws - 1), 0, tw - 1);
        if (Xc == prevX) continue;
        prevX = Xc;
        const auto xcol = FS.column(Xc);
        for (int Y = 0; Y <= th1; Y += th1 > 0 ? th1 : 1) {
            const uint32_t got = FS.col_px(xcol, Y, rs_u) & 0xffffffu, want = b.bgr(f, ox + Xc, oy + Y);
            CHECK(got == want, "%s: col_px(%d, %d) = %06x, plain indexing gives %06x", name, Xc, Y, got, want);
        }
    }
    // the window fetch: sixteen lanes a row
    static_assert(!Src::EVEN_QUADS && Src::PB == 4 && !Src::FROM_HLS, "one B G R dword per pixel, quads at any pixel");
    CHECK(FS.quad_shift(wx0) == 0, "%s: a quad shift", name);
    const int npiece = (ws + 3) >> 2;
    bool quads0 = false;
    for (int pc = 0; pc < 16; ++pc) {
        const auto W0 = FS.window(wx0, npiece, pc, th1, rs_u, tw);
        if (pc == 0) {
            quads0 = W0.quads;
            ++(quads0 ? g_quads : g_exact)[b.colour];
            // the condition, restated
            CHECK(quads0 == (wx0 >= 0 && wx0 + 4 * npiece <= tw), "%s: quads %d for wx0 %d, %d pieces, tw %d", name, (int)quads0, wx0, npiece, tw);
            if (quads0 && wx0 + 4 * npiece == tw) ++g_flush;
        }
        CHECK(W0.quads == quads0, "%s: quads is not wave-uniform", name);
        if (!quads0) break;
        const int X0 = wx0 + 4 * (pc < npiece - 1 ? pc : npiece - 1);   // the lane's first pixel, crop column
        CHECK(X0 >= 0 && X0 + 4 <= tw, "%s: the quad at column %d leaves the crop", name, X0);
        const int rows[4] = {0, 1, ws / 2, ylast};
        for (int k = 0; k < 4; ++k) {
            const int Y = clampi(wy0 + rows[k], 0, th1);
            const size_t at = (size_t)(frame - ds.base) + p32::dial_off(oy + Y, (size_t)rs_u, ox + X0);
            CHECK(at + p32::DIAL_BYTES <= ds.readable && at % 4 == 0, "%s: a window load at %zu of %zu readable bytes", name, at, ds.readable);
            ++g_phase[((uintptr_t)(ds.base + at) & 15) >> 2];
            if (at + p32::DIAL_BYTES == ds.readable) ++g_last_word;
            auto Wk = W0;
            const u32x4v px4 = Wk.unpack(k, Wk.request(k, Y));
            for (int j = 0; j < 4; ++j) {
                const uint32_t got = px4[j] & 0xffffffu, want = b.bgr(f, ox + X0 + j, oy + Y);
                CHECK(got == want, "%s: window pixel (%d, %d) = %06x, plain indexing gives %06x (frame %d, match %d %d, wx0 %d, ws %d, pc %d)", name, X0 + j, Y, got,
                      want, f, mx, my, wx0, ws, pc);
            }
        }
    }
}

static void dial_sweep()
{
    for (int colour = 0; colour < 2; ++colour)
        for (size_t phase = 0; phase < 16; phase += 4)
            for (int wadd = 0; wadd < 4; ++wadd)
                for (int x0 = 0; x0 < 4; ++x0)
                    for (int short1 = 0; short1 < 2; ++short1)
                        for (int place = 0; place < 2; ++place)
                            for (int ni = 0; ni < 2; ++ni) {
                                const int padded = (wadd + x0 + place) % 2;
                                const int W = 53 + wadd, H = 14, n = ni ? 3 : 1;
                                const int cols = W - x0 - short1, th = 6, rows = th + 2, tw = cols - 3;
                                const int y0 = place ? H - rows : (x0 & 1);
                                const Buf b = make_buf(colour, n, H, W, padded * 4 * (1 + wadd), 0, POSITIONS[(wadd + x0 + 3 * place + (int)phase / 4) % NPOS], phase);
                                DialsSrc ds;
                                ds.base = b.mem; ds.frame_stride = b.frame_stride; ds.row_stride = b.row_stride;
                                ds.x0 = x0; ds.y0 = y0; ds.crop_rows = rows; ds.crop_cols = cols; ds.readable = b.readable();
                                melf_params P = {};
                                P.tw = tw; P.th = th;
                                const int farx = cols - tw, fary = rows - th;
                                const int mxs[4] = {0, 1, farx - 1, farx};
                                for (int R = 3; R <= 9; ++R) {
                                    const int ws = 2 * R + 5, np4 = 4 * ((ws + 3) >> 2);
                                    // windows that leave the crop on either side, that start on its first column, and whose last quad is
                                    // flush with the template's last column (tw - np4) or one column past it
                                    const int wx0s[7] = {-1, 0, 1, tw - np4 - 1, tw - np4, tw - np4 + 1, tw - ws};
                                    for (int wi = 0; wi < 7; ++wi)
                                        for (int mi = 0; mi < 4; ++mi) {
                                            // (the last frame's last rows with the far match: the crop's right edge on the buffer's last word)
                                            const int f = (R + wi + mi) % 2 ? n - 1 : 0, my = (wi + mi) % 2 ? fary : 0;
                                            if (colour == 0) dial_case<DialWord32<true>>(b, ds, P, f, mxs[mi], my, wx0s[wi], wi % 3 - 1 + (my ? th : 0), ws);
                                            else dial_case<DialWord32<false>>(b, ds, P, f, mxs[mi], my, wx0s[wi], wi % 3 - 1 + (my ? th : 0), ws);
                                        }
                                }
                                Buf c = b;
                                c.release();
                            }
}

// ---- 3. the prep arm ------------------------------------------------------------------------------------------------------------------
static long long g_loads = 0, g_safe = 0, g_lane = 0, g_px = 0;
static void load(const Buf& b, size_t off, size_t len, const char* what)
{
    ++g_loads;
    CHECK(off <= b.readable() && off + len <= b.readable() && off % 4 == 0, "%s: load [%zu, %zu) of %zu readable bytes (n %d H %d W %d pitch %d)", what, off, off + len,
          b.readable(), b.n, b.H, b.W, b.row_stride);
}
static void prep_case(const Buf& b, int x0, int y0, int rows, int cols, int nkb)
{
    const size_t readable = b.readable();
    constexpr int PB = prep::packed_pb(4), WIN = prep::packed_win(4);
    static_assert(PB == 4 && WIN == 128, "the arm loads what PX 4 loads: eight 16-byte loads of 4-byte pixels");
    for (int grp = 0; grp < (b.n + 31) / 32; ++grp)
        for (int y = 0; y < rows; ++y) {
            const bool rows_safe = prep::packed_rows_safe(grp, b.n, b.frame_stride, y0 + y, b.row_stride, x0, nkb, PB, WIN, readable);
            for (int nn = 0; nn < 32; ++nn)
                for (int kb = 0; kb < nkb; ++kb) {
                    const int f = grp * 32 + nn;
                    if (!(f < b.n && kb * 32 < cols)) continue;   // `live`
                    const int xbeg = kb * 32, npx = cols - xbeg < 32 ? cols - xbeg : 32;
                    const size_t o = prep::packed_x_off(x0 + xbeg, PB);
                    const size_t row = (size_t)f * b.frame_stride + (size_t)(y0 + y) * b.row_stride;
                    CHECK(o == (size_t)(x0 + xbeg) * 4, "prep: offset of pixel %d", x0 + xbeg);
                    if (rows_safe || prep::packed_lane_ok(f, b.frame_stride, y0 + y, b.row_stride, o, WIN, readable)) {
                        if (rows_safe) ++g_safe; else ++g_lane;
                        for (int i = 0; i < 8; ++i) load(b, row + o + 16 * (size_t)i, 16, "prep window");
                    } else {
                        ++g_px;
                        for (int k = 0; k < npx; ++k) load(b, row + o + 4 * (size_t)k, 4, "prep word");
                    }
                }
        }
}
static void prep_sweep()
{
    for (int colour = 0; colour < 2; ++colour)
        for (int cols = 8; cols <= 100; ++cols)
            for (int x0 = 0; x0 < 8; ++x0)
                for (int e = 0; e < 3; ++e)           // the frame's right edge: the crop's, one and seven pixels further
                    for (int place = 0; place < 2; ++place)
                        for (int ni = 0; ni < 3; ++ni) {
                            if (ni == 2 && (cols + x0) % 5) continue;   // a second frame group: a fifth of the configurations
                            const int W = x0 + cols + (e == 2 ? 7 : e), H = 9, rows = 4;
                            const int n = ni == 0 ? 1 : (ni == 1 ? 3 : 34);
                            Buf b = make_buf(colour, n, H, W, ((cols + x0) % 3) * 4, 0, POSITIONS[(cols + x0) % NPOS], 4 * (size_t)((cols + e) % 4));
                            const int nkb = (cols + 31) / 32;
                            const int y0 = place ? H - rows : 0;
                            prep_case(b, x0, y0, rows, cols, nkb);
                            if (ni == 0) prep_case(b, x0, y0, rows, cols, nkb + 1);
                            b.release();
                        }
}

int main()
{
    check_sweep();
    dial_sweep();
    prep_sweep();
    printf("checks %lld  descriptors accepted: YUV %lld, RGB %lld, each rejected in every way of the table  dial windows: YUV quads %lld exact %lld, RGB quads %lld "
           "exact %lld  window loads at base + 0, 4, 8, 12 mod 16: %lld %lld %lld %lld  flush windows %lld, loads ending on the buffer's last word %lld\n",
           g_checks, g_accepted[0], g_accepted[1], g_quads[0], g_exact[0], g_quads[1], g_exact[1], g_phase[0], g_phase[1], g_phase[2], g_phase[3], g_flush,
           g_last_word);
    printf("prep loads %lld  lanes: row-safe %lld, lane-safe %lld, word by word %lld  failures %lld\n", g_loads, g_safe, g_lane, g_px, g_fail);
    for (int k = 0; k < P32_MESSAGES; ++k)
        if (!g_msg[k]) {
            fprintf(stderr, "message %d of check_packed32 was never produced\n", k);
            return 1;
        }
    if (!g_accepted[0] || !g_accepted[1] || !g_rejected || !g_quads[0] || !g_exact[0] || !g_quads[1] || !g_exact[1] || !g_phase[0] || !g_phase[1] || !g_phase[2] ||
        !g_phase[3] || !g_flush || !g_last_word || !g_safe || !g_lane || !g_px) {
        fprintf(stderr, "a path was never taken: the sweep does not cover it\n");
        return 1;
    }
    return g_fail ? 1 : 0;
}
