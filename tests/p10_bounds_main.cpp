// Stand-alone program for the packed 10-bit YUV 4:2:2 frames (melf_process_yuv422_10*: v210 and Y210 / Y212 / Y216), on the CPU.
// Three parts:
//   1. check_yuv422_10 (meterelf_amd/csrc/melf_frame_checks.h, the function the entry points call) over accepted and rejected
//      descriptors: the extent of every accepted one is the header's formula, every rejected one names its condition -- every
//      message of the check's table is produced (counted) --, and pitches and strides at the ends of 32 and 64 bits overflow
//      nothing (the sanitizers watch the arithmetic).
//   2. The dial sources DialV210 and DialY210 of meterelf_amd/csrc/melf_frame_src.h, the header the kernels compile, driven the way
//      k_dials_body.inc drives them (px for the colour core, col_px for the exact path, window / request / unpack for the window
//      fetch) on frames malloc'd to exactly (n - 1) * frame_stride + extent as the check leaves them: under -fsanitize=address the
//      allocation's red zones are the bounds check.  Every pixel that leaves a source equals this program's plain indexing of the
//      layout (the table of include/meterelf_hip.h, written out below) through yuv_bgr / yuv_chroma of melf_device.h.  Swept: frame
//      widths with W % 6 of 0, 2 and 4; the crop's origin at all six residues mod 6, its right edge on the frame's and one pixel
//      short of it, the crop at the frame's first rows and at its last; the only, the first and the last frame; padded and tight
//      rows; window sizes 2 R + 5 at origins -1, 0, 1, tw - ws - 1, tw - ws, tw - ws + 1 (the crop's first and last columns); match
//      positions 0, 1, far - 1, far: every fx0 % 6 is met by the quads (counted, and asserted).
//   3. The prep functions of meterelf_amd/csrc/melf_p10_addr.h as PX 26 and PX 27 of prep_lplane_body.inc use them: every load of
//      every live lane lies inside the buffer (v210: inside the row's own groups), and holds the lane's pixels, for every x0 % 6,
//      every block count, one, three and 34 frames, the crop at the frame's first rows and at its last.
// Built and run by tests/test_yuv422_10_frames.py (test_checks_and_load_bounds), plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

// the device intrinsics of the header, as host functions (gfx9 ISA: v_perm_b32, v_alignbyte_b32, v_alignbit_b32; the two sources run
// here use the first only: the other sources' text names the rest)
static inline uint32_t host_perm(uint32_t hi, uint32_t lo, uint32_t sel)
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
static inline int host_readfirstlane(int v) { return v; }
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
static int64_t row_bytes(int fmt, int64_t W) { return fmt == MELF_YUV422_10_V210 ? (W + 5) / 6 * 16 : W * 4; }
static int64_t align_of(int fmt) { return fmt == MELF_YUV422_10_V210 ? 16 : 8; }
static melf_yuv422_10_frames desc_of(int fmt, int n, int H, int W, int64_t pad, int64_t spad)
{
    melf_yuv422_10_frames d = {};
    d.format = fmt; d.matrix = MELF_YUV_BT709_LIMITED; d.n = n; d.H = H; d.W = W;
    d.row_pitch = row_bytes(fmt, W) + pad;
    d.frame_stride = (int64_t)(H - 1) * d.row_pitch + row_bytes(fmt, W) + spad;
    return d;
}
static const void* base_at(size_t phase) { return (const void*)(uintptr_t)(4096 + phase); }   // never read: NULL and alignment only

static long long g_msg[P10_MESSAGES + 1] = {0};   // how often each message of the check's table was produced; the last: the matrix message
static void expect(const melf_yuv422_10_frames* d, const void* base, const char* word, const char* what)
{
    FrameBatch b = {};
    const char* msg = check_yuv422_10(base, d, &b);
    if (msg) {
        int k = 0;
        while (k < P10_MESSAGES && msg != YUV422_10_MESSAGES[k]) ++k;
        CHECK(k < P10_MESSAGES || msg == UNKNOWN_YUV_MATRIX, "check: \"%s\" is not a message of the table", msg);
        ++g_msg[k];
    }
    if (!word) CHECK(msg == nullptr, "check: %s is not taken: %s", what, msg ? msg : "");
    else CHECK(msg && strstr(msg, word), "check: %s gives \"%s\", expected a message with \"%s\"", what, msg ? msg : "(taken)", word);
}

static long long g_accepted = 0, g_rejected = 0;
static void check_sweep()
{
    for (int fmt = 0; fmt < 2; ++fmt) {
        const int64_t a = align_of(fmt);
        for (int W = 2; W <= 62; W += 2)
            for (int H = 1; H <= 5; H += 2)
                for (int n = 0; n <= 3; ++n)
                    for (int pi = 0; pi < 3; ++pi)
                        for (int si = 0; si < 2; ++si) {
                            const melf_yuv422_10_frames d = desc_of(fmt, n, H, W, pi * a, si * 3 * a);
                            FrameBatch b = {};
                            const char* msg = check_yuv422_10(n ? base_at(fmt ? 8 : 0) : nullptr, &d, &b);
                            ++g_accepted;
                            CHECK(msg == nullptr, "check: a descriptor of the sweep is not taken: %s (fmt %d n %d H %d W %d)", msg ? msg : "", fmt, n, H, W);
                            if (msg) continue;
                            // the header's extent: (H - 1) * row_pitch + a row's whole groups / macropixels
                            const int64_t row = fmt == MELF_YUV422_10_V210 ? (int64_t)p10::v210_row_bytes(W) : (int64_t)4 * W;
                            CHECK((int64_t)b.lay.extent == (int64_t)(H - 1) * d.row_pitch + row && row == row_bytes(fmt, W), "check: extent %zu (fmt %d H %d W %d)", b.lay.extent, fmt, H, W);
                            CHECK(b.n == n && b.H == H && b.W == W && b.row_stride == d.row_pitch && b.frame_stride == (size_t)d.frame_stride &&
                                      b.lay.pix == (fmt ? PIX_Y210 : PIX_V210) && b.lay.mx == yuv_matrix(d.matrix),
                                  "check: the batch is not the descriptor's");
                            // every rejected neighbour names its condition
                            melf_yuv422_10_frames e;
                            const void* const base = base_at(0);
                            ++g_rejected;
                            e = d; e.format = 2; expect(&e, base, "unknown packed 10-bit", "format 2");
                            e = d; e.format = -1; expect(&e, base, "unknown packed 10-bit", "format -1");
                            e = d; e.matrix = 1; expect(&e, base, "unknown YUV matrix", "matrix 1");
                            e = d; e.matrix = 5; expect(&e, base, "unknown YUV matrix", "matrix 5");
                            e = d; e.reserved = 1; expect(&e, base, "reserved", "reserved 1");
                            e = d; e.H = 0; expect(&e, base, "bad batch shape", "H 0");
                            e = d; e.W = 0; expect(&e, base, "bad batch shape", "W 0");
                            e = d; e.W = -2; expect(&e, base, "bad batch shape", "W -2");
                            e = d; e.n = -1; expect(&e, base, "bad batch shape", "n -1");
                            e = d; e.W = W + 1; e.row_pitch += 2 * a; e.frame_stride += 2 * a * H; expect(&e, base, "even width", "an odd W");
                            e = d; e.row_pitch = row - a; expect(&e, base, "row_pitch smaller", "a short pitch");
                            e = d; e.row_pitch = row - 1; expect(&e, base, "row_pitch smaller", "a short pitch");
                            e = d; e.row_pitch = (int64_t)INT32_MAX + 1; e.frame_stride = INT64_MAX & ~(int64_t)15; expect(&e, base, "row_pitch too large", "pitch 2^31");
                            e = d; e.frame_stride = (int64_t)b.lay.extent - a; expect(&e, base, "frame_stride smaller", "a short stride");
                            e = d; e.frame_stride = 0; expect(&e, base, "frame_stride smaller", "stride 0");
                            e = d; e.frame_stride = -a; expect(&e, base, "frame_stride smaller", "a negative stride");
                            e = d; e.row_pitch += a / 2; e.frame_stride = (int64_t)(H - 1) * e.row_pitch + row + 8 * a; e.frame_stride -= e.frame_stride % a;
                            expect(&e, base, "aligned row_pitch", "a misaligned pitch");
                            e = d; e.frame_stride += a / 2; expect(&e, base, "aligned row_pitch", "a misaligned stride");
                            e = d; e.frame_stride += 4; expect(&e, base, "aligned row_pitch", "a misaligned stride");
                            if (n) {
                                expect(&d, nullptr, "frames pointer is NULL", "NULL frames");
                                expect(&d, base_at((size_t)a / 2), "aligned base", "a misaligned base");
                                expect(&d, base_at(4), "aligned base", "a misaligned base");
                                expect(&d, base_at(1), "aligned base", "a misaligned base");
                                if (fmt) expect(&d, base_at(8), nullptr, "Y210 at 8 within 16");
                            } else {
                                expect(&d, nullptr, nullptr, "n == 0 with NULL frames");
                                expect(&d, base_at(1), nullptr, "n == 0 with any pointer");
                            }
                        }
        expect(nullptr, base_at(0), "descriptor is NULL", "a NULL descriptor");
        // the ends of 32 and 64 bits: nothing may overflow (the sanitizers watch), and what is taken has the formula's extent
        const int64_t values[] = {INT32_MAX, (int64_t)INT32_MAX + 1, (int64_t)INT32_MAX - 1, (int64_t)INT32_MAX - 15, (int64_t)INT32_MAX - 7, (int64_t)1 << 32,
                                  INT64_MAX, INT64_MAX - 1, INT64_MAX - 7, INT64_MAX - 15, INT64_MAX - 16, -1, -8, -16, INT32_MIN, INT64_MIN, INT64_MIN + 16, 0};
        const int dims[] = {1, 2, 6, INT32_MAX - 1, INT32_MAX, INT32_MIN, -1, 0};
        for (int64_t pitch : values)
            for (int64_t stride : values)
                for (int W : dims)
                    for (int H : dims)
                        for (int n : {0, 1, 3, INT32_MAX}) {
                            melf_yuv422_10_frames d = desc_of(fmt, n, 2, 2, 0, 0);
                            d.H = H; d.W = W; d.row_pitch = pitch; d.frame_stride = stride;
                            FrameBatch b = {};
                            const char* msg = check_yuv422_10(base_at(0), &d, &b);
                            ++g_checks;
                            if (msg) continue;
                            const bool fine = W > 0 && H > 0 && W % 2 == 0 && pitch >= row_bytes(fmt, W) && pitch <= INT32_MAX && pitch % a == 0 && stride % a == 0 &&
                                              (__int128)stride >= (__int128)(H - 1) * pitch + row_bytes(fmt, W);
                            CHECK(fine && (__int128)b.lay.extent == (__int128)(H - 1) * pitch + row_bytes(fmt, W),
                                  "check: an edge descriptor is taken (fmt %d n %d H %d W %d pitch %lld stride %lld)", fmt, n, H, W, (long long)pitch, (long long)stride);
                        }
    }
}

// ---- the layouts by plain indexing: the table of include/meterelf_hip.h ----------------------------------------------------------------
struct Pos { int word, bit; };
static const Pos V210_Y0[3] = {{0, 10}, {1, 20}, {3, 0}}, V210_Y1[3] = {{1, 0}, {2, 10}, {3, 20}}, V210_U[3] = {{0, 0}, {1, 10}, {2, 20}},
                 V210_V[3] = {{0, 20}, {2, 0}, {3, 10}};
static uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint32_t v210_field(const uint8_t* group, Pos at) { return ((le32(group + 4 * at.word) >> at.bit) & 1023u) >> 2; }

struct Buf {
    uint8_t *alloc = nullptr, *mem = nullptr;   // mem: the frames' base; the allocation ends where the frames end
    int fmt = 0, n = 0, H = 0, W = 0, row_stride = 0;
    size_t frame_stride = 0, extent = 0;
    const YuvMatrix* mx = nullptr;
    size_t readable() const { return (size_t)(n - 1) * frame_stride + extent; }
    void release() { free(alloc); alloc = mem = nullptr; }
    // Y | U << 8 | V << 16 of frame pixel (fx, fy)
    uint32_t yuv(int f, int fx, int fy) const
    {
        const uint8_t* row = mem + (size_t)f * frame_stride + (size_t)fy * row_stride;
        if (fmt == MELF_YUV422_10_V210) {
            const uint8_t* g = row + (size_t)(fx / 6) * 16;
            const int q = fx % 6 / 2;
            return v210_field(g, fx & 1 ? V210_Y1[q] : V210_Y0[q]) | v210_field(g, V210_U[q]) << 8 | v210_field(g, V210_V[q]) << 16;
        }
        const uint8_t* m = row + (size_t)(fx / 2) * 8;   // Y0 U Y1 V, 16-bit little-endian words: the high bytes
        return (uint32_t)m[fx & 1 ? 5 : 1] | (uint32_t)m[3] << 8 | (uint32_t)m[7] << 16;
    }
    uint32_t bgr(int f, int fx, int fy) const
    {
        const uint32_t s = yuv(f, fx, fy);
        return yuv_bgr((int)(s & 255u), yuv_chroma<false>((int)((s >> 8) & 255u), (int)(s >> 16), *mx), *mx) & 0xffffffu;
    }
};
// the frames of a descriptor as its check leaves them, malloc'd to exactly what it says is readable, random bytes
static Buf make_buf(int fmt, int n, int H, int W, int64_t pad, int64_t spad)
{
    const melf_yuv422_10_frames d = desc_of(fmt, n, H, W, pad, spad);
    FrameBatch fb = {};
    const char* msg = check_yuv422_10(base_at(0), &d, &fb);
    if (msg) { fprintf(stderr, "a descriptor of the sweep is not taken: %s (n %d H %d W %d)\nfailures 1\n", msg, n, H, W); exit(1); }
    Buf b;
    b.fmt = fmt; b.n = fb.n; b.H = fb.H; b.W = fb.W; b.row_stride = fb.row_stride; b.frame_stride = fb.frame_stride; b.extent = fb.lay.extent; b.mx = fb.lay.mx;
    // exactly the readable bytes, ending where the allocation ends; where malloc's block is not 16-byte aligned the base moves up
    // to the next multiple of 16 and those few bytes in front of it belong to the allocation too
    b.alloc = (uint8_t*)malloc(b.readable() + 16);
    if (!b.alloc) { fprintf(stderr, "out of memory\n"); exit(2); }
    const size_t slack = (size_t)(-(uintptr_t)b.alloc & 15);
    uint8_t* const fitted = (uint8_t*)realloc(b.alloc, b.readable() + slack);
    if (fitted != b.alloc && ((uintptr_t)fitted & 15) != ((uintptr_t)b.alloc & 15)) { fprintf(stderr, "realloc moved the block to another phase\n"); exit(2); }
    b.alloc = fitted;
    b.mem = b.alloc + slack;
    for (size_t i = 0; i < b.readable(); ++i) b.mem[i] = (uint8_t)rnd();
    return b;
}

// ---- 2. the dial sources ------------------------------------------------------------------------------------------------------------
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static long long g_quads[2] = {0, 0}, g_exact[2] = {0, 0}, g_phase[2][6] = {{0}, {0}};

template <class Src>
static void dial_case(const Buf& b, const DialsSrc& ds, const melf_params& P, int f, int mx, int my, int wx0, int wy0, int ws)
{
    const char* const name = b.fmt ? "DialY210" : "DialV210";
    const uint8_t* const frame = ds.base + (size_t)f * ds.frame_stride;
    const typename Src::Args sargs{*b.mx};
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
    static_assert(Src::EVEN_QUADS && Src::PB == 4, "the sources of these frames start their quads at even pixels");
    const int qshift = FS.quad_shift(wx0);
    const int npiece = (ws + qshift + 3) >> 2;
    CHECK(qshift == ((ox + wx0) & 1) && npiece == p10::quad_count(ws, qshift), "%s: quad shift / count", name);
    bool quads0 = false;
    for (int pc = 0; pc < 16; ++pc) {
        const auto W0 = FS.window(wx0 - qshift, npiece, pc, th1, rs_u, tw);
        if (pc == 0) {
            quads0 = W0.quads;
            ++(quads0 ? g_quads : g_exact)[b.fmt];
        }
        CHECK(W0.quads == quads0, "%s: quads is not wave-uniform", name);
        if (!quads0) break;
        const int X0 = wx0 - qshift + 4 * (pc < npiece - 1 ? pc : npiece - 1);   // the lane's first pixel, crop column
        CHECK(4 * npiece - qshift >= ws && npiece <= 16, "%s: %d pieces do not hold %d columns", name, npiece, ws);
        CHECK(((ox + X0) & 1) == 0 && X0 >= 0 && X0 + 4 <= tw, "%s: the quad at column %d is odd in the frame or leaves the crop", name, X0);
        ++g_phase[b.fmt][(ox + X0) % 6];
        const int rows[4] = {0, 1, ws / 2, ylast};
        for (int k = 0; k < 4; ++k) {
            const int Y = clampi(wy0 + rows[k], 0, th1);
            const u32x4v px4 = W0.unpack(k, W0.request(k, Y));
            for (int j = 0; j < 4; ++j) {
                const uint32_t got = px4[j] & 0xffffffu, want = b.bgr(f, ox + X0 + j, oy + Y);
                CHECK(got == want, "%s: window pixel (%d, %d) = %06x, plain indexing gives %06x (frame %d, match %d %d, wx0 %d, ws %d, pc %d, fx0 %% 6 = %d)", name,
                      X0 + j, Y, got, want, f, mx, my, wx0, ws, pc, (ox + X0) % 6);
            }
        }
    }
}

static void dial_sweep()
{
    for (int fmt = 0; fmt < 2; ++fmt)
        for (int wmod = 0; wmod < 6; wmod += 2)
            for (int x0 = 0; x0 < 6; ++x0)
                for (int short1 = 0; short1 < 2; ++short1)
                    for (int place = 0; place < 2; ++place)
                        for (int ni = 0; ni < 2; ++ni)
                            for (int padded = 0; padded < 2; ++padded) {
                                const int W = 54 + wmod + 6 * ((x0 + place) % 2), H = 14, n = ni ? 3 : 1;
                                const int cols = W - x0 - short1, th = 6, rows = th + 2, tw = cols - 3;
                                const int y0 = place ? H - rows : (x0 & 1);
                                const Buf b = make_buf(fmt, n, H, W, padded * align_of(fmt), 0);
                                DialsSrc ds;
                                ds.base = b.mem; ds.frame_stride = b.frame_stride; ds.row_stride = b.row_stride;
                                ds.x0 = x0; ds.y0 = y0; ds.crop_rows = rows; ds.crop_cols = cols; ds.readable = b.readable();
                                melf_params P = {};
                                P.tw = tw; P.th = th;
                                const int farx = cols - tw, fary = rows - th;
                                const int mxs[4] = {0, 1, farx - 1, farx};
                                for (int R = 3; R <= 9; ++R) {
                                    const int ws = 2 * R + 5;
                                    const int wx0s[6] = {-1, 0, 1, tw - ws - 1, tw - ws, tw - ws + 1};
                                    for (int wi = 0; wi < 6; ++wi)
                                        for (int mi = 0; mi < 4; ++mi) {
                                            const int f = (R + wi + mi) % 2 ? n - 1 : 0, my = (wi + mi) % 2 ? fary : 0;
                                            if (fmt == 0) dial_case<DialV210>(b, ds, P, f, mxs[mi], my, wx0s[wi], wi % 3 - 1, ws);
                                            else dial_case<DialY210>(b, ds, P, f, mxs[mi], my, wx0s[wi], wi % 3 - 1, ws);
                                        }
                                }
                                Buf c = b;
                                c.release();
                            }
}

// ---- 3. the prep arms ---------------------------------------------------------------------------------------------------------------
static long long g_loads = 0, g_v_safe = 0, g_v_lane = 0, g_v7 = 0, g_y_safe = 0, g_y_lane = 0, g_y_px = 0;
static void load(const Buf& b, size_t off, size_t len, size_t align, const char* what)
{
    ++g_loads;
    CHECK(off <= b.readable() && off + len <= b.readable() && off % align == 0, "%s: load [%zu, %zu) of %zu readable bytes, alignment %zu (n %d H %d W %d pitch %d)", what, off,
          off + len, b.readable(), align, b.n, b.H, b.W, b.row_stride);
}
static void prep_case(const Buf& b, int x0, int y0, int rows, int cols, int nkb)
{
    const size_t readable = b.readable(), pitch = (size_t)b.row_stride;
    for (int grp = 0; grp < (b.n + 31) / 32; ++grp)
        for (int y = 0; y < rows; ++y) {
            const bool rows_safe = b.fmt ? p10::y210_rows_safe(grp, b.n, b.frame_stride, y0 + y, pitch, x0, nkb, readable) : p10::v210_rows_safe(x0, cols, nkb);
            for (int nn = 0; nn < 32; ++nn)
                for (int kb = 0; kb < nkb; ++kb) {
                    const int f = grp * 32 + nn;
                    if (!(f < b.n && kb * 32 < cols)) continue;   // `live`
                    const int xbeg = kb * 32, npx = cols - xbeg < 32 ? cols - xbeg : 32;
                    const int xs = (x0 + xbeg) & ~1, xend = x0 + xbeg + npx;
                    const size_t fo = (size_t)f * b.frame_stride;
                    if (b.fmt == MELF_YUV422_10_V210) {
                        const int cnt = p10::v210_prep_groups(xs, xend);
                        const size_t o = p10::v210_prep_off(fo, y0 + y, pitch, xs);
                        CHECK(cnt >= 1 && cnt <= p10::V210_PREP_GROUPS, "v210 prep: %d groups", cnt);
                        CHECK(p10::v210_slot(xs) == xs / 2 % 3 && o == fo + (size_t)(y0 + y) * pitch + (size_t)(xs / 6) * 16, "v210 prep: slot / offset of pixel %d", xs);
                        if (rows_safe) ++g_v_safe; else ++g_v_lane;
                        if (cnt == 7) ++g_v7;
                        for (int i = 0; i < p10::V210_PREP_GROUPS; ++i) {
                            if (!(i == 0 || (i < 6 && rows_safe) || i < cnt)) continue;   // the arm's own condition
                            load(b, o + (size_t)i * 16, 16, 16, "v210 prep group");
                            // ... and inside the row's own groups
                            CHECK(xs / 6 + i < p10::v210_groups(b.W), "v210 prep: group %d of the window at pixel %d leaves the row of %d pixels", i, xs, b.W);
                        }
                        // the groups loaded hold the lane's pixels
                        CHECK((xend - 1) / 6 < xs / 6 + cnt, "v210 prep: %d groups from pixel %d miss pixel %d", cnt, xs, xend - 1);
                        // a full lane: six groups, or seven from pair slot 2 at an odd first pixel
                        if (npx == 32) CHECK(cnt == ((xs / 2 % 3 == 2 && ((x0 + xbeg) & 1)) ? 7 : 6), "v210 prep: a full lane at pixel %d takes %d groups", x0 + xbeg, cnt);
                    } else {
                        const size_t o = p10::y210_prep_off(fo, y0 + y, pitch, xs);
                        if (rows_safe || p10::y210_lane_ok(o, readable)) {
                            if (rows_safe) ++g_y_safe; else ++g_y_lane;
                            load(b, o, p10::Y210_PREP_BYTES, 8, "Y210 prep window");
                            CHECK(xs <= x0 + xbeg && xs + 34 >= xend, "Y210 prep: window at %d misses pixels [%d, %d)", xs, x0 + xbeg, xend);
                        } else {
                            ++g_y_px;
                            for (int k = 0; k < npx; ++k) load(b, fo + p10::y210_px_off(y0 + y, pitch, x0 + xbeg + k), p10::PX_BYTES, 8, "Y210 prep macropixel");
                        }
                    }
                }
        }
}
static void prep_sweep()
{
    for (int fmt = 0; fmt < 2; ++fmt)
        for (int cols = 8; cols <= 100; ++cols)
            for (int x0 = 0; x0 < 12; ++x0)
                for (int e = 0; e < 3; ++e)           // the frame's right edge: the crop's, one and seven pixels further
                    for (int place = 0; place < 2; ++place)
                        for (int ni = 0; ni < 3; ++ni) {
                            if (ni == 2 && (cols + x0) % 5) continue;   // a second frame group: a fifth of the configurations
                            const int W = (x0 + cols + (e == 2 ? 7 : e) + 1) & ~1, H = 9, rows = 4;
                            const int n = ni == 0 ? 1 : (ni == 1 ? 3 : 34);
                            Buf b = make_buf(fmt, n, H, W, ((cols + x0) % 3) * align_of(fmt), 0);
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
    printf("checks %lld  descriptors: accepted %lld, rejected in 25 ways each  dial windows: v210 quads %lld exact %lld, y210 quads %lld exact %lld  "
           "v210 quads at fx0 %% 6 = 0, 2, 4: %lld %lld %lld\n",
           g_checks, g_accepted, g_quads[0], g_exact[0], g_quads[1], g_exact[1], g_phase[0][0], g_phase[0][2], g_phase[0][4]);
    printf("prep loads %lld  v210 lanes: row-safe %lld, by their own count %lld, with a seventh group %lld  y210 lanes: row-safe %lld, lane-safe %lld, "
           "macropixel loads %lld  failures %lld\n",
           g_loads, g_v_safe, g_v_lane, g_v7, g_y_safe, g_y_lane, g_y_px, g_fail);
    for (int k = 0; k <= P10_MESSAGES; ++k)
        if (!g_msg[k]) {
            fprintf(stderr, "message %d of check_yuv422_10 was never produced\n", k);
            return 1;
        }
    if (!g_quads[0] || !g_exact[0] || !g_quads[1] || !g_exact[1] || !g_phase[0][0] || !g_phase[0][2] || !g_phase[0][4] || g_phase[0][1] || g_phase[0][3] ||
        g_phase[0][5] || !g_v_safe || !g_v_lane || !g_v7 || !g_y_safe || !g_y_lane || !g_y_px || !g_rejected) {
        fprintf(stderr, "a path was never taken: the sweep does not cover it\n");
        return 1;
    }
    return g_fail ? 1 : 0;
}
