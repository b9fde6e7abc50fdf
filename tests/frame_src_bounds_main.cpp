// Stand-alone run of the dial reader's frame sources (meterelf_amd/csrc/melf_frame_src.h, the header the kernels compile) on the
// CPU: every source type the dial kernels instantiate is built and driven the way k_dials_body.inc drives it -- px for the colour
// core, column / col_px for the exact path, window / request / unpack for the window fetch -- on frames that are malloc'd to
// exactly (n - 1) * frame_stride + extent as the family's check_* (meterelf_amd/csrc/melf_frame_checks.h, the function the entry
// points call) leaves them for this program's descriptors: the last row unpadded, the planes back to back, at the tightest no stride
// padding behind a frame.  A descriptor the check does not take ends the program.  The loads are the header's own, so under -fsanitize=address the allocation's red zones
// are the bounds check: a load that starts before the buffer or ends behind it stops the program with the sanitizer's report.  A
// sibling of y16_bounds_main.cpp, which sweeps the 16-bit family's address functions and asserts the bounds itself.
// Built and run by tests/test_dials_instantiations.py (test_frame_src_bounds_sweep) with the ROCm tree's clang++ as a plain C++
// compiler (the header needs ext_vector_type), plain and with -fsanitize=address,undefined -fno-sanitize=alignment: the sources
// load unaligned dwords on purpose, which the device does in hardware and x86 does too.
//
// Base phases: where a family's check accepts a base of byte phase p != 0 (3-byte pixels, 4:2:0, planar YUV, planar RGB: 1 .. 3;
// 16-bit YUV: 2) the allocation is p bytes longer and the base starts p bytes in.  A load that starts up to p bytes BEFORE such a
// base lies inside the allocation and is not seen; at phase 0 it is.
//
// Values, since the sources run anyway: every pixel that leaves unpack equals bgr(px(X, Y)) of the same source, and px equals this
// program's own plain indexing of the planes (random bytes) through yuv_bgr / yuv_chroma of melf_device.h.  That pins the
// bookkeeping of the moved loads (cshift, mshifted, fodd, mshift, the byte-permute selectors) at every parity and edge.
//
// Swept per source type: crop widths 8 .. 72 (template width = crop width - 3, so that the match position takes both parities at
// both ends), crop origin parity in x, the crop's right edge on the frame's and one pixel short of it, the crop at the frame's first
// and last rows -- all crossed; the origin's parity in y drawn per configuration from a seeded generator.  Per configuration two
// parts.  (a) All window sizes 2 R + 5, R = 3 .. 29, at window origins -1, 0, 1, tw - ws - 1, tw - ws, tw - ws + 1 crossed, wy0
// of -1, 0, th - ws + 1 in rotation; the frame (the only, the first, the last of three), the base phase, row and stride padding,
// plane order and the match position (0, 1, far - 1, far per axis; far = crop size - template size) drawn.  (b) At every fourth
// width: frame x every base phase x the four match corners (0, 0), (far, far), (1, far - 1), (far - 1, 1) CROSSED (padded or
// tightest: drawn), at R = 3, 4 and every window origin -- so that the last frame's far corner against the buffer's last bytes, at
// every phase, is met by construction.  Every pc, every row group of NR = ws rounded up to 8.  The program counts, per source
// type, the windows that took the quads and the exact path and the lanes whose chroma / macropixel load was moved left, and
// fails if a count that the type can reach is zero.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

// the four device intrinsics of the header, as host functions (gfx9 ISA: v_perm_b32, v_alignbyte_b32, v_alignbit_b32)
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
static inline uint32_t host_alignbyte(uint32_t hi, uint32_t lo, uint32_t n) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (n & 3u))); }
static inline uint32_t host_alignbit(uint32_t hi, uint32_t lo, uint32_t n) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (n & 31u)); }
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
#include "tight_frames.h"

using namespace melf;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}
static int pick(int n) { return (int)(rnd() % (uint32_t)n); }

static long long g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                                                 \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(cond)) { if (g_fail++ < 20) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } \
    } while (0)

// n frames at `base`, the allocation exactly [base - phase, base + readable)
struct Buf {
    uint8_t *mem = nullptr, *base = nullptr;
    int n = 0, H = 0, W = 0, row_stride = 0, c_pitch = 0;
    size_t frame_stride = 0, extent = 0, phase = 0;
    int64_t off[3] = {0, 0, 0};   // plane offsets: U, V / B, G, R
    size_t readable() const { return (size_t)(n - 1) * frame_stride + extent; }
    void alloc()
    {
        const size_t len = phase + readable();
        mem = (uint8_t*)malloc(len);
        if (!mem) { fprintf(stderr, "out of memory\n"); exit(2); }
        for (size_t i = 0; i < len; ++i) mem[i] = (uint8_t)rnd();
        base = mem + phase;
    }
    void release() { free(mem); mem = base = nullptr; }
    const uint8_t* frame(int f) const { return base + (size_t)f * frame_stride; }
};

// d through its check (tight_frames.h): the frames as the launchers would be handed them
template <class D, class Check>
static Buf checked_buf(const Check& check, D& d, int spad, size_t phase)
{
    FrameBatch fb = {};
    const char* const msg = tight_frames(check, d, spad, phase, &fb);
    if (msg) {
        fprintf(stderr, "a descriptor of the sweep is not taken: %s (n %d H %d W %d)\nfailures 1\n", msg, d.n, d.H, d.W);
        exit(1);
    }
    Buf b;
    b.n = fb.n; b.H = fb.H; b.W = fb.W; b.phase = phase;
    b.row_stride = fb.row_stride; b.frame_stride = fb.frame_stride; b.extent = fb.lay.extent;
    const FrameLayout& lay = fb.lay;
    if (lay.pix == PIX_PLANAR) { b.off[0] = lay.planes.b_off; b.off[1] = lay.planes.g_off; b.off[2] = lay.planes.r_off; }
    else if (lay.pix == PIX_YUVP) { b.off[0] = lay.yuvp.u_off; b.off[1] = lay.yuvp.v_off; b.c_pitch = lay.yuvp.c_pitch; }
    else if (lay.pix == PIX_YUV16) { b.off[0] = lay.y16.u_off; b.off[1] = lay.y16.v_off; b.c_pitch = lay.y16.c_pitch; }
    else if (pix_yuv(lay.pix)) { b.off[0] = lay.yuv.u_off; b.off[1] = lay.yuv.v_off; b.c_pitch = lay.yuv.c_pitch; }
    return b;
}

struct Crop { int x0, y0, rows, cols, tw, th; };
struct Count {
    const char* name;
    bool can_quad, can_move;
    long long quads, exact, moved;
};

static DialsSrc dials_src(const Buf& b, const Crop& c)
{
    DialsSrc s;
    s.base = b.base; s.frame_stride = b.frame_stride; s.row_stride = b.row_stride;
    s.x0 = c.x0; s.y0 = c.y0; s.crop_rows = c.rows; s.crop_cols = c.cols;
    s.readable = b.readable();
    return s;
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One dial (one wave) of one frame, as k_dials_body.inc lines 78-103 and 129-137 drive the source.  ref(f, fx, fy): the B G R
// dword of frame pixel (fx, fy) by plain indexing; moved(W): the lane's chroma / macropixel load starts left of its first sample.
template <class Src, class Ref, class Moved>
static void dial_case(Count& cnt, const DialsSrc& ds, const typename Src::Args& sargs, const melf_params& P, int f, int mx, int my, int wx0, int wy0,
                      int ws, const Ref& ref, const Moved& moved)
{
    const uint8_t* const frame = ds.base + (size_t)f * ds.frame_stride;
    const Src FS(ds, sargs, P, frame, mx, my);
    const int tw = P.tw, th1 = P.th - 1, ylast = ws - 1, rs_u = (int)FS.rstride;
    const int ox = Src::FROM_HLS ? 0 : ds.x0 + mx, oy = Src::FROM_HLS ? 0 : ds.y0 + my;
    auto want = [&](int X, int Y) { return ref(f, ox + X, oy + Y) & 0xffffffu; };
    // the 5x5 colour core, at clamped coordinates
    {
        const int xs[5] = {-1, 0, tw / 2, tw - 1, tw}, ys[4] = {-1, 1, th1 - 1, th1 + 1};
        for (int a = 0; a < 5; ++a)
            for (int b = 0; b < 4; ++b) {
                const int X = clampi(xs[a], 0, tw - 1), Y = clampi(ys[b], 0, th1);
                const uint32_t got = FS.px(X, Y) & 0xffffffu;
                CHECK(got == want(X, Y), "%s: px(%d, %d) = %06x, plain indexing gives %06x (frame %d, match %d %d)", cnt.name, X, Y, got, want(X, Y), f, mx, my);
            }
    }
    // the exact path: a lane's column at clamped rows (a column or row the clamp repeats is loaded once here)
    for (int lane = 0, prevX = -1; lane < 64; ++lane) {
        const int Xc = clampi(wx0 + (lane < ws - 1 ? lane : ws - 1), 0, tw - 1);
        if (Xc == prevX) continue;
        prevX = Xc;
        const auto xcol = FS.column(Xc);
        for (int k = 0, prevY = -1; k < ws; ++k) {
            const int Y = clampi(wy0 + (k < ylast ? k : ylast), 0, th1);
            if (Y == prevY) continue;
            prevY = Y;
            const uint32_t got = FS.col_px(xcol, Y, rs_u) & 0xffffffu;
            CHECK(got == want(Xc, Y), "%s: col_px(%d, %d) = %06x, plain indexing gives %06x", cnt.name, Xc, Y, got, want(Xc, Y));
        }
    }
    // the window fetch: sixteen lanes a row, four rows a group, NR rows requested up front
    const int qshift = Src::EVEN_QUADS ? FS.quad_shift(wx0) : 0;
    const int npiece = Src::EVEN_QUADS ? (ws + qshift + 3) >> 2 : (ws + 3) >> 2;
    const int NG = ((ws + 7) & ~7) / 4;
    bool quads0 = false;
    for (int pc = 0; pc < 16; ++pc) {
        const auto W0 = FS.window(Src::EVEN_QUADS ? wx0 - qshift : wx0, npiece, pc, th1, rs_u, tw);
        if (pc == 0) {
            quads0 = W0.quads;
            if (quads0) ++cnt.quads; else ++cnt.exact;
        }
        CHECK(W0.quads == quads0, "%s: quads is not wave-uniform", cnt.name);
        if (!quads0) break;
        if (moved(W0)) ++cnt.moved;
        const int X0 = wx0 - qshift + 4 * (pc < npiece - 1 ? pc : npiece - 1);   // the lane's first pixel, crop column
        CHECK(4 * npiece - qshift >= ws && npiece <= 16, "%s: %d pieces do not hold %d columns", cnt.name, npiece, ws);
        for (int rg = 0; rg < 4; ++rg) {
            auto W = W0;   // a lane's own copy: request() keeps the lane's byte phases
            u32x4v raw[16];
            for (int g = 0; g < NG; ++g) raw[g] = W.request(g, clampi(wy0 + (4 * g + rg < ylast ? 4 * g + rg : ylast), 0, th1));
            for (int g = 0; g < NG; ++g) {
                const int Y = clampi(wy0 + (4 * g + rg < ylast ? 4 * g + rg : ylast), 0, th1);
                const u32x4v q = W.unpack(g, raw[g]);
                uint32_t pxs[4];
                if (Src::PB == 4) {
                    pxs[0] = q.x; pxs[1] = q.y; pxs[2] = q.z; pxs[3] = q.w;
                } else {   // the lane's 12 bytes in x, y, z
                    uint8_t b[16];
                    memcpy(b, &q, 16);
                    for (int j = 0; j < 4; ++j) pxs[j] = (uint32_t)b[3 * j] | (uint32_t)b[3 * j + 1] << 8 | (uint32_t)b[3 * j + 2] << 16;
                }
                for (int j = 0; j < 4; ++j) {
                    const uint32_t got = FS.bgr(pxs[j]) & 0xffffffu, same = FS.px(X0 + j, Y) & 0xffffffu;
                    CHECK(got == same && got == want(X0 + j, Y), "%s: unpack gives %06x at (%d, %d), px %06x, plain indexing %06x (pc %d g %d rg %d wx0 %d ws %d)",
                          cnt.name, got, X0 + j, Y, same, want(X0 + j, Y), pc, g, rg, wx0, ws);
                }
            }
        }
    }
}

// what a family adds to the sweep: its frames at their tightest, its source's arguments, its plain indexing
struct Cfg { int n, H, W, pad, spad, tw, th; size_t phase; int variant; };

template <class Src, class Fam>
static void sweep(Count& cnt, const Fam& fam)
{
    for (int cw = 8; cw <= 72; ++cw)
        for (int xpar = 0; xpar < 2; ++xpar)
            for (int edge = 0; edge < 2; ++edge)
                for (int place = 0; place < 2; ++place) {
                    const int ypar = pick(2);
                    Crop c;
                    c.cols = cw; c.rows = 10 + (place ? ypar : 0);
                    c.tw = c.cols - 3; c.th = c.rows - 3;
                    c.x0 = place ? 2 + xpar : xpar;
                    const int H = 14, W = c.x0 + cw + edge;
                    if (fam.even_w && (W & 1)) continue;   // (the neighbouring widths hold this parity and edge)
                    c.y0 = place ? H - c.rows : ypar;
                    // one configuration of the frames: fsel the only frame, the first or the last of three; no_pad: the tightest buffer
                    auto with_frames = [&](int fsel, size_t phase, bool no_pad, const auto& windows) {
                        Cfg g;
                        g.n = fsel == 0 ? 1 : 3; g.H = H; g.W = W; g.tw = c.tw; g.th = c.th;
                        g.pad = no_pad ? 0 : fam.pads[pick(fam.npads)] * pick(2); g.spad = no_pad ? 0 : fam.pads[pick(fam.npads)] * pick(2);
                        g.phase = phase;
                        g.variant = pick(1 << 16);
                        Buf b = fam.make(g);
                        b.alloc();
                        DialsSrc ds = dials_src(b, c);
                        melf_params P;
                        memset(&P, 0, sizeof P);
                        P.tw = c.tw; P.th = c.th;
                        if (Src::FROM_HLS) {   // melf_read_dials: packed crops of the template's size
                            ds.x0 = ds.y0 = 0; ds.crop_rows = c.th; ds.crop_cols = c.tw;
                        }
                        windows(b, g, ds, P, fsel == 2 ? 2 : 0);
                        b.release();
                    };
                    const int farx = Src::FROM_HLS ? 0 : c.cols - c.tw, fary = Src::FROM_HLS ? 0 : c.rows - c.th;
                    // (a) every window size at every window origin; frame, phase (0 half of the time), padding and match position drawn
                    with_frames(pick(3), (size_t)fam.phases[pick(2) * pick(fam.nphases)], false, [&](const Buf& b, const Cfg& g, const DialsSrc& ds, const melf_params& P, int f) {
                        for (int R = 3; R <= 29; ++R) {
                            const int ws = 2 * R + 5;
                            const int wx0s[6] = {-1, 0, 1, c.tw - ws - 1, c.tw - ws, c.tw - ws + 1}, wy0s[3] = {-1, 0, c.th - ws + 1};
                            for (int wi = 0; wi < 6; ++wi) {
                                const int ms[4] = {0, 1, -1, 0}, kx = pick(4), ky = pick(4);
                                const int mx = kx < 2 ? (ms[kx] < farx ? ms[kx] : farx) : farx + ms[kx], my = ky < 2 ? (ms[ky] < fary ? ms[ky] : fary) : fary + ms[ky];
                                fam.run(cnt, b, g, ds, P, f, mx < 0 ? 0 : mx, my < 0 ? 0 : my, wx0s[wi], wy0s[(wi + R) % 3], ws);
                            }
                        }
                    });
                    // (b) every fourth width (both parities of the origin; the frame's width even there, so every family runs it with
                    // the crop's right edge on the frame's): frame x base phase x match corner CROSSED (padded or tightest: drawn), at a
                    // window size whose last piece ends one column behind the window (ws = 11) and one whose last piece ends three
                    // behind it (13), at every window origin.  The buffer's last bytes under the far corner of the last frame are met here at
                    // every phase, by construction and not by the draw.
                    if ((cw + xpar) % 4 != 0) continue;
                    for (int fsel = 0; fsel < 3; ++fsel)
                        for (int pi = 0; pi < fam.nphases; ++pi)
                                with_frames(fsel, (size_t)fam.phases[pi], pick(2), [&](const Buf& b, const Cfg& g, const DialsSrc& ds, const melf_params& P, int f) {
                                    const int corners[4][2] = {{0, 0}, {farx, fary}, {farx ? 1 : 0, fary ? fary - 1 : 0}, {farx ? farx - 1 : 0, fary ? 1 : 0}};
                                    const int Rs[2] = {3, 4};
                                    for (int ci = 0; ci < 4; ++ci)
                                        for (int ri = 0; ri < 2; ++ri) {
                                            const int ws = 2 * Rs[ri] + 5;
                                            const int wx0s[6] = {-1, 0, 1, c.tw - ws - 1, c.tw - ws, c.tw - ws + 1}, wy0s[3] = {-1, 0, c.th - ws + 1};
                                            for (int wi = 0; wi < 6; ++wi)
                                                fam.run(cnt, b, g, ds, P, f, corners[ci][0], corners[ci][1], wx0s[wi], wy0s[(wi + ri + ci) % 3], ws);
                                        }
                                });
                }
    printf("%-28s windows: quads %lld, exact path %lld, lanes with a moved load %lld\n", cnt.name, cnt.quads, cnt.exact, cnt.moved);
    if ((cnt.can_quad && cnt.quads == 0) || cnt.exact == 0 || (cnt.can_move && cnt.moved == 0)) {
        ++g_fail;
        fprintf(stderr, "%s: a path was never taken: the sweep does not cover it\n", cnt.name);
    }
}

static const int PADS_BYTE[4] = {0, 1, 2, 6}, PADS_DWORD[3] = {0, 4, 8}, PADS_WORD[3] = {0, 2, 6};
static const int PHASES_ANY[4] = {0, 1, 2, 3}, PHASES_NONE[1] = {0}, PHASES_WORD[2] = {0, 2};
static const YuvMatrix MATRICES[4] = {YUV_BT601_LIMITED_MATRIX, YUV_BT601_FULL_MATRIX, YUV_BT709_LIMITED_MATRIX, YUV_BT709_FULL_MATRIX};
static const auto never_moved = [](const auto&) { return false; };

// ---- packed pixels (check_frames): rows of W * PB bytes, 4-byte pixels 4-byte aligned throughout ------------------------------
template <int PB, bool RT_ORDER, bool FROM_HLS>
struct PackedFam {
    using Src = DialPacked<PB, RT_ORDER, FROM_HLS>;
    bool even_w = false;
    const int* pads = PB == 4 ? PADS_DWORD : PADS_BYTE;
    int npads = PB == 4 ? 3 : 4;
    const int* phases = PB == 4 ? PHASES_NONE : PHASES_ANY;
    int nphases = PB == 4 ? 1 : 4;
    Buf make(const Cfg& g) const
    {
        if (FROM_HLS) {   // melf_read_dials: n packed th x tw crops of three bytes a pixel (no descriptor: the entry point's own arguments)
            Buf b;
            b.n = g.n; b.H = g.H; b.W = g.W; b.phase = 0;
            b.row_stride = g.tw * 3; b.extent = (size_t)g.th * b.row_stride; b.frame_stride = b.extent;
            return b;
        }
        melf_frames d = {PB == 4 ? MELF_PIX_BGRA : MELF_PIX_BGR, g.n, g.H, g.W, (int64_t)g.W * PB + g.pad, 0};
        return checked_buf(check_frames, d, g.spad, g.phase);
    }
    void run(Count& cnt, const Buf& b, const Cfg& g, const DialsSrc& ds, const melf_params& P, int f, int mx, int my, int wx0, int wy0, int ws) const
    {
        const bool rgb = RT_ORDER && (g.variant & 1);
        const typename Src::Args a{rgb ? 0x00020002u : 0u};
        const int rs = FROM_HLS ? P.tw * 3 : b.row_stride;
        auto ref = [&](int fr, int fx, int fy) {
            const uint8_t* p = b.frame(fr) + (size_t)fy * rs + (size_t)fx * PB;
            return rgb ? (uint32_t)p[2] | (uint32_t)p[1] << 8 | (uint32_t)p[0] << 16 : (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
        };
        dial_case<Src>(cnt, ds, a, P, f, mx, my, wx0, wy0, ws, ref, never_moved);
    }
};

// ---- planar / semi-planar 8-bit YUV (check_yuv, check_yuv_planar) -----------------------------------------------------------------
// The Y plane, then the chroma: semi-planar one plane of pairs (either order), planar two planes back to back (either order).
// f420: MELF_YUV_NV12 / MELF_YUV_I420 for melf_yuv_frames (NV12: an even u_offset), -1 for melf_yuv_planar_frames.  The caller's side of
// the layout -- the pitches and where the chroma starts -- is written here; what a frame then spans is the check's.
struct YuvGeom { int sub_x, sub_y, c_step, f420; };
static Buf make_yuv(const Cfg& g, const YuvGeom& y, bool vfirst)
{
    const int cw = (g.W >> y.sub_x) * y.c_step, ch = g.H >> y.sub_y;
    const int64_t y_pitch = g.W + g.pad, c_pitch = cw + g.pad;
    const int64_t y_end = (int64_t)(g.H - 1) * y_pitch + g.W, c_len = (int64_t)(ch - 1) * c_pitch + (y.c_step == 2 ? cw - 1 : cw);
    const int64_t lo = y.f420 == MELF_YUV_NV12 ? (y_end + 1) & ~(int64_t)1 : y_end, hi = y.c_step == 2 ? lo + 1 : lo + c_len;
    const int64_t u_off = vfirst ? hi : lo, v_off = vfirst ? lo : hi;
    if (y.f420 >= 0) {
        melf_yuv_frames d = {y.f420, MELF_YUV_BT601_LIMITED, g.n, g.H, g.W, 0, y_pitch, c_pitch, u_off, v_off, 0};
        return checked_buf(check_yuv, d, g.spad, g.phase);
    }
    melf_yuv_planar_frames d = {MELF_YUV_BT601_LIMITED, g.n, g.H, g.W, y.sub_x, y.sub_y, y.c_step, 0, y_pitch, c_pitch, u_off, v_off, 0};
    return checked_buf(check_yuv_planar, d, g.spad, g.phase);
}
static uint32_t ref_yuv(const Buf& b, const YuvGeom& y, const YuvMatrix& m, int fr, int fx, int fy)
{
    const uint8_t* F = b.frame(fr);
    const size_t co = (size_t)(fy >> y.sub_y) * (size_t)b.c_pitch + (size_t)((fx >> y.sub_x) * y.c_step);
    return yuv_bgr(F[(size_t)fy * b.row_stride + fx], yuv_chroma<false>(F[b.off[0] + co], F[b.off[1] + co], m), m);
}
template <bool PLANAR>
struct Yuv420Fam {
    using Src = DialYuv420<PLANAR>;
    bool even_w = true;
    const int* pads = PADS_BYTE; int npads = 4;
    const int* phases = PHASES_ANY; int nphases = 4;
    YuvGeom yg{1, 1, PLANAR ? 1 : 2, PLANAR ? MELF_YUV_I420 : MELF_YUV_NV12};
    Buf make(const Cfg& g) const { return make_yuv(g, yg, PLANAR && (g.variant & 1)); }   // I420 / YV12; NV12: U first
    void run(Count& cnt, const Buf& b, const Cfg& g, const DialsSrc& ds, const melf_params& P, int f, int mx, int my, int wx0, int wy0, int ws) const
    {
        const YuvMatrix& m = MATRICES[(g.variant >> 1) & 3];
        const YuvPlanes yp = {b.off[0], b.off[1], b.c_pitch, 0};
        const typename Src::Args a{yp, m};
        auto ref = [&](int fr, int fx, int fy) { return ref_yuv(b, yg, m, fr, fx, fy); };
        dial_case<Src>(cnt, ds, a, P, f, mx, my, wx0, wy0, ws, ref, [](const auto& W) { return W.cstart != (W.fx0 >> 1); });
    }
};
template <int SUBX, int CSTEP>
struct YuvPlanarFam {
    using Src = DialYuvPlanar<SUBX, CSTEP>;
    bool even_w = SUBX == 1;
    const int* pads = PADS_BYTE; int npads = 4;
    const int* phases = PHASES_ANY; int nphases = 4;
    Buf make(const Cfg& g) const { return make_yuv(g, YuvGeom{SUBX, (g.variant >> 3) & 1, CSTEP, -1}, g.variant & 1); }
    void run(Count& cnt, const Buf& b, const Cfg& g, const DialsSrc& ds, const melf_params& P, int f, int mx, int my, int wx0, int wy0, int ws) const
    {
        const YuvGeom yg{SUBX, (g.variant >> 3) & 1, CSTEP, -1};
        const YuvMatrix& m = MATRICES[(g.variant >> 1) & 3];
        const YuvPlanarPlanes yp = {b.off[0], b.off[1], b.c_pitch, SUBX, yg.sub_y, CSTEP};
        const typename Src::Args a{yp, m};
        auto ref = [&](int fr, int fx, int fy) { return ref_yuv(b, yg, m, fr, fx, fy); };
        dial_case<Src>(cnt, ds, a, P, f, mx, my, wx0, wy0, ws, ref, [](const auto& W) { return SUBX && W.cstart != (W.fx0 >> 1); });
    }
};

// ---- packed YUV 4:2:2 (check_yuv422): macropixels of 4 bytes, everything 4-byte aligned, even width --------------------------------
struct P422Fam {
    using Src = DialP422;
    bool even_w = true;
    const int* pads = PADS_DWORD; int npads = 3;
    const int* phases = PHASES_NONE; int nphases = 1;
    Buf make(const Cfg& g) const
    {
        melf_yuv422_frames d = {MELF_YUV422_YUYV + g.variant % 3, MELF_YUV_BT601_LIMITED, g.n, g.H, g.W, 0, (int64_t)g.W * 2 + g.pad, 0};
        return checked_buf(check_yuv422, d, g.spad, 0);
    }
    void run(Count& cnt, const Buf& b, const Cfg& g, const DialsSrc& ds, const melf_params& P, int f, int mx, int my, int wx0, int wy0, int ws) const
    {
        const int fmt = g.variant % 3;   // YUYV, UYVY, YVYU: where Y0, U, Y1, V lie in a macropixel
        static const int at[3][4] = {{0, 1, 2, 3}, {1, 0, 3, 2}, {0, 3, 2, 1}};
        const YuvMatrix& m = MATRICES[(g.variant >> 4) & 3];
        const Src::Args a{p422_sel(PIX_YUYV + fmt), m};
        auto ref = [&](int fr, int fx, int fy) {
            const uint8_t* mp = b.frame(fr) + (size_t)fy * b.row_stride + (size_t)(fx >> 1) * 4;
            return yuv_bgr(mp[at[fmt][fx & 1 ? 2 : 0]], yuv_chroma<false>(mp[at[fmt][1]], mp[at[fmt][3]], m), m);
        };
        dial_case<Src>(cnt, ds, a, P, f, mx, my, wx0, wy0, ws, ref, [](const auto& W) { return W.mshifted; });
    }
};

// ---- planar RGB (check_planes): three planes back to back in any order, any alignment ---------------------------------------------
struct PlanarRgbFam {
    using Src = DialPlanarRgb;
    bool even_w = false;
    const int* pads = PADS_BYTE; int npads = 4;
    const int* phases = PHASES_ANY; int nphases = 4;
    Buf make(const Cfg& g) const
    {
        static const int order[3][3] = {{0, 1, 2}, {2, 1, 0}, {1, 2, 0}};   // B G R, R G B, and a rotation
        const int* const o = order[g.variant % 3];
        const int64_t pitch = g.W + g.pad, span = (int64_t)(g.H - 1) * pitch + g.W;   // the caller's side: the three planes back to back
        melf_planar_frames d = {g.n, g.H, g.W, 0, o[0] * span, o[1] * span, o[2] * span, pitch, 0};
        return checked_buf(check_planes, d, g.spad, g.phase);
    }
    void run(Count& cnt, const Buf& b, const Cfg&, const DialsSrc& ds, const melf_params& P, int f, int mx, int my, int wx0, int wy0, int ws) const
    {
        const PlanarPlanes pl = {b.off[0], b.off[1], b.off[2]};
        const Src::Args a{pl};
        auto ref = [&](int fr, int fx, int fy) {
            const uint8_t* F = b.frame(fr) + (size_t)fy * b.row_stride + fx;
            return (uint32_t)F[b.off[0]] | (uint32_t)F[b.off[1]] << 8 | (uint32_t)F[b.off[2]] << 16;
        };
        dial_case<Src>(cnt, ds, a, P, f, mx, my, wx0, wy0, ws, ref, never_moved);
    }
};

// ---- 16-bit YUV (check_yuv16): 2-byte samples, everything 2-byte aligned, even width ------------------------------------------------
template <int CSTEP>
struct Yuv16Fam {
    using Src = DialYuv16<CSTEP>;
    bool even_w = true;
    const int* pads = PADS_WORD; int npads = 3;
    const int* phases = PHASES_WORD; int nphases = 2;
    Buf make(const Cfg& g) const
    {
        const int sub_y = (g.variant >> 3) & 1;
        const bool vfirst = g.variant & 1;
        const int cw = (g.W >> 1) * CSTEP * 2, ch = g.H >> sub_y;   // the caller's side: the pitches, the planes back to back
        const int64_t y_pitch = g.W * 2 + g.pad, c_pitch = cw + g.pad;
        const int64_t y_end = (int64_t)(g.H - 1) * y_pitch + (int64_t)g.W * 2, c_len = (int64_t)(ch - 1) * c_pitch + (CSTEP == 2 ? cw - 2 : cw);
        const int64_t lo = y_end, hi = CSTEP == 2 ? lo + 2 : lo + c_len;
        melf_yuv16_frames d = {MELF_YUV_BT601_LIMITED, g.n, g.H, g.W, sub_y, CSTEP, (g.variant >> 5) % 9, 0, y_pitch, c_pitch, vfirst ? hi : lo, vfirst ? lo : hi, 0};
        return checked_buf(check_yuv16, d, g.spad, g.phase);
    }
    void run(Count& cnt, const Buf& b, const Cfg& g, const DialsSrc& ds, const melf_params& P, int f, int mx, int my, int wx0, int wy0, int ws) const
    {
        const int sub_y = (g.variant >> 3) & 1, shift = (g.variant >> 5) % 9;
        const YuvMatrix& m = MATRICES[(g.variant >> 1) & 3];
        const Yuv16Planes yp = {b.off[0], b.off[1], b.c_pitch, sub_y, CSTEP, shift};
        const typename Src::Args a{yp, m};
        auto s16 = [&](const uint8_t* p) { return (int)y16::reduce((uint32_t)p[0] | (uint32_t)p[1] << 8, (uint32_t)shift); };
        auto ref = [&](int fr, int fx, int fy) {
            const uint8_t* F = b.frame(fr);
            const size_t co = (size_t)(fy >> sub_y) * (size_t)b.c_pitch + (size_t)(fx >> 1) * 2 * CSTEP;
            return yuv_bgr(s16(F + (size_t)fy * b.row_stride + (size_t)fx * 2), yuv_chroma<false>(s16(F + b.off[0] + co), s16(F + b.off[1] + co), m), m);
        };
        dial_case<Src>(cnt, ds, a, P, f, mx, my, wx0, wy0, ws, ref, never_moved);
    }
};

template <class Fam>
static void run_family(const char* name, bool can_quad, bool can_move)
{
    Count cnt{name, can_quad, can_move, 0, 0, 0};
    const Fam fam{};
    sweep<typename Fam::Src>(cnt, fam);
}

int main()
{
    // the byte permute, by hand: the selectors' four kinds (a byte of either operand, constant 0)
    if (host_perm(0x44332211u, 0x88776655u, 0x07060100u) != 0x44336655u || host_perm(0u, 0xaabbccddu, 0x0c000102u) != 0x00ddccbbu ||
        host_alignbyte(0x44332211u, 0x88776655u, 3) != 0x33221188u || host_alignbit(0x44332211u, 0x88776655u, 8) != 0x11887766u) {
        fprintf(stderr, "the host forms of the byte permutes are wrong\n");
        return 1;
    }
    run_family<PackedFam<3, false, false>>("DialPacked<3, false>", true, false);
    run_family<PackedFam<4, false, false>>("DialPacked<4, false>", true, false);
    run_family<PackedFam<3, true, false>>("DialPacked<3, true>", true, false);
    run_family<PackedFam<4, true, false>>("DialPacked<4, true>", true, false);
    run_family<PackedFam<3, false, true>>("DialPacked<3, false, HLS>", false, false);   // FROM_HLS: no window fetch by construction
    run_family<Yuv420Fam<false>>("DialYuv420<false> (NV12)", true, true);
    run_family<Yuv420Fam<true>>("DialYuv420<true> (I420)", true, true);
    run_family<YuvPlanarFam<0, 1>>("DialYuvPlanar<0, 1>", true, false);   // a sample per pixel: nothing to move
    run_family<YuvPlanarFam<0, 2>>("DialYuvPlanar<0, 2>", true, false);
    run_family<YuvPlanarFam<1, 1>>("DialYuvPlanar<1, 1>", true, true);
    run_family<YuvPlanarFam<1, 2>>("DialYuvPlanar<1, 2>", true, true);
    run_family<P422Fam>("DialP422", true, true);
    run_family<PlanarRgbFam>("DialPlanarRgb", true, false);
    run_family<Yuv16Fam<1>>("DialYuv16<1>", true, false);
    run_family<Yuv16Fam<2>>("DialYuv16<2>", true, false);
    printf("checks %lld  failures %lld\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
