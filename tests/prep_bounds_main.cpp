// Stand-alone sweep of the load addresses of the prep kernels' 8-bit arms (meterelf_amd/csrc/prep_lplane_body.inc: PX 3, 4, 20, 21,
// 22, 23 and 24 in its four SUBX / CSTEP forms), on the CPU, against buffers of exact extent -- what y16_bounds_main.cpp's prep_case
// does for PX 25.  Every load of every live lane must lie inside [base, base + readable), readable = (n - 1) * frame_stride + extent
// as the family's check_* (meterelf_amd/csrc/melf_frame_checks.h, the function the entry points call) leaves them for this program's
// descriptors: the last row unpadded, the planes back to back, the stride a frame and the swept padding.  A descriptor the check
// does not take is a failure.  The aligned dword windows must start on a dword of the address space and hold the lane's samples.
//
// The arms compute their addresses with the functions of meterelf_amd/csrc/melf_prep_addr.h (rows_safe, the lane's own test, the
// windows' offsets and spans, and the launcher's prep_window_readable), and this program calls the same functions: a change of the
// kernel's arithmetic is a change of what is swept here.  What stays in this file is what the header does not hold: the byte phase of
// a window (the address's low two bits), the per-sample loads of the last path, and the frames.
// The PX 3 and PX 20 / 21 arms test their windows against the buffer's end only; their first dword is kept behind the base by the
// launcher (launch_match_prep hands the kernel prep_window_readable as src.readable): without it this sweep reports the window of
// the buffer's very first samples starting 1 .. 3 bytes before a base that is not 4-byte aligned.
// PX 1 (single-channel images) has no window: its lanes load their own bytes one by one, inside the image by `live` and npx.
//
// Swept: crop widths 8 .. 96 (one to three blocks) ending on the frame's right edge or one pixel short of it; crop origin parities;
// the crop at the frame's first rows and at its last, in frames of 12 rows and of 4 (where the planes behind the first are
// shorter than a window, so that the first plane's own test decides); every row of the crop; every live lane; the planner's nkb and nkb + 1; 1, 3
// and 34 frames (a second frame group); base phases 0 .. 3 where the family's check accepts them; row and stride padding of 0, 1, 2
// and 6 bytes (0, 4, 8 where everything is 4-byte aligned); both plane orders.  Each arm must take each of its three paths -- every
// window of the row safe, the lane's windows safe, sample by sample -- at least once.
// Built and run by tests/test_dials_instantiations.py (test_prep_bounds_sweep), plain and under -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../meterelf_amd/csrc/melf_prep_addr.h"
#include "tight_frames.h"

namespace prep = melf::prep;

struct Frames {
    int n, H, W, row_stride, c_pitch;
    int64_t frame_stride, extent, phase;
    int64_t off[3];   // U, V / B, G, R
    int64_t readable() const { return (int64_t)(n - 1) * frame_stride + extent; }
};
struct Crop { int x0, y0, rows, cols; };
struct Arm {
    const char* name;
    long long row_safe, lane_safe, samples;
};

static long long g_loads = 0, g_fail = 0, g_before = 0;   // g_before: failures that start before the base
static const char* g_arm = "";
static void fail(const Frames& f, const char* what, int64_t a, int64_t b)
{
    if (a < 0) ++g_before;
    if (g_fail++ < 20)
        fprintf(stderr, "%s: %s [%lld, %lld) of %lld readable bytes, phase %lld (n %d H %d W %d row_stride %d c_pitch %d frame_stride %lld)\n", g_arm, what,
                (long long)a, (long long)b, (long long)f.readable(), (long long)f.phase, f.n, f.H, f.W, f.row_stride, f.c_pitch, (long long)f.frame_stride);
}
// one load of len bytes at byte off from the base (signed: a start before the base is negative)
static void load(const Frames& f, int64_t off, int64_t len, int64_t align, const char* what)
{
    ++g_loads;
    if (off < 0 || off + len > f.readable() || (f.phase + off) % align) fail(f, what, off, off + len);
}
// the aligned window [first, first + span) holds the lane's bytes [lo, hi)
static void holds(const Frames& f, int64_t first, int64_t span, int64_t lo, int64_t hi, const char* what)
{
    if (first > lo || first + span < hi) fail(f, what, first, first + span);
}

template <class Rows, class Lane>
static void prep_rows(Arm& arm, const Frames& f, const Crop& c, int nkb, const Rows& rows_safe_of, const Lane& lane)
{
    g_arm = arm.name;
    const int groups = (f.n + 31) / 32;
    for (int grp = 0; grp < groups; ++grp)
        for (int y = 0; y < c.rows; ++y) {
            const bool rows_safe = rows_safe_of(grp, y);
            for (int n = 0; n < 32; ++n)
                for (int kb = 0; kb < nkb; ++kb) {
                    const int fr = grp * 32 + n;
                    if (!(kb < nkb && fr < f.n && y < c.rows && kb * 32 < c.cols)) continue;   // `live`
                    const int xbeg = kb * 32, npx = c.cols - xbeg < 32 ? c.cols - xbeg : 32;
                    const int path = lane(rows_safe, fr, y, xbeg, npx);
                    if (path == 0) ++arm.row_safe; else if (path == 1) ++arm.lane_safe; else ++arm.samples;
                }
        }
}
// ---- PX 3 / PX 4: packed pixels -----------------------------------------------------------------------------------------------------
template <int PX>
static void packed_case(Arm& arm, const Frames& f, const Crop& c, int nkb)
{
    constexpr int PB = prep::packed_pb(PX), WIN = prep::packed_win(PX);
    // what the launcher hands the kernel as src.readable (launch_match_prep: the PX 3 arm has no test for its windows' first dword)
    const size_t readable = PX == 3 ? prep::prep_window_readable(prep::ARM_PX3, (size_t)f.phase, c.x0, c.y0, (size_t)f.readable()) : (size_t)f.readable();
    prep_rows(
        arm, f, c, nkb,
        [&](int grp, int y) { return prep::packed_rows_safe(grp, f.n, (size_t)f.frame_stride, c.y0 + y, f.row_stride, c.x0, nkb, PB, WIN, readable); },
        [&](bool rows_safe, int fr, int y, int xbeg, int npx) {
            const int64_t prow = (int64_t)fr * f.frame_stride + (int64_t)(c.y0 + y) * f.row_stride;   // (the body's prow)
            const size_t o = prep::packed_x_off(c.x0 + xbeg, PB);
            const int64_t p = prow + (int64_t)o;
            if (rows_safe || prep::packed_lane_ok(fr, (size_t)f.frame_stride, c.y0 + y, f.row_stride, o, WIN, readable)) {
                if (PX == 3) {
                    const int64_t mis = (f.phase + p) & 3;   // aligned dwords from the dword that holds the first byte
                    load(f, p - mis, WIN, 4, "PX 3 window");
                    holds(f, p - mis, WIN, p, p + 96, "PX 3 window misses the lane's pixels");
                } else {
                    load(f, p, WIN, 4, "PX 4 window");
                }
                return rows_safe ? 0 : 1;
            }
            for (int k = 0; k < npx; ++k) load(f, p + (int64_t)k * PB, PB == 4 ? 4 : 3, PB == 4 ? 4 : 1, "packed pixel");
            return 2;
        });
}

// ---- PX 20 / PX 21: NV12, I420 -------------------------------------------------------------------------------------------------------
template <bool NV12>
static void yuv420_case(Arm& arm, const Frames& f, const Crop& c, int nkb)
{
    const int64_t u_off = f.off[0], v_off = f.off[1];
    const size_t readable = prep::prep_window_readable(prep::ARM_YUV420, (size_t)f.phase, c.x0, c.y0, (size_t)f.readable());   // (as for PX 3)
    constexpr int CS = prep::yuv420_c_span(NV12);
    prep_rows(
        arm, f, c, nkb,
        [&](int grp, int y) {
            const size_t yuv_last = (size_t)prep::last_frame(grp, f.n) * (size_t)f.frame_stride;
            return prep::yuv420_rows_safe(yuv_last, c.y0 + y, f.row_stride, prep::yuv420_xlast(c.x0, nkb), u_off, v_off, prep::yuv420_crow(c.y0 + y, f.c_pitch), NV12,
                                          readable);
        },
        [&](bool rows_safe, int fr, int y, int xbeg, int npx) {
            const size_t yuv_crow = prep::yuv420_crow(c.y0 + y, f.c_pitch);
            const int xs = (c.x0 + xbeg) & ~1;
            const size_t fo = (size_t)fr * (size_t)f.frame_stride;
            const size_t yo = prep::yuv420_y_off(fo, c.y0 + y, f.row_stride, xs);
            const size_t uo = prep::yuv420_c_off(fo, u_off, yuv_crow, xs, NV12), vo = prep::yuv420_c_off(fo, v_off, yuv_crow, xs, false);
            if (rows_safe || prep::yuv420_lane_ok(yo, uo, vo, NV12, readable)) {
                const int64_t my = (f.phase + yo) & 3, mu = (f.phase + uo) & 3, mv = (f.phase + vo) & 3;
                load(f, (int64_t)yo - my, prep::YUV420_Y_SPAN, 4, "4:2:0 Y window");
                holds(f, (int64_t)yo - my, prep::YUV420_Y_SPAN, yo, yo + 34, "4:2:0 Y window misses the lane's pixels");
                load(f, (int64_t)uo - mu, CS, 4, NV12 ? "NV12 UV window" : "I420 U window");
                holds(f, (int64_t)uo - mu, CS, uo, uo + (NV12 ? 34 : 17), "4:2:0 chroma window misses the lane's samples");
                if (!NV12) {
                    load(f, (int64_t)vo - mv, CS, 4, "I420 V window");
                    holds(f, (int64_t)vo - mv, CS, vo, vo + 17, "I420 V window misses the lane's samples");
                }
                if (xs > c.x0 + xbeg || xs + 34 < c.x0 + xbeg + npx) fail(f, "4:2:0 window misses pixels", xs, xs + 34);
                return rows_safe ? 0 : 1;
            }
            for (int k = 0; k < npx; ++k) {   // the body's byte loads: the crop's own samples
                const int cx = (c.x0 + xbeg + k) >> 1;
                load(f, (int64_t)fo + (int64_t)(c.y0 + y) * f.row_stride + c.x0 + xbeg + k, 1, 1, "4:2:0 Y sample");
                load(f, (int64_t)fo + u_off + (int64_t)yuv_crow + (NV12 ? 2 * cx : cx), 1, 1, "4:2:0 U sample");
                load(f, (int64_t)fo + v_off + (int64_t)yuv_crow + (NV12 ? 2 * cx : cx), 1, 1, "4:2:0 V sample");
            }
            return 2;
        });
}

// ---- PX 22: packed 4:2:2 ---------------------------------------------------------------------------------------------------------------
static void p422_case(Arm& arm, const Frames& f, const Crop& c, int nkb)
{
    const size_t readable = (size_t)f.readable();
    prep_rows(
        arm, f, c, nkb,
        [&](int grp, int y) { return prep::p422_rows_safe(grp, f.n, (size_t)f.frame_stride, c.y0 + y, f.row_stride, c.x0, nkb, readable); },
        [&](bool rows_safe, int fr, int y, int xbeg, int npx) {
            const int64_t prow = (int64_t)fr * f.frame_stride + (int64_t)(c.y0 + y) * f.row_stride;
            const int xs = (c.x0 + xbeg) & ~1;
            const size_t o = prep::p422_x_off(xs);
            if (rows_safe || prep::p422_lane_ok(fr, (size_t)f.frame_stride, c.y0 + y, f.row_stride, o, readable)) {
                load(f, prow + (int64_t)o, 64, 4, "4:2:2 window");                                   // four 16-byte loads, 4-byte aligned
                load(f, prow + (int64_t)o + 64, prep::P422_SPAN - 64, 4, "4:2:2 window's 17th macropixel");
                if (xs > c.x0 + xbeg || xs + 34 < c.x0 + xbeg + npx) fail(f, "4:2:2 window misses pixels", xs, xs + 34);
                return rows_safe ? 0 : 1;
            }
            for (int k = 0; k < npx; ++k) load(f, prow + (int64_t)((c.x0 + xbeg + k) >> 1) * 4, 4, 4, "4:2:2 macropixel");
            return 2;
        });
}

// ---- PX 23: planar RGB -------------------------------------------------------------------------------------------------------------------
static void planar_case(Arm& arm, const Frames& f, const Crop& c, int nkb)
{
    const size_t readable = (size_t)f.readable();
    const uint32_t pl_bm = (uint32_t)(f.phase & 3);
    auto min3 = [](int64_t a, int64_t b, int64_t d) { return a < b ? (a < d ? a : d) : (b < d ? b : d); };
    auto max3 = [](int64_t a, int64_t b, int64_t d) { return a > b ? (a > d ? a : d) : (b > d ? b : d); };
    const size_t pl_lo = (size_t)min3(f.off[0], f.off[1], f.off[2]), pl_hi = (size_t)max3(f.off[0], f.off[1], f.off[2]);
    prep_rows(
        arm, f, c, nkb,
        [&](int grp, int y) {
            return prep::planar_rows_safe(pl_bm, grp, f.n, (size_t)f.frame_stride, pl_lo, pl_hi, prep::planar_row(c.y0 + y, f.row_stride, c.x0), nkb, readable);
        },
        [&](bool rows_safe, int fr, int y, int xbeg, int npx) {
            const size_t o = prep::planar_lane_off(fr, (size_t)f.frame_stride, c.y0 + y, f.row_stride, c.x0 + xbeg);
            size_t op[3];
            uint32_t m[3];
            for (int k = 0; k < 3; ++k) {
                op[k] = o + (size_t)f.off[k];
                m[k] = (pl_bm + (uint32_t)op[k]) & 3u;
            }
            if (rows_safe || prep::planar_lane_ok(op[0], m[0], op[1], m[1], op[2], m[2], readable)) {
                for (int k = 0; k < 3; ++k) {
                    load(f, (int64_t)op[k] - m[k], prep::PLANAR_SPAN, 4, "planar window");
                    holds(f, (int64_t)op[k] - m[k], prep::PLANAR_SPAN, op[k], op[k] + 32, "planar window misses the lane's samples");
                }
                return rows_safe ? 0 : 1;
            }
            for (int k = 0; k < 3; ++k)
                for (int j = 0; j < npx; ++j) load(f, (int64_t)op[k] + j, 1, 1, "planar sample");
            return 2;
        });
}

// ---- PX 24: planar / semi-planar YUV (load_window: k_match_mfma.hip) -----------------------------------------------------------------------
template <int SUBX, int CSTEP>
static void yuvp_case(Arm& arm, const Frames& f, const Crop& c, int nkb, int sub_y)
{
    constexpr int CB = prep::yuvp_cb(SUBX, CSTEP), CWIN = prep::yuvp_cwin(SUBX, CSTEP);
    const size_t readable = (size_t)f.readable();
    const int64_t u_off = f.off[0], v_off = f.off[1];
    const uint32_t yp_bm = (uint32_t)(f.phase & 3);
    const size_t yp_c0 = (size_t)(u_off < v_off ? u_off : v_off), yp_c1 = (size_t)(u_off < v_off ? v_off : u_off);
    const int yp_x0 = c.x0 & ~1, yp_xlast = yp_x0 + 32 * (nkb - 1);
    prep_rows(
        arm, f, c, nkb,
        [&](int grp, int y) {
            const size_t yp_first = (size_t)grp * 32 * (size_t)f.frame_stride, yp_last = (size_t)prep::last_frame(grp, f.n) * (size_t)f.frame_stride;
            const size_t yp_yrow = (size_t)(c.y0 + y) * (size_t)f.row_stride, yp_crow = (size_t)((c.y0 + y) >> sub_y) * (size_t)f.c_pitch;
            return prep::yuvp_rows_safe(yp_bm, yp_first, yp_last, yp_yrow, yp_crow, yp_c0, yp_c1, yp_x0, yp_xlast, SUBX, CSTEP, CWIN, readable);
        },
        [&](bool rows_safe, int fr, int y, int xbeg, int npx) {
            const size_t yp_yrow = (size_t)(c.y0 + y) * (size_t)f.row_stride, yp_crow = (size_t)((c.y0 + y) >> sub_y) * (size_t)f.c_pitch;
            const int xs = (c.x0 + xbeg) & ~1;
            const size_t fo = (size_t)fr * (size_t)f.frame_stride, yo = fo + yp_yrow + (size_t)xs, cx = prep::yuvp_cx(xs, SUBX, CSTEP);
            const size_t uo = fo + (CSTEP == 2 ? yp_c0 : (size_t)u_off) + yp_crow + cx, vo = fo + (size_t)v_off + yp_crow + cx;
            const uint32_t my = (yp_bm + (uint32_t)yo) & 3u, mu = (yp_bm + (uint32_t)uo) & 3u, mv = (yp_bm + (uint32_t)vo) & 3u;
            if (rows_safe || prep::yuvp_lane_ok(yo, my, uo, mu, vo, mv, CSTEP, CWIN, readable)) {
                load(f, (int64_t)yo - my, prep::YUVP_Y_SPAN, 4, "planar YUV Y window");
                holds(f, (int64_t)yo - my, prep::YUVP_Y_SPAN, yo, yo + 34, "planar YUV Y window misses the lane's pixels");
                load(f, (int64_t)uo - mu, CWIN, 4, CSTEP == 2 ? "planar YUV UV window" : "planar YUV U window");
                holds(f, (int64_t)uo - mu, CWIN, uo, uo + CB, "planar YUV chroma window misses the lane's samples");
                if (CSTEP == 1) {
                    load(f, (int64_t)vo - mv, CWIN, 4, "planar YUV V window");
                    holds(f, (int64_t)vo - mv, CWIN, vo, vo + CB, "planar YUV V window misses the lane's samples");
                }
                if (xs > c.x0 + xbeg || xs + 34 < c.x0 + xbeg + npx) fail(f, "planar YUV window misses pixels", xs, xs + 34);
                return rows_safe ? 0 : 1;
            }
            for (int k = 0; k < npx; ++k) {   // the body's byte loads: the crop's own samples
                const int ci = ((c.x0 + xbeg + k) >> SUBX) * CSTEP;
                load(f, (int64_t)(fo + yp_yrow) + c.x0 + xbeg + k, 1, 1, "planar YUV Y sample");
                load(f, (int64_t)(fo + yp_crow) + u_off + ci, 1, 1, "planar YUV U sample");
                load(f, (int64_t)(fo + yp_crow) + v_off + ci, 1, 1, "planar YUV V sample");
            }
            return 2;
        });
}

// ---- the frames: this program's descriptors, and what the family's check leaves of them ----------------------------------------------------
// d through its check (tight_frames.h), as this program's Frames
template <class D, class Check>
static Frames checked_frames(const Check& check, D& d, int spad, int phase)
{
    melf::FrameBatch b = {};
    const char* const msg = tight_frames(check, d, spad, (size_t)phase, &b);
    if (msg && g_fail++ < 20) fprintf(stderr, "a descriptor of the sweep is not taken: %s (n %d H %d W %d)\n", msg, d.n, d.H, d.W);
    Frames f = {};
    f.n = b.n; f.H = b.H; f.W = b.W; f.phase = phase;
    f.row_stride = b.row_stride; f.frame_stride = (int64_t)b.frame_stride; f.extent = (int64_t)b.lay.extent;
    if (b.lay.pix == melf::PIX_PLANAR) {
        f.off[0] = b.lay.planes.b_off; f.off[1] = b.lay.planes.g_off; f.off[2] = b.lay.planes.r_off;
    } else if (b.lay.pix == melf::PIX_YUVP) {
        f.off[0] = b.lay.yuvp.u_off; f.off[1] = b.lay.yuvp.v_off; f.c_pitch = b.lay.yuvp.c_pitch;
    } else if (melf::pix_yuv(b.lay.pix)) {
        f.off[0] = b.lay.yuv.u_off; f.off[1] = b.lay.yuv.v_off; f.c_pitch = b.lay.yuv.c_pitch;
    }
    return f;
}
static Frames packed_frames(int n, int H, int W, int PB, int pad, int spad, int phase)
{
    melf_frames d = {PB == 4 ? MELF_PIX_BGRA : MELF_PIX_BGR, n, H, W, (int64_t)W * PB + pad, 0};
    return checked_frames(melf::check_frames, d, spad, phase);
}
static Frames p422_frames(int n, int H, int W, int pad, int spad)
{
    melf_yuv422_frames d = {MELF_YUV422_YUYV, MELF_YUV_BT601_LIMITED, n, H, W, 0, (int64_t)W * 2 + pad, 0};
    return checked_frames(melf::check_yuv422, d, spad, 0);
}
// f420: MELF_YUV_NV12 / MELF_YUV_I420 for melf_yuv_frames (NV12: an even u_offset), -1 for melf_yuv_planar_frames.  The caller's side of
// the layout -- the pitches, and the chroma right behind the Y plane's last sample, planar V right behind U's (or the reverse) -- is
// written here; what a frame then spans is the check's.
static Frames yuv_frames(int n, int H, int W, int sub_x, int sub_y, int c_step, int f420, bool vfirst, int pad, int spad, int phase)
{
    const int cw = (W >> sub_x) * c_step, ch = H >> sub_y;
    const int64_t y_pitch = W + pad, c_pitch = cw + pad;
    const int64_t y_end = (int64_t)(H - 1) * y_pitch + W, c_len = (int64_t)(ch - 1) * c_pitch + (c_step == 2 ? cw - 1 : cw);
    const int64_t lo = f420 == MELF_YUV_NV12 ? (y_end + 1) & ~(int64_t)1 : y_end, hi = c_step == 2 ? lo + 1 : lo + c_len;
    const int64_t u_off = vfirst ? hi : lo, v_off = vfirst ? lo : hi;
    if (f420 >= 0) {
        melf_yuv_frames d = {f420, MELF_YUV_BT601_LIMITED, n, H, W, 0, y_pitch, c_pitch, u_off, v_off, 0};
        return checked_frames(melf::check_yuv, d, spad, phase);
    }
    melf_yuv_planar_frames d = {MELF_YUV_BT601_LIMITED, n, H, W, sub_x, sub_y, c_step, 0, y_pitch, c_pitch, u_off, v_off, 0};
    return checked_frames(melf::check_yuv_planar, d, spad, phase);
}
static Frames planar_frames(int n, int H, int W, int order, int pad, int spad, int phase)
{
    static const int orders[3][3] = {{0, 1, 2}, {2, 1, 0}, {1, 2, 0}};
    const int64_t pitch = W + pad, span = (int64_t)(H - 1) * pitch + W;   // the caller's side: the three planes back to back
    melf_planar_frames d = {n, H, W, 0, orders[order][0] * span, orders[order][1] * span, orders[order][2] * span, pitch, 0};
    return checked_frames(melf::check_planes, d, spad, phase);
}

static Arm g_arms[11] = {{"PX 3", 0, 0, 0},          {"PX 4", 0, 0, 0},          {"PX 20 (NV12)", 0, 0, 0},   {"PX 21 (I420)", 0, 0, 0},
                         {"PX 22", 0, 0, 0},         {"PX 23", 0, 0, 0},         {"PX 24 <0, 1>", 0, 0, 0},   {"PX 24 <0, 2>", 0, 0, 0},
                         {"PX 24 <1, 1>", 0, 0, 0},  {"PX 24 <1, 2>", 0, 0, 0},  {nullptr, 0, 0, 0}};

int main()
{
    const int pads_byte[4] = {0, 1, 2, 6}, pads_dword[3] = {0, 4, 8}, nfs[3] = {1, 3, 34};
    long long cases = 0;
    for (int cw = 8; cw <= 96; ++cw)
        for (int xpar = 0; xpar < 2; ++xpar)
            for (int ypar = 0; ypar < 2; ++ypar)
                for (int edge = 0; edge < 2; ++edge)
                    for (int place = 0; place < 2; ++place)
                        for (int pi = 0; pi < 4; ++pi)
                            for (int ni = 0; ni < 3; ++ni)
                              for (int low = 0; low < 2; ++low) {   // low: frames so low that the planes behind Y are shorter than a window
                                Crop c;
                                const int H = low ? 4 : 12, rows0 = low ? 2 : 7;
                                c.cols = cw; c.rows = place ? rows0 + ypar : rows0;
                                c.x0 = place ? 2 + xpar : xpar;
                                const int W = c.x0 + cw + edge, n = nfs[ni];
                                c.y0 = place ? H - c.rows : ypar;   // the crop at the frame's first rows, at its last
                                const int spad_i = (pi + cw) & 3, order = (cw + pi + ni) % 3;
                                const bool vfirst = (cw + pi + xpar) & 1;
                                const int nkb0 = (cw + 31) / 32;
                                for (int dk = 0; dk < 2; ++dk) {   // the planner's block count, and one more
                                    const int nkb = nkb0 + dk;
                                    for (int ph = 0; ph < 4; ++ph) {
                                        ++cases;
                                        packed_case<3>(g_arms[0], packed_frames(n, H, W, 3, pads_byte[pi], pads_byte[spad_i], ph), c, nkb);
                                        planar_case(g_arms[5], planar_frames(n, H, W, order, pads_byte[pi], pads_byte[spad_i], ph), c, nkb);
                                        for (int sub_y = 0; sub_y < 2; ++sub_y) {
                                            yuvp_case<0, 1>(g_arms[6], yuv_frames(n, H, W, 0, sub_y, 1, -1, vfirst, pads_byte[pi], pads_byte[spad_i], ph), c, nkb, sub_y);
                                            yuvp_case<0, 2>(g_arms[7], yuv_frames(n, H, W, 0, sub_y, 2, -1, vfirst, pads_byte[pi], pads_byte[spad_i], ph), c, nkb, sub_y);
                                        }
                                        if (W & 1) continue;   // horizontally subsampled chroma: an even width
                                        yuv420_case<true>(g_arms[2], yuv_frames(n, H, W, 1, 1, 2, MELF_YUV_NV12, false, pads_byte[pi], pads_byte[spad_i], ph), c, nkb);
                                        yuv420_case<false>(g_arms[3], yuv_frames(n, H, W, 1, 1, 1, MELF_YUV_I420, vfirst, pads_byte[pi], pads_byte[spad_i], ph), c, nkb);
                                        for (int sub_y = 0; sub_y < 2; ++sub_y) {
                                            yuvp_case<1, 1>(g_arms[8], yuv_frames(n, H, W, 1, sub_y, 1, -1, vfirst, pads_byte[pi], pads_byte[spad_i], ph), c, nkb, sub_y);
                                            yuvp_case<1, 2>(g_arms[9], yuv_frames(n, H, W, 1, sub_y, 2, -1, vfirst, pads_byte[pi], pads_byte[spad_i], ph), c, nkb, sub_y);
                                        }
                                    }
                                    if (pi < 3) {   // everything 4-byte aligned: phase 0, pads of whole dwords
                                        packed_case<4>(g_arms[1], packed_frames(n, H, W, 4, pads_dword[pi], pads_dword[spad_i % 3], 0), c, nkb);
                                        if (!(W & 1)) p422_case(g_arms[4], p422_frames(n, H, W, pads_dword[pi], pads_dword[spad_i % 3]), c, nkb);
                                    }
                                }
                            }
    printf("cases %lld  loads %lld\n", cases, g_loads);
    for (const Arm* a = g_arms; a->name; ++a) {
        printf("%-14s lanes: row-safe %lld, lane-safe %lld, sample loads %lld\n", a->name, a->row_safe, a->lane_safe, a->samples);
        if (a->row_safe == 0 || a->lane_safe == 0 || a->samples == 0) {
            ++g_fail;
            fprintf(stderr, "%s: a path was never taken: the sweep does not cover it\n", a->name);
        }
    }
    printf("failures %lld (%lld of them loads that start before the base)\n", g_fail, g_before);
    return g_fail ? 1 : 0;
}
