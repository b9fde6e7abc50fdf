// Stand-alone sweep of the address arithmetic of the 16-bit YUV kernels (meterelf_amd/csrc/melf_y16_addr.h: the functions the dial
// source's window fetch and the prep arm compute their loads with), on the CPU: every load of every lane must lie inside
// [base, base + readable) and start on a sample, readable = (n - 1) * frame_stride + extent as check_yuv16 (meterelf_amd/csrc/
// melf_frame_checks.h, the function the entry points call) leaves them for this program's descriptors -- a descriptor it does not
// take is a failure; the aligned dword windows of the prep arm must start on a dword of the address space.  Built and run by
// tests/test_yuv16_frames.py (test_load_bounds_sweep) with the host compiler, plain and under -fsanitize=address,undefined.
//
// Swept: crop origin parities; crop widths 8 .. 72; pitches with 0, 2 and 6 bytes of padding; both c_step; both sub_y; base
// phases 0 and 2; the first, the last and the only frame (and a second frame group for prep); the crop at the frame's first rows
// and at its last; every lane (pc) of every quad count of the window sizes 2 R + 5, R = 3 .. 29, at window origins inside, at and
// across both edges of the crop's columns, at both parities of the match position.
#include <stdio.h>
#include <stdlib.h>

#include "../meterelf_amd/csrc/melf_y16_addr.h"
#include "tight_frames.h"

using namespace melf;

struct Frames {            // what check_yuv16 leaves of a descriptor
    int n, H, W, sub_y, c_step;
    size_t y_pitch, c_pitch, frame_stride, extent;   // extent: of one frame, to the end of its last sample
    int64_t u_off, v_off;
    size_t phase;          // byte phase of the base (0 or 2)
    size_t readable() const { return (size_t)(n - 1) * frame_stride + extent; }
};

static long long g_loads = 0, g_fail = 0;
// The caller's side of the layout -- the pitches, and the planes back to back with no byte between their spans -- is written here;
// the stride is the smallest check_yuv16 takes and `pad` bytes, and what a frame spans is the check's.
static Frames make_frames(int n, int H, int W, int sub_y, int c_step, int pad, bool vfirst, size_t phase)
{
    melf_yuv16_frames d = {};
    d.matrix = MELF_YUV_BT601_LIMITED; d.n = n; d.H = H; d.W = W; d.sub_y = sub_y; d.c_step = c_step; d.shift = 8;
    const int64_t cw = (int64_t)(W >> 1) * c_step * 2, ch = H >> sub_y;
    d.y_pitch = (int64_t)W * 2 + pad;
    d.c_pitch = cw + pad;
    const int64_t y_end = (int64_t)(H - 1) * d.y_pitch + (int64_t)W * 2, c_len = (ch - 1) * d.c_pitch + (c_step == 2 ? cw - 2 : cw);
    const int64_t lo = y_end, hi = c_step == 2 ? y_end + 2 : y_end + c_len;
    d.u_offset = vfirst ? hi : lo;
    d.v_offset = vfirst ? lo : hi;
    FrameBatch b = {};
    const char* const msg = tight_frames(check_yuv16, d, pad, phase, &b);
    if (msg && g_fail++ < 20) fprintf(stderr, "a descriptor of the sweep is not taken: %s (n %d H %d W %d)\n", msg, n, H, W);
    Frames f;
    f.n = b.n; f.H = b.H; f.W = b.W; f.sub_y = b.lay.y16.sub_y; f.c_step = b.lay.y16.c_step; f.phase = phase;
    f.y_pitch = (size_t)b.row_stride; f.c_pitch = (size_t)b.lay.y16.c_pitch; f.frame_stride = b.frame_stride; f.extent = b.lay.extent;
    f.u_off = b.lay.y16.u_off; f.v_off = b.lay.y16.v_off;
    return f;
}

static void load(const Frames& f, size_t off, size_t len, size_t align, const char* what)
{
    ++g_loads;
    const bool inside = off + len <= f.readable();   // (off is unsigned: a start before the base wraps and fails here)
    if (!inside || off > f.readable() || (f.phase + off) % align) {
        if (g_fail++ < 20)
            fprintf(stderr, "%s: load [%zu, %zu) of %zu readable bytes, phase %zu, alignment %zu (n %d H %d W %d sub_y %d c_step %d y_pitch %zu)\n", what, off,
                    off + len, f.readable(), f.phase, align, f.n, f.H, f.W, f.sub_y, f.c_step, f.y_pitch);
    }
}

// ---- the dial window, as DialYuv16::window / request and k_dials_body.inc use the header ----
static long long g_quads = 0, g_exact = 0;
static void dial_case(const Frames& f, int frame, int x0, int y0, int tw, int th, int mx, int my, int wx0, int wy0, int ws)
{
    const size_t fo = (size_t)frame * f.frame_stride;
    const int fx_m = x0 + mx, fy_m = y0 + my, th1 = th - 1;
    const int shift = y16::quad_shift(fx_m, wx0), npiece = y16::quad_count(ws, shift), qx0 = wx0 - shift;
    const size_t c_lo = (size_t)(f.u_off < f.v_off ? f.u_off : f.v_off);
    if (y16::quads_inside(qx0, npiece, tw)) {
        ++g_quads;
        // every window column is a pixel of some lane's quad
        if (4 * npiece - shift < ws || npiece > 16) { ++g_fail; fprintf(stderr, "dial: %d quads do not hold %d columns at shift %d\n", npiece, ws, shift); }
        for (int pc = 0; pc < 16; ++pc) {
            const int fx0 = y16::lane_fx0(fx_m, qx0, npiece, pc);
            if (fx0 & 1) { ++g_fail; fprintf(stderr, "dial: odd first pixel %d\n", fx0); }
            // the four pixels are pixels of the crop's columns under the template
            if (fx0 < fx_m || fx0 + 4 > fx_m + tw) { ++g_fail; fprintf(stderr, "dial: quad at %d leaves the crop columns [%d, %d)\n", fx0, fx_m, fx_m + tw); }
            const int rows[3] = {0, ws / 2, ws - 1};
            for (int k = 0; k < 3; ++k) {
                int Y = wy0 + rows[k];
                Y = Y < 0 ? 0 : (Y > th1 ? th1 : Y);
                const int fy = fy_m + Y;
                load(f, fo + y16::dial_y_off(fy, f.y_pitch, fx0), y16::DIAL_Y_BYTES, 2, "dial Y");
                const size_t co = y16::dial_c_off(fy, f.sub_y, f.c_pitch, fx0, f.c_step);
                if (f.c_step == 1) {
                    load(f, fo + (size_t)f.u_off + co, (size_t)y16::dial_c_bytes(1), 2, "dial U");
                    load(f, fo + (size_t)f.v_off + co, (size_t)y16::dial_c_bytes(1), 2, "dial V");
                    // ... and inside the plane's own row: the two samples of the quad's pairs
                    if (co % f.c_pitch + 4 > (size_t)f.W) { ++g_fail; fprintf(stderr, "dial: chroma load leaves its row\n"); }
                } else {
                    load(f, fo + c_lo + co, (size_t)y16::dial_c_bytes(2), 2, "dial UV");
                    if (co % f.c_pitch + 8 > (size_t)f.W * 2) { ++g_fail; fprintf(stderr, "dial: chroma load leaves its row\n"); }
                }
            }
        }
    } else {
        ++g_exact;
    }
    // the colour core and the exact path: one pixel at clamped template coordinates
    const int xs[3] = {0, tw / 2, tw - 1}, ys[2] = {0, th1};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 2; ++b) {
            const int fx = fx_m + xs[a], fy = fy_m + ys[b];
            load(f, fo + y16::px_y_off(fy, f.y_pitch, fx), 2, 2, "px Y");
            const size_t co = y16::px_c_off(fy, f.sub_y, f.c_pitch, fx, f.c_step);
            load(f, fo + (size_t)f.u_off + co, 2, 2, "px U");
            load(f, fo + (size_t)f.v_off + co, 2, 2, "px V");
        }
}

// ---- the prep arm (PX 25 of prep_lplane_body.inc) ----
static long long g_rows_safe = 0, g_lane_ok = 0, g_lane_samples = 0;
static void prep_case(const Frames& f, int x0, int y0, int rows, int cols, int nkb)
{
    const size_t readable = f.readable();
    const int groups = (f.n + 31) / 32;
    for (int grp = 0; grp < groups; ++grp)
        for (int y = 0; y < rows; ++y) {
            const y16::PrepRow r = y16::prep_row(f.phase, f.frame_stride, f.y_pitch, x0, y0, y, grp, f.n, nkb, f.u_off, f.v_off, f.c_pitch, f.sub_y);
            const bool rows_safe = y16::prep_rows_safe(r, f.c_step, readable);
            for (int n = 0; n < 32; ++n)
                for (int kb = 0; kb < nkb; ++kb) {
                    const int fr = grp * 32 + n;
                    if (!(fr < f.n && kb * 32 < cols)) continue;   // `live`
                    const int xbeg = kb * 32, npx = cols - xbeg < 32 ? cols - xbeg : 32;
                    const int xs = (x0 + xbeg) & ~1;
                    const size_t fo = (size_t)fr * f.frame_stride;
                    const int cb = y16::prep_c_bytes(f.c_step);
                    const size_t yo = y16::prep_y_off(r, fo, xs);
                    const size_t uo = y16::prep_c_off(r, fo, f.c_step == 2 ? r.c0 : (size_t)f.u_off, xs, f.c_step);
                    const size_t vo = y16::prep_c_off(r, fo, (size_t)f.v_off, xs, f.c_step);
                    const uint32_t my = (r.bm + (uint32_t)yo) & 3u, mu = (r.bm + (uint32_t)uo) & 3u, mv = (r.bm + (uint32_t)vo) & 3u;
                    const bool lane_ok = y16::prep_window_ok(yo, my, y16::PREP_Y_BYTES, readable) && y16::prep_window_ok(uo, mu, cb, readable) &&
                                         (f.c_step == 2 || y16::prep_window_ok(vo, mv, cb, readable));
                    if (rows_safe || lane_ok) {
                        if (rows_safe) ++g_rows_safe; else ++g_lane_ok;
                        // aligned dwords from the dword that holds the first sample (load_window, k_match_mfma.hip)
                        load(f, yo - my, (size_t)y16::span(y16::PREP_Y_BYTES), 4, "prep Y window");
                        load(f, uo - mu, (size_t)y16::span(cb), 4, f.c_step == 2 ? "prep UV window" : "prep U window");
                        if (f.c_step == 1) load(f, vo - mv, (size_t)y16::span(cb), 4, "prep V window");
                        // the windows hold the lane's samples: 34 from the even pixel on
                        if (xs > x0 + xbeg || xs + 34 < x0 + xbeg + npx) { ++g_fail; fprintf(stderr, "prep: window at %d misses pixels [%d, %d)\n", xs, x0 + xbeg, x0 + xbeg + npx); }
                    } else {
                        ++g_lane_samples;
                        for (int k = 0; k < npx; ++k) {
                            const int fx = x0 + xbeg + k;
                            const size_t co = y16::px_c_off(y0 + y, f.sub_y, f.c_pitch, fx, f.c_step);
                            load(f, fo + y16::px_y_off(y0 + y, f.y_pitch, fx), 2, 2, "prep Y sample");
                            load(f, fo + (size_t)f.u_off + co, 2, 2, "prep U sample");
                            load(f, fo + (size_t)f.v_off + co, 2, 2, "prep V sample");
                        }
                    }
                }
        }
}

int main()
{
    // the reduction, by hand
    if (y16::reduce(0xffffu, 8) != 255 || y16::reduce(0x8040u, 8) != 0x80 || y16::reduce(1023u, 2) != 255 || y16::reduce(1024u, 2) != 255 ||
        y16::reduce(514u, 2) != 128 || y16::reduce(300u, 0) != 255 || y16::reduce(7u, 0) != 7 || y16::reduce(4095u, 4) != 255) {
        fprintf(stderr, "reduce16 is wrong\n");
        return 1;
    }
    const int pads[3] = {0, 2, 6};
    for (int cw = 8; cw <= 72; ++cw)
        for (int xpar = 0; xpar < 2; ++xpar)
            for (int ypar = 0; ypar < 2; ++ypar)
                for (int pi = 0; pi < 3; ++pi)
                    for (int cstep = 1; cstep <= 2; ++cstep)
                        for (int sub_y = 0; sub_y < 2; ++sub_y)
                            for (int ph = 0; ph < 2; ++ph) {
                                const int th = 6, crop_rows = th + 1;
                                for (int place = 0; place < 2; ++place) {   // the crop at the frame's first rows, at its last
                                    const int x0 = place == 0 ? xpar : 2 + xpar;
                                    const int W = (x0 + cw + 1) & ~1;           // the crop's right edge is the frame's (or a pixel short of it)
                                    const int H = 12;
                                    const int y0 = place == 0 ? ypar : H - crop_rows - ypar;
                                    const bool vfirst = (cw + pi) & 1;
                                    const int nfs[3] = {1, 3, 34};
                                    for (int ni = 0; ni < 3; ++ni) {
                                        const Frames f = make_frames(nfs[ni], H, W, sub_y, cstep, pads[pi], vfirst, ph ? 2 : 0);
                                        // prep: every row of the crop, every live lane; the planner's block count and one more
                                        const int nkb = (cw + 31) / 32;
                                        prep_case(f, x0, y0, crop_rows, cw, nkb);
                                        if (ni == 0) prep_case(f, x0, y0, crop_rows, cw, nkb + 1);
                                        if (ni == 2) continue;   // dials: the first, the last and the only frame
                                        const int tw = cw - 1;
                                        const int frames_at[2] = {0, f.n - 1};
                                        for (int fi = 0; fi < (f.n > 1 ? 2 : 1); ++fi)
                                            for (int R = 3; R <= 29; ++R) {
                                                const int ws = 2 * R + 5;
                                                const int wx0s[6] = {-1, 0, 1, tw - ws - 1, tw - ws, tw - ws + 1};
                                                for (int wi = 0; wi < 6; ++wi)
                                                    for (int mx = 0; mx < 2; ++mx)
                                                        dial_case(f, frames_at[fi], x0, y0, tw, th, mx, (R + wi) & 1, wx0s[wi], wi % 3 - 1, ws);
                                            }
                                    }
                                }
                            }
    printf("loads %lld  dial windows: quads %lld, exact path %lld  prep lanes: row-safe %lld, lane-safe %lld, sample loads %lld  failures %lld\n", g_loads,
           g_quads, g_exact, g_rows_safe, g_lane_ok, g_lane_samples, g_fail);
    if (g_quads == 0 || g_rows_safe == 0 || g_lane_ok == 0 || g_lane_samples == 0) {
        fprintf(stderr, "a path was never taken: the sweep does not cover it\n");
        return 1;
    }
    return g_fail ? 1 : 0;
}
