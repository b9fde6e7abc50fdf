// The address functions the kernels and their launchers share, evaluated at FAR arguments on the CPU: frames, rows and planes that
// lie 2 GiB, 4 GiB and more from the base.  The bounds programs beside this one (prep_bounds, y16_bounds, p10_bounds, p32_bounds,
// stage_runs, plane_runs, orient_runs) run the same headers against heap buffers of exact but small extent; frame_checks_main.cpp
// checks the descriptor checks with 128-bit arithmetic.  Here every function of
//   melf_prep_addr.h  melf_y16_addr.h  melf_p10_addr.h  melf_p32_addr.h  melf_gather_addr.h  melf_orient_addr.h  melf_stage_plan.h
//   melf_jpeg_orient_addr.h (where it takes sizes)
// that forms a byte offset, or decides whether one may be read, is compared with the same formula written in unsigned __int128, at
//   frame index f       0, 15, 16, 31, 32, 1023                     frame_stride  2^27 + 4096, 2^31 - 16, 2^31, 2^32 + 64, 2^36
//   rows                0, 63, 64, 127, 128, 191, 192, last         pitches       tight, 2^25 + 64, INT32_MAX rounded down to the family's alignment
//   plane offsets       tight, 2^32 + 64, 2^33 + 128, 2^40          x0            both parities
//   (grp, nframes)      every pair with nframes 1, 32, 33, 64
// No memory is touched: nothing is allocated at these sizes.  A decision (rows_safe, lane_ok, readable) is evaluated with `readable`
// exactly the 128-bit sum (true) and one byte short of it (false), so an offset that wrapped inside the function flips an answer.
// Under -fsanitize=undefined an int product that overflows ends the run: that is half of the point.
// The comparator is checked first: it must tell a value from the same value truncated to 32 and to 31 bits.
// Prints the evaluations per header and ends with `failures 0`.  Built and run by tests/test_far_addresses.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../meterelf_amd/csrc/melf_gather_addr.h"
#include "../meterelf_amd/csrc/melf_jpeg_orient_addr.h"
#include "../meterelf_amd/csrc/melf_orient_addr.h"
#include "../meterelf_amd/csrc/melf_p10_addr.h"
#include "../meterelf_amd/csrc/melf_p32_addr.h"
#include "../meterelf_amd/csrc/melf_prep_addr.h"
#include "../meterelf_amd/csrc/melf_y16_addr.h"

using namespace melf;
typedef unsigned __int128 u128;

static long failures = 0, evals = 0;
static const char* g_header = "";

// ---- the comparator --------------------------------------------------------------------------------------------------------------
static bool same(uint64_t got, u128 want) { return (u128)got == want; }
static void eq(const char* what, uint64_t got, u128 want)
{
    ++evals;
    if (same(got, want)) return;
    if (failures++ < 20)
        printf("%s: %s: got %llu, the 128-bit formula gives %llu + 2^64 * %llu\n", g_header, what, (unsigned long long)got, (unsigned long long)(uint64_t)want,
               (unsigned long long)(uint64_t)(want >> 64));
}
static void eqb(const char* what, bool got, bool want)
{
    ++evals;
    if (got == want) return;
    if (failures++ < 20) printf("%s: %s: answered %d, the 128-bit formula %d\n", g_header, what, (int)got, (int)want);
}
// a decision `sum <= readable`: call(readable) at readable == sum (true) and sum - 1 (false)
template <class F>
static void decision(const char* what, u128 sum, F call)
{
    if (sum >> 63) { eqb("the test's own sum leaves 63 bits", false, true); return; }
    eqb(what, call((size_t)sum), true);
    eqb(what, call((size_t)sum - 1), false);
}

// ---- what is swept ---------------------------------------------------------------------------------------------------------------
static const int FRAMES[] = {0, 15, 16, 31, 32, 1023};
static const uint64_t STRIDES[] = {(1ull << 27) + 4096, (1ull << 31) - 16, 1ull << 31, (1ull << 32) + 64, 1ull << 36};
static const int H = 252, W = 302, COLS = 250, NKB = 8;   // the far-row frames of tests/test_far_addresses.py; blocks of 32 columns
static const int ROWS[] = {0, 63, 64, 127, 128, 191, 192, H - 1};
static const int64_t FAR_OFFS[] = {-1 /* tight: the caller's own */, (1ll << 32) + 64, (1ll << 33) + 128, 1ll << 40};
static const int X0S[] = {50, 51};
struct Group { int grp, nframes; };
static const Group GROUPS[] = {{0, 1}, {0, 32}, {0, 33}, {1, 33}, {0, 64}, {1, 64}};
static int pitch_of(int k, int tight, int align) { return k == 0 ? tight : (k == 1 ? (1 << 25) + 64 : INT32_MAX / align * align); }
// a plane offset: the tight one, or the far one -- behind the tight one where the planes in front of it reach further than that
static int64_t off_of(int64_t far, int64_t tight) { return far < 0 ? tight : (far >= tight ? far : tight + far); }
static u128 last_of(const Group& g) { return (u128)(g.grp * 32 + 31 < g.nframes - 1 ? g.grp * 32 + 31 : g.nframes - 1); }
static u128 U(int64_t v) { return (u128)(uint64_t)v; }   // every swept quantity is >= 0

static long section(const char* name)
{
    static long before = 0;
    if (*g_header) printf("%-26s %10ld evaluations\n", g_header, evals - before);
    before = evals;
    g_header = name;
    return before;
}

// ---- melf_prep_addr.h ---------------------------------------------------------------------------------------------------------------
static void sweep_prep()
{
    section("melf_prep_addr.h");
    for (const Group& g : GROUPS) eq("last_frame", (uint64_t)prep::last_frame(g.grp, g.nframes), last_of(g));
    for (uint64_t fs : STRIDES)
        for (int row : ROWS)
            for (int pk = 0; pk < 3; ++pk)
                for (int x0 : X0S) {
                    // packed pixels, PX 3 / PX 4; packed 4:2:2
                    for (int px : {3, 4}) {
                        const int pb = prep::packed_pb(px), win = prep::packed_win(px), rs = pitch_of(pk, W * pb, px == 4 ? 4 : 1);
                        for (const Group& g : GROUPS)
                            decision("packed_rows_safe", last_of(g) * fs + U(row) * U(rs) + U(x0 + 32 * (NKB - 1)) * U(pb) + U(win),
                                     [&](size_t rd) { return prep::packed_rows_safe(g.grp, g.nframes, fs, row, rs, x0, NKB, pb, win, rd); });
                        const size_t o = prep::packed_x_off(x0 + 32, pb);
                        eq("packed_x_off", o, U(x0 + 32) * U(pb));
                        for (int f : FRAMES)
                            decision("packed_lane_ok", U(f) * fs + U(row) * U(rs) + o + U(win), [&](size_t rd) { return prep::packed_lane_ok(f, fs, row, rs, o, win, rd); });
                    }
                    {
                        const int rs = pitch_of(pk, 2 * W, 4);
                        for (const Group& g : GROUPS)
                            decision("p422_rows_safe", last_of(g) * fs + U(row) * U(rs) + U((x0 & ~1) + 32 * (NKB - 1)) * 2 + 68,
                                     [&](size_t rd) { return prep::p422_rows_safe(g.grp, g.nframes, fs, row, rs, x0, NKB, rd); });
                        const size_t o = prep::p422_x_off((x0 & ~1) + 32);
                        eq("p422_x_off", o, U((x0 & ~1) + 32) * 2);
                        for (int f : FRAMES)
                            decision("p422_lane_ok", U(f) * fs + U(row) * U(rs) + o + 68, [&](size_t rd) { return prep::p422_lane_ok(f, fs, row, rs, o, rd); });
                    }
                    // planes: 4:2:0 (PX 20 / 21), planar RGB (PX 23), planar YUV (PX 24)
                    const int rs = pitch_of(pk, W, 1);
                    for (int64_t far : FAR_OFFS)
                        for (int cpk = 0; cpk < 3; ++cpk) {
                            for (int nv12 = 0; nv12 < 2; ++nv12) {
                                const int cp = pitch_of(cpk, nv12 ? W : W / 2, 1), xlast = prep::yuv420_xlast(x0, NKB), xs = (x0 & ~1) + 32;
                                const int64_t u_off = off_of(far, (int64_t)H * rs), v_off = nv12 ? u_off + 1 : u_off + (int64_t)(H / 2) * cp;
                                const size_t crow = prep::yuv420_crow(row, cp);
                                eq("yuv420_crow", crow, U(row >> 1) * U(cp));
                                eq("yuv420_xlast", (uint64_t)xlast, U((x0 & ~1) + 32 * (NKB - 1)));
                                for (int f : FRAMES) {
                                    const size_t fo = (size_t)f * fs;
                                    const size_t yo = prep::yuv420_y_off(fo, row, rs, xs), uo = prep::yuv420_c_off(fo, u_off, crow, xs, nv12 != 0),
                                                 vo = prep::yuv420_c_off(fo, v_off, crow, xs, nv12 != 0);
                                    eq("yuv420_y_off", yo, U(f) * fs + U(row) * U(rs) + U(xs));
                                    eq("yuv420_c_off", uo, U(f) * fs + U(u_off) + U(row >> 1) * U(cp) + U(nv12 ? xs : xs >> 1));
                                    eq("yuv420_c_off", vo, U(f) * fs + U(v_off) + U(row >> 1) * U(cp) + U(nv12 ? xs : xs >> 1));
                                    // the last window of the three ends the buffer: V's (I420), the interleaved plane's (NV12)
                                    decision("yuv420_lane_ok", (u128)(nv12 ? uo + 40 : vo + 24), [&](size_t rd) { return prep::yuv420_lane_ok(yo, uo, vo, nv12 != 0, rd); });
                                    decision("yuv420_rows_safe", U(f) * fs + U(v_off) + U(row >> 1) * U(cp) + U(nv12 ? xlast : xlast >> 1) + 40,
                                             [&](size_t rd) { return prep::yuv420_rows_safe(fo, row, rs, xlast, u_off, v_off, crow, nv12 != 0, rd); });
                                }
                            }
                            for (int subx = 0; subx < 2; ++subx)
                                for (int cstep = 1; cstep <= 2; ++cstep) {
                                    const int cp = pitch_of(cpk, (W >> subx) * cstep, 1), cwin = prep::yuvp_cwin(subx, cstep), xs = (x0 & ~1) + 32;
                                    const int64_t c0 = off_of(far, (int64_t)H * rs), c1 = cstep == 2 ? c0 + 1 : c0 + (int64_t)H * cp;
                                    eq("yuvp_cx", prep::yuvp_cx(xs, subx, cstep), U((xs >> subx) * cstep));
                                    for (const Group& g : GROUPS) {
                                        const size_t first = (size_t)g.grp * 32 * fs, last = (size_t)last_of(g) * fs, yrow = (size_t)row * rs, crow = (size_t)row * cp;
                                        const int x0e = x0 & ~1, xlast = x0e + 32 * (NKB - 1);
                                        decision("yuvp_rows_safe", last_of(g) * fs + U(cstep == 2 ? c0 : c1) + U(row) * U(cp) + U((xlast >> subx) * cstep) + U(cwin),
                                                 [&](size_t rd) { return prep::yuvp_rows_safe(0, first, last, yrow, crow, (size_t)c0, (size_t)c1, x0e, xlast, subx, cstep, cwin, rd); });
                                    }
                                }
                        }
                    for (int64_t far : FAR_OFFS) {
                        const int64_t span = (int64_t)(H - 1) * rs + W, g_off = off_of(far, span), r_off = 2 * g_off;
                        eq("planar_row", prep::planar_row(row, rs, x0), U(row) * U(rs) + U(x0));
                        for (const Group& g : GROUPS)
                            decision("planar_rows_safe", last_of(g) * fs + U(r_off) + U(row) * U(rs) + U(x0) + U(32 * (NKB - 1)) + 36,
                                     [&](size_t rd) { return prep::planar_rows_safe(0, g.grp, g.nframes, fs, 0, (size_t)r_off, prep::planar_row(row, rs, x0), NKB, rd); });
                        for (int f : FRAMES) {
                            const size_t lane = prep::planar_lane_off(f, fs, row, rs, x0 + 32);
                            eq("planar_lane_off", lane, U(f) * fs + U(row) * U(rs) + U(x0 + 32));
                            const size_t ob = lane, og = lane + (size_t)g_off, orr = lane + (size_t)r_off;
                            decision("planar_lane_ok", U(f) * fs + U(r_off) + U(row) * U(rs) + U(x0 + 32) - (orr & 3) + 36,
                                     [&](size_t rd) { return prep::planar_lane_ok(ob, (uint32_t)(ob & 3), og, (uint32_t)(og & 3), orr, (uint32_t)(orr & 3), rd); });
                        }
                    }
                }
    eq("prep_window_readable", prep::prep_window_readable(prep::ARM_PX3, 1, 0, 0, (size_t)1 << 40), 0);
    eq("prep_window_readable", prep::prep_window_readable(prep::ARM_PX3, 1, 0, 1, (size_t)1 << 40), (u128)1 << 40);
}

// ---- melf_y16_addr.h ----------------------------------------------------------------------------------------------------------------
static void sweep_y16()
{
    section("melf_y16_addr.h");
    for (int row : ROWS)
        for (int pk = 0; pk < 3; ++pk)
            for (int cpk = 0; cpk < 3; ++cpk)
                for (int x0 : X0S)
                    for (int cstep = 1; cstep <= 2; ++cstep)
                        for (int sub_y = 0; sub_y < 2; ++sub_y) {
                            const int yp = pitch_of(pk, 2 * W, 2), cp = pitch_of(cpk, (W / 2) * cstep * 2, 2);
                            const u128 y_want = U(row) * U(yp) + U(x0) * 2, c_want = U(row >> sub_y) * U(cp) + U(x0 >> 1) * 2 * U(cstep);
                            eq("dial_y_off", y16::dial_y_off(row, (size_t)yp, x0), y_want);
                            eq("px_y_off", y16::px_y_off(row, (size_t)yp, x0), y_want);
                            eq("dial_c_off", y16::dial_c_off(row, sub_y, (size_t)cp, x0, cstep), c_want);
                            eq("px_c_off", y16::px_c_off(row, sub_y, (size_t)cp, x0, cstep), c_want);
                            for (uint64_t fs : STRIDES)
                                for (int64_t far : FAR_OFFS)
                                    for (const Group& g : GROUPS) {
                                        const int64_t u_off = off_of(far, (int64_t)H * yp), v_off = cstep == 2 ? u_off + 2 : u_off + (int64_t)H * cp;
                                        const y16::PrepRow r = y16::prep_row(0, fs, (size_t)yp, x0, 0, row, g.grp, g.nframes, NKB, v_off, u_off, (size_t)cp, sub_y);
                                        const u128 crow = U(row >> sub_y) * U(cp);
                                        eq("PrepRow.first", r.first, U(g.grp * 32) * fs);
                                        eq("PrepRow.last", r.last, last_of(g) * fs);
                                        eq("PrepRow.yrow", r.yrow, U(row) * U(yp));
                                        eq("PrepRow.crow", r.crow, crow);
                                        eq("PrepRow.c0", r.c0, U(u_off));
                                        eq("PrepRow.c1", r.c1, U(v_off));
                                        const int xs = r.x0e + 32;
                                        eq("prep_y_off", y16::prep_y_off(r, r.last, xs), last_of(g) * fs + U(row) * U(yp) + U(xs) * 2);
                                        const size_t co = y16::prep_c_off(r, r.last, r.c1, xs, cstep);
                                        eq("prep_c_off", co, last_of(g) * fs + U(v_off) + crow + U(xs >> 1) * 2 * U(cstep));
                                        decision("prep_rows_safe",
                                                 last_of(g) * fs + U(cstep == 2 ? u_off : v_off) + crow + U(r.xlast >> 1) * 2 * U(cstep) + U(y16::span(y16::prep_c_bytes(cstep))),
                                                 [&](size_t rd) { return y16::prep_rows_safe(r, cstep, rd); });
                                        decision("prep_window_ok", (u128)co + U(y16::span(34)), [&](size_t rd) { return y16::prep_window_ok(co, 0, 34, rd); });
                                    }
                        }
}

// ---- melf_p10_addr.h, melf_p32_addr.h -------------------------------------------------------------------------------------------------
static void sweep_p10_p32()
{
    section("melf_p10_addr.h");
    for (int row : ROWS)
        for (int pk = 0; pk < 3; ++pk)
            for (int x = X0S[0]; x < X0S[0] + 14; ++x) {   // every phase of a group, both parities
                const int vp = pitch_of(pk, (int)p10::v210_row_bytes(W), 16), yp = pitch_of(pk, 4 * W, 8), xe = x & ~1;
                eq("v210_px_off", p10::v210_px_off(row, (size_t)vp, x), U(row) * U(vp) + U(x / 6) * 16 + U(x % 6 / 2) * 4);
                eq("y210_px_off", p10::y210_px_off(row, (size_t)yp, x), U(row) * U(yp) + U(x >> 1) * 8);
                eq("v210_dial_off", p10::v210_dial_off(row, (size_t)vp, xe), U(row) * U(vp) + U(xe / 6) * 16 + (xe % 6 == 4 ? 8u : 0u));
                eq("y210_dial_off", p10::y210_dial_off(row, (size_t)yp, xe), U(row) * U(yp) + U(xe) * 4);
                for (uint64_t fs : STRIDES) {
                    for (int f : FRAMES) {
                        eq("v210_prep_off", p10::v210_prep_off((size_t)f * fs, row, (size_t)vp, xe), U(f) * fs + U(row) * U(vp) + U(xe / 6) * 16);
                        const size_t o = p10::y210_prep_off((size_t)f * fs, row, (size_t)yp, xe);
                        eq("y210_prep_off", o, U(f) * fs + U(row) * U(yp) + U(xe) * 4);
                        decision("y210_lane_ok", (u128)o + 136, [&](size_t rd) { return p10::y210_lane_ok(o, rd); });
                    }
                    for (const Group& g : GROUPS)
                        decision("y210_rows_safe", last_of(g) * fs + U(row) * U(yp) + U(xe + 32 * (NKB - 1)) * 4 + 136,
                                 [&](size_t rd) { return p10::y210_rows_safe(g.grp, g.nframes, fs, row, (size_t)yp, x, NKB, rd); });
                }
            }
    section("melf_p32_addr.h");
    for (int row : ROWS)
        for (int pk = 0; pk < 3; ++pk)
            for (int x0 : X0S) {
                const int rp = pitch_of(pk, 4 * W, 4);
                eq("px_off", p32::px_off(row, (size_t)rp, x0 + COLS - 1), U(row) * U(rp) + U(x0 + COLS - 1) * 4);
                eq("dial_off", p32::dial_off(row, (size_t)rp, x0), U(row) * U(rp) + U(x0) * 4);
            }
}

// ---- melf_stage_plan.h (the RowRuns of every family's plan) and melf_gather_addr.h ----------------------------------------------------
static const int PH = 512;   // frames of the plans: the crop's first row goes through ROWS_P
static const int ROWS_P[] = {0, 63, 64, 127, 128, 191, 192, PH - 12};
struct WantRun { u128 src_off; uint64_t pitch, row_bytes; uint32_t rows; };

static void check_plan(const char* name, const char* msg, const FrameBatch& b, const int* rect, int nruns, const WantRun* want)
{
    if (msg) { printf("%s: the descriptor is not taken: %s\n", name, msg); ++failures; return; }
    Crop cr;
    if (!clamp_crop(rect, b.H, b.W, &cr)) { printf("%s: bad crop\n", name); ++failures; return; }
    const StagePlan sp = stage_plan(b, cr);
    eq(name, (uint64_t)sp.runs.count, U(nruns));
    for (int k = 0; k < nruns && k < sp.runs.count; ++k) {
        const RowRun& r = sp.runs.run[k];
        eq(name, r.src_off, want[k].src_off);
        eq(name, r.src_pitch, want[k].pitch);
        eq(name, r.row_bytes, want[k].row_bytes);
        eq(name, r.rows, want[k].rows);
        // k_gather_rows: the pieces of the run's first and last row
        const uint32_t pieces = gather::row_pieces(r.row_bytes);
        for (uint32_t row : {0u, r.rows - 1})
            for (uint32_t piece : {0u, pieces - 1}) {
                const gather::Piece p = gather::piece_of(r, row, piece);
                const u128 src = want[k].src_off + U(row) * want[k].pitch + U(piece) * 16;
                eq("piece_of.src_off", p.src_off, src);
                eq("piece_of.dst_off", p.dst_off, U((int64_t)r.dst_off) + U(row) * r.dst_pitch + U(piece) * 16);
                const uint64_t bytes = p.bytes;
                ++evals;
                if (bytes == 0 || bytes > 16) { printf("%s: a piece of %llu bytes\n", name, (unsigned long long)bytes); ++failures; continue; }
                eqb("piece_readable", gather::piece_readable(p, (uint64_t)(src + bytes)), true);
                eqb("piece_readable", gather::piece_readable(p, (uint64_t)(src + bytes) - 1), false);
            }
    }
    // wave_rows / plane_rows: the run a wave takes keeps its 64-bit offsets; plane_rows takes them from the split
    PlaneSplit ps = {};
    ps.count = sp.runs.count;
    for (int k = 0; k < sp.runs.count; ++k) { ps.src_off[k] = (uint64_t)FAR_OFFS[1 + k]; ps.extent[k] = (1ull << 41) + (uint64_t)k; }
    const uint32_t waves = gather::frame_waves(sp.runs);
    uint32_t w0 = 0;
    for (int k = 0; k < sp.runs.count; ++k) {
        for (uint32_t w : {w0, w0 + gather::run_waves(sp.runs.run[k]) - 1}) {
            if (w >= waves) { printf("%s: wave %u of %u\n", name, w, waves); ++failures; continue; }
            const gather::WaveRows wr = gather::wave_rows(sp.runs, w);
            eq("wave_rows.src_off", wr.run.src_off, want[k].src_off);
            eq("wave_rows.src_pitch", wr.run.src_pitch, want[k].pitch);
            const gather::PlaneRows pr = gather::plane_rows(sp.runs, ps, w);
            eq("plane_rows.k", pr.k, U(k));
            eq("plane_rows.src_off", pr.wr.run.src_off, U(FAR_OFFS[1 + k]));
            eq("plane_rows.extent", pr.extent, ((u128)1 << 41) + U(k));
            eq("plane_rows.row0", pr.wr.row0, U((int64_t)(w - w0)) * 8);
        }
        w0 += gather::run_waves(sp.runs.run[k]);
    }
}

static void sweep_plans()
{
    section("melf_stage_plan.h + gather");
    const void* const base = (const void*)(uintptr_t)64;
    for (int y0 : ROWS_P)
        for (int pk = 0; pk < 3; ++pk)
            for (int x0 : X0S) {
                const int rect[4] = {x0, y0, x0 + COLS, y0 + COLS};
                const uint32_t rows = (uint32_t)((y0 + COLS < PH ? y0 + COLS : PH) - y0);
                FrameBatch b;
                for (int pix = MELF_PIX_BGR; pix <= MELF_PIX_RGBA; ++pix) {
                    const int bpp = pix_bytes(pix), rp = pitch_of(pk, W * bpp, bpp == 4 ? 4 : 1);
                    melf_frames d = {};
                    d.pixel_format = pix; d.n = 1; d.H = PH; d.W = W; d.row_pitch = rp; d.frame_stride = (int64_t)PH * rp;
                    const WantRun want = {U(y0) * U(rp) + U(x0) * U(bpp), (uint64_t)rp, (uint64_t)(COLS * bpp), rows};
                    check_plan("packed_plan", check_frames(base, &d, &b), b, rect, 1, &want);
                }
                {
                    const int rp = pitch_of(pk, 2 * W, 4), ex0 = x0 & ~1, ex1 = (x0 + COLS + 1) & ~1;
                    melf_yuv422_frames d = {};
                    d.format = MELF_YUV422_UYVY; d.n = 1; d.H = PH; d.W = W; d.row_pitch = rp; d.frame_stride = (int64_t)PH * rp;
                    const WantRun want = {U(y0) * U(rp) + U(ex0) * 2, (uint64_t)rp, (uint64_t)((ex1 - ex0) * 2), rows};
                    check_plan("p422_plan", check_yuv422(base, &d, &b), b, rect, 1, &want);
                }
                for (int fmt : {MELF_YUV422_10_V210, MELF_YUV422_10_Y210}) {
                    const bool v210 = fmt == MELF_YUV422_10_V210;
                    const int unit = v210 ? 6 : 2, ub = v210 ? 16 : 8, rp = pitch_of(pk, v210 ? (int)p10::v210_row_bytes(W) : 4 * W, ub);
                    const int ex0 = x0 / unit * unit, ex1 = (x0 + COLS + unit - 1) / unit * unit;
                    melf_yuv422_10_frames d = {};
                    d.format = fmt; d.matrix = MELF_YUV_BT709_LIMITED; d.n = 1; d.H = PH; d.W = W; d.row_pitch = rp; d.frame_stride = (int64_t)PH * rp;
                    const WantRun want = {U(y0) * U(rp) + U(ex0 / unit) * U(ub), (uint64_t)rp, (uint64_t)((ex1 - ex0) / unit * ub), rows};
                    check_plan("yuv422_10_plan", check_yuv422_10(base, &d, &b), b, rect, 1, &want);
                }
                {
                    const int rp = pitch_of(pk, 4 * W, 4);
                    melf_packed32_frames d = {};
                    d.colour = MELF_P32_YUV; d.n = 1; d.H = PH; d.W = W; d.pos[0] = 12; d.pos[1] = 2; d.pos[2] = 22; d.row_pitch = rp; d.frame_stride = (int64_t)PH * rp;
                    const WantRun want = {U(y0) * U(rp) + U(x0) * 4, (uint64_t)rp, (uint64_t)(COLS * 4), rows};
                    check_plan("packed32_plan", check_packed32(base, &d, &b), b, rect, 1, &want);
                }
                for (int64_t far : FAR_OFFS)
                    for (int cpk = 0; cpk < 3; ++cpk) {
                        {   // planar RGB: the far planes
                            const int rp = pitch_of(pk, W, 1);
                            const int64_t span = (int64_t)(PH - 1) * rp + W, g = off_of(far, span), r = 2 * g;
                            if (cpk == 0) {
                                melf_planar_frames d = {};
                                d.n = 1; d.H = PH; d.W = W; d.b_offset = 0; d.g_offset = g; d.r_offset = r; d.row_pitch = rp; d.frame_stride = r + span;
                                const u128 in_plane = U(y0) * U(rp) + U(x0);
                                const WantRun want[3] = {{in_plane, (uint64_t)rp, (uint64_t)COLS, rows}, {U(g) + in_plane, (uint64_t)rp, (uint64_t)COLS, rows},
                                                         {U(r) + in_plane, (uint64_t)rp, (uint64_t)COLS, rows}};
                                check_plan("planar_plan", check_planes(base, &d, &b), b, rect, 3, want);
                            }
                        }
                        for (int nv12 = 0; nv12 < 2; ++nv12) {   // melf_yuv_frames
                            const int yp = pitch_of(pk, W, 1), cp = pitch_of(cpk, nv12 ? W : W / 2, 1);
                            const int64_t u = off_of(far, (int64_t)PH * yp), v = nv12 ? u + 1 : u + (int64_t)(PH / 2) * cp;
                            melf_yuv_frames d = {};
                            d.format = nv12 ? MELF_YUV_NV12 : MELF_YUV_I420; d.n = 1; d.H = PH; d.W = W; d.y_pitch = yp; d.c_pitch = cp; d.u_offset = u; d.v_offset = v;
                            d.frame_stride = v + (int64_t)(PH / 2) * cp;
                            const int ex0 = x0 & ~1, ey0 = y0 & ~1, sw = ((x0 + COLS + 1) & ~1) - ex0, sh = (int)(((y0 + rows + 1) & ~1u)) - ey0;
                            const u128 c = U(ey0 >> 1) * U(cp) + U(ex0 >> 1) * (nv12 ? 2 : 1);
                            const uint64_t cb = (uint64_t)((sw >> 1) * (nv12 ? 2 : 1));
                            const WantRun want[3] = {{U(ey0) * U(yp) + U(ex0), (uint64_t)yp, (uint64_t)sw, (uint32_t)sh}, {U(u) + c, (uint64_t)cp, cb, (uint32_t)(sh >> 1)},
                                                     {U(v) + c, (uint64_t)cp, cb, (uint32_t)(sh >> 1)}};
                            check_plan("yuv420_plan", check_yuv(base, &d, &b), b, rect, nv12 ? 2 : 3, want);
                        }
                        for (int form = 0; form < 8; ++form) {   // melf_yuv_planar_frames: sub_x, sub_y, c_step
                            const int sx = form & 1, sy = (form >> 1) & 1, step = 1 + (form >> 2);
                            const int yp = pitch_of(pk, W, 1), cp = pitch_of(cpk, (W >> sx) * step, 1), ch = PH >> sy;
                            const int64_t lo = off_of(far, (int64_t)PH * yp), hi = step == 2 ? lo + 1 : lo + (int64_t)ch * cp;
                            melf_yuv_planar_frames d = {};
                            d.n = 1; d.H = PH; d.W = W; d.sub_x = sx; d.sub_y = sy; d.c_step = step; d.y_pitch = yp; d.c_pitch = cp; d.u_offset = hi; d.v_offset = lo;   // V first
                            d.frame_stride = hi + (int64_t)ch * cp;
                            const int bx = 1 << sx, by = 1 << sy, ex0 = x0 & ~(bx - 1), ey0 = y0 & ~(by - 1);
                            const int sw = ((x0 + COLS + bx - 1) & ~(bx - 1)) - ex0, sh = (((int)(y0 + rows) + by - 1) & ~(by - 1)) - ey0;
                            const u128 c = U(ey0 >> sy) * U(cp) + U(ex0 >> sx) * U(step);
                            const uint64_t cb = (uint64_t)((sw >> sx) * step);
                            const WantRun semi[2] = {{U(ey0) * U(yp) + U(ex0), (uint64_t)yp, (uint64_t)sw, (uint32_t)sh}, {U(lo) + c, (uint64_t)cp, cb, (uint32_t)(sh >> sy)}};
                            const WantRun planar[3] = {semi[0], {U(hi) + c, (uint64_t)cp, cb, (uint32_t)(sh >> sy)}, {U(lo) + c, (uint64_t)cp, cb, (uint32_t)(sh >> sy)}};
                            check_plan("yuv_planar_plan", check_yuv_planar(base, &d, &b), b, rect, step == 2 ? 2 : 3, step == 2 ? semi : planar);
                        }
                        for (int form = 0; form < 4; ++form) {   // melf_yuv16_frames: sub_y, c_step
                            const int sy = form & 1, step = 1 + (form >> 1);
                            const int yp = pitch_of(pk, 2 * W, 2), cp = pitch_of(cpk, (W >> 1) * step * 2, 2), ch = PH >> sy;
                            const int64_t u = off_of(far, (int64_t)PH * yp), v = step == 2 ? u + 2 : u + (int64_t)ch * cp;
                            melf_yuv16_frames d = {};
                            d.matrix = MELF_YUV_BT709_LIMITED; d.n = 1; d.H = PH; d.W = W; d.sub_y = sy; d.c_step = step; d.shift = 8; d.y_pitch = yp; d.c_pitch = cp;
                            d.u_offset = u; d.v_offset = v; d.frame_stride = v + (int64_t)ch * cp;
                            const int by = 1 << sy, ex0 = x0 & ~1, ey0 = y0 & ~(by - 1);
                            const int sw = ((x0 + COLS + 1) & ~1) - ex0, sh = (((int)(y0 + rows) + by - 1) & ~(by - 1)) - ey0;
                            const u128 c = U(ey0 >> sy) * U(cp) + U(ex0 >> 1) * U(step) * 2;
                            const uint64_t cb = (uint64_t)((sw >> 1) * step * 2);
                            const WantRun want[3] = {{U(ey0) * U(yp) + U(ex0) * 2, (uint64_t)yp, (uint64_t)(2 * sw), (uint32_t)sh}, {U(u) + c, (uint64_t)cp, cb, (uint32_t)(sh >> sy)},
                                                     {U(v) + c, (uint64_t)cp, cb, (uint32_t)(sh >> sy)}};
                            check_plan("yuv16_plan", check_yuv16(base, &d, &b), b, rect, step == 2 ? 2 : 3, want);
                        }
                    }
            }
}

// ---- melf_orient_addr.h ---------------------------------------------------------------------------------------------------------------
static void sweep_orient()
{
    section("melf_orient_addr.h");
    const uint32_t ph = PH, pw = 480, n = COLS;
    for (int code = MELF_ORIENT_NORMAL; code <= MELF_ORIENT_ROT90CCW; ++code)
        for (int64_t far : FAR_OFFS)
            for (int pk = 0; pk < 3; ++pk)
                for (uint32_t eb = 1; eb <= 4; ++eb)
                    for (uint32_t o0 : {50u, 51u}) {
                        const bool tr = orient::transposes(code), fr = orient::flips_rows(code), fc = orient::flips_cols(code);
                        const uint32_t pitch = (uint32_t)pitch_of(pk, (int)(pw * eb), eb == 3 ? 1 : (int)eb);
                        const orient::Plane pl = orient::plane_of((uint64_t)off_of(far, 0), pitch, (int)ph, (int)pw, (int)eb, code, 0);
                        eq("plane_of.off", pl.off, U(off_of(far, 0)));
                        eq("plane_of.pitch", pl.pitch, U(pitch));
                        eq("plane_of.o_pitch", pl.o_pitch, U((tr ? ph : pw) * eb));
                        orient::Runs rr = {};
                        rr.count = 1; rr.code = code;
                        orient::Run& r = rr.run[0];
                        r.src_off = pl.off; r.dst_off = 0; r.src_pitch = pl.pitch; r.dst_pitch = (n * eb + 63) & ~63u;
                        r.rows = n; r.cols = n; r.oy0 = o0; r.ox0 = o0 + 2; r.ph = ph; r.pw = pw; r.eb = eb;
                        // the stored (row, col) of element (y, x) of the oriented plane: the public header's table
                        auto stored = [&](uint32_t y, uint32_t x, u128* row, u128* col) {
                            const uint32_t oy = r.oy0 + y, ox = r.ox0 + x, a = tr ? ox : oy, b = tr ? oy : ox;
                            *row = fr ? ph - 1 - a : a;
                            *col = fc ? pw - 1 - b : b;
                        };
                        for (uint32_t y : {0u, n - 1})
                            for (uint32_t x : {0u, n - 1}) {
                                u128 row, col;
                                stored(y, x, &row, &col);
                                eq("elem_src_off", orient::elem_src_off(r, code, y, x), U(off_of(far, 0)) + row * pitch + col * eb);
                            }
                        const uint32_t tiles = orient::frame_tiles(rr);
                        for (uint32_t t : {0u, tiles - 1}) {
                            const orient::Tile tl = orient::tile_of(rr, t);
                            eq("tile_of.src_off", tl.run.src_off, U(off_of(far, 0)));
                            eq("tile_of.src_pitch", tl.run.src_pitch, U(pitch));
                            // the tile's source rectangle starts at the smallest stored row and column of its four corners
                            u128 row0 = ~(u128)0, col0 = ~(u128)0;
                            for (uint32_t y : {tl.r0, tl.r0 + tl.nr - 1})
                                for (uint32_t x : {tl.c0, tl.c0 + tl.nc - 1}) {
                                    u128 row, col;
                                    stored(y, x, &row, &col);
                                    row0 = row < row0 ? row : row0;
                                    col0 = col < col0 ? col : col0;
                                }
                            const uint32_t lp = orient::load_pieces(tl), sp = orient::store_pieces(tl);
                            for (uint32_t s : {0u, tl.srows - 1})
                                for (uint32_t piece : {0u, lp - 1}) {
                                    const orient::Load l = orient::load_of(tl, s, piece);
                                    const u128 src = U(off_of(far, 0)) + (row0 + s) * pitch + col0 * eb + U(piece) * 16;
                                    eq("load_of.src_off", l.src_off, src);
                                    eqb("load_readable", orient::load_readable(l, (uint64_t)(src + l.bytes)), true);
                                    eqb("load_readable", orient::load_readable(l, (uint64_t)(src + l.bytes) - 1), false);
                                }
                            for (uint32_t row : {0u, tl.nr - 1})
                                for (uint32_t piece : {0u, sp - 1})
                                    eq("store_of.dst_off", orient::store_of(tl, row, piece).dst_off, U(tl.r0 + row) * r.dst_pitch + U(tl.c0) * eb + U(piece) * 16);
                        }
                    }
    // oriented_plan of far stored batches: the runs' source side is the stored planes' own offsets and pitches
    const void* const base = (const void*)(uintptr_t)64;
    for (int code = MELF_ORIENT_NORMAL; code <= MELF_ORIENT_ROT90CCW; ++code)
        for (int64_t far : FAR_OFFS)
            for (int pk = 0; pk < 3; ++pk) {
                const int rp = pitch_of(pk, W, 1);
                const int64_t span = (int64_t)(PH - 1) * rp + W, g = off_of(far, span);
                melf_planar_frames d = {};
                d.n = 1; d.H = PH; d.W = W; d.b_offset = 2 * g; d.g_offset = g; d.r_offset = 0; d.row_pitch = rp; d.frame_stride = 2 * g + span;
                FrameBatch b;
                if (check_planes(base, &d, &b) || orient::orientable(b, code)) { printf("oriented_plan: the planar batch is not taken\n"); ++failures; continue; }
                const int H2 = orient::oriented_h(b, code), W2 = orient::oriented_w(b, code);
                const int rect[4] = {20, 10, 20 + COLS, 10 + COLS};
                Crop cr;
                if (!clamp_crop(rect, H2, W2, &cr)) { printf("oriented_plan: bad crop\n"); ++failures; continue; }
                const orient::Plan p = orient::oriented_plan(b, code, cr);
                eq("oriented_plan.count", (uint64_t)p.runs.count, 3);
                eq("oriented_plan.extent", p.runs.extent, U(2 * g + span));
                const int64_t offs[3] = {2 * g, g, 0};
                for (int k = 0; k < 3 && k < p.runs.count; ++k) {
                    eq("oriented_plan.src_off", p.runs.run[k].src_off, U(offs[k]));
                    eq("oriented_plan.src_pitch", p.runs.run[k].src_pitch, U(rp));
                    eq("oriented_plan.oy0", p.runs.run[k].oy0, U(cr.y0));
                    eq("oriented_plan.ox0", p.runs.run[k].ox0, U(cr.x0));
                }
            }
}

// ---- melf_jpeg_orient_addr.h: the functions that take the frame's size ------------------------------------------------------------------
static void sweep_jpeg_orient()
{
    section("melf_jpeg_orient_addr.h");
    typedef __int128 i128;
    for (int code = 1; code <= 8; ++code)
        for (int Hs : {16, 4096, 65535})
            for (int Ws : {16, 4100, 65535}) {
                const bool t = jpeg_orient::transposed(code), fx = jpeg_orient::flips_x(code), fy = jpeg_orient::flips_y(code);
                const int Hu = jpeg_orient::swapped_h(code, Hs, Ws), Wu = jpeg_orient::swapped_w(code, Hs, Ws);
                eq("swapped_h", (uint64_t)Hu, U(t ? Ws : Hs));
                eq("swapped_w", (uint64_t)Wu, U(t ? Hs : Ws));
                for (int corner = 0; corner < 4; ++corner) {
                    const int x0 = corner & 1 ? Wu - 9 : 0, y0 = corner & 2 ? Hu - 7 : 0, rect[4] = {x0, y0, x0 + 9, y0 + 7};
                    const i128 u0 = t ? rect[1] : rect[0], u1 = t ? rect[3] : rect[2], v0 = t ? rect[0] : rect[1], v1 = t ? rect[2] : rect[3];
                    const i128 sx0 = fx ? Ws - u1 : u0, sx1 = fx ? Ws - u0 : u1, sy0 = fy ? Hs - v1 : v0, sy1 = fy ? Hs - v0 : v1;
                    const jpeg_orient::Window r = jpeg_orient::stored_rect(rect, code, Hs, Ws);
                    eq("stored_rect.x0", (uint64_t)r.x0, (u128)sx0); eq("stored_rect.x1", (uint64_t)r.x1, (u128)sx1);
                    eq("stored_rect.y0", (uint64_t)r.y0, (u128)sy0); eq("stored_rect.y1", (uint64_t)r.y1, (u128)sy1);
                    const jpeg_orient::Window w = jpeg_orient::window(rect, code, Hs, Ws);
                    auto lo = [](i128 v) { v = (v - 16) / 16 * 16; return v < 0 ? (i128)0 : v; };
                    auto hi = [](i128 v, i128 lim) { v = (v + 31) / 16 * 16; return v > lim ? lim : v; };
                    eq("window.x0", (uint64_t)w.x0, (u128)(sx0 < 16 ? 0 : lo(sx0))); eq("window.x1", (uint64_t)w.x1, (u128)hi(sx1, Ws));
                    eq("window.y0", (uint64_t)w.y0, (u128)(sy0 < 16 ? 0 : lo(sy0))); eq("window.y1", (uint64_t)w.y1, (u128)hi(sy1, Hs));
                    // a stored pixel of the rectangle lands inside the upright rectangle
                    int x, y;
                    jpeg_orient::upright_of(code, Hs, Ws, r.x0, r.y0, &x, &y);
                    const i128 u = fx ? Ws - 1 - sx0 : sx0, v = fy ? Hs - 1 - sy0 : sy0;
                    eq("upright_of.x", (uint64_t)x, (u128)(t ? v : u));
                    eq("upright_of.y", (uint64_t)y, (u128)(t ? u : v));
                    eqb("upright_of inside", x >= rect[0] && x < rect[2] && y >= rect[1] && y < rect[3], true);
                }
            }
}

int main()
{
    // the comparator tells a far offset from its 32-bit and its 31-bit truncation (and takes the offset itself)
    const u128 far = (u128)32 * STRIDES[0] + (u128)191 * ((1u << 25) + 64) + 906;
    const uint64_t t32 = (uint64_t)far & 0xffffffffull, t31 = (uint64_t)far & 0x7fffffffull;
    if (same(t32, far) || same(t31, far) || !same((uint64_t)far, far) || same((uint64_t)(far + ((u128)1 << 64)), far + ((u128)1 << 64))) {
        printf("the comparator does not tell a truncated offset from the offset\nfailures 1\n");
        return 1;
    }
    printf("comparator: 32-bit and 31-bit truncations of %llu are mismatches\n", (unsigned long long)(uint64_t)far);
    sweep_prep();
    sweep_y16();
    sweep_p10_p32();
    sweep_plans();
    sweep_orient();
    sweep_jpeg_orient();
    section("");
    printf("evaluations %ld\n", evals);
    printf("failures %ld\n", failures);
    return failures ? 1 : 0;
}
