// A frame's planes in separate allocations (melf_process_plane_list*): plane_list_check and plane_split of melf_stage_plan.h and the
// address arithmetic of k_plane_rows (melf_gather_addr.h: wave_run, plane_rows), swept on the CPU.
//
// For each of the four families with more than one plane: the descriptors of tests/stage_runs_main.cpp -- the same W and H, padded
// and unpadded pitches, every format code, subsampling, c_step, order of an interleaved pair and shift -- with the plane offsets
// counted from each plane's own pointer, and the same rectangles.  A case fills a contiguous reference frame of the canonical
// descriptor with random bytes, stages it through the existing one-allocation walk (wave_rows, piece_of: what k_gather_rows does),
// then mallocs every plane on its own, to exactly its readable extent, at ONE base phase per plane and case -- not at all of them:
// the address arithmetic does not depend on the phase, as in stage_runs_main.cpp -- out of those the family's alignment allows (the
// phases rotate from case to case, every plane slot at its own pace, and the tally says that every slot met every phase), copies the
// reference frame's bytes of that plane into it, and walks the split runs the way k_plane_rows does: wave by wave, piece by piece.
//   (i)   every source access lies inside its own plane's extent (and the sanitizer build's red zones say the same),
//   (ii)  the staged frame is byte-identical to the one-allocation walk's,
//   (iii) every wave's run index names the run wave_rows returns.
// Descriptor rules, on every accepted descriptor: a nonzero offset of a planar layout, an interleaved pair other than {0, bytes per
// sample} and a wrong nplanes are rejected; and once, the four one-plane families and an unknown family.
// Prints the cases per family and ends with `failures 0`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../meterelf_amd/csrc/melf_gather_addr.h"

using namespace melf;

static const int TPL_H = 10, TPL_W = 12;   // the "template": the smallest crop
static long failures = 0;
static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 24);
}

#define FAIL(...)                                                     \
    do {                                                              \
        if (failures < 20) { printf(__VA_ARGS__); printf("\n"); }     \
        ++failures;                                                   \
    } while (0)

struct Tally {
    const char* name;
    long cases = 0, rejected = 0, odd_origin = 0, edge = 0, tail_pieces = 0, full_pieces = 0, rules = 0;
    long phases[STAGE_MAX_RUNS] = {0, 0, 0};   // per plane slot: bit p set when a plane of that slot lay at phase p modulo 16
};

// ---- the existing one-allocation walk (k_gather_rows on the CPU, as tests/stage_runs_main.cpp has it, without its checks) --------
static void gather_whole(const uint8_t* frame, size_t extent, const RowRuns& runs, uint8_t* staged)
{
    const uint32_t waves = gather::frame_waves(runs);
    for (uint32_t w = 0; w < waves; ++w) {
        const gather::WaveRows wr = gather::wave_rows(runs, w);
        const uint32_t ppr = gather::row_pieces(wr.run.row_bytes), total = ppr * wr.nrows;
        for (uint32_t i = 0; i < total; ++i) {
            const uint32_t r = i / ppr, piece = i - r * ppr;
            const gather::Piece p = gather::piece_of(wr.run, wr.row0 + r, piece);
            if (!gather::piece_readable(p, extent)) { FAIL("one-allocation walk: a piece is not readable"); continue; }
            uint8_t v[16] = {0};
            memcpy(v, frame + p.src_off, p.bytes);
            memcpy(staged + p.dst_off, v, 16);
        }
    }
}

// ---- the walk of k_plane_rows ---------------------------------------------------------------------------------------------------
struct Planes {
    const uint8_t* ptr[STAGE_MAX_RUNS];
    uint64_t extent[STAGE_MAX_RUNS];   // what was malloc'd of each
    int nplanes;
};
template <class T>
static T load_at(const Planes& pl, uint32_t k, uint64_t off)
{
    if (off + sizeof(T) > pl.extent[k]) { FAIL("plane %u: source access [%llu, +%zu) outside its extent %llu", k, (unsigned long long)off, sizeof(T), (unsigned long long)pl.extent[k]); return T(); }
    T v;
    memcpy(&v, pl.ptr[k] + off, sizeof(T));
    return v;
}
static void gather_planes(const Planes& pl, const RowRuns& runs, const PlaneSplit& split, uint8_t* staged, size_t stride, Tally* t)
{
    const uint32_t waves = gather::frame_waves(runs);
    for (uint32_t w = 0; w < waves; ++w) {
        const gather::PlaneRows pr = gather::plane_rows(runs, split, w);
        const gather::WaveRows wr0 = gather::wave_rows(runs, w);
        // (iii) the run index names wave_rows' run, and everything but the source offset is that run's
        if (pr.k != gather::wave_run(runs, w) || (int)pr.k >= runs.count || (int)pr.k >= pl.nplanes) { FAIL("wave %u: run index %u", w, pr.k); continue; }
        if (memcmp(&runs.run[pr.k], &wr0.run, sizeof(RowRun))) FAIL("wave %u: run index %u does not name wave_rows' run", w, pr.k);
        RowRun same = pr.wr.run;
        same.src_off = wr0.run.src_off;
        if (memcmp(&same, &wr0.run, sizeof(RowRun)) || pr.wr.row0 != wr0.row0 || pr.wr.nrows != wr0.nrows) FAIL("wave %u: plane_rows' rows are not wave_rows'", w);
        if (pr.wr.run.src_off != split.src_off[pr.k] || pr.extent != split.extent[pr.k]) FAIL("wave %u: not the split of run %u", w, pr.k);
        if (pr.extent != pl.extent[pr.k]) FAIL("wave %u: extent %llu of plane %u, allocated %llu", w, (unsigned long long)pr.extent, pr.k, (unsigned long long)pl.extent[pr.k]);
        const uint32_t ppr = gather::row_pieces(pr.wr.run.row_bytes), total = ppr * pr.wr.nrows;
        for (uint32_t i = 0; i < total; ++i) {   // lane i % 64 in iteration i / 64
            const uint32_t r = i / ppr, piece = i - r * ppr;
            const gather::Piece p = gather::piece_of(pr.wr.run, pr.wr.row0 + r, piece);
            if (!gather::piece_readable(p, pr.extent)) { FAIL("plane %u row %u piece %u: not readable", pr.k, pr.wr.row0 + r, piece); continue; }
            uint8_t v[16] = {0};
            if (p.bytes == (uint32_t)gather::PIECE) {
                struct B16 { uint8_t b[16]; };
                const B16 x = load_at<B16>(pl, pr.k, p.src_off);
                memcpy(v, x.b, 16);
                ++t->full_pieces;
            } else {
                if (p.bytes == 0 || p.bytes > 15) FAIL("tail piece of %u bytes", p.bytes);
                uint32_t got = 0;
                if (gather::tail_has(p.bytes, 8)) { const uint64_t x = load_at<uint64_t>(pl, pr.k, p.src_off + gather::tail_at(p.bytes, 8)); memcpy(v + gather::tail_at(p.bytes, 8), &x, 8); got += 8; }
                if (gather::tail_has(p.bytes, 4)) { const uint32_t x = load_at<uint32_t>(pl, pr.k, p.src_off + gather::tail_at(p.bytes, 4)); memcpy(v + gather::tail_at(p.bytes, 4), &x, 4); got += 4; }
                if (gather::tail_has(p.bytes, 2)) { const uint16_t x = load_at<uint16_t>(pl, pr.k, p.src_off + gather::tail_at(p.bytes, 2)); memcpy(v + gather::tail_at(p.bytes, 2), &x, 2); got += 2; }
                if (gather::tail_has(p.bytes, 1)) { const uint8_t x = load_at<uint8_t>(pl, pr.k, p.src_off + gather::tail_at(p.bytes, 1)); v[gather::tail_at(p.bytes, 1)] = x; got += 1; }
                if (got != p.bytes) FAIL("tail loads fetch %u of %u bytes", got, p.bytes);
                ++t->tail_pieces;
            }
            if (p.dst_off % 16 || p.dst_off + 16 > stride) { FAIL("store at %llu outside the staged frame of %zu bytes (or misaligned)", (unsigned long long)p.dst_off, stride); continue; }
            memcpy(staged + p.dst_off, v, 16);
        }
    }
}

// ---- one case -------------------------------------------------------------------------------------------------------------------
static void run_case(const PlaneList& pl, const int rect[4], long counter, Tally* t)
{
    const FrameBatch& b = pl.batch;
    Crop cr;
    if (!clamp_crop(rect, b.H, b.W, &cr) || cr.rows < TPL_H || cr.cols < TPL_W) { FAIL("%s: bad test rectangle", t->name); return; }
    const StagePlan sp = stage_plan(b, cr);
    if (sp.runs.count != pl.nplanes) { FAIL("%s: %d runs for %d planes", t->name, sp.runs.count, pl.nplanes); return; }
    const PlaneSplit split = plane_split(sp.runs, pl);
    const size_t extent = b.lay.extent, stride = sp.staged.frame_stride;
    ++t->cases;
    t->odd_origin += (cr.x0 & 1) && (cr.y0 & 1);
    t->edge += (cr.x0 == 0 && cr.y0 == 0) || (cr.x1 == b.W && cr.y1 == b.H);
    // the contiguous reference frame and what the one-allocation walk makes of it
    uint8_t* frame = (uint8_t*)malloc(extent);
    for (size_t i = 0; i < extent; ++i) frame[i] = (uint8_t)rnd();
    uint8_t* want = (uint8_t*)malloc(stride);
    uint8_t* got = (uint8_t*)malloc(stride);
    memset(want, 0xA5, stride);
    memset(got, 0xA5, stride);
    gather_whole(frame, extent, sp.runs, want);
    // every plane a malloc of its own of exactly its extent, ending where the allocation ends, at its own phase
    const long phases = 16 / (long)pl.align;
    Planes planes = {};
    uint8_t* alloc[STAGE_MAX_RUNS] = {nullptr, nullptr, nullptr};
    planes.nplanes = pl.nplanes;
    for (int k = 0; k < pl.nplanes; ++k) {
        const size_t phase = (size_t)((counter * (2 * k + 1) + 5 * k) % phases) * pl.align;
        if (pl.offset[k] + pl.extent[k] > extent) { FAIL("%s: plane %d lies outside the canonical frame", t->name, k); continue; }
        alloc[k] = (uint8_t*)malloc(pl.extent[k] + phase);
        memcpy(alloc[k] + phase, frame + pl.offset[k], pl.extent[k]);
        planes.ptr[k] = alloc[k] + phase;
        planes.extent[k] = pl.extent[k];
        if ((uintptr_t)planes.ptr[k] & (pl.align - 1)) FAIL("%s: test plane misaligned", t->name);
        t->phases[k] |= 1l << ((uintptr_t)planes.ptr[k] & 15);
        if (split.src_off[k] > pl.extent[k]) FAIL("%s: run %d starts behind its plane's extent", t->name, k);
    }
    if (!failures) gather_planes(planes, sp.runs, split, got, stride, t);
    if (memcmp(want, got, stride)) FAIL("%s: staged frame differs (W %d H %d rect %d %d %d %d)", t->name, b.W, b.H, rect[0], rect[1], rect[2], rect[3]);
    for (int k = 0; k < pl.nplanes; ++k) free(alloc[k]);
    free(got);
    free(want);
    free(frame);
}

// the rectangles of tests/stage_runs_main.cpp
template <class F>
static void each_rect(int W, int H, F f)
{
    const int colsv[3] = {TPL_W, TPL_W + 5, W}, rowsv[3] = {TPL_H, TPL_H + 3, H};
    for (int ci = 0; ci < 3; ++ci)
        for (int ri = 0; ri < 3; ++ri) {
            const int cols = colsv[ci], rows = rowsv[ri];
            if (cols > W || rows > H) continue;
            const int xs[5] = {0, 1, 2, W - cols - 1, W - cols}, ys[4] = {0, 1, H - rows - 1, H - rows};
            for (int xi = 0; xi < 5; ++xi)
                for (int yi = 0; yi < 4; ++yi) {
                    const int x0 = xs[xi], y0 = ys[yi];
                    if (x0 < 0 || y0 < 0 || x0 + cols > W || y0 + rows > H) continue;
                    if ((xi >= 3 && x0 <= 2) || (yi >= 2 && y0 <= 1)) continue;   // the same origin again
                    const int rect[4] = {x0, y0, x0 + cols, y0 + rows};
                    f(rect);
                }
        }
}
static const int WS[] = {0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 20, 36, 39, 40}, HS[] = {0, 1, 2, 3, 15, 40};

static void expect_rejected(Tally* t, int family, const void* d, int nplanes, const char* want_msg, const char* what)
{
    PlaneList pl;
    const char* msg = plane_list_check(family, d, nplanes, &pl);
    ++t->rules;
    if (!msg) FAIL("%s: %s is accepted", t->name, what);
    else if (want_msg && msg != want_msg) FAIL("%s: %s is rejected with \"%s\"", t->name, what, msg);
}

// A YUV descriptor (any of the three structs): accepted -> the rules, then every rectangle
template <class Desc>
static void sweep_yuv(Tally* t, int family, Desc d, int bps, bool semi, long* counter)
{
    PlaneList pl;
    const int nplanes = semi ? 2 : 3;
    d.n = 1;
    if (const char* msg = plane_list_check(family, &d, nplanes, &pl)) { (void)msg; ++t->rejected; return; }
    if (pl.nplanes != nplanes || pl.align != (unsigned)bps) FAIL("%s: nplanes %d align %u", t->name, pl.nplanes, pl.align);
    // the extents the header states
    if (pl.extent[0] != (uint64_t)((d.H - 1) * d.y_pitch + (int64_t)d.W * bps)) FAIL("%s: Y extent", t->name);
    {
        Desc bad = d;
        expect_rejected(t, family, &bad, semi ? 3 : 2, PLANE_LIST_NPLANES, "a wrong nplanes");
        expect_rejected(t, family, &bad, 1, PLANE_LIST_NPLANES, "nplanes 1");
        if (semi) {
            bad.u_offset = d.u_offset + bps; bad.v_offset = d.v_offset + bps;   // still adjacent: the family's own rule passes
            expect_rejected(t, family, &bad, nplanes, PLANE_LIST_SEMI_OFFSETS, "an interleaved pair other than {0, bytes per sample}");
            bad.u_offset = 0; bad.v_offset = 0;
            expect_rejected(t, family, &bad, nplanes, nullptr, "an interleaved pair {0, 0}");
        } else {
            bad.u_offset = bps;
            expect_rejected(t, family, &bad, nplanes, PLANE_LIST_PLANAR_OFFSETS, "a nonzero u_offset of a planar layout");
            bad.u_offset = 0; bad.v_offset = 64;
            expect_rejected(t, family, &bad, nplanes, PLANE_LIST_PLANAR_OFFSETS, "a nonzero v_offset of a planar layout");
        }
    }
    each_rect(d.W, d.H, [&](const int* rect) { run_case(pl, rect, (*counter)++, t); });
}

int main()
{
    Tally tal[4] = {{"yuv"}, {"yuv_planar"}, {"yuv16"}, {"planes"}};
    long counter = 0;
    // the one-plane families and an unknown one
    {
        melf_frames d = {MELF_PIX_BGR, 1, 16, 16, 48, 0};
        Tally none = {"one-plane"};
        const int one[4] = {MELF_LIST_FRAMES, MELF_LIST_YUV422, MELF_LIST_YUV422_10, MELF_LIST_PACKED32};
        for (int f : one)
            for (int np = 1; np <= 3; ++np) expect_rejected(&none, f, &d, np, PLANE_LIST_ONE_PLANE, "a one-plane family");
        expect_rejected(&none, -1, &d, 3, PLANE_LIST_UNKNOWN_FAMILY, "family -1");
        expect_rejected(&none, 8, &d, 3, PLANE_LIST_UNKNOWN_FAMILY, "family 8");
        const int many[4] = {MELF_LIST_YUV, MELF_LIST_YUV_PLANAR, MELF_LIST_YUV16, MELF_LIST_PLANES};
        for (int f : many) expect_rejected(&none, f, nullptr, 3, nullptr, "a NULL descriptor");
        printf("one-plane and unknown families: %ld rejections\n", none.rules);
    }
    for (int wi : WS)
        for (int hi : HS) {
            const int W = TPL_W + wi, H = TPL_H + hi;
            for (int pad = 0; pad < 2; ++pad) {
                // melf_yuv_frames: NV12 and I420 (YV12 is the same descriptor: the caller exchanges two pointers), every matrix
                for (int v = 0; v < 2; ++v) {
                    const bool nv12 = v == 0;
                    const int64_t yp = W + (pad ? 5 : 0), cp = (nv12 ? W : W / 2) + (pad ? 3 : 0);
                    static const int matrices[4] = {MELF_YUV_BT601_LIMITED, MELF_YUV_BT601_FULL, MELF_YUV_BT709_LIMITED, MELF_YUV_BT709_FULL};
                    melf_yuv_frames d = {nv12 ? MELF_YUV_NV12 : MELF_YUV_I420, matrices[counter & 3], 1, H, W, 0, yp, cp, 0, nv12 ? 1 : 0, 0};
                    sweep_yuv(&tal[0], MELF_LIST_YUV, d, 1, nv12, &counter);
                }
                // melf_yuv_planar_frames: the four subsamplings, planar, and semi-planar with U first and V first
                for (int sx = 0; sx < 2; ++sx)
                    for (int sy = 0; sy < 2; ++sy)
                        for (int form = 0; form < 3; ++form) {
                            const int step = form == 0 ? 1 : 2;
                            const bool vfirst = form == 2;
                            const int64_t yp = W + (pad ? 5 : 0), cs = W >> sx, cp = cs * step + (pad ? 3 : 0);
                            melf_yuv_planar_frames d = {0, 1, H, W, sx, sy, step, 0, yp, cp, step == 2 && vfirst ? 1 : 0, step == 2 && !vfirst ? 1 : 0, 0};
                            sweep_yuv(&tal[1], MELF_LIST_YUV_PLANAR, d, 1, step == 2, &counter);
                        }
                // melf_yuv16_frames: 4:2:0 and 4:2:2, planar, and semi-planar with U first and V first, the shifts of the named formats
                for (int sy = 0; sy < 2; ++sy)
                    for (int form = 0; form < 3; ++form) {
                        static const int shifts[4] = {8, 2, 4, 0};
                        const int step = form == 0 ? 1 : 2;
                        const bool vfirst = form == 2;
                        const int64_t yp = 2 * W + (pad ? 6 : 0), cs = W >> 1, cp = cs * step * 2 + (pad ? 4 : 0);
                        melf_yuv16_frames d = {3, 1, H, W, sy, step, shifts[counter & 3], 0, yp, cp, step == 2 && vfirst ? 2 : 0, step == 2 && !vfirst ? 2 : 0, 0};
                        sweep_yuv(&tal[2], MELF_LIST_YUV16, d, 2, step == 2, &counter);
                    }
                // melf_planar_frames (the six orders of three planes are one descriptor here: the caller orders three pointers)
                {
                    Tally* t = &tal[3];
                    const int64_t rp = W + (pad ? 5 : 0);
                    melf_planar_frames d = {1, H, W, 0, 0, 0, 0, rp, 0};
                    PlaneList pl;
                    if (plane_list_check(MELF_LIST_PLANES, &d, 3, &pl)) { ++t->rejected; continue; }
                    for (int k = 0; k < 3; ++k)
                        if (pl.extent[k] != (uint64_t)((H - 1) * rp + W)) FAIL("planes: extent of plane %d", k);
                    expect_rejected(t, MELF_LIST_PLANES, &d, 2, PLANE_LIST_NPLANES, "nplanes 2");
                    expect_rejected(t, MELF_LIST_PLANES, &d, 4, PLANE_LIST_NPLANES, "nplanes 4");
                    for (int k = 0; k < 3; ++k) {
                        melf_planar_frames bad = d;
                        (k == 0 ? bad.b_offset : k == 1 ? bad.g_offset : bad.r_offset) = (H - 1) * rp + W;
                        expect_rejected(t, MELF_LIST_PLANES, &bad, 3, PLANE_LIST_PLANAR_OFFSETS, "a nonzero plane offset");
                    }
                    each_rect(W, H, [&](const int* rect) { run_case(pl, rect, counter++, t); });
                }
            }
        }
    for (const Tally& t : tal) {
        printf("family %s: cases %ld odd_origin %ld edge %ld rejected %ld full_pieces %ld tail_pieces %ld rules %ld phases 0x%lx 0x%lx 0x%lx\n", t.name, t.cases,
               t.odd_origin, t.edge, t.rejected, t.full_pieces, t.tail_pieces, t.rules, t.phases[0], t.phases[1], t.phases[2]);
        if (t.cases == 0 || t.odd_origin == 0 || t.edge == 0 || t.full_pieces == 0 || t.tail_pieces == 0 || t.rules == 0) FAIL("family %s: the sweep misses a kind of case", t.name);
        const long all = !strcmp(t.name, "yuv16") ? 0x5555l : 0xffffl;   // every phase the alignment allows
        for (int k = 0; k < 3; ++k)
            if (t.phases[k] != all) FAIL("family %s: plane slot %d met the phases 0x%lx, not 0x%lx", t.name, k, t.phases[k], all);
    }
    printf("failures %ld\n", failures);
    return failures ? 1 : 0;
}
