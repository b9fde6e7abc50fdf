// Stand-alone host program over the wide lists (melf_process_wide_list*, melf_process_wide_plane_list*): the two checks
// (melf_frame_checks.h: check_wide_list; melf_stage_plan.h: check_wide_plane_list), the host packers and the address arithmetic of
// k_narrow_list_rows / k_narrow_plane_rows (melf_narrow_addr.h).  Two modes; tests/test_wide_list.py builds it under the host
// sanitizers and runs both.
//
//   wide_list_main extents
//       A shape sweep -- four sample types; packed BGR / RGB / BGRA / RGBA and planar; H 1, 8, 9, 17 (one row, exactly one wave's
//       rows, one more, three blocks); W 1, 5, 15, 16, 32, 37, 400 (a tail-only row, 15 samples, whole pieces with no tail, whole
//       pieces and a 15-sample tail, more than 64 pieces in a wave's block); row padding 0 and 3 samples; the whole frame and a crop
//       that touches its right and bottom edge.  Every frame of a list is a malloc block of its own that ends with the frame's last
//       sample, every plane of a plane list one that ends with the plane's, their bases one sample behind a 16-byte boundary.  The
//       list and the plane-list packer, and the kernels' per-wave walk restated on the CPU with the same address functions, write
//       staged frames that must equal narrow::pack_item's on the contiguous batch of the same samples, byte for byte: a read one
//       byte outside any extent is an AddressSanitizer report.
//
//   wide_list_main checks
//       The two checks swept from accepted descriptors, one mutation per rejection; counts, through WIDE_LIST_MESSAGES and
//       WIDE_PLANE_LIST_MESSAGES, that every message was produced.
//   Both print `failures 0`.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../meterelf_amd/csrc/melf_frame_checks.h"
#include "../meterelf_amd/csrc/melf_narrow_addr.h"

using namespace melf;

static int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                   \
    } while (0)

static uint32_t rng_state = 2468;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// a sample's bits: mostly small in-range values, now and then NaN, +-inf, a negative or a large one (u16: any word)
static uint32_t sample_bits(int type, uint32_t r)
{
    if (type == MELF_WIDE_U16) return r & 0xffffu;
    static const float special[6] = {-1.5f, 1.0e30f, -0.0f, 300.0f, 0.0f, 0.0f};
    float f = (float)(r & 255u) * 0.25f;
    const uint32_t pick = (r >> 8) & 31u;
    if (pick < 4) f = special[pick];
    uint32_t b;
    memcpy(&b, &f, 4);
    if (pick == 4) b = 0x7fc00000u;   // NaN
    if (pick == 5) b = 0x7f800000u;   // +inf
    if (pick == 6) b = 0xff800000u;   // -inf
    if (type == MELF_WIDE_F32) return b;
    if (type == MELF_WIDE_BF16) return b >> 16;
    // float16: from the value's float32 bits, exact for the values above that fit, inf otherwise
    const uint32_t sign = (b >> 16) & 0x8000u, e = (b >> 23) & 255u, m = b & 0x7fffffu;
    if (e == 255u) return sign | 0x7c00u | (m ? 0x200u : 0u);
    if (e == 0u) return sign;
    const int he = (int)e - 127 + 15;
    if (he >= 31) return sign | 0x7c00u;
    if (he <= 0) return sign;
    return sign | ((uint32_t)he << 10) | (m >> 13);
}

// a block of its own for `bytes` bytes that ends where they end, their first byte one sample behind a 16-byte boundary
struct Exact {
    uint8_t* block;
    uint8_t* at;
    Exact(const uint8_t* src, size_t bytes, int ss) : block((uint8_t*)malloc(bytes + (size_t)ss)), at(block + ss)
    {
        memcpy(at, src, bytes);
        if ((uintptr_t)block % 16 != 0 || (uintptr_t)at % 16 != (uintptr_t)ss) { printf("FAIL malloc alignment\n"); ++failures; }
    }
    ~Exact() { free(block); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

// The per-wave body of the three kernels restated on the CPU: the same walk over a wave's pieces, the same address functions, the
// same bounds test; the conversion is the host's narrow_samples
static void wave_rows_on_cpu(const uint8_t* src, uint8_t* dst, const gather::WaveRows& wr, uint32_t plane, uint64_t extent, const narrow::Rule& rule, int ss)
{
    const uint32_t ppr = gather::row_pieces(wr.run.row_bytes), total = ppr * wr.nrows;
    for (uint32_t i = 0; i < total; ++i) {
        const uint32_t r = i / ppr, piece = i - r * ppr;
        const narrow::Samples p = narrow::samples_of(wr.run, wr.row0 + r, piece);
        EXPECT(narrow::samples_readable(p, extent), "piece outside its extent: sample %llu + %u of %llu", (unsigned long long)p.sample, p.count,
               (unsigned long long)extent);
        if (!narrow::samples_readable(p, extent)) continue;
        memset(dst + p.dst_off, 0, 16);
        narrow::narrow_samples(dst + p.dst_off, src + p.sample * (uint64_t)ss, p.count, p.j0, plane, rule);
    }
}

static size_t n_geometries = 0, n_frames = 0, n_planes = 0;

static void one_geometry(int type, bool planar, int pix, int H, int W, int pad, const int rect[4])
{
    const int n = 2;
    const int ss = narrow::sample_bytes(type), ch = planar ? 1 : pix_bytes(pix);
    melf_wide_frames d = {};
    d.sample_type = type; d.layout = planar ? MELF_WIDE_PLANAR : MELF_WIDE_PACKED; d.pixel_format = planar ? 0 : pix;
    d.shift = 4; d.rounding = (H & 1) ? MELF_ROUND_FLOOR : MELF_ROUND_NEAREST;
    const float sc[3] = {1.0f, 2.0f, 3.5f}, of[3] = {0.25f, 7.0f, 20.5f};
    for (int k = 0; k < 3; ++k) { d.scale[k] = sc[k]; d.offset[k] = of[k]; }
    d.n = n; d.H = H; d.W = W;
    d.row_pitch = (int64_t)(W * ch + pad) * ss;
    const int64_t span = (int64_t)(H - 1) * d.row_pitch + (int64_t)W * ch * ss;   // bytes of the packed plane / of one plane
    // the contiguous batch: planes in the order R, B, G with a gap of 2 samples, frames 5 samples further apart than their extent
    if (planar) { d.r_offset = 0; d.b_offset = span + 2 * ss; d.g_offset = d.b_offset + span + 2 * ss; }
    const int64_t extent = planar ? d.g_offset + span : span;
    d.frame_stride = extent + 5 * ss;
    const size_t total = (size_t)(n - 1) * d.frame_stride + extent;
    std::vector<uint8_t> batch_mem(total + 16);
    uint8_t* batch = batch_mem.data();
    for (size_t i = 0; i < total / ss; ++i) {
        const uint32_t b = sample_bits(type, rnd());
        memcpy(batch + i * ss, &b, ss);
    }
    WideBatch wb;
    const char* msg = check_wide(batch, &d, &wb);
    EXPECT(msg == nullptr, "check_wide rejects the batch: %s", msg ? msg : "");
    if (msg) return;
    Crop cr;
    EXPECT(clamp_crop(rect, H, W, &cr), "empty crop");
    const StagePlan sp = narrow::wide_plan(wb, cr);
    const size_t stride = sp.staged.frame_stride;
    ++n_geometries;

    // the reference: the batch packer on the contiguous batch
    std::vector<uint8_t> want((size_t)n * stride, 0xa5);
    for (int i = 0; i < n; ++i)
        for (int item = 0; item < sp.items; ++item) narrow::pack_item(batch + (size_t)i * d.frame_stride, want.data() + i * stride, item, sp, wb.rule, ss);

    // ---- the frame list: every frame a block of its own of exactly one frame's extent ----
    {
        std::vector<Exact*> own;
        std::vector<const void*> ptrs;
        for (int i = 0; i < n; ++i) {
            own.push_back(new Exact(batch + (size_t)i * d.frame_stride, (size_t)extent, ss));
            ptrs.push_back(own.back()->at);
            ++n_frames;
        }
        melf_wide_frames dl = d;
        dl.frame_stride = 1;   // not looked at
        WideBatch wl;
        int bad = 0;
        msg = check_wide_list(&dl, ptrs.data(), &wl, &bad);
        EXPECT(msg == nullptr && bad == -1, "check_wide_list rejects the list: %s", msg ? msg : "");
        if (!msg) {
            EXPECT(wl.b.n == n && (int64_t)wl.b.lay.extent * ss == extent, "the list's batch: n %d, extent %zu samples", wl.b.n, wl.b.lay.extent);
            const StagePlan sl = narrow::wide_plan(wl, cr);
            EXPECT(sl.staged.frame_stride == stride && sl.items == sp.items, "the list's plan differs from the batch's");
            std::vector<uint8_t> got((size_t)n * stride, 0xa5), walked((size_t)n * stride, 0xa5);
            for (int i = 0; i < n; ++i) {
                for (int item = 0; item < sl.items; ++item) narrow::pack_item((const uint8_t*)ptrs[i], got.data() + i * stride, item, sl, wl.rule, ss);
                // k_narrow_list_rows: wave by wave, src = frames[f]
                const uint32_t waves = gather::frame_waves(sl.runs);
                for (uint32_t w = 0; w < waves; ++w)
                    wave_rows_on_cpu((const uint8_t*)ptrs[i], walked.data() + i * stride, gather::wave_rows(sl.runs, w), gather::wave_run(sl.runs, w),
                                     wl.b.lay.extent, wl.rule, ss);
            }
            EXPECT(got == want, "frame list packer: type %d planar %d pix %d H %d W %d pad %d", type, planar, pix, H, W, pad);
            // the walk writes whole 16-byte pieces (zeros behind a row's end), the packer the row's bytes: compare the rows' bytes
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < sl.runs.count; ++k)
                    for (uint32_t y = 0; y < sl.runs.run[k].rows; ++y) {
                        const size_t at = i * stride + (size_t)sl.runs.run[k].dst_off + (size_t)y * sl.runs.run[k].dst_pitch;
                        EXPECT(!memcmp(walked.data() + at, want.data() + at, sl.runs.run[k].row_bytes),
                               "list kernel walk: type %d planar %d pix %d H %d W %d pad %d frame %d run %d row %u", type, planar, pix, H, W, pad, i, k, y);
                    }
        }
        for (Exact* e : own) delete e;
    }

    // ---- the plane list: every plane a block of its own of exactly (H - 1) * pitch + W * ss bytes ----
    if (planar) {
        std::vector<Exact*> own;
        std::vector<const void*> ptrs;
        const int64_t off[3] = {d.b_offset, d.g_offset, d.r_offset};   // slots 0 / 1 / 2 = B / G / R
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
                own.push_back(new Exact(batch + (size_t)i * d.frame_stride + off[k], (size_t)span, ss));
                ptrs.push_back(own.back()->at);
                ++n_planes;
            }
        melf_wide_frames dp = d;
        dp.b_offset = dp.g_offset = dp.r_offset = 0;
        dp.frame_stride = 0;   // not looked at
        WidePlaneList w;
        int bf = 0, bp = 0;
        msg = check_wide_plane_list(&dp, ptrs.data(), 3, &w, &bf, &bp);
        EXPECT(msg == nullptr && bf == -1 && bp == -1, "check_wide_plane_list rejects the list: %s", msg ? msg : "");
        if (!msg) {
            const StagePlan sl = narrow::wide_plan(w.wb, cr);
            EXPECT(sl.staged.frame_stride == stride && sl.items == sp.items && sl.runs.count == 3, "the plane list's plan differs from the batch's");
            const PlaneSplit split = narrow::wide_plane_split(sl.runs, w.pl);
            for (int k = 0; k < 3; ++k)
                EXPECT((int64_t)split.extent[k] * ss == span && split.src_off[k] == (uint64_t)cr.y0 * (uint64_t)(d.row_pitch / ss) + (uint64_t)cr.x0,
                       "split of plane %d: off %llu extent %llu", k, (unsigned long long)split.src_off[k], (unsigned long long)split.extent[k]);
            std::vector<uint8_t> got((size_t)n * stride, 0xa5), walked((size_t)n * stride, 0xa5);
            for (int i = 0; i < n; ++i) {
                for (int item = 0; item < sl.items; ++item) narrow::pack_item(ptrs.data() + (size_t)i * 3, got.data() + i * stride, item, sl, split, w.wb.rule, ss);
                // k_narrow_plane_rows: wave by wave, src = planes[f * 3 + k]
                const uint32_t waves = gather::frame_waves(sl.runs);
                for (uint32_t wv = 0; wv < waves; ++wv) {
                    const gather::PlaneRows pr = gather::plane_rows(sl.runs, split, wv);
                    EXPECT(pr.k < 3, "run index %u", pr.k);
                    wave_rows_on_cpu((const uint8_t*)ptrs[(size_t)i * 3 + pr.k], walked.data() + i * stride, pr.wr, pr.k, pr.extent, w.wb.rule, ss);
                }
            }
            EXPECT(got == want, "plane list packer: type %d H %d W %d pad %d", type, H, W, pad);
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < 3; ++k)
                    for (uint32_t y = 0; y < sl.runs.run[k].rows; ++y) {
                        const size_t at = i * stride + (size_t)sl.runs.run[k].dst_off + (size_t)y * sl.runs.run[k].dst_pitch;
                        EXPECT(!memcmp(walked.data() + at, want.data() + at, sl.runs.run[k].row_bytes),
                               "plane kernel walk: type %d H %d W %d pad %d frame %d plane %d row %u", type, H, W, pad, i, k, y);
                    }
        }
        for (Exact* e : own) delete e;
    }
}

static int extents()
{
    const int widths[7] = {1, 5, 15, 16, 32, 37, 400};
    const int heights[4] = {1, 8, 9, 17};
    const int forms[5][2] = {{0, MELF_PIX_BGR}, {0, MELF_PIX_RGB}, {0, MELF_PIX_BGRA}, {0, MELF_PIX_RGBA}, {1, 0}};
    for (int type = MELF_WIDE_U16; type <= MELF_WIDE_F32; ++type)
        for (const auto& form : forms)
            for (const int W : widths)
                for (const int H : heights)
                    for (int pad = 0; pad <= 3; pad += 3) {
                        const int whole[4] = {0, 0, W, H};
                        const int edge[4] = {W / 3, H / 3, W + 7, H + 7};   // clamped: touches the right and the bottom edge
                        one_geometry(type, form[0] != 0, form[1], H, W, pad, whole);
                        one_geometry(type, form[0] != 0, form[1], H, W, pad, edge);
                    }
    printf("extents: %zu geometries, %zu frames and %zu planes in blocks of their own\n", n_geometries, n_frames, n_planes);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- checks ---
static long list_produced[WLIST_MSGS], plane_produced[WPLIST_MSGS];
static long accepted = 0;

static melf_wide_frames make(int type, bool planar, int pix, int H, int W, int pad)
{
    const int ss = narrow::sample_bytes(type), ch = planar ? 1 : pix_bytes(pix);
    melf_wide_frames d = {};
    d.sample_type = type; d.layout = planar ? MELF_WIDE_PLANAR : MELF_WIDE_PACKED; d.pixel_format = planar ? 0 : pix;
    d.shift = type == MELF_WIDE_U16 ? 8 : 0;
    for (int k = 0; k < 3; ++k) { d.scale[k] = 255.0f; d.offset[k] = 0.0f; }
    d.n = 4; d.H = H; d.W = W;
    d.row_pitch = (int64_t)(W * ch + pad) * ss;
    d.frame_stride = -7;   // not looked at by either check
    if (planar) {          // one frame's planes in the order G, B, R, a gap of 2 samples between them
        const int64_t span = (int64_t)(H - 1) * d.row_pitch + (int64_t)W * ss;
        d.g_offset = 0; d.b_offset = span + 2 * ss; d.r_offset = 2 * (span + 2 * ss);
    }
    return d;
}

static void expect_list(int line, const melf_wide_frames* d, const void* const* ptrs, const char* want, int want_bad)
{
    WideBatch wb;
    int bad = 99;
    const char* msg = check_wide_list(d, ptrs, &wb, &bad);
    if (msg != want || bad != want_bad) {
        if (++failures <= 20) printf("FAIL line %d: want '%s' at %d, got '%s' at %d\n", line, want ? want : "accepted", want_bad, msg ? msg : "accepted", bad);
        return;
    }
    for (int k = 0; k < WLIST_MSGS; ++k) list_produced[k] += msg == WIDE_LIST_MESSAGES[k];
}
static void expect_planes(int line, const melf_wide_frames* d, const void* const* ptrs, int nplanes, const char* want, int want_frame, int want_plane)
{
    WidePlaneList w;
    int bf = 99, bp = 99;
    const char* msg = check_wide_plane_list(d, ptrs, nplanes, &w, &bf, &bp);
    if (msg != want || bf != want_frame || bp != want_plane) {
        if (++failures <= 20)
            printf("FAIL line %d: want '%s' at %d / %d, got '%s' at %d / %d\n", line, want ? want : "accepted", want_frame, want_plane, msg ? msg : "accepted", bf, bp);
        return;
    }
    for (int k = 0; k < WPLIST_MSGS; ++k) plane_produced[k] += msg == WIDE_PLANE_LIST_MESSAGES[k];
}
#define LIST(d, ptrs, want, bad) expect_list(__LINE__, d, ptrs, want, bad)
#define PLANES(d, ptrs, np, want, bf, bp) expect_planes(__LINE__, d, ptrs, np, want, bf, bp)

static int checks()
{
    alignas(64) static uint8_t memory[512];   // never read: the checks look at the pointers' values only
    const int pixes[4] = {MELF_PIX_BGR, MELF_PIX_RGB, MELF_PIX_BGRA, MELF_PIX_RGBA};
    for (int type = MELF_WIDE_U16; type <= MELF_WIDE_F32; ++type) {
        const int ss = narrow::sample_bytes(type);
        for (int lead = 0; lead <= 1; ++lead)
            for (int pad = 0; pad <= 3; pad += 3)
                for (int form = 0; form < 5; ++form) {
                    const bool planar = form == 4;
                    melf_wide_frames base = make(type, planar, planar ? 0 : pixes[form], 5, 7, pad);
                    const int n = base.n;
                    // pointers with the sample's own alignment (lead 1: and no more), some of them repeated
                    const void* ptrs[12];
                    for (int i = 0; i < 12; ++i) ptrs[i] = memory + 64 + (i % 5) * 16 + lead * ss;
                    melf_wide_frames d;

                    // ---- the frame list ----
                    LIST(&base, ptrs, nullptr, -1);
                    {
                        WideBatch wb;
                        int bad;
                        if (!check_wide_list(&base, ptrs, &wb, &bad)) {
                            ++accepted;
                            const int64_t span = (int64_t)(base.H - 1) * base.row_pitch + (int64_t)base.W * (planar ? 1 : pix_bytes(base.pixel_format)) * ss;
                            EXPECT(wb.b.n == n && wb.ss == ss && (int64_t)wb.b.lay.extent * ss == base.r_offset + span, "the batch of an accepted list");
                        }
                    }
                    LIST(nullptr, ptrs, WIDE_MESSAGES[WIDE_DESC_NULL], -1);
                    d = base; d.H = 0; LIST(&d, ptrs, WIDE_MESSAGES[WIDE_SHAPE], -1);
                    d = base; d.row_pitch += 1; LIST(&d, ptrs, WIDE_MESSAGES[WIDE_ALIGN], -1);
                    d = base; d.reserved2 = 1; LIST(&d, ptrs, WIDE_MESSAGES[WIDE_RESERVED], -1);
                    d = base; d.n = -1; LIST(&d, ptrs, WIDE_MESSAGES[WIDE_SHAPE], -1);
                    d = base; d.n = 0; LIST(&d, nullptr, nullptr, -1);
                    LIST(&base, nullptr, WIDE_LIST_MESSAGES[WLIST_TABLE_NULL], -1);
                    for (int i = 0; i < n; ++i) {
                        const void* keep = ptrs[i];
                        ptrs[i] = nullptr; LIST(&base, ptrs, WIDE_LIST_MESSAGES[WLIST_PTR_NULL], i);
                        ptrs[i] = (const uint8_t*)keep + 1; LIST(&base, ptrs, WIDE_LIST_MESSAGES[WLIST_PTR_ALIGN], i);
                        if (ss == 4) { ptrs[i] = (const uint8_t*)keep + 2; LIST(&base, ptrs, WIDE_LIST_MESSAGES[WLIST_PTR_ALIGN], i); }
                        ptrs[i] = keep;
                    }
                    ptrs[n] = nullptr; LIST(&base, ptrs, nullptr, -1);   // behind the list: not looked at
                    ptrs[n] = memory + 64;

                    // ---- the plane list ----
                    if (!planar) {
                        PLANES(&base, ptrs, 3, WIDE_PLANE_LIST_MESSAGES[WPLIST_PACKED], -1, -1);
                        d = base; d.pixel_format = 9; PLANES(&d, ptrs, 3, WIDE_MESSAGES[WIDE_FORMAT], -1, -1);
                        continue;
                    }
                    base.b_offset = base.g_offset = base.r_offset = 0;   // of a plane list: from each plane's own pointer
                    PLANES(&base, ptrs, 3, nullptr, -1, -1);
                    {
                        WidePlaneList w;
                        int bf, bp;
                        if (!check_wide_plane_list(&base, ptrs, 3, &w, &bf, &bp)) {
                            ++accepted;
                            const int64_t span = (int64_t)(base.H - 1) * base.row_pitch + (int64_t)base.W * ss;
                            EXPECT(w.wb.b.n == n && w.pl.batch.n == n && w.pl.nplanes == 3 && (int)w.pl.align == ss, "the plane list of an accepted descriptor");
                            for (int k = 0; k < 3; ++k)
                                EXPECT((int64_t)w.pl.extent[k] * ss == span && (int64_t)w.pl.offset[k] * ss == k * span, "slot %d: offset %llu extent %llu samples",
                                       k, (unsigned long long)w.pl.offset[k], (unsigned long long)w.pl.extent[k]);
                            EXPECT(w.wb.b.lay.planes.b_off * ss == 0 && w.wb.b.lay.planes.g_off * ss == span && w.wb.b.lay.planes.r_off * ss == 2 * span,
                                   "the canonical planes are not B, G, R back to back");
                        }
                    }
                    PLANES(nullptr, ptrs, 3, WIDE_MESSAGES[WIDE_DESC_NULL], -1, -1);
                    d = base; d.W = 0; PLANES(&d, ptrs, 3, WIDE_MESSAGES[WIDE_SHAPE], -1, -1);
                    d = base; d.row_pitch = (int64_t)base.W * ss - ss; PLANES(&d, ptrs, 3, WIDE_MESSAGES[WIDE_PITCH_SMALL], -1, -1);
                    d = base; d.row_pitch += 1; PLANES(&d, ptrs, 3, WIDE_MESSAGES[WIDE_ALIGN], -1, -1);
                    d = base; d.sample_type = 4; PLANES(&d, ptrs, 3, WIDE_MESSAGES[WIDE_TYPE], -1, -1);
                    d = base; d.b_offset = ss; PLANES(&d, ptrs, 3, WIDE_PLANE_LIST_MESSAGES[WPLIST_OFFSETS], -1, -1);
                    d = base; d.g_offset = 4096; PLANES(&d, ptrs, 3, WIDE_PLANE_LIST_MESSAGES[WPLIST_OFFSETS], -1, -1);
                    d = base; d.r_offset = -(int64_t)ss; PLANES(&d, ptrs, 3, WIDE_PLANE_LIST_MESSAGES[WPLIST_OFFSETS], -1, -1);
                    for (const int np : {0, 1, 2, 4, -3}) PLANES(&base, ptrs, np, WIDE_PLANE_LIST_MESSAGES[WPLIST_NPLANES], -1, -1);
                    d = base; d.n = 0; PLANES(&d, nullptr, 3, nullptr, -1, -1);
                    PLANES(&base, nullptr, 3, WIDE_PLANE_LIST_MESSAGES[WPLIST_TABLE_NULL], -1, -1);
                    for (int i = 0; i < n; ++i)
                        for (int k = 0; k < 3; ++k) {
                            const void* keep = ptrs[i * 3 + k];
                            ptrs[i * 3 + k] = nullptr; PLANES(&base, ptrs, 3, WIDE_PLANE_LIST_MESSAGES[WPLIST_PTR_NULL], i, k);
                            ptrs[i * 3 + k] = (const uint8_t*)keep + 1; PLANES(&base, ptrs, 3, WIDE_PLANE_LIST_MESSAGES[WPLIST_PTR_ALIGN], i, k);
                            ptrs[i * 3 + k] = keep;
                        }
                }
    }
    // a plane too large for three of them to have a canonical descriptor: check_wide's own message
    {
        melf_wide_frames d = make(MELF_WIDE_U16, true, 0, INT32_MAX, 1, 0);
        d.row_pitch = INT32_MAX - 1;
        const void* ptrs[12];
        for (int i = 0; i < 12; ++i) ptrs[i] = memory + 64;
        PLANES(&d, ptrs, 3, WIDE_MESSAGES[WIDE_OFFSET_LARGE], -1, -1);
    }
    int seen = 0;
    printf("accepted %ld; messages of the frame list:\n", accepted);
    for (int k = 0; k < WLIST_MSGS; ++k) { printf("%8ld  %s\n", list_produced[k], WIDE_LIST_MESSAGES[k]); seen += list_produced[k] > 0; }
    printf("of the plane list:\n");
    for (int k = 0; k < WPLIST_MSGS; ++k) { printf("%8ld  %s\n", plane_produced[k], WIDE_PLANE_LIST_MESSAGES[k]); seen += plane_produced[k] > 0; }
    printf("messages %d of %d\n", seen, (int)WLIST_MSGS + (int)WPLIST_MSGS);
    if (seen != WLIST_MSGS + WPLIST_MSGS || accepted == 0) ++failures;
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "extents")) return extents();
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    printf("usage: wide_list_main extents | checks\n");
    return 2;
}
