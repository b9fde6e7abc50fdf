// The oriented plans and the address arithmetic of k_orient_tiles (melf_orient_addr.h), swept on the CPU.
//
// For each of the six families that can be oriented and each of the eight EXIF codes: descriptors the family's check accepts -- small
// H and W up to more than two tiles, every format code, subsampling, c_step and plane order, padded and unpadded pitches, every base
// alignment phase the check takes -- and rectangles on the ORIENTED frame with even and odd origins, inside it and touching its edges.
// A case puts random bytes into a malloc of exactly the descriptor's extent at that phase and then
//   (a) builds the oriented frame O naively, pixel by pixel, from the table of include/meterelf_hip.h and the public header's
//       addressing of a pixel's samples (nothing of melf_orient_addr.h but the tight layout O is laid out in), takes stage_plan of
//       it and copies the plan's rows plainly: the reference staged frame;
//   (b) executes the oriented plan the way k_orient_tiles does: tile by tile, every load piece into a simulated LDS tile, every store
//       piece out of it, every offset, width and path from the functions the kernel calls;
//   (c) packs the same runs element by element with elem_src_off, as the host call does.
// Then every source access of (b) and (c) lies in [0, extent) (and the sanitizer build's red zones say the same), every store lies
// inside the staged frame (a malloc of exactly its stride), every byte of every run's rows is written exactly once, the bytes of a
// last piece behind a row's end are zeros, and the rows of (b) and (c) equal those of (a) byte for byte.  The combinations the header
// rejects are rejected.  Prints one line per family and code and ends with `failures 0`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../meterelf_amd/csrc/melf_orient_addr.h"

using namespace melf;

static long failures = 0;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
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
    long cases[9] = {}, odd_origin[9] = {}, edge[9] = {}, rejected[9] = {}, tiles[9] = {}, tail_loads[9] = {};
};

// ---- the table of include/meterelf_hip.h, literally: O[y][x] = S[*sy][*sx], S of H rows x W columns ----
static void stored_of(int code, int y, int x, int H, int W, int* sy, int* sx)
{
    switch (code) {
    case 1: *sy = y; *sx = x; break;
    case 2: *sy = y; *sx = W - 1 - x; break;
    case 3: *sy = H - 1 - y; *sx = W - 1 - x; break;
    case 4: *sy = H - 1 - y; *sx = x; break;
    case 5: *sy = x; *sx = y; break;
    case 6: *sy = H - 1 - x; *sx = y; break;
    case 7: *sy = H - 1 - x; *sx = W - 1 - y; break;
    default: *sy = x; *sx = W - 1 - y; break;
    }
}

// ---- the public header's addressing: the bytes that make pixel (x, y) of a frame of batch b ----
struct Sample { uint64_t off; int len; };
static int pixel_samples(const FrameBatch& b, int x, int y, Sample s[3])
{
    const FrameLayout& L = b.lay;
    const uint64_t rs = (uint64_t)b.row_stride;
    if (pix_yuv(L.pix)) {
        const int step = L.pix == PIX_NV12 ? 2 : 1;
        s[0] = {y * rs + x, 1};
        s[1] = {(uint64_t)L.yuv.u_off + (uint64_t)(y >> 1) * L.yuv.c_pitch + (uint64_t)(x >> 1) * step, 1};
        s[2] = {(uint64_t)L.yuv.v_off + (uint64_t)(y >> 1) * L.yuv.c_pitch + (uint64_t)(x >> 1) * step, 1};
        return 3;
    }
    if (pix_p32(L.pix)) { s[0] = {y * rs + 4 * (uint64_t)x, 4}; return 1; }
    if (L.pix == PIX_YUVP) {
        const YuvPlanarPlanes& p = L.yuvp;
        s[0] = {y * rs + x, 1};
        s[1] = {(uint64_t)p.u_off + (uint64_t)(y >> p.sub_y) * p.c_pitch + (uint64_t)(x >> p.sub_x) * p.c_step, 1};
        s[2] = {(uint64_t)p.v_off + (uint64_t)(y >> p.sub_y) * p.c_pitch + (uint64_t)(x >> p.sub_x) * p.c_step, 1};
        return 3;
    }
    if (L.pix == PIX_YUV16) {
        const Yuv16Planes& p = L.y16;
        s[0] = {y * rs + 2 * (uint64_t)x, 2};
        s[1] = {(uint64_t)p.u_off + (uint64_t)(y >> p.sub_y) * p.c_pitch + (uint64_t)(x >> 1) * p.c_step * 2, 2};
        s[2] = {(uint64_t)p.v_off + (uint64_t)(y >> p.sub_y) * p.c_pitch + (uint64_t)(x >> 1) * p.c_step * 2, 2};
        return 3;
    }
    if (L.pix == PIX_PLANAR) {
        s[0] = {(uint64_t)L.planes.b_off + y * rs + x, 1};
        s[1] = {(uint64_t)L.planes.g_off + y * rs + x, 1};
        s[2] = {(uint64_t)L.planes.r_off + y * rs + x, 1};
        return 3;
    }
    s[0] = {y * rs + (uint64_t)x * pix_bytes(L.pix), pix_bytes(L.pix)};
    return 1;
}

// ---- the kernel's walk over a frame, on the CPU ----
struct Access {
    const uint8_t* frame;
    size_t extent;
    uint8_t* staged;
    size_t stride;
    std::vector<uint8_t>* writes;   // per staged byte: how often it was stored
};
static void load_bytes(const Access& a, uint64_t off, uint32_t n, uint8_t* to)
{
    if (off + n > a.extent) { FAIL("source access [%llu, +%u) outside the extent %zu", (unsigned long long)off, n, a.extent); return; }
    memcpy(to, a.frame + off, n);
}
static void orient_frame(const Access& a, const orient::Runs& runs, Tally* t)
{
    const int code = runs.code;
    const uint32_t tiles = orient::frame_tiles(runs);
    std::vector<int> seen(tiles, 0);
    for (uint32_t ti = 0; ti < tiles; ++ti) {   // workgroup ti
        const orient::Tile tl = orient::tile_of(runs, ti);
        ++t->tiles[code];
        if ((int)tl.k >= runs.count || memcmp(&runs.run[tl.k], &tl.run, sizeof(orient::Run))) { FAIL("tile %u: not a run of the plan", ti); continue; }
        const uint32_t eb = tl.run.eb, lds_bytes = orient::TILE * orient::lds_pitch(eb);
        if (tl.nr == 0 || tl.nc == 0 || tl.nr > (uint32_t)orient::TILE || tl.nc > (uint32_t)orient::TILE || tl.srows * tl.scols != tl.nr * tl.nc)
            FAIL("tile %u: %u x %u from %u x %u", ti, tl.nr, tl.nc, tl.srows, tl.scols);
        if (tl.srow0 + tl.srows > tl.run.ph || tl.scol0 + tl.scols > tl.run.pw) { FAIL("tile %u: source rectangle outside the stored plane", ti); continue; }
        std::vector<uint8_t> lds(lds_bytes, 0xCD), filled(lds_bytes, 0);
        const uint32_t lpr = orient::load_pieces(tl);
        for (uint32_t i = 0; i < lpr * tl.srows; ++i) {   // thread i % THREADS in iteration i / THREADS
            const uint32_t s = i / lpr, piece = i - s * lpr;
            const orient::Load l = orient::load_of(tl, s, piece);
            if (!orient::load_readable(l, a.extent)) { FAIL("tile %u row %u piece %u: not readable", ti, s, piece); continue; }
            uint8_t v[16] = {0};
            if (l.bytes == (uint32_t)orient::PIECE) {
                load_bytes(a, l.src_off, 16, v);
            } else {
                if (l.bytes == 0 || l.bytes > 15) FAIL("tail piece of %u bytes", l.bytes);
                uint32_t got = 0;
                for (uint32_t w = 8; w >= 1; w /= 2)
                    if (orient::tail_has(l.bytes, w)) { load_bytes(a, l.src_off + orient::tail_at(l.bytes, w), w, v + orient::tail_at(l.bytes, w)); got += w; }
                if (got != l.bytes) FAIL("tail loads fetch %u of %u bytes", got, l.bytes);
                ++t->tail_loads[code];
            }
            if (l.lds_off % 4 || l.lds_off + 16 > lds_bytes) { FAIL("LDS store at %u outside the tile of %u bytes (or misaligned)", l.lds_off, lds_bytes); continue; }
            memcpy(&lds[l.lds_off], v, 16);
            for (uint32_t q = 0; q < l.bytes; ++q) ++filled[l.lds_off + q];
        }
        const orient::LdsMap m = orient::lds_map(tl, code);
        const uint32_t spr = orient::store_pieces(tl);
        for (uint32_t i = 0; i < spr * tl.nr; ++i) {
            const uint32_t r = i / spr, piece = i - r * spr;
            const orient::Store st = orient::store_of(tl, r, piece);
            uint8_t v[16] = {0};
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t d = piece * 16 + j, e = d / eb, q = d - e * eb;
                if (e >= tl.nc) continue;
                const uint32_t at = orient::lds_elem(m, r, e) + q;
                if (at >= lds_bytes || filled[at] != 1) { FAIL("tile %u: LDS byte %u read but loaded %d times", ti, at, at < lds_bytes ? filled[at] : -1); continue; }
                if (eb > 1 && q == 0 && orient::lds_elem(m, r, e) % (eb == 3 ? 1 : eb)) FAIL("tile %u: misaligned LDS element", ti);
                v[j] = lds[at];
            }
            if (st.bytes == 0 || st.bytes > 16 || (st.bytes < 16 && st.bytes != tl.nc * eb - piece * 16)) FAIL("store piece of %u bytes", st.bytes);
            if (st.dst_off % 16 || st.dst_off + 16 > a.stride) { FAIL("store at %llu outside the staged frame of %zu bytes (or misaligned)", (unsigned long long)st.dst_off, a.stride); continue; }
            for (int q = 0; q < 16; ++q) ++(*a.writes)[st.dst_off + q];
            memcpy(a.staged + st.dst_off, v, 16);
        }
    }
}

// ---- one case ----
static void run_case(const FrameBatch& b, int code, const int rect[4], size_t phase, Tally* t)
{
    const int H2 = orient::oriented_h(b, code), W2 = orient::oriented_w(b, code);
    Crop cr;
    if (!clamp_crop(rect, H2, W2, &cr)) { FAIL("%s: bad test rectangle", t->name); return; }
    const size_t extent = b.lay.extent;
    uint8_t* alloc = (uint8_t*)malloc(extent + phase);   // the frame ends where the allocation ends
    uint8_t* frame = alloc + phase;
    for (size_t i = 0; i < extent; ++i) frame[i] = (uint8_t)rnd();
    ++t->cases[code];
    t->odd_origin[code] += (cr.x0 & 1) && (cr.y0 & 1);
    t->edge[code] += cr.x0 == 0 || cr.y0 == 0 || cr.x1 == W2 || cr.y1 == H2;
    // (a) the oriented frame, naively, and the family's plan of it with a plain row copy
    const orient::Oriented o = orient::oriented_batch(b, code);
    if (o.batch.H != H2 || o.batch.W != W2) FAIL("%s: oriented batch of %d x %d", t->name, o.batch.H, o.batch.W);
    std::vector<uint8_t> O(o.batch.lay.extent, 0);
    for (int y = 0; y < H2; ++y)
        for (int x = 0; x < W2; ++x) {
            int sy, sx;
            stored_of(code, y, x, b.H, b.W, &sy, &sx);
            Sample so[3], ss[3];
            const int n = pixel_samples(o.batch, x, y, so);
            pixel_samples(b, sx, sy, ss);
            for (int q = 0; q < n; ++q) {
                if (ss[q].off + ss[q].len > extent || so[q].off + so[q].len > O.size()) { FAIL("%s: a sample outside its frame", t->name); continue; }
                memcpy(&O[so[q].off], frame + ss[q].off, so[q].len);
            }
        }
    const StagePlan ref = stage_plan(o.batch, cr);
    const size_t stride = ref.staged.frame_stride;
    std::vector<uint8_t> want(stride, 0xA5);
    for (int k = 0; k < ref.runs.count; ++k)
        for (uint32_t y = 0; y < ref.runs.run[k].rows; ++y)
            memcpy(&want[ref.runs.run[k].dst_off + (size_t)y * ref.runs.run[k].dst_pitch], &O[ref.runs.run[k].src_off + (size_t)y * ref.runs.run[k].src_pitch],
                   ref.runs.run[k].row_bytes);
    // (b) the kernel's walk
    const orient::Plan op = orient::oriented_plan(b, code, cr);
    if (memcmp(&op.sp.staged, &ref.staged, sizeof ref.staged) || memcmp(op.sp.rect, ref.rect, sizeof ref.rect) || op.sp.items != ref.items ||
        op.runs.count != ref.runs.count || op.runs.extent != extent)
        FAIL("%s: the oriented plan's destination side is not stage_plan's of the oriented geometry", t->name);
    uint8_t* staged = (uint8_t*)malloc(stride);
    memset(staged, 0xA5, stride);
    std::vector<uint8_t> writes(stride, 0);
    const Access a = {frame, extent, staged, stride, &writes};
    orient_frame(a, op.runs, t);
    // (c) the host packer's elements
    std::vector<uint8_t> packed(stride, 0xA5);
    for (int k = 0; k < op.runs.count; ++k) {
        const orient::Run& r = op.runs.run[k];
        for (uint32_t y = 0; y < r.rows; ++y)
            for (uint32_t x = 0; x < r.cols; ++x) {
                const uint64_t off = orient::elem_src_off(r, code, y, x);
                if (off + r.eb > extent) { FAIL("%s: element source [%llu, +%u) outside the extent", t->name, (unsigned long long)off, r.eb); continue; }
                memcpy(&packed[r.dst_off + (size_t)y * r.dst_pitch + (size_t)x * r.eb], frame + off, r.eb);
            }
    }
    size_t expected_writes = 0;
    for (int k = 0; k < ref.runs.count; ++k) {
        const RowRun& rr = ref.runs.run[k];
        const size_t padded = (rr.row_bytes + 15) / 16 * 16;
        if (op.runs.run[k].dst_off != rr.dst_off || op.runs.run[k].dst_pitch != rr.dst_pitch || op.runs.run[k].rows != rr.rows ||
            (size_t)op.runs.run[k].cols * op.runs.run[k].eb != rr.row_bytes)
            FAIL("%s: run %d differs from the plan's", t->name, k);
        for (uint32_t y = 0; y < rr.rows; ++y) {
            const size_t at = rr.dst_off + (size_t)y * rr.dst_pitch;
            if (memcmp(staged + at, &want[at], rr.row_bytes)) FAIL("%s code %d: run %d row %u differs (H %d W %d rect %d %d %d %d)", t->name, code, k, y, b.H, b.W, rect[0], rect[1], rect[2], rect[3]);
            if (memcmp(&packed[at], &want[at], rr.row_bytes)) FAIL("%s code %d: run %d row %u of the host packer differs", t->name, code, k, y);
            for (size_t q = 0; q < padded; ++q) {
                if (writes[at + q] != 1) { FAIL("%s code %d: run %d row %u byte %zu written %d times", t->name, code, k, y, q, writes[at + q]); break; }
                if (q >= rr.row_bytes && staged[at + q] != 0) { FAIL("%s: a byte behind a row's end is not zero", t->name); break; }
            }
            expected_writes += padded;
        }
    }
    size_t total = 0;
    for (uint8_t w : writes) total += w;
    if (total != expected_writes) FAIL("%s code %d: %zu bytes stored, the runs' pieces hold %zu", t->name, code, total, expected_writes);
    free(staged);
    free(alloc);
}

// rectangles of the oriented W x H frame: the whole frame, odd and even origins, touching its edges and inside it
template <class F>
static void each_rect(int W, int H, F f)
{
    const int rects[9][4] = {{0, 0, W, H}, {1, 1, W, H}, {1, 1, W - 1, H - 1}, {0, 0, W - 1, H - 1}, {3, 1, W, H - 1}, {1, 3, W - 1, H},
                             {2, 2, W - 2, H - 2}, {0, 1, W - 3, H}, {5, 3, W - 2, H - 1}};
    for (const int* r : rects)
        if (r[2] > r[0] && r[3] > r[1]) f(r);
}
static const int SIZES[][2] = {{2, 2}, {4, 6}, {6, 4}, {10, 14}, {22, 10}, {66, 6}, {6, 66}, {70, 66}, {64, 130}, {130, 70}};   // H, W

template <class Desc>
static void sweep_desc(Tally* t, Desc d, const char* (*check)(const void*, const Desc*, FrameBatch*), unsigned align, long* counter)
{
    FrameBatch b;
    d.n = 1;
    if (const char* msg = check((const void*)(uintptr_t)64, &d, &b)) { FAIL("%s: the sweep's descriptor is not taken: %s", t->name, msg); return; }
    if (!orient::orientable(b, 0) || !orient::orientable(b, 9) || !orient::orientable(b, -1)) FAIL("%s: a code outside 1 .. 8 is taken", t->name);
    for (int code = 1; code <= 8; ++code) {
        // what the header says is taken
        bool taken = true;
        if (code >= 5 && b.lay.pix == PIX_YUVP) taken = b.lay.yuvp.sub_x == b.lay.yuvp.sub_y;
        if (code >= 5 && b.lay.pix == PIX_YUV16) taken = b.lay.y16.sub_y == 1;
        if ((orient::orientable(b, code) == nullptr) != taken) FAIL("%s code %d: orientable() disagrees with the header", t->name, code);
        if (!taken) { ++t->rejected[code]; continue; }
        each_rect(orient::oriented_w(b, code), orient::oriented_h(b, code), [&](const int* rect) {
            const size_t phases = align >= 16 ? 1 : 16 / align;
            const size_t phase = (size_t)((*counter)++ % (long)phases) * align;
            run_case(b, code, rect, phase, t);
        });
    }
}

int main()
{
    Tally tal[6] = {{"frames"}, {"yuv"}, {"yuv_planar"}, {"yuv16"}, {"packed32"}, {"planes"}};
    long counter = 0;
    for (const int* hw : SIZES) {
        const int H = hw[0], W = hw[1];
        for (int pad = 0; pad < 2; ++pad) {
            for (int pf = MELF_PIX_BGR; pf <= MELF_PIX_RGBA; ++pf) {
                const int bpp = pf >= MELF_PIX_BGRA ? 4 : 3;
                melf_frames d = {pf, 1, H, W, (int64_t)W * bpp + (pad ? (bpp == 4 ? 12 : 7) : 0), 0};
                d.frame_stride = (H - 1) * d.row_pitch + (int64_t)W * bpp;
                sweep_desc(&tal[0], d, check_frames, bpp == 4 ? 4 : 1, &counter);
            }
            for (int v = 0; v < 3; ++v) {   // NV12, I420, YV12
                const bool nv12 = v == 0;
                const int64_t yp = W + (pad ? 5 : 0), cp = (nv12 ? W : W / 2) + (pad ? 3 : 0), c0 = yp * H + (pad ? 6 : 0);
                const int64_t clen = (int64_t)(H / 2 - 1) * cp + (nv12 ? W : W / 2);
                melf_yuv_frames d = {nv12 ? MELF_YUV_NV12 : MELF_YUV_I420, MELF_YUV_BT601_LIMITED, 1, H, W, 0, yp, cp,
                                     nv12 ? c0 : (v == 1 ? c0 : c0 + clen + pad), nv12 ? c0 + 1 : (v == 1 ? c0 + clen + pad : c0), 0};
                d.frame_stride = c0 + 2 * clen + 2;
                sweep_desc(&tal[1], d, check_yuv, 1, &counter);
            }
            for (int sx = 0; sx < 2; ++sx)
                for (int sy = 0; sy < 2; ++sy)
                    for (int step = 1; step <= 2; ++step) {
                        const int vfirst = (int)(counter & 1);
                        const int64_t yp = W + (pad ? 5 : 0), cs = W >> sx, ch = H >> sy, cp = cs * step + (pad ? 3 : 0), c0 = yp * H + (pad ? 7 : 0);
                        const int64_t clen = (ch - 1) * cp + (cs - 1) * step + 1;
                        const int64_t lo = c0, hi = step == 2 ? c0 + 1 : c0 + clen + pad;
                        melf_yuv_planar_frames d = {0, 1, H, W, sx, sy, step, 0, yp, cp, vfirst ? hi : lo, vfirst ? lo : hi, 0};
                        d.frame_stride = hi + clen;
                        sweep_desc(&tal[2], d, check_yuv_planar, 1, &counter);
                    }
            for (int sy = 0; sy < 2; ++sy)
                for (int step = 1; step <= 2; ++step)
                    for (int vfirst = 0; vfirst < 2; ++vfirst) {
                        const int64_t yp = 2 * W + (pad ? 6 : 0), cs = W >> 1, ch = H >> sy, cp = cs * step * 2 + (pad ? 4 : 0), c0 = yp * H + (pad ? 10 : 0);
                        const int64_t clen = (ch - 1) * cp + ((cs - 1) * step + 1) * 2;
                        const int64_t lo = c0, hi = step == 2 ? c0 + 2 : c0 + clen + 2 * pad;
                        melf_yuv16_frames d = {3, 1, H, W, sy, step, 6, 0, yp, cp, vfirst ? hi : lo, vfirst ? lo : hi, 0};
                        d.frame_stride = hi + clen;
                        sweep_desc(&tal[3], d, check_yuv16, 2, &counter);
                    }
            for (int k = 0; k < 2; ++k) {   // a YUV and an RGB word
                melf_packed32_frames d = {k, k ? 0 : 3, 1, H, W, {k ? 22 : 12, k ? 12 : 2, k ? 2 : 22}, (int64_t)W * 4 + (pad ? 12 : 0), 0, 0, 0};
                d.frame_stride = d.row_pitch * H;
                sweep_desc(&tal[4], d, check_packed32, 4, &counter);
            }
            for (int order = 0; order < 6; order += 2 - pad) {
                static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
                const int64_t rp = W + (pad ? 5 : 0), span = (int64_t)(H - 1) * rp + W, gap = span + (pad ? 3 : 0);
                melf_planar_frames d = {1, H, W, 0, perm[order][0] * gap + pad, perm[order][1] * gap + pad, perm[order][2] * gap + pad, rp, 0};
                d.frame_stride = 2 * gap + pad + span;
                sweep_desc(&tal[5], d, check_planes, 1, &counter);
            }
        }
    }
    // the two packed 4:2:2 families are rejected whatever the code
    {
        FrameBatch b;
        melf_yuv422_frames d = {MELF_YUV422_YUYV, 0, 1, 4, 8, 0, 16, 64};
        melf_yuv422_10_frames e = {MELF_YUV422_10_Y210, 3, 1, 4, 8, 0, 32, 128};
        long rejected = 0;
        if (check_yuv422((const void*)(uintptr_t)64, &d, &b)) FAIL("the packed 4:2:2 descriptor is not taken");
        for (int code = 1; code <= 8; ++code) rejected += orient::orientable(b, code) != nullptr;
        if (check_yuv422_10((const void*)(uintptr_t)64, &e, &b)) FAIL("the packed 10-bit 4:2:2 descriptor is not taken");
        for (int code = 1; code <= 8; ++code) rejected += orient::orientable(b, code) != nullptr;
        printf("packed 4:2:2 families: rejected %ld of 16\n", rejected);
        if (rejected != 16) FAIL("a packed 4:2:2 family is taken");
    }
    for (const Tally& t : tal)
        for (int code = 1; code <= 8; ++code) {
            printf("family %s code %d: cases %ld odd_origin %ld edge %ld rejected %ld tiles %ld tail_loads %ld\n", t.name, code, t.cases[code], t.odd_origin[code],
                   t.edge[code], t.rejected[code], t.tiles[code], t.tail_loads[code]);
            if (t.cases[code] <= 200 || t.odd_origin[code] <= 50 || t.edge[code] <= 50 || t.tail_loads[code] == 0 || t.tiles[code] <= t.cases[code])
                FAIL("family %s code %d: the sweep misses a kind of case", t.name, code);
        }
    printf("failures %ld\n", failures);
    return failures ? 1 : 0;
}
