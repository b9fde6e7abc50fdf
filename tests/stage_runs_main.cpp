// The staging plans of melf_stage_plan.h and the gather kernel's address arithmetic (melf_gather_addr.h), swept on the CPU.
//
// For every family: descriptors the family's check accepts -- W and H from the template's size to 40 beyond it, every format code,
// subsampling, c_step, plane order and shift, padded and unpadded pitches, every base alignment phase the check takes -- and
// rectangles with even and odd origins that touch the frame's first row and column and its last.  A case puts random bytes into a
// malloc of exactly the descriptor's extent at that phase, makes the plan, and executes its row runs the way k_gather_rows does:
// wave by wave, piece by piece, every offset, width and path from the functions the kernel calls.  Then
//   (i)   every source access lies in [0, extent) (and the sanitizer build's red zones say the same),
//   (ii)  every destination access lies inside the staged frame (a malloc of exactly its stride), and no two runs write one byte,
//   (iii) for every pixel of the crop, the samples the public header's addressing gives in the staged frame at the plan's rect are
//         those of the caller's frame at the meter_rect, chroma included, at the same phase inside a macropixel / group / block.
// Prints the cases per family and ends with `failures 0`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../meterelf_amd/csrc/melf_gather_addr.h"

using namespace melf;

static const int TPL_H = 10, TPL_W = 12;   // the "template": the smallest crop
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
    long cases = 0, rejected = 0, odd_origin = 0, edge = 0, tail_pieces = 0, full_pieces = 0, phases = 0;
};

// ---- the kernel's walk over a frame, on the CPU --------------------------------------------------------------------------------
struct Access {
    const uint8_t* frame;
    size_t extent;
    uint8_t* staged;
    size_t stride;
    std::vector<int8_t>* owner;   // per staged byte: the run that wrote it, -1 none
};
template <class T>
static T load_at(const Access& a, uint64_t off)
{
    if (off + sizeof(T) > a.extent) { FAIL("source access [%llu, +%zu) outside the extent %zu", (unsigned long long)off, sizeof(T), a.extent); return T(); }
    T v;
    memcpy(&v, a.frame + off, sizeof(T));
    return v;
}
static void gather_frame(const Access& a, const RowRuns& runs, Tally* t)
{
    const uint32_t waves = gather::frame_waves(runs);
    for (uint32_t w = 0; w < waves; ++w) {
        const gather::WaveRows wr = gather::wave_rows(runs, w);
        int k = -1;
        for (int q = 0; q < runs.count; ++q)
            if (!memcmp(&runs.run[q], &wr.run, sizeof(RowRun))) k = q;
        if (k < 0) { FAIL("wave %u: not a run of the plan", w); continue; }
        const uint32_t ppr = gather::row_pieces(wr.run.row_bytes), total = ppr * wr.nrows;
        for (uint32_t i = 0; i < total; ++i) {   // lane i % 64 in iteration i / 64
            const uint32_t r = i / ppr, piece = i - r * ppr;
            const gather::Piece p = gather::piece_of(wr.run, wr.row0 + r, piece);
            if (!gather::piece_readable(p, a.extent)) { FAIL("run %d row %u piece %u: not readable", k, wr.row0 + r, piece); continue; }
            uint8_t v[16] = {0};
            if (p.bytes == (uint32_t)gather::PIECE) {
                struct B16 { uint8_t b[16]; };
                const B16 x = load_at<B16>(a, p.src_off);
                memcpy(v, x.b, 16);
                ++t->full_pieces;
            } else {
                if (p.bytes == 0 || p.bytes > 15) FAIL("tail piece of %u bytes", p.bytes);
                uint32_t got = 0;
                if (gather::tail_has(p.bytes, 8)) { const uint64_t x = load_at<uint64_t>(a, p.src_off + gather::tail_at(p.bytes, 8)); memcpy(v + gather::tail_at(p.bytes, 8), &x, 8); got += 8; }
                if (gather::tail_has(p.bytes, 4)) { const uint32_t x = load_at<uint32_t>(a, p.src_off + gather::tail_at(p.bytes, 4)); memcpy(v + gather::tail_at(p.bytes, 4), &x, 4); got += 4; }
                if (gather::tail_has(p.bytes, 2)) { const uint16_t x = load_at<uint16_t>(a, p.src_off + gather::tail_at(p.bytes, 2)); memcpy(v + gather::tail_at(p.bytes, 2), &x, 2); got += 2; }
                if (gather::tail_has(p.bytes, 1)) { const uint8_t x = load_at<uint8_t>(a, p.src_off + gather::tail_at(p.bytes, 1)); v[gather::tail_at(p.bytes, 1)] = x; got += 1; }
                if (got != p.bytes) FAIL("tail loads fetch %u of %u bytes", got, p.bytes);
                ++t->tail_pieces;
            }
            if (p.dst_off % 16 || p.dst_off + 16 > a.stride) { FAIL("store at %llu outside the staged frame of %zu bytes (or misaligned)", (unsigned long long)p.dst_off, a.stride); continue; }
            for (int q = 0; q < 16; ++q) {
                int8_t& o = (*a.owner)[p.dst_off + q];
                if (o >= 0 && o != k) FAIL("staged byte %llu written by runs %d and %d", (unsigned long long)p.dst_off + q, o, k);
                if (o == k && (uint32_t)q < p.bytes) FAIL("staged byte %llu written twice", (unsigned long long)p.dst_off + q);
                o = (int8_t)k;
            }
            memcpy(a.staged + p.dst_off, v, 16);
        }
    }
}

// ---- the public header's addressing: the bytes that make pixel (x, y) of a frame of batch b, and its phase inside a unit --------
struct Sample { uint64_t off; int len; };
static int pixel_samples(const FrameBatch& b, int x, int y, Sample s[3], int* phase)
{
    const FrameLayout& L = b.lay;
    const uint64_t rs = (uint64_t)b.row_stride;
    *phase = 0;
    if (pix_yuv(L.pix)) {
        const int step = L.pix == PIX_NV12 ? 2 : 1;
        s[0] = {y * rs + x, 1};
        s[1] = {(uint64_t)L.yuv.u_off + (uint64_t)(y >> 1) * L.yuv.c_pitch + (uint64_t)(x >> 1) * step, 1};
        s[2] = {(uint64_t)L.yuv.v_off + (uint64_t)(y >> 1) * L.yuv.c_pitch + (uint64_t)(x >> 1) * step, 1};
        *phase = (x & 1) | (y & 1) << 1;
        return 3;
    }
    if (pix_p422(L.pix)) { s[0] = {y * rs + 4 * (uint64_t)(x >> 1), 4}; *phase = x & 1; return 1; }
    if (L.pix == PIX_V210) { s[0] = {y * rs + 16 * (uint64_t)(x / 6), 16}; *phase = x % 6; return 1; }
    if (L.pix == PIX_Y210) { s[0] = {y * rs + 8 * (uint64_t)(x >> 1), 8}; *phase = x & 1; return 1; }
    if (pix_p32(L.pix)) { s[0] = {y * rs + 4 * (uint64_t)x, 4}; return 1; }
    if (L.pix == PIX_YUVP) {
        const YuvPlanarPlanes& p = L.yuvp;
        s[0] = {y * rs + x, 1};
        s[1] = {(uint64_t)p.u_off + (uint64_t)(y >> p.sub_y) * p.c_pitch + (uint64_t)(x >> p.sub_x) * p.c_step, 1};
        s[2] = {(uint64_t)p.v_off + (uint64_t)(y >> p.sub_y) * p.c_pitch + (uint64_t)(x >> p.sub_x) * p.c_step, 1};
        *phase = (x & ((1 << p.sub_x) - 1)) | (y & ((1 << p.sub_y) - 1)) << 1;
        return 3;
    }
    if (L.pix == PIX_YUV16) {
        const Yuv16Planes& p = L.y16;
        s[0] = {y * rs + 2 * (uint64_t)x, 2};
        s[1] = {(uint64_t)p.u_off + (uint64_t)(y >> p.sub_y) * p.c_pitch + (uint64_t)(x >> 1) * p.c_step * 2, 2};
        s[2] = {(uint64_t)p.v_off + (uint64_t)(y >> p.sub_y) * p.c_pitch + (uint64_t)(x >> 1) * p.c_step * 2, 2};
        *phase = (x & 1) | (y & ((1 << p.sub_y) - 1)) << 1;
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

// the layout members that must travel unchanged from the caller's frames to the staged ones
static bool same_reading(const FrameLayout& a, const FrameLayout& s)
{
    if (a.pix != s.pix || a.mx != s.mx) return false;
    if (a.pix == PIX_YUVP) return a.yuvp.sub_x == s.yuvp.sub_x && a.yuvp.sub_y == s.yuvp.sub_y && a.yuvp.c_step == s.yuvp.c_step && (a.yuvp.c_step == 1 || (a.yuvp.u_off < a.yuvp.v_off) == (s.yuvp.u_off < s.yuvp.v_off));
    if (a.pix == PIX_YUV16) return a.y16.sub_y == s.y16.sub_y && a.y16.c_step == s.y16.c_step && a.y16.shift == s.y16.shift && (a.y16.c_step == 1 || (a.y16.u_off < a.y16.v_off) == (s.y16.u_off < s.y16.v_off));
    if (pix_p32(a.pix)) return !memcmp(&a.p32, &s.p32, sizeof a.p32);
    if (pix_yuv(a.pix)) return a.pix == PIX_NV12 ? s.yuv.v_off == s.yuv.u_off + 1 : true;
    return true;
}

// ---- one case -------------------------------------------------------------------------------------------------------------------
static void run_case(const FrameBatch& b, const int rect[4], size_t phase, Tally* t)
{
    Crop cr;
    if (!clamp_crop(rect, b.H, b.W, &cr) || cr.rows < TPL_H || cr.cols < TPL_W) { FAIL("%s: bad test rectangle", t->name); return; }
    const StagePlan sp = stage_plan(b, cr);
    const size_t extent = b.lay.extent, stride = sp.staged.frame_stride;
    uint8_t* alloc = (uint8_t*)malloc(extent + phase);   // the frame ends where the allocation ends
    uint8_t* frame = alloc + phase;
    for (size_t i = 0; i < extent; ++i) frame[i] = (uint8_t)rnd();
    uint8_t* staged = (uint8_t*)malloc(stride);
    memset(staged, 0xA5, stride);
    std::vector<int8_t> owner(stride, -1);
    ++t->cases;
    t->odd_origin += (cr.x0 & 1) && (cr.y0 & 1);
    t->edge += (cr.x0 == 0 && cr.y0 == 0) || (cr.x1 == b.W && cr.y1 == b.H);
    t->phases |= 1l << phase;
    // the plan itself
    const RowRuns& rr = sp.runs;
    if (rr.count < 1 || rr.count > STAGE_MAX_RUNS) FAIL("%s: %d runs", t->name, rr.count);
    if (stride % 64 || sp.staged.row_stride % 64)
        FAIL("%s: staged strides not multiples of 64", t->name);
    if (sp.staged.lay.extent > stride) FAIL("%s: staged extent beyond the staged frame", t->name);
    if (!same_reading(b.lay, sp.staged.lay)) FAIL("%s: the staged layout reads differently", t->name);
    if (sp.rect[2] - sp.rect[0] != cr.cols || sp.rect[3] - sp.rect[1] != cr.rows || sp.rect[0] < 0 || sp.rect[1] < 0 || sp.rect[2] > sp.staged.W ||
        sp.rect[3] > sp.staged.H)
        FAIL("%s: rect {%d %d %d %d} in a %d x %d staged frame for a %d x %d crop", t->name, sp.rect[0], sp.rect[1], sp.rect[2], sp.rect[3], sp.staged.W,
             sp.staged.H, cr.cols, cr.rows);
    for (int k = 0; k < rr.count; ++k)
        if (rr.run[k].dst_off % 64 || rr.run[k].dst_pitch % 64 || rr.run[k].row_bytes > rr.run[k].dst_pitch || rr.run[k].rows == 0)
            FAIL("%s: run %d: destination not at a 64-byte pitch", t->name, k);
    // the host packer's work items cover every row of every run once
    {
        std::vector<int> seen[STAGE_MAX_RUNS];
        for (int k = 0; k < rr.count; ++k) seen[k].assign(rr.run[k].rows, 0);
        for (int item = 0; item < sp.items; ++item) {
            int k0, k1; uint32_t r0, r1;
            stage_item(sp, item, &k0, &k1, &r0, &r1);
            for (int k = k0; k < k1; ++k)
                for (uint32_t r = r0; r < r1; ++r) ++seen[k][r];
        }
        for (int k = 0; k < rr.count; ++k)
            for (int c : seen[k])
                if (c != 1) { FAIL("%s: a row of run %d is packed %d times by the work items", t->name, k, c); break; }
    }
    const Access a = {frame, extent, staged, stride, &owner};
    gather_frame(a, rr, t);
    // (iii) pixel by pixel
    for (int y = 0; y < cr.rows && failures < 20; ++y)
        for (int x = 0; x < cr.cols; ++x) {
            Sample so[3], ss[3];
            int po, ps;
            const int no = pixel_samples(b, cr.x0 + x, cr.y0 + y, so, &po), ns = pixel_samples(sp.staged, sp.rect[0] + x, sp.rect[1] + y, ss, &ps);
            if (no != ns || po != ps) { FAIL("%s: pixel (%d, %d): phase %d in the frame, %d in the staged frame", t->name, x, y, po, ps); break; }
            for (int q = 0; q < no; ++q) {
                if (so[q].off + so[q].len > extent || ss[q].off + ss[q].len > sp.staged.lay.extent) { FAIL("%s: pixel (%d, %d): sample outside", t->name, x, y); break; }
                if (memcmp(frame + so[q].off, staged + ss[q].off, so[q].len)) { FAIL("%s: pixel (%d, %d) sample %d differs (W %d H %d rect %d %d %d %d)", t->name, x, y, q, b.W, b.H, rect[0], rect[1], rect[2], rect[3]); break; }
                for (int i = 0; i < ss[q].len; ++i)
                    if (owner[ss[q].off + i] < 0) { FAIL("%s: pixel (%d, %d): staged sample never written", t->name, x, y); break; }
            }
        }
    free(staged);
    free(alloc);
}

// rectangles of a W x H frame: crops of the template's size, a little larger, and the whole frame, at even and odd origins, touching
// the first row and column and the last
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

// A family's sweep: descs(W, H, pad, emit) calls emit(descriptor, check, amask) for every descriptor variant of that size; every
// accepted one is run with every rectangle, the base phase and the padding changing from case to case so that all combinations occur
template <class Desc>
static void sweep_desc(Tally* t, Desc d, const char* (*check)(const void*, const Desc*, FrameBatch*), unsigned align, long* counter)
{
    FrameBatch b;
    d.n = 1;
    if (const char* msg = check((const void*)(uintptr_t)64, &d, &b)) { (void)msg; ++t->rejected; return; }
    each_rect(d.W, d.H, [&](const int* rect) {
        const size_t phases = align >= 16 ? 1 : 16 / align;   // the residues modulo 16 the check takes
        const size_t phase = (size_t)((*counter)++ % (long)phases) * align;
        run_case(b, rect, phase, t);
    });
}

int main()
{
    Tally tal[8] = {{"frames"}, {"yuv"}, {"yuv422"}, {"yuv_planar"}, {"yuv16"}, {"yuv422_10"}, {"packed32"}, {"planes"}};
    long counter = 0;
    for (int wi : WS)
        for (int hi : HS) {
            const int W = TPL_W + wi, H = TPL_H + hi;
            for (int pad = 0; pad < 2; ++pad) {
                // melf_frames: the four pixel formats
                for (int pf = MELF_PIX_BGR; pf <= MELF_PIX_RGBA; ++pf) {
                    const int bpp = pf >= MELF_PIX_BGRA ? 4 : 3;
                    melf_frames d = {pf, 1, H, W, (int64_t)W * bpp + (pad ? (bpp == 4 ? 12 : 7) : 0), 0};
                    d.frame_stride = (H - 1) * d.row_pitch + (int64_t)W * bpp;
                    sweep_desc(&tal[0], d, check_frames, bpp == 4 ? 4 : 1, &counter);
                }
                // melf_yuv_frames: NV12, I420, YV12 (the offsets exchanged), every matrix
                for (int v = 0; v < 3; ++v) {
                    const bool nv12 = v == 0;
                    const int64_t yp = W + (pad ? 5 : 0), cp = (nv12 ? W : W / 2) + (pad ? 3 : 0), c0 = yp * H + (pad ? 6 : 0);
                    const int64_t clen = (int64_t)(H / 2 - 1) * cp + (nv12 ? W : W / 2);
                    static const int matrices[4] = {MELF_YUV_BT601_LIMITED, MELF_YUV_BT601_FULL, MELF_YUV_BT709_LIMITED, MELF_YUV_BT709_FULL};
                    melf_yuv_frames d = {nv12 ? MELF_YUV_NV12 : MELF_YUV_I420, matrices[counter & 3], 1, H, W, 0, yp, cp,
                                         nv12 ? c0 : (v == 1 ? c0 : c0 + clen + pad), nv12 ? c0 + 1 : (v == 1 ? c0 + clen + pad : c0), 0};
                    d.frame_stride = c0 + 2 * clen + 2;
                    sweep_desc(&tal[1], d, check_yuv, 1, &counter);
                }
                // melf_yuv422_frames: the three byte orders
                for (int f = MELF_YUV422_YUYV; f <= MELF_YUV422_YVYU; ++f) {
                    melf_yuv422_frames d = {f, 0, 1, H, W, 0, (int64_t)W * 2 + (pad ? 8 : 0), 0};
                    d.frame_stride = (d.row_pitch * H + 3) & ~3;
                    sweep_desc(&tal[2], d, check_yuv422, 4, &counter);
                }
                // melf_yuv_planar_frames: the four subsamplings, planar and semi-planar, U first and V first
                for (int sx = 0; sx < 2; ++sx)
                    for (int sy = 0; sy < 2; ++sy)
                        for (int step = 1; step <= 2; ++step)
                            for (int vfirst = 0; vfirst < 2; ++vfirst) {
                                const int64_t yp = W + (pad ? 5 : 0), cs = W >> sx, ch = H >> sy, cp = cs * step + (pad ? 3 : 0), c0 = yp * H + (pad ? 7 : 0);
                                const int64_t clen = (ch - 1) * cp + (cs - 1) * step + 1;
                                const int64_t lo = c0, hi = step == 2 ? c0 + 1 : c0 + clen + pad;
                                melf_yuv_planar_frames d = {0, 1, H, W, sx, sy, step, 0, yp, cp, vfirst ? hi : lo, vfirst ? lo : hi, 0};
                                d.frame_stride = hi + clen;
                                sweep_desc(&tal[3], d, check_yuv_planar, 1, &counter);
                            }
                // melf_yuv16_frames: 4:2:0 and 4:2:2, planar and semi-planar, U first and V first, the shifts of the named formats
                for (int sy = 0; sy < 2; ++sy)
                    for (int step = 1; step <= 2; ++step)
                        for (int vfirst = 0; vfirst < 2; ++vfirst) {
                            static const int shifts[4] = {8, 2, 4, 0};
                            const int64_t yp = 2 * W + (pad ? 6 : 0), cs = W >> 1, ch = H >> sy, cp = cs * step * 2 + (pad ? 4 : 0), c0 = yp * H + (pad ? 10 : 0);
                            const int64_t clen = (ch - 1) * cp + ((cs - 1) * step + 1) * 2;
                            const int64_t lo = c0, hi = step == 2 ? c0 + 2 : c0 + clen + 2 * pad;
                            melf_yuv16_frames d = {3, 1, H, W, sy, step, shifts[counter & 3], 0, yp, cp, vfirst ? hi : lo, vfirst ? lo : hi, 0};
                            d.frame_stride = hi + clen;
                            sweep_desc(&tal[4], d, check_yuv16, 2, &counter);
                        }
                // melf_yuv422_10_frames: v210 (16-byte aligned) and Y210 (8-byte aligned)
                for (int f = MELF_YUV422_10_V210; f <= MELF_YUV422_10_Y210; ++f) {
                    const bool v210 = f == MELF_YUV422_10_V210;
                    const int64_t row = v210 ? (int64_t)(W + 5) / 6 * 16 : (int64_t)W * 4;
                    melf_yuv422_10_frames d = {f, 3, 1, H, W, 0, row + (pad ? (v210 ? 32 : 8) : 0), 0};
                    d.frame_stride = d.row_pitch * H;
                    sweep_desc(&tal[5], d, check_yuv422_10, v210 ? 16 : 8, &counter);
                }
                // melf_packed32_frames: YUV and RGB, the positions of the named layouts
                {
                    static const int pos[7][4] = {{0, 16, 8, 0}, {0, 8, 16, 24}, {0, 8, 0, 16}, {0, 12, 2, 22}, {0, 14, 4, 24}, {1, 22, 12, 2}, {1, 2, 12, 22}};
                    for (int k = 0; k < 7; ++k) {
                        melf_packed32_frames d = {pos[k][0], pos[k][0] ? 0 : 3, 1, H, W, {pos[k][1], pos[k][2], pos[k][3]}, (int64_t)W * 4 + (pad ? 12 : 0), 0, 0, 0};
                        d.frame_stride = d.row_pitch * H;
                        sweep_desc(&tal[6], d, check_packed32, 4, &counter);
                    }
                }
                // melf_planar_frames: the six orders of three planes, with and without gaps
                for (int order = 0; order < 6; ++order) {
                    static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
                    const int64_t rp = W + (pad ? 5 : 0), span = (int64_t)(H - 1) * rp + W, gap = span + (pad ? 3 : 0);
                    melf_planar_frames d = {1, H, W, 0, perm[order][0] * gap + pad, perm[order][1] * gap + pad, perm[order][2] * gap + pad, rp, 0};
                    d.frame_stride = 2 * gap + pad + span;
                    sweep_desc(&tal[7], d, check_planes, 1, &counter);
                }
            }
        }
    for (const Tally& t : tal) {
        printf("family %s: cases %ld odd_origin %ld edge %ld rejected %ld full_pieces %ld tail_pieces %ld phases 0x%lx\n", t.name, t.cases, t.odd_origin, t.edge,
               t.rejected, t.full_pieces, t.tail_pieces, t.phases);
        if (t.cases == 0 || t.odd_origin == 0 || t.edge == 0 || t.full_pieces == 0) FAIL("family %s: the sweep misses a kind of case", t.name);
    }
    printf("failures %ld\n", failures);
    return failures ? 1 : 0;
}
