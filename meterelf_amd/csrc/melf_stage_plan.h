// The staging plans of the eight frame families: what the small staged frame of a format looks like -- the meter crop's rows, copied
// as they are, its origin rounded to whole chroma blocks, macropixels or v210 groups where the format needs it -- and the row runs
// that copy a caller's frame into it.  Pure host functions of a checked FrameBatch (melf_frame_checks.h) and the crop: no HIP, no
// context.  Two users, one statement of a format's staged frame: the host-fed path (melf_api.hip: stage_host_frames packs the runs
// on the CPU into pinned memory) and the frame lists (melf_process_frame_list*: k_gather_rows copies the runs of separately
// allocated device frames into a staged batch in HBM).  The kernels then read the staged frames as frames of their own, with the
// rectangle where the plan says.  tests/stage_runs_main.cpp sweeps the plans on the CPU.  The plane lists (melf_process_plane_list*:
// one pointer per PLANE) take the same plans of a canonical one-allocation descriptor and split their runs by plane: the end of this
// file; tests/plane_runs_main.cpp sweeps that.
#pragma once
#include "melf_frame_checks.h"

namespace melf {

// The meter crop of H x W frames: {x0, y0, x1, y1} clamped to the frame as numpy slicing img[y0:y1, x0:x1] clamps
// (meterelf/_image.py:54-55)
struct Crop {
    int x0, y0, x1, y1, rows, cols;
};
// r = {x0, y0, x1, y1}; false: the clamped crop is empty or starts before the frame (the caller also wants it to hold the template)
inline bool clamp_crop(const int* r, int H, int W, Crop* cr)
{
    cr->x0 = r[0] < W ? r[0] : W; cr->x1 = r[2] < W ? r[2] : W;
    cr->y0 = r[1] < H ? r[1] : H; cr->y1 = r[3] < H ? r[3] : H;
    cr->rows = cr->y1 - cr->y0; cr->cols = cr->x1 - cr->x0;
    return cr->x0 >= 0 && cr->y0 >= 0 && cr->rows > 0 && cr->cols > 0;
}

// One run of rows: `rows` rows of row_bytes bytes, from frame + src_off + r * src_pitch to staged + dst_off + r * dst_pitch.  A
// plane of the frame is one run (Y / U / V, Y / UV, B / G / R, or the one packed plane).  dst_off and dst_pitch are multiples of 64;
// src_off and src_pitch have the alignment the family's check leaves the frame's base and pitches.  Every run of a plan reads from
// the one frame pointer; for a frame whose planes lie in separate allocations (melf_process_plane_list*) plane_split, at the end of
// this file, gives each run a pointer slot of its own -- the run's index -- and its offset from that plane's pointer.
struct RowRun {
    uint64_t src_off, dst_off;
    uint32_t src_pitch, dst_pitch;
    uint32_t row_bytes, rows;
};
constexpr int STAGE_MAX_RUNS = 3;
struct RowRuns {
    RowRun run[STAGE_MAX_RUNS];
    int count;
};

struct StagePlan {
    FrameBatch staged;   // the staged frames as the kernels read them (n: set per chunk); frame_stride: bytes of a staged frame,
                         // rows at a 64-byte pitch, + 128 spare bytes (the prep kernel's aligned windows reach past the last sample)
    int rect[4];         // the meter crop inside a staged frame
    int items;           // the host packer's work items per frame: blocks of 32 rows (see stage_item)
    RowRuns runs;        // the rows of the caller's frame that make a staged frame
};

inline size_t pitch64(size_t row_bytes) { return (row_bytes + 63) & ~(size_t)63; }
inline RowRun row_run(size_t src_off, size_t src_pitch, size_t dst_off, size_t dst_pitch, size_t row_bytes, int rows)
{
    return RowRun{(uint64_t)src_off, (uint64_t)dst_off, (uint32_t)src_pitch, (uint32_t)dst_pitch, (uint32_t)row_bytes, (uint32_t)rows};
}

// One packed plane (the pixel layouts of melf_frames, packed 4:2:2, packed 10-bit 4:2:2, 32-bit packed 4:4:4): the staged frame is
// the crop's rows from pixel ex0 on, sw pixels wide, unit_bytes per unit_px pixels, no vertical rounding.  Work items: the rows in
// blocks of 32.
inline StagePlan one_plane_plan(const FrameBatch& b, const Crop& cr, int ex0, int sw, int unit_px, int unit_bytes, const FrameLayout& lay_of_extent0)
{
    const int crows = cr.rows;
    const size_t rbytes = (size_t)(sw / unit_px) * unit_bytes, x_off = (size_t)(ex0 / unit_px) * unit_bytes;
    const size_t pitch = pitch64(rbytes);
    FrameLayout lay = lay_of_extent0;
    lay.extent = crows * pitch;
    StagePlan sp = {{0, crows, sw, crows * pitch + 128, (int)pitch, lay}, {cr.x0 - ex0, 0, cr.x0 - ex0 + cr.cols, crows}, (crows + 31) / 32, {}};
    sp.runs.count = 1;
    sp.runs.run[0] = row_run((size_t)cr.y0 * (size_t)b.row_stride + x_off, (size_t)b.row_stride, 0, pitch, rbytes, crows);
    return sp;
}

// The pixel layouts of melf_process_batch / melf_process_frames: the staged frame is the crop, its rows (cols * bytes per pixel, read
// at the caller's row pitch) packed as they are at a 64-byte pitch
inline StagePlan packed_plan(const FrameBatch& b, const Crop& cr)
{
    return one_plane_plan(b, cr, cr.x0, cr.cols, 1, pix_bytes(b.lay.pix), FrameLayout::packed(b.lay.pix, 0));
}

// Packed YUV 4:2:2: a small frame of the same format, the rows of the crop (every row has its own chroma), its x origin rounded down
// and its far corner up to even, i.e. to whole macropixels (inside the frame: W is even); the kernels read it with the rectangle
// shifted by the rounding (0 or 1 pixel), under the caller's matrix
inline StagePlan p422_plan(const FrameBatch& b, const Crop& cr)
{
    const int ex0 = cr.x0 & ~1;
    return one_plane_plan(b, cr, ex0, ((cr.x1 + 1) & ~1) - ex0, 2, 4, FrameLayout::yuv422(b.lay.pix, *b.lay.mx, 0));
}

// Packed 10-bit YUV 4:2:2 (v210, Y210): as p422_plan, the x origin rounded down and the far corner up to whole groups of 6 pixels
// (v210: rows hold whole groups, so the far corner stays inside the row) or whole macropixels (Y210)
inline StagePlan yuv422_10_plan(const FrameBatch& b, const Crop& cr)
{
    const bool v210 = b.lay.pix == PIX_V210;
    const int unit = v210 ? 6 : 2;
    const int ex0 = cr.x0 / unit * unit;
    return one_plane_plan(b, cr, ex0, (cr.x1 + unit - 1) / unit * unit - ex0, unit, v210 ? 16 : 8, FrameLayout::yuv422_10(b.lay.pix, *b.lay.mx, 0));
}

// 32-bit packed 4:4:4 (AYUV, Y410, X2RGB10 ..): the staged frame is the crop, its rows of words at a 64-byte pitch (4-byte aligned
// like the caller's), read under the same positions and matrix
inline StagePlan packed32_plan(const FrameBatch& b, const Crop& cr)
{
    return one_plane_plan(b, cr, cr.x0, cr.cols, 1, 4, FrameLayout::packed32(b.lay.pix, b.lay.p32, b.lay.mx, 0));
}

// Planar / semi-planar YUV of any subsampling and sample size (4:2:0 of melf_yuv_frames, melf_yuv_planar_frames, melf_yuv16_frames):
// a small frame of the same layout -- the same subsampling, sample step and order of U and V, and for 16-bit samples the same shift --,
// the Y rows of the crop with its origin rounded down (and its far corner up) to whole chroma blocks (1 << sub_x by 1 << sub_y; inside
// the frame: W and H are whole blocks) and the chroma rows under them; the kernels read it with the rectangle shifted by the rounding
// (0 or 1 pixel each way), under the caller's matrix.  Semi-planar: the interleaved pairs are one run from the lower of the two
// offsets.  Work items: the Y rows in blocks of 32, and the chroma rows as one more.
// bps: bytes per sample; step: samples from one sample of a chroma plane to the next; u_off, v_off, c_pitch: the source's, in
// bytes; layout(u_off, v_off, c_pitch, extent): the small frame's FrameLayout, the source's with these four replaced.
template <class MakeLayout>
inline StagePlan yuv_planes_plan(const FrameBatch& b, const Crop& cr, int bps, int sx, int sy, int step, int64_t u_off, int64_t v_off, int c_pitch,
                                 MakeLayout layout)
{
    const bool semi = step == 2;
    const size_t y_pitch = (size_t)b.row_stride;
    const int bx = 1 << sx, by = 1 << sy;
    const int ex0 = cr.x0 & ~(bx - 1), ey0 = cr.y0 & ~(by - 1);
    const int sw = ((cr.x1 + bx - 1) & ~(bx - 1)) - ex0, sh = ((cr.y1 + by - 1) & ~(by - 1)) - ey0;
    const int crows = sh >> sy;                                      // chroma rows of the small frame
    const size_t ybytes = (size_t)sw * (size_t)bps, ypitch = pitch64(ybytes);
    const size_t cbytes = (size_t)(sw >> sx) * (size_t)step * (size_t)bps;   // bytes of a chroma row (semi-planar: of both)
    const size_t cpitch = pitch64(cbytes);
    const size_t c0 = (size_t)sh * ypitch;                           // the first chroma byte of the small frame
    const int64_t src_lo = u_off < v_off ? u_off : v_off;
    const int64_t su_off = semi ? (int64_t)c0 + (u_off - src_lo) : (int64_t)c0;
    const int64_t sv_off = semi ? (int64_t)c0 + (v_off - src_lo) : (int64_t)(c0 + (size_t)crows * cpitch);
    const size_t crop_stride = c0 + (size_t)crows * cpitch * (semi ? 1 : 2) + 128;
    StagePlan sp = {{0, sh, sw, crop_stride, (int)ypitch, layout(su_off, sv_off, (int)cpitch, crop_stride)},
                    {cr.x0 - ex0, cr.y0 - ey0, cr.x0 - ex0 + cr.cols, cr.y0 - ey0 + cr.rows}, (sh + 31) / 32 + 1, {}};
    const size_t cx = (size_t)(ex0 >> sx) * (size_t)step * (size_t)bps;
    const size_t crow0 = (size_t)(ey0 >> sy) * (size_t)c_pitch + cx;
    sp.runs.run[0] = row_run((size_t)ey0 * y_pitch + (size_t)ex0 * (size_t)bps, y_pitch, 0, ypitch, ybytes, sh);
    if (semi) {
        sp.runs.count = 2;
        sp.runs.run[1] = row_run((size_t)src_lo + crow0, (size_t)c_pitch, c0, cpitch, cbytes, crows);
    } else {
        sp.runs.count = 3;
        sp.runs.run[1] = row_run((size_t)u_off + crow0, (size_t)c_pitch, (size_t)su_off, cpitch, cbytes, crows);
        sp.runs.run[2] = row_run((size_t)v_off + crow0, (size_t)c_pitch, (size_t)sv_off, cpitch, cbytes, crows);
    }
    return sp;
}

// YUV 4:2:0 of melf_yuv_frames (NV12: v_off == u_off + 1; I420 / YV12: two planes)
inline StagePlan yuv420_plan(const FrameBatch& b, const Crop& cr)
{
    const int pix = b.lay.pix;
    const YuvMatrix* mx = b.lay.mx;
    const YuvPlanes src = b.lay.yuv;
    return yuv_planes_plan(b, cr, 1, 1, 1, pix == PIX_NV12 ? 2 : 1, src.u_off, src.v_off, src.c_pitch,
                           [=](int64_t u_off, int64_t v_off, int c_pitch, size_t stride) {
                               const YuvPlanes p = {u_off, v_off, c_pitch, 0};
                               return FrameLayout::yuv420(pix, p, *mx, stride);
                           });
}

inline StagePlan yuv_planar_plan(const FrameBatch& b, const Crop& cr)
{
    const YuvPlanarPlanes src = b.lay.yuvp;
    const YuvMatrix* mx = b.lay.mx;
    return yuv_planes_plan(b, cr, 1, src.sub_x, src.sub_y, src.c_step, src.u_off, src.v_off, src.c_pitch,
                           [=](int64_t u_off, int64_t v_off, int c_pitch, size_t stride) {
                               YuvPlanarPlanes p = src;
                               p.u_off = u_off; p.v_off = v_off; p.c_pitch = c_pitch;
                               return FrameLayout::yuv_planar(p, *mx, stride);
                           });
}

// 16-bit samples: sub_x is 1, the sample 2 bytes
inline StagePlan yuv16_plan(const FrameBatch& b, const Crop& cr)
{
    const Yuv16Planes src = b.lay.y16;
    const YuvMatrix* mx = b.lay.mx;
    return yuv_planes_plan(b, cr, 2, 1, src.sub_y, src.c_step, src.u_off, src.v_off, src.c_pitch,
                           [=](int64_t u_off, int64_t v_off, int c_pitch, size_t stride) {
                               Yuv16Planes p = src;
                               p.u_off = u_off; p.v_off = v_off; p.c_pitch = c_pitch;
                               return FrameLayout::yuv16(p, *mx, stride);
                           });
}

// Planar RGB: a small planar frame, the crop's rows of the B, the G and the R plane, one plane after the other, which the kernels
// read with the rectangle at its origin.  Work items: the crop's rows of one plane in blocks of 32.
inline StagePlan planar_plan(const FrameBatch& b, const Crop& cr)
{
    const int crows = cr.rows, ccols = cr.cols;
    const size_t row_pitch = (size_t)b.row_stride, pitch = pitch64((size_t)ccols), plane = (size_t)crows * pitch;
    const size_t crop_stride = 3 * plane + 128;
    const PlanarPlanes in_frame = {0, (int64_t)plane, (int64_t)(2 * plane)};
    const int rblocks = (crows + 31) / 32;
    StagePlan sp = {{0, crows, ccols, crop_stride, (int)pitch, FrameLayout::planar(in_frame, crop_stride)}, {0, 0, ccols, crows}, 3 * rblocks, {}};
    const int64_t src_off[3] = {b.lay.planes.b_off, b.lay.planes.g_off, b.lay.planes.r_off};
    sp.runs.count = 3;
    for (int p = 0; p < 3; ++p)
        sp.runs.run[p] = row_run((size_t)src_off[p] + (size_t)cr.y0 * row_pitch + (size_t)cr.x0, row_pitch, (size_t)p * plane, pitch, (size_t)ccols, crows);
    return sp;
}

// The plan of a checked batch of any family, by its layout's pix
inline StagePlan stage_plan(const FrameBatch& b, const Crop& cr)
{
    const int pix = b.lay.pix;
    if (pix_yuv(pix)) return yuv420_plan(b, cr);
    if (pix_p422(pix)) return p422_plan(b, cr);
    if (pix_p10(pix)) return yuv422_10_plan(b, cr);
    if (pix_p32(pix)) return packed32_plan(b, cr);
    if (pix == PIX_YUVP) return yuv_planar_plan(b, cr);
    if (pix == PIX_YUV16) return yuv16_plan(b, cr);
    if (pix == PIX_PLANAR) return planar_plan(b, cr);
    return packed_plan(b, cr);
}

// Work item `item` (0 .. items - 1) of a plan as rows of its runs: the rows [*r0, *r1) of the runs [*k0, *k1).  Plans of one run
// per 32-row block and run (packed: items == blocks; planar RGB: 3 x blocks) give one run's block; the YUV plans (items == the Y
// blocks + 1) give a Y block, or as the last item every row of the chroma runs.
inline void stage_item(const StagePlan& sp, int item, int* k0, int* k1, uint32_t* r0, uint32_t* r1)
{
    const RowRuns& rr = sp.runs;
    const int rblocks = (int)((rr.run[0].rows + 31) / 32);
    if (sp.items == rblocks + 1 && rr.count > 1 && item == rblocks) {
        *k0 = 1; *k1 = rr.count; *r0 = 0; *r1 = rr.run[1].rows;
        return;
    }
    const int k = item / rblocks, part = item - k * rblocks;
    *k0 = k; *k1 = k + 1;
    *r0 = (uint32_t)part * 32;
    *r1 = *r0 + 32 < rr.run[k].rows ? *r0 + 32 : rr.run[k].rows;
}

// ---- a frame's planes in separate allocations (melf_process_plane_list*) ----
// The caller's descriptor gives the geometry of one frame whose planes each have a pointer of their own: the plane offsets in it
// count from the plane's OWN pointer.  plane_list_check turns it into the canonical one-allocation descriptor of the same geometry --
// the planes back to back, each from an even offset --, runs the family's unchanged check on that, and leaves the batch, the
// canonical offset of every plane slot and the bytes readable from every plane's pointer.  The plan of that batch (stage_plan) has
// one run per plane, run k reading plane slot k; plane_split restates the runs' source offsets from the planes' own pointers.
// Slots: 0 = Y, 1 = the U plane or the one interleaved chroma plane, 2 = the V plane; melf_planar_frames: 0 / 1 / 2 = B / G / R.
struct PlaneList {
    FrameBatch batch;                      // the canonical one-allocation batch; n: the list's length
    int nplanes;                           // pointers per frame: 2 (Y and interleaved chroma) or 3
    unsigned align;                        // every plane pointer is a multiple of this: 2 for 16-bit samples, 1 otherwise
    uint64_t offset[STAGE_MAX_RUNS];       // slot k's first byte in the canonical frame
    uint64_t extent[STAGE_MAX_RUNS];       // bytes readable from slot k's pointer: (rows - 1) * pitch + the bytes of a row
};
// Run k of a plan as k_plane_rows and the host packer read it: from plane slot k, src_off[k] bytes behind that plane's pointer, of
// which extent[k] bytes are readable
struct PlaneSplit {
    uint64_t src_off[STAGE_MAX_RUNS], extent[STAGE_MAX_RUNS];
    int count;
};
inline PlaneSplit plane_split(const RowRuns& runs, const PlaneList& pl)
{
    PlaneSplit ps = {};
    ps.count = runs.count;
    for (int k = 0; k < STAGE_MAX_RUNS; ++k)
        if (k < runs.count) {
            ps.src_off[k] = runs.run[k].src_off - pl.offset[k];
            ps.extent[k] = pl.extent[k];
        }
    return ps;
}

constexpr const char* PLANE_LIST_ONE_PLANE =
    "frames of this family have one plane: a list of such frames goes through melf_process_frame_list*";
constexpr const char* PLANE_LIST_UNKNOWN_FAMILY =
    "unknown family of the plane list (accepted: MELF_LIST_YUV, MELF_LIST_YUV_PLANAR, MELF_LIST_YUV16, MELF_LIST_PLANES)";
constexpr const char* PLANE_LIST_PLANAR_OFFSETS =
    "plane offsets of a plane list count from the plane's own pointer: every offset of a planar layout must be 0";
constexpr const char* PLANE_LIST_SEMI_OFFSETS =
    "plane offsets of a plane list count from the plane's own pointer: a semi-planar layout needs {u_offset, v_offset} = {0, bytes "
    "per sample} or the reverse";
constexpr const char* PLANE_LIST_NPLANES =
    "nplanes does not fit the descriptor: 2 for NV12 and c_step 2 (Y and the interleaved chroma plane), 3 otherwise";

// The Y / chroma geometry of the three YUV descriptors -> the canonical offsets.  H, W, the pitches and the chroma shape are used
// only where they are in range (the family's check, run on the result, rejects them otherwise, whatever the offsets): 0 elsewhere.
struct PlaneGeom {
    int64_t y_end, c0, c1, c_extent;
};
inline PlaneGeom yuv_plane_geom(int H, int W, int64_t y_pitch, int64_t c_pitch, int c_rows, int c_samples, int step, int bps)
{
    PlaneGeom g = {0, 0, 0, 0};
    if (H <= 0 || W <= 0 || y_pitch < 0 || y_pitch > INT32_MAX || c_pitch < 0 || c_pitch > INT32_MAX || c_rows <= 0 || c_samples <= 0) return g;
    g.y_end = plane_span(H, y_pitch, W, 1, bps);
    g.c0 = (g.y_end + 1) & ~(int64_t)1;
    g.c_extent = (int64_t)(c_rows - 1) * c_pitch + (int64_t)c_samples * step * bps;
    g.c1 = g.c0 + ((g.c_extent + 1) & ~(int64_t)1);
    return g;
}
// Fills the canonical offsets of a YUV descriptor copy *d (u_offset / v_offset, frame_stride, n) from the caller's; vfirst: V is the
// first sample of an interleaved pair
template <class Desc>
inline void yuv_canonical(Desc* d, const PlaneGeom& g, bool semi, bool vfirst, int bps)
{
    d->u_offset = semi ? g.c0 + (vfirst ? bps : 0) : g.c0;
    d->v_offset = semi ? g.c0 + (vfirst ? 0 : bps) : g.c1;
    d->frame_stride = INT64_MAX & ~(int64_t)15;   // as the frame lists: a stride every check takes
    d->n = d->n > 0 ? 1 : d->n;
}
inline void yuv_plane_slots(PlaneList* pl, const PlaneGeom& g, bool semi)
{
    pl->nplanes = semi ? 2 : 3;
    pl->offset[0] = 0; pl->offset[1] = (uint64_t)g.c0; pl->offset[2] = semi ? 0 : (uint64_t)g.c1;
    pl->extent[0] = (uint64_t)g.y_end; pl->extent[1] = (uint64_t)g.c_extent; pl->extent[2] = semi ? 0 : (uint64_t)g.c_extent;
}

// family: MELF_LIST_*; desc: the family's descriptor with the plane offsets counted from each plane's own pointer; nplanes: the
// caller's.  Returns the error message, or nullptr with *pl filled (n == 0 passes).  The pointers themselves -- NULL, pl->align --
// are the caller's to check: it knows their indices.
inline const char* plane_list_check(int family, const void* desc, int nplanes, PlaneList* pl)
{
    const void* const base = (const void*)(uintptr_t)64;   // a pointer that breaks no family's rule
    *pl = PlaneList{};
    pl->align = 1;
    switch (family) {
    case MELF_LIST_FRAMES: case MELF_LIST_YUV422: case MELF_LIST_YUV422_10: case MELF_LIST_PACKED32: return PLANE_LIST_ONE_PLANE;
    case MELF_LIST_YUV: {
        if (!desc) return check_yuv(nullptr, nullptr, &pl->batch);
        melf_yuv_frames d = *(const melf_yuv_frames*)desc;
        const int n = d.n;
        const bool semi = d.format == MELF_YUV_NV12;
        const int64_t u = d.u_offset, v = d.v_offset;
        const PlaneGeom g = yuv_plane_geom(d.H, d.W, d.y_pitch, d.c_pitch, d.H / 2, d.W / 2, semi ? 2 : 1, 1);
        yuv_canonical(&d, g, semi, false, 1);
        if (const char* msg = check_yuv(base, &d, &pl->batch)) return msg;
        if (semi ? (u != 0 || v != 1) : (u != 0 || v != 0)) return semi ? PLANE_LIST_SEMI_OFFSETS : PLANE_LIST_PLANAR_OFFSETS;
        yuv_plane_slots(pl, g, semi);
        pl->batch.n = n;
        break;
    }
    case MELF_LIST_YUV_PLANAR: {
        if (!desc) return check_yuv_planar(nullptr, nullptr, &pl->batch);
        melf_yuv_planar_frames d = *(const melf_yuv_planar_frames*)desc;
        const int n = d.n;
        const bool semi = d.c_step == 2, vfirst = d.v_offset < d.u_offset;
        const int64_t u = d.u_offset, v = d.v_offset;
        const bool subs = (d.sub_x == 0 || d.sub_x == 1) && (d.sub_y == 0 || d.sub_y == 1);
        const PlaneGeom g = yuv_plane_geom(d.H, d.W, d.y_pitch, d.c_pitch, subs ? d.H >> d.sub_y : 0, subs ? d.W >> d.sub_x : 0, semi ? 2 : 1, 1);
        yuv_canonical(&d, g, semi, vfirst, 1);
        if (const char* msg = check_yuv_planar(base, &d, &pl->batch)) return msg;
        if (semi ? !((u == 0 && v == 1) || (u == 1 && v == 0)) : (u != 0 || v != 0)) return semi ? PLANE_LIST_SEMI_OFFSETS : PLANE_LIST_PLANAR_OFFSETS;
        yuv_plane_slots(pl, g, semi);
        pl->batch.n = n;
        break;
    }
    case MELF_LIST_YUV16: {
        if (!desc) return check_yuv16(nullptr, nullptr, &pl->batch);
        melf_yuv16_frames d = *(const melf_yuv16_frames*)desc;
        const int n = d.n;
        const bool semi = d.c_step == 2, vfirst = d.v_offset < d.u_offset;
        const int64_t u = d.u_offset, v = d.v_offset;
        const bool subs = d.sub_y == 0 || d.sub_y == 1;
        const PlaneGeom g = yuv_plane_geom(d.H, d.W, d.y_pitch, d.c_pitch, subs ? d.H >> d.sub_y : 0, d.W >> 1, semi ? 2 : 1, 2);
        yuv_canonical(&d, g, semi, vfirst, 2);
        if (const char* msg = check_yuv16(base, &d, &pl->batch)) return msg;
        if (semi ? !((u == 0 && v == 2) || (u == 2 && v == 0)) : (u != 0 || v != 0)) return semi ? PLANE_LIST_SEMI_OFFSETS : PLANE_LIST_PLANAR_OFFSETS;
        yuv_plane_slots(pl, g, semi);
        pl->align = 2;
        pl->batch.n = n;
        break;
    }
    case MELF_LIST_PLANES: {
        if (!desc) return check_planes(nullptr, nullptr, &pl->batch);
        melf_planar_frames d = *(const melf_planar_frames*)desc;
        const int n = d.n;
        const bool zero = d.b_offset == 0 && d.g_offset == 0 && d.r_offset == 0;
        const bool in_range = d.H > 0 && d.W > 0 && d.row_pitch >= 0 && d.row_pitch <= INT32_MAX;
        const int64_t span = in_range ? plane_span(d.H, d.row_pitch, d.W, 1, 1) : 0;
        d.b_offset = 0; d.g_offset = span; d.r_offset = 2 * span;
        d.frame_stride = INT64_MAX & ~(int64_t)15;
        d.n = n > 0 ? 1 : n;
        if (const char* msg = check_planes(base, &d, &pl->batch)) return msg;
        if (!zero) return PLANE_LIST_PLANAR_OFFSETS;
        pl->nplanes = 3;
        for (int k = 0; k < 3; ++k) { pl->offset[k] = (uint64_t)(k * span); pl->extent[k] = (uint64_t)span; }
        pl->batch.n = n;
        break;
    }
    default: return PLANE_LIST_UNKNOWN_FAMILY;
    }
    if (nplanes != pl->nplanes) return PLANE_LIST_NPLANES;
    return nullptr;
}

// ---- planar frames of WIDE samples whose planes lie in separate allocations (melf_process_wide_plane_list*) ----
// The wide descriptor in the plane lists' way: MELF_WIDE_PLANAR only, b_ / g_ / r_offset counted from each plane's own pointer (0),
// three pointers per frame, slots 0 / 1 / 2 = B / G / R.  The canonical one-allocation descriptor -- the planes back to back -- goes
// through the unchanged check_wide (its messages WIDE_MESSAGES' own), which leaves the batch IN SAMPLES; so the PlaneList is in
// samples too: offset[k] and extent[k] count samples, plane_split of the batch's plan gives run k's first sample from plane slot k's
// pointer and the samples readable from it, and align is the sample size in bytes.  What is particular to the list has a message
// table of its own; tests/wide_list_main.cpp sweeps the check and counts, through the table, that every message was produced.
struct WidePlaneList {
    WideBatch wb;    // wb.b == pl.batch: the canonical batch, n the list's length
    PlaneList pl;
};
enum WidePlaneListMsg { WPLIST_PACKED, WPLIST_OFFSETS, WPLIST_NPLANES, WPLIST_TABLE_NULL, WPLIST_PTR_NULL, WPLIST_PTR_ALIGN, WPLIST_MSGS };
constexpr const char* WIDE_PLANE_LIST_MESSAGES[WPLIST_MSGS] = {
    "a plane list of wide frames takes MELF_WIDE_PLANAR only: packed wide frames in separate allocations go through melf_process_wide_list*",
    "plane offsets of a wide plane list count from the plane's own pointer: b_offset, g_offset and r_offset must be 0",
    "nplanes of a wide plane list must be 3 (B, G, R)",
    "the wide list's array of plane pointers is NULL",
    "plane pointer of wide frames is NULL",
    "wide frames need plane pointers that are multiples of the sample size",
};
// planes: n * nplanes pointers, frame-major.  Returns the message, or nullptr with *w filled (n == 0 passes).  *bad_frame, *bad_plane:
// -1, or the indices of the pointer the message is about ("frame i, plane k of the list: ").
inline const char* check_wide_plane_list(const melf_wide_frames* f, const void* const* planes, int nplanes, WidePlaneList* w, int* bad_frame,
                                         int* bad_plane)
{
    *bad_frame = *bad_plane = -1;
    *w = WidePlaneList{};
    if (!f) return check_wide(nullptr, nullptr, &w->wb);
    melf_wide_frames d = wide_one_frame(*f);
    const bool planar = d.layout == MELF_WIDE_PLANAR;
    const bool zero = d.b_offset == 0 && d.g_offset == 0 && d.r_offset == 0;
    const bool typed = d.sample_type >= MELF_WIDE_U16 && d.sample_type <= MELF_WIDE_F32;
    const bool in_range = typed && d.H > 0 && d.W > 0 && d.row_pitch >= 0 && d.row_pitch <= INT32_MAX;
    const int64_t span = in_range ? plane_span(d.H, d.row_pitch, d.W, 1, narrow::sample_bytes(d.sample_type)) : 0;   // bytes
    if (planar) { d.b_offset = 0; d.g_offset = span; d.r_offset = 2 * span; }
    if (const char* msg = check_wide((const void*)(uintptr_t)64, &d, &w->wb)) return msg;
    if (!planar) return WIDE_PLANE_LIST_MESSAGES[WPLIST_PACKED];
    if (!zero) return WIDE_PLANE_LIST_MESSAGES[WPLIST_OFFSETS];
    if (nplanes != 3) return WIDE_PLANE_LIST_MESSAGES[WPLIST_NPLANES];
    const int ss = w->wb.ss;
    w->wb.b.n = f->n;
    PlaneList& pl = w->pl;
    pl.batch = w->wb.b;
    pl.nplanes = 3;
    pl.align = (unsigned)ss;
    for (int k = 0; k < 3; ++k) { pl.offset[k] = (uint64_t)(k * (span / ss)); pl.extent[k] = (uint64_t)(span / ss); }
    if (f->n == 0) return nullptr;
    if (!planes) return WIDE_PLANE_LIST_MESSAGES[WPLIST_TABLE_NULL];
    for (int i = 0; i < f->n; ++i)
        for (int k = 0; k < 3; ++k) {
            const void* p = planes[(size_t)i * 3 + k];
            *bad_frame = i; *bad_plane = k;
            if (!p) return WIDE_PLANE_LIST_MESSAGES[WPLIST_PTR_NULL];
            if ((uintptr_t)p & ((uintptr_t)ss - 1)) return WIDE_PLANE_LIST_MESSAGES[WPLIST_PTR_ALIGN];
        }
    *bad_frame = *bad_plane = -1;
    return nullptr;
}

}  // namespace melf
