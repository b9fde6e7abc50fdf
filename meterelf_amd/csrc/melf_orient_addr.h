// Address arithmetic of k_orient_tiles (k_orient.hip): the staged frame of a batch whose stored frames are mirrored or transposed
// (EXIF orientations 1-8, include/meterelf_hip.h: MELF_ORIENT_*), which tile of which run a workgroup takes, what it loads from
// where into its LDS tile and what it stores where.  Plain C++, the sibling of melf_gather_addr.h: the kernel computes its addresses
// with these functions, the host packer of melf_process_oriented uses elem_src_off, and tests/orient_runs_main.cpp executes the same
// functions on the CPU against frames of exact extent.  Source offsets count BYTES from a stored frame's first byte, destination
// offsets from its staged frame.
//
// The destination side is not restated here: oriented_plan describes the ORIENTED frame O as a tight frame of the same family
// (oriented_batch: H' x W', every plane at its tight pitch) and takes stage_plan (melf_stage_plan.h) of it -- the staged frame, the
// rectangle, the layout and the runs' destination side are exactly what the family's plan gives for an upright frame of that
// geometry.  A run of the plan is a rectangle of one plane of O: rows x cols ELEMENTS of eb bytes (1: Y, planar chroma, B / G / R;
// 2: interleaved 8-bit pairs, 16-bit samples; 3: BGR / RGB; 4: BGRA, packed32, 16-bit pairs) from the element (oy0, ox0) of that
// plane, read back from the run's offset in the tight frame.  Element (y, x) of the plane of O is element src_elem(y, x) of the
// stored plane of ph rows x pw elements: the table of the public header, on the plane's own sample grid.
//
// A tile is TILE x TILE elements of a run's destination.  Its source is a rectangle of the stored plane too (tile_of): the
// workgroup loads that rectangle along the STORED rows -- contiguous bytes, in 16-byte pieces from the rectangle's first byte, at
// whatever alignment the stored row has, the last piece of a row by the binary digits of its length as in melf_gather_addr.h -- into
// LDS row by row at a pitch of TILE * eb + 4 bytes (an odd number of dwords: a transposed read walks down a column of the tile and
// meets every bank once), and then reads LDS in destination order: byte j of 16-byte piece p of destination row r is byte
// (16 p + j) % eb of element (16 p + j) / eb, which lies in LDS at lds_map's a0 + r * sr + e * se.  TILE * eb is a multiple of 16,
// so a piece never straddles two tiles and every piece of a destination row is written once; the bytes of a row's last piece behind
// the row's end are written as zeros (they lie in the pitch padding), as k_gather_rows writes them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "melf_stage_plan.h"

#if defined(__HIPCC__)
#define MELF_ORIENT_FN __host__ __device__ __forceinline__
#else
#define MELF_ORIENT_FN inline
#endif

namespace melf {
namespace orient {

constexpr int TILE = 64;       // elements of a tile's edge
constexpr int PIECE = 16;      // bytes of a piece: one 16-byte load / store
constexpr int THREADS = 256;   // of a workgroup: one tile

// O[y][x] = S[row][col] with (a, b) = transposes ? (x, y) : (y, x), row = flips_rows ? ph - 1 - a : a, col = flips_cols ? pw - 1 - b : b
MELF_ORIENT_FN bool transposes(int code) { return code >= MELF_ORIENT_TRANSPOSE; }
MELF_ORIENT_FN bool flips_rows(int code)
{
    return code == MELF_ORIENT_ROT180 || code == MELF_ORIENT_FLIP || code == MELF_ORIENT_ROT90CW || code == MELF_ORIENT_TRANSVERSE;
}
MELF_ORIENT_FN bool flips_cols(int code)
{
    return code == MELF_ORIENT_MIRROR || code == MELF_ORIENT_ROT180 || code == MELF_ORIENT_TRANSVERSE || code == MELF_ORIENT_ROT90CCW;
}

// One run: a rectangle of one plane of the oriented frame, and the stored plane it comes from
struct Run {
    uint64_t src_off, dst_off;       // the stored plane's first byte in a stored frame; the run's first byte in a staged frame
    uint32_t src_pitch, dst_pitch;   // bytes between the stored plane's rows; between the run's staged rows (a multiple of 64)
    uint32_t rows, cols;             // the run: rows x cols elements ...
    uint32_t oy0, ox0;               // ... from this element of the oriented plane
    uint32_t ph, pw;                 // the stored plane: rows, elements per row
    uint32_t eb;                     // bytes of an element: 1 .. 4
    uint32_t pad;
};
struct Runs {
    Run run[STAGE_MAX_RUNS];
    int count;
    int code;          // MELF_ORIENT_*
    uint64_t extent;   // bytes readable from a stored frame's first byte
};

// the stored element that element (y, x) of run r (counted from the run's origin) shows
MELF_ORIENT_FN uint64_t elem_src_off(const Run& r, int code, uint32_t y, uint32_t x)
{
    const uint32_t oy = r.oy0 + y, ox = r.ox0 + x;
    const uint32_t a = transposes(code) ? ox : oy, b = transposes(code) ? oy : ox;
    const uint32_t row = flips_rows(code) ? r.ph - 1 - a : a, col = flips_cols(code) ? r.pw - 1 - b : b;
    return r.src_off + (uint64_t)row * r.src_pitch + (uint64_t)col * r.eb;
}

// ---- the tile decomposition ----
MELF_ORIENT_FN uint32_t tiles_across(const Run& r) { return (r.cols + TILE - 1) / TILE; }
MELF_ORIENT_FN uint32_t run_tiles(const Run& r) { return tiles_across(r) * ((r.rows + TILE - 1) / TILE); }
MELF_ORIENT_FN uint32_t frame_tiles(const Runs& rr)
{
    uint32_t t = 0;
    for (int k = 0; k < STAGE_MAX_RUNS; ++k)
        if (k < rr.count) t += run_tiles(rr.run[k]);
    return t;
}
MELF_ORIENT_FN uint32_t lds_pitch(uint32_t eb) { return TILE * eb + 4; }

// Tile t of a frame (t < frame_tiles), run after run, a run's tiles row-major
struct Tile {
    Run run;
    uint32_t k;                  // the run's index
    uint32_t r0, c0, nr, nc;     // destination: rows [r0, r0 + nr) x elements [c0, c0 + nc) of the run
    uint32_t srow0, scol0;       // source: from this row and element of the stored plane ...
    uint32_t srows, scols;       // ... srows rows of scols elements (transposes: nc x nr, else nr x nc)
};
MELF_ORIENT_FN Tile tile_of(const Runs& rr, uint32_t t)
{
    const uint32_t t0 = run_tiles(rr.run[0]), t1 = rr.count > 1 ? run_tiles(rr.run[1]) : 0;
    Tile o;
    o.k = t < t0 ? 0u : (t < t0 + t1 ? 1u : 2u);
    const uint32_t b = o.k == 0 ? t : (o.k == 1 ? t - t0 : t - t0 - t1);
    // (masks, not an index: a runtime index into the by-value runs would put them into the private segment -- melf_gather_addr.h)
    const uint64_t m0 = 0 - (uint64_t)(o.k == 0), m1 = 0 - (uint64_t)(o.k == 1), m2 = 0 - (uint64_t)(o.k == 2);
#define MELF_ORIENT_SEL(field) o.run.field = (decltype(o.run.field))((rr.run[0].field & m0) | (rr.run[1].field & m1) | (rr.run[2].field & m2))
    MELF_ORIENT_SEL(src_off); MELF_ORIENT_SEL(dst_off); MELF_ORIENT_SEL(src_pitch); MELF_ORIENT_SEL(dst_pitch); MELF_ORIENT_SEL(rows);
    MELF_ORIENT_SEL(cols); MELF_ORIENT_SEL(oy0); MELF_ORIENT_SEL(ox0); MELF_ORIENT_SEL(ph); MELF_ORIENT_SEL(pw); MELF_ORIENT_SEL(eb);
#undef MELF_ORIENT_SEL
    o.run.pad = 0;
    const uint32_t across = tiles_across(o.run), ty = b / across, tx = b - ty * across;
    o.r0 = ty * TILE; o.c0 = tx * TILE;
    o.nr = o.run.rows - o.r0 < (uint32_t)TILE ? o.run.rows - o.r0 : (uint32_t)TILE;
    o.nc = o.run.cols - o.c0 < (uint32_t)TILE ? o.run.cols - o.c0 : (uint32_t)TILE;
    const bool tr = transposes(rr.code);
    const uint32_t a0 = tr ? o.run.ox0 + o.c0 : o.run.oy0 + o.r0, b0 = tr ? o.run.oy0 + o.r0 : o.run.ox0 + o.c0;
    o.srows = tr ? o.nc : o.nr; o.scols = tr ? o.nr : o.nc;
    o.srow0 = flips_rows(rr.code) ? o.run.ph - a0 - o.srows : a0;
    o.scol0 = flips_cols(rr.code) ? o.run.pw - b0 - o.scols : b0;
    return o;
}

// ---- the load side: row s of the source rectangle in pieces of 16 bytes ----
MELF_ORIENT_FN uint32_t load_pieces(const Tile& t) { return (t.scols * t.run.eb + PIECE - 1) / PIECE; }
struct Load {
    uint64_t src_off;   // in the stored frame
    uint32_t lds_off;   // in the LDS tile: 4-byte aligned
    uint32_t bytes;     // 16: one 16-byte load; 1 .. 15: the tail, loads of 8, 4, 2 and 1 bytes (tail_has / tail_at)
};
MELF_ORIENT_FN Load load_of(const Tile& t, uint32_t s, uint32_t piece)
{
    Load l;
    l.src_off = t.run.src_off + (uint64_t)(t.srow0 + s) * t.run.src_pitch + (uint64_t)t.scol0 * t.run.eb + (uint64_t)piece * PIECE;
    l.lds_off = s * lds_pitch(t.run.eb) + piece * PIECE;
    const uint32_t left = t.scols * t.run.eb - piece * PIECE;
    l.bytes = left < (uint32_t)PIECE ? left : (uint32_t)PIECE;
    return l;
}
// the piece's bytes are inside what may be read of the frame (always, for the runs of a plan made from the frame's checked
// descriptor; the kernel drops a piece that is not)
MELF_ORIENT_FN bool load_readable(const Load& l, uint64_t extent) { return l.src_off + l.bytes <= extent; }
// Tail: the load of width w (8, 4, 2, 1) is made if bit w of the byte count is set, at this offset inside the piece
MELF_ORIENT_FN bool tail_has(uint32_t bytes, uint32_t w) { return (bytes & w) != 0; }
MELF_ORIENT_FN uint32_t tail_at(uint32_t bytes, uint32_t w) { return bytes & ~(2 * w - 1) & 15u; }

// ---- the store side: row r of the tile's destination in pieces of 16 bytes ----
MELF_ORIENT_FN uint32_t store_pieces(const Tile& t) { return (t.nc * t.run.eb + PIECE - 1) / PIECE; }
struct Store {
    uint64_t dst_off;   // in the staged frame: 16-byte aligned
    uint32_t bytes;     // of the piece that belong to the row; the others are written as zeros
};
MELF_ORIENT_FN Store store_of(const Tile& t, uint32_t r, uint32_t piece)
{
    Store s;
    s.dst_off = t.run.dst_off + (uint64_t)(t.r0 + r) * t.run.dst_pitch + (uint64_t)t.c0 * t.run.eb + (uint64_t)piece * PIECE;
    const uint32_t left = t.nc * t.run.eb - piece * PIECE;
    s.bytes = left < (uint32_t)PIECE ? left : (uint32_t)PIECE;
    return s;
}
// Element e of the tile's destination row r lies in LDS at a0 + r * sr + e * se (bytes)
struct LdsMap {
    int32_t a0, sr, se;
};
MELF_ORIENT_FN LdsMap lds_map(const Tile& t, int code)
{
    const int32_t lp = (int32_t)lds_pitch(t.run.eb), eb = (int32_t)t.run.eb;
    const int32_t down = flips_rows(code) ? -lp : lp, along = flips_cols(code) ? -eb : eb;
    LdsMap m;
    m.a0 = (flips_rows(code) ? (int32_t)(t.srows - 1) * lp : 0) + (flips_cols(code) ? (int32_t)(t.scols - 1) * eb : 0);
    m.sr = transposes(code) ? along : down;
    m.se = transposes(code) ? down : along;
    return m;
}
MELF_ORIENT_FN uint32_t lds_elem(const LdsMap& m, uint32_t r, uint32_t e) { return (uint32_t)(m.a0 + (int32_t)r * m.sr + (int32_t)e * m.se); }

// ---- the oriented plan (host) ----
constexpr const char* ORIENT_RANGE = "orientation outside 1 .. 8 (the EXIF / TIFF tag 0x0112 values, MELF_ORIENT_*)";
constexpr const char* ORIENT_PACKED422 =
    "packed 4:2:2 frames (MELF_LIST_YUV422, MELF_LIST_YUV422_10) cannot be oriented in place: a mirrored macropixel is not a permutation "
    "of equal-sized elements";
constexpr const char* ORIENT_SUBSAMPLING =
    "orientations 5 .. 8 transpose the frame: they need chroma subsampled alike in both directions (sub_x == sub_y; 16-bit frames: sub_y == 1)";

// nullptr, or why frames of this checked batch cannot be read under the orientation
inline const char* orientable(const FrameBatch& b, int code)
{
    if (code < MELF_ORIENT_NORMAL || code > MELF_ORIENT_ROT90CCW) return ORIENT_RANGE;
    const int pix = b.lay.pix;
    if (pix_p422(pix) || pix_p10(pix)) return ORIENT_PACKED422;
    if (!transposes(code)) return nullptr;
    if (pix == PIX_YUVP && b.lay.yuvp.sub_x != b.lay.yuvp.sub_y) return ORIENT_SUBSAMPLING;
    if (pix == PIX_YUV16 && b.lay.y16.sub_y != 1) return ORIENT_SUBSAMPLING;
    return nullptr;
}
inline int oriented_h(const FrameBatch& b, int code) { return transposes(code) ? b.W : b.H; }
inline int oriented_w(const FrameBatch& b, int code) { return transposes(code) ? b.H : b.W; }

// The stored planes of a batch, in the order of its plan's runs, and where the same planes lie in the tight oriented frame
struct Plane {
    uint64_t off;      // first byte in a stored frame
    uint32_t pitch;    // bytes between its rows
    uint32_t h, w;     // rows, elements per row
    uint32_t eb;
    uint64_t o_off;    // the oriented plane's first byte in the tight oriented frame ...
    uint32_t o_pitch;  // ... and its (tight) pitch
};
struct Oriented {
    FrameBatch batch;              // the tight oriented frames: what stage_plan is asked about
    Plane plane[STAGE_MAX_RUNS];
    int count;
};
inline Plane plane_of(uint64_t off, int64_t pitch, int h, int w, int eb, int code, uint64_t o_off)
{
    return Plane{off, (uint32_t)pitch, (uint32_t)h, (uint32_t)w, (uint32_t)eb, o_off, (uint32_t)((transposes(code) ? h : w) * eb)};
}
// b: a checked batch that orientable() takes
inline Oriented oriented_batch(const FrameBatch& b, int code)
{
    Oriented o = {};
    const int H2 = oriented_h(b, code), W2 = oriented_w(b, code), pix = b.lay.pix;
    FrameLayout lay = b.lay;
    int y_eb = 1;
    if (pix == PIX_PLANAR) {
        const uint64_t plane = (uint64_t)H2 * W2;
        const int64_t src[3] = {b.lay.planes.b_off, b.lay.planes.g_off, b.lay.planes.r_off};
        for (int p = 0; p < 3; ++p) o.plane[p] = plane_of((uint64_t)src[p], b.row_stride, b.H, b.W, 1, code, p * plane);
        o.count = 3;
        lay.planes = PlanarPlanes{0, (int64_t)plane, (int64_t)(2 * plane)};
        lay.extent = (size_t)(3 * plane);
    } else if (pix_yuv(pix) || pix == PIX_YUVP || pix == PIX_YUV16) {
        // bytes per sample, subsampling, samples of a pair, the stored chroma offsets and pitch
        int bps = 1, sx = 1, sy = 1, step = pix == PIX_NV12 ? 2 : 1, c_pitch = b.lay.yuv.c_pitch;
        int64_t u = b.lay.yuv.u_off, v = b.lay.yuv.v_off;
        if (pix == PIX_YUVP) { sx = b.lay.yuvp.sub_x; sy = b.lay.yuvp.sub_y; step = b.lay.yuvp.c_step; c_pitch = b.lay.yuvp.c_pitch; u = b.lay.yuvp.u_off; v = b.lay.yuvp.v_off; }
        if (pix == PIX_YUV16) { bps = 2; sy = b.lay.y16.sub_y; step = b.lay.y16.c_step; c_pitch = b.lay.y16.c_pitch; u = b.lay.y16.u_off; v = b.lay.y16.v_off; }
        y_eb = bps;
        const bool semi = step == 2;
        const int ch = b.H >> sy, cw = b.W >> sx, ch2 = H2 >> sy, cw2 = W2 >> sx;   // chroma planes: stored, oriented
        const uint64_t c0 = (uint64_t)H2 * W2 * bps, cplane = (uint64_t)ch2 * cw2 * step * bps;
        const int64_t lo = u < v ? u : v;
        o.plane[0] = plane_of(0, b.row_stride, b.H, b.W, bps, code, 0);
        int64_t u2, v2;
        if (semi) {
            o.plane[1] = plane_of((uint64_t)lo, c_pitch, ch, cw, 2 * bps, code, c0);
            o.count = 2;
            u2 = (int64_t)c0 + (u - lo); v2 = (int64_t)c0 + (v - lo);
        } else {
            o.plane[1] = plane_of((uint64_t)u, c_pitch, ch, cw, bps, code, c0);
            o.plane[2] = plane_of((uint64_t)v, c_pitch, ch, cw, bps, code, c0 + cplane);
            o.count = 3;
            u2 = (int64_t)c0; v2 = (int64_t)(c0 + cplane);
        }
        const int c_pitch2 = cw2 * step * bps;
        if (pix == PIX_YUVP) { lay.yuvp.u_off = u2; lay.yuvp.v_off = v2; lay.yuvp.c_pitch = c_pitch2; }
        else if (pix == PIX_YUV16) { lay.y16.u_off = u2; lay.y16.v_off = v2; lay.y16.c_pitch = c_pitch2; }
        else { lay.yuv.u_off = u2; lay.yuv.v_off = v2; lay.yuv.c_pitch = c_pitch2; }
        lay.extent = (size_t)(c0 + cplane * (semi ? 1 : 2));
    } else {
        y_eb = pix_p32(pix) ? 4 : pix_bytes(pix);
        o.plane[0] = plane_of(0, b.row_stride, b.H, b.W, y_eb, code, 0);
        o.count = 1;
        lay.extent = (size_t)H2 * W2 * y_eb;
    }
    o.batch = FrameBatch{b.n, H2, W2, lay.extent, W2 * y_eb, lay};
    return o;
}

// The plan of a batch under an orientation: sp -- the staged frame, the rect in it, the work items, the destination side of the
// runs -- is stage_plan's of the oriented geometry; runs adds the source side.  cr: the crop, clamped to the ORIENTED frame.
struct Plan {
    StagePlan sp;
    Runs runs;
};
inline Plan oriented_plan(const FrameBatch& b, int code, const Crop& cr)
{
    const Oriented o = oriented_batch(b, code);
    Plan p = {};
    p.sp = stage_plan(o.batch, cr);
    p.runs.count = p.sp.runs.count;
    p.runs.code = code;
    p.runs.extent = b.lay.extent;
    for (int k = 0; k < p.sp.runs.count && k < o.count; ++k) {
        const RowRun& rr = p.sp.runs.run[k];
        const Plane& pl = o.plane[k];
        const uint64_t rel = rr.src_off - pl.o_off;   // the run's first element in the tight oriented plane
        Run& r = p.runs.run[k];
        r.src_off = pl.off; r.dst_off = rr.dst_off;
        r.src_pitch = pl.pitch; r.dst_pitch = rr.dst_pitch;
        r.rows = rr.rows; r.cols = rr.row_bytes / pl.eb;
        r.oy0 = (uint32_t)(rel / pl.o_pitch); r.ox0 = (uint32_t)(rel % pl.o_pitch) / pl.eb;
        r.ph = pl.h; r.pw = pl.w; r.eb = pl.eb; r.pad = 0;
    }
    return p;
}

}  // namespace orient
}  // namespace melf
