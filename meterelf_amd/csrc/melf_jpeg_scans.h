// Multi-scan sequential JPEG files (melf_ctx_set_jpeg_multiscan), host-only: the scan plan the parser, the chunk layout and
// tests/jpeg_scans_main.cpp share.  Such a file sends its three components in three scans of one component each.  A
// non-interleaved scan of component c is, bit for bit, the entropy-coded segment of a greyscale file of the component's size:
// one block is an MCU, the component's REAL blocks (no MCU padding) come in raster order, the scan has its own DC predictor,
// restart interval and tables.  So every scan goes through k_jpeg_clean / k_jpeg_huff / k_jpeg_huff_rst as a one-component
// record of its own that writes the component's blocks into an area of its own ("planar coefficients"), and k_jpeg_idct reads
// block (bx, by) of component c at area c + by * real_blocks_x + bx.  Here is the arithmetic of that:
//   component()    a component's size in samples and in real blocks
//   scan_window()  the window a scan's record is decoded on, in the component's samples, from the file's window in luma pixels
//   area_first()   where a component's area begins among the file's coefficient blocks (the areas keep the MCU-padded sizes of the
//                  interleaved layout, of which a planar component fills the first real_blocks_x * real_blocks_y blocks)
//   scan_rule()    which scripts are taken
#pragma once
#include <cstdint>

namespace melf {
namespace jpeg_scans {

struct Window { int x0, y0, x1, y1; };   // [x0, x1) x [y0, y1)

struct Comp {
    int w, h;       // samples
    int rbx, rby;   // real blocks: ceil(w / 8), ceil(h / 8)
    int pbx, pby;   // blocks of the MCU-padded grid
};

// Component c (0 = luma with factors hs0 x vs0, 1 / 2 = chroma with factors 1 x 1) of a W x H frame.
inline Comp component(const int W, const int H, const int hs0, const int vs0, const int c)
{
    Comp k;
    k.w = c == 0 ? W : (W + hs0 - 1) / hs0;
    k.h = c == 0 ? H : (H + vs0 - 1) / vs0;
    k.rbx = (k.w + 7) / 8;
    k.rby = (k.h + 7) / 8;
    const int mcus_x = (W + 8 * hs0 - 1) / (8 * hs0), mcus_y = (H + 8 * vs0 - 1) / (8 * vs0);
    k.pbx = mcus_x * (c == 0 ? hs0 : 1);
    k.pby = mcus_y * (c == 0 ? vs0 : 1);
    return k;
}

// First block of component c's area, counted from the file's first coefficient block.
inline uint32_t area_first(const int W, const int H, const int hs0, const int vs0, const int c)
{
    uint32_t o = 0;
    for (int q = 0; q < c; ++q) {
        const Comp k = component(W, H, hs0, vs0, q);
        o += (uint32_t)k.pbx * (uint32_t)k.pby;
    }
    return o;
}

// Block (bx, by) of a planar component, counted from its area's first block: decode order of a one-component scan.
inline uint32_t block_index(const Comp& k, const int bx, const int by) { return (uint32_t)by * (uint32_t)k.rbx + (uint32_t)bx; }

// The window of component c's scan record, in the component's samples.  The file's window win (luma pixels, 0 <= x0 < x1 <= W, same
// for y) makes k_jpeg_idct transform the blocks of the MCUs floor(x0 / mw) .. ceil(x1 / mw) (mw = 8 hs0; rows alike): the scan must
// leave exactly the real ones among those blocks decoded.  For a chroma component that is the file's window divided by the sampling
// factors and rounded OUTWARDS to MCUs -- not a subset of the luma window.  The result is never empty and lies inside the real grid.
inline Window scan_window(const Window& win, const int W, const int H, const int hs0, const int vs0, const int c)
{
    const Comp k = component(W, H, hs0, vs0, c);
    const int mw = 8 * hs0, mh = 8 * vs0;
    const int mcus_x = (W + mw - 1) / mw, mcus_y = (H + mh - 1) / mh;
    const int mx0 = win.x0 / mw, my0 = win.y0 / mh;
    int mx1 = (win.x1 + mw - 1) / mw, my1 = (win.y1 + mh - 1) / mh;
    if (mx1 > mcus_x) mx1 = mcus_x;
    if (my1 > mcus_y) my1 = mcus_y;
    const int fx = c == 0 ? hs0 : 1, fy = c == 0 ? vs0 : 1;
    int bx1 = mx1 * fx, by1 = my1 * fy;
    if (bx1 > k.rbx) bx1 = k.rbx;
    if (by1 > k.rby) by1 = k.rby;
    Window r;
    r.x0 = mx0 * fx * 8; r.y0 = my0 * fy * 8; r.x1 = bx1 * 8; r.y1 = by1 * 8;
    return r;
}

// One SOS of a sequential three-component file whose first scan is not the interleaved one: nullptr when the scan is one of the
// script that is taken -- exactly three scans of one component each, every component once, in any order, each a full sequential scan
// (Ss = 0, Se = 63, Ah = Al = 0) -- or why the file is not.  ns: components of the scan; comp: the frame's index of its (first)
// component, -1 when the frame has none of that id; seen: bit c set when component c has had its scan.
inline const char* scan_rule(const int ns, const int comp, const unsigned seen, const int Ss, const int Se, const int AhAl)
{
    if (ns == 2) return "scan of two components (partially interleaved script)";
    if (ns != 1) return "scan of all components behind a scan of one (partially interleaved script)";
    if (comp < 0) return "scan of a component the frame header does not have";
    if (seen & (1u << comp)) return "component sent twice in a sequential file";
    if (Ss != 0 || Se != 63 || AhAl != 0) return "not a full sequential scan";
    return nullptr;
}

}  // namespace jpeg_scans
}  // namespace melf
