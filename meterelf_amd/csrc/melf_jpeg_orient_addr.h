// Where a JPEG file that carries an EXIF orientation (codes 2-8 of include/meterelf_hip.h's table) is decoded: the pixel window of
// the STORED frame that holds an upright rectangle, and the place of a stored pixel in the upright frame.  Host and device code
// share it (k_jpeg.hip); the CPU tests compile it alone and sweep it (tests/test_jpeg_orient.py).
//
// With S the stored frame of Hs rows x Ws columns, every code is two axis flips and, for 5-8, a transposition behind them:
//     u = flips_x ? Ws - 1 - sx : sx,   v = flips_y ? Hs - 1 - sy : sy,   O[v][u] = S[sy][sx]  (codes 1-4),  O[u][v] = S[sy][sx]  (5-8)
// which is the header's table read from the stored side.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MELF_JO_FN __host__ __device__ inline
#else
#define MELF_JO_FN inline
#endif

namespace melf {
namespace jpeg_orient {

// Window margin and alignment, in pixels: the MCU edge of 4:2:0, and what the window has always been cut with.  It is NOT the largest
// MCU edge of every file the decoder takes: a 4:1:1 MCU is 32 x 8, a 4:4:0 MCU 8 x 16 (melf_ctx_set_jpeg_samplings).  The window
// stays as it is for them, bit for bit, because nothing below needs the MCU: the MARGIN is the chroma filter's reach -- one chroma
// sample, i.e. 2 pixels along a filtered axis (4:4:0 filters down the columns, 4:1:1 not at all), 16 covers it -- and the ALIGNMENT
// is the 4:2:0 colour kernel's (8 pixels, even rows).  The decode stages take the window in pixels and round it outwards to each
// file's own MCUs themselves (k_jpeg.hip, JpegWindow), so a 32-wide MCU that the window cuts in the middle is decoded whole.
constexpr int MCU = 16;

struct Window { int x0, y0, x1, y1; };   // pixels of the stored frame, [x0, x1) x [y0, y1)

MELF_JO_FN bool transposed(int code) { return code >= 5; }
MELF_JO_FN bool flips_x(int code) { return code == 2 || code == 3 || code == 7 || code == 8; }   // along the stored rows
MELF_JO_FN bool flips_y(int code) { return code == 3 || code == 4 || code == 6 || code == 7; }   // along the stored columns

// stored size of a file whose upright frame is H x W, and the reverse: the same swap
MELF_JO_FN int swapped_h(int code, int H, int W) { return transposed(code) ? W : H; }
MELF_JO_FN int swapped_w(int code, int H, int W) { return transposed(code) ? H : W; }

// The upright rectangle rect = {x0, y0, x1, y1} (half open, not clamped) in stored coordinates.
MELF_JO_FN Window stored_rect(const int* rect, int code, int Hs, int Ws)
{
    const bool t = transposed(code);
    const int u0 = t ? rect[1] : rect[0], u1 = t ? rect[3] : rect[2];   // along the stored rows
    const int v0 = t ? rect[0] : rect[1], v1 = t ? rect[2] : rect[3];   // along the stored columns
    Window r;
    r.x0 = flips_x(code) ? Ws - u1 : u0; r.x1 = flips_x(code) ? Ws - u0 : u1;
    r.y0 = flips_y(code) ? Hs - v1 : v0; r.y1 = flips_y(code) ? Hs - v0 : v1;
    return r;
}

// What is decoded past the Huffman stage: the mapped rectangle grown by one MCU on every side (the chroma filter's context), aligned
// to whole MCUs, clamped to the stored frame; the whole frame without a rectangle or when nothing is left.  Code 1: exactly the
// window an upright file has always had.
MELF_JO_FN Window window(const int* rect, int code, int Hs, int Ws)
{
    const Window whole = {0, 0, Ws, Hs};
    if (!rect) return whole;
    const Window r = stored_rect(rect, code, Hs, Ws);
    Window w;
    w.x0 = (r.x0 - MCU) & ~(MCU - 1); w.y0 = (r.y0 - MCU) & ~(MCU - 1);
    w.x1 = (r.x1 + MCU + MCU - 1) & ~(MCU - 1); w.y1 = (r.y1 + MCU + MCU - 1) & ~(MCU - 1);
    if (w.x0 < 0) w.x0 = 0;
    if (w.y0 < 0) w.y0 = 0;
    if (w.x1 > Ws) w.x1 = Ws;
    if (w.y1 > Hs) w.y1 = Hs;
    if (w.x1 <= w.x0 || w.y1 <= w.y0) return whole;
    return w;
}

// The upright place of the stored pixel (sx, sy).
MELF_JO_FN void upright_of(int code, int Hs, int Ws, int sx, int sy, int* x, int* y)
{
    const int u = flips_x(code) ? Ws - 1 - sx : sx, v = flips_y(code) ? Hs - 1 - sy : sy;
    *x = transposed(code) ? v : u;
    *y = transposed(code) ? u : v;
}

}  // namespace jpeg_orient
}  // namespace melf
