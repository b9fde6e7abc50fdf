// Address arithmetic of the kernels that read packed 10-bit YUV 4:2:2 frames (melf_process_yuv422_10*: v210 and Y210 / Y212 / Y216):
// pixel -> group / pair slot, the first byte and the length of every load of the dial sources' window fetch (DialV210, DialY210,
// melf_frame_src.h), of the one-pixel loads and of the prep arms (PX 26, 27, prep_lplane_body.inc), the decisions that guard them (the
// dial window's quads, the prep row's rows_safe and a lane's own test), and the selection of a sample's eight bits.  Plain C++, the
// sibling of melf_y16_addr.h: the kernels compute their addresses with these functions, and tests/p10_bounds_main.cpp sweeps the
// same functions on the CPU against buffers of exact extent.  Every offset counts BYTES from a frame's first byte (dials, one
// pixel) or from the caller's base (prep); x counts pixels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MELF_P10_FN __host__ __device__ __forceinline__
#else
#define MELF_P10_FN inline
#endif

namespace melf {
namespace p10 {

// ---- v210: the group ----------------------------------------------------------------------------------------------------------------
// A row is whole groups of 16 bytes: four little-endian words of three 10-bit fields (bits 0-9, 10-19, 20-29; bits 30-31 ignored).
// The twelve fields of a group in order are U Y V Y  U Y V Y  U Y V Y: six pixels as three pairs, pair q = fields 4 q .. 4 q + 3.
constexpr int V210_GROUP_BYTES = 16;
MELF_P10_FN int v210_groups(int W) { return (int)(((uint32_t)W + 5u) / 6u); }            // groups of a row of W pixels
MELF_P10_FN size_t v210_row_bytes(int W) { return (size_t)v210_groups(W) * V210_GROUP_BYTES; }
constexpr int field_word(int i) { return i / 3; }           // field i of a group: its word ...
constexpr int field_bit(int i) { return (i % 3) * 10; }     // ... and its first bit there
constexpr int pair_u(int q) { return 4 * q; }
constexpr int pair_y(int q, int second) { return 4 * q + 1 + 2 * second; }
constexpr int pair_v(int q) { return 4 * q + 2; }
// the 8-bit sample of a 10-bit field: (field >> 2) & 255, one 8-bit field extract at bit offset + 2 (include/meterelf_hip.h)
MELF_P10_FN uint32_t field8(uint32_t word, int bit) { return (word >> (bit + 2)) & 255u; }
// the group and the pair slot of a pixel
MELF_P10_FN int v210_group(int fx) { return (int)((uint32_t)fx / 6u); }
MELF_P10_FN int v210_phase(int fx) { return (int)((uint32_t)fx % 6u); }                   // 0 .. 5
MELF_P10_FN int v210_slot(int fx) { return v210_phase(fx) >> 1; }                         // 0 .. 2

// ---- one pixel (the colour core, the exact path, the dot4 matcher, the stage kernel, a prep lane at the buffer's end) ----------------
// v210: the three fields of a pixel of pair slot q lie in words q and q + 1 of its group (q + 1 <= 3): 8 bytes, 4-byte aligned,
// inside the group.  Y210: the pixel's macropixel, 8 bytes, 8-byte aligned: the dwords Y0 U and Y1 V.
constexpr int PX_BYTES = 8;
MELF_P10_FN size_t v210_px_off(int fy, size_t pitch, int fx) { return (size_t)fy * pitch + (size_t)v210_group(fx) * V210_GROUP_BYTES + (size_t)v210_slot(fx) * 4; }
MELF_P10_FN size_t y210_px_off(int fy, size_t pitch, int fx) { return (size_t)fy * pitch + (size_t)(fx >> 1) * 8; }
// field i of the group, from a = word q and b = word q + 1
MELF_P10_FN uint32_t v210_sample(uint32_t a, uint32_t b, int q, int i)
{
    const int w = (int)((uint32_t)i / 3u);
    return field8(w == q ? a : b, (i - 3 * w) * 10);
}
// Y | U << 8 | V << 16 of the pixel: q its pair slot, second: the pair's second pixel
MELF_P10_FN uint32_t v210_px_yuv(uint32_t a, uint32_t b, int q, int second)
{
    return v210_sample(a, b, q, pair_y(q, second)) | v210_sample(a, b, q, pair_u(q)) << 8 | v210_sample(a, b, q, pair_v(q)) << 16;
}
// the same from the macropixel's dwords d0 = Y0 U, d1 = Y1 V (16-bit words, the sample their high byte)
MELF_P10_FN uint32_t y210_px_yuv(uint32_t d0, uint32_t d1, int second)
{
    return (((second ? d1 : d0) >> 8) & 255u) | (d0 >> 24) << 8 | (d1 >> 24) << 16;
}

// ---- dial window ------------------------------------------------------------------------------------------------------------------
// A lane fetches four pixels of a window row as 16 bytes, when the four start at an EVEN pixel of the frame: two whole pairs.  So
// the lanes' quads start at the even pixel at or left of the window's first column, exactly as for the 16-bit planes
// (melf_y16_addr.h): shift = parity of that column in the frame (wave-uniform), the window's column k is pixel k + shift of the
// quads, and a window of ws columns takes (ws + shift + 3) / 4 quads.
MELF_P10_FN int quad_shift(int fx_m, int wx0) { return (fx_m + wx0) & 1; }
MELF_P10_FN int quad_count(int ws, int shift) { return (ws + shift + 3) >> 2; }
// wave-uniform: the quads (from crop column qx0 = wx0 - shift on) lie inside the crop's columns, sixteen lanes hold them
MELF_P10_FN bool quads_inside(int qx0, int npiece, int tw) { return qx0 >= 0 && qx0 + 4 * npiece <= tw && npiece <= 16; }
// the lane's first pixel in the frame (even when the quads are used)
MELF_P10_FN int lane_fx0(int fx_m, int qx0, int npiece, int pc) { return fx_m + qx0 + 4 * (pc < npiece - 1 ? pc : npiece - 1); }
constexpr int DIAL_BYTES = 16;
// v210, quad from the even pixel fx0, p = fx0 % 6: for p 0 and 2 all its fields lie in its own group, the aligned 16 bytes (never
// "from word 1 on" for p 2: in a row's last group that load would leave the row); for p 4 they lie in words 2, 3 of its group and
// words 0, 1 of the next -- which exists: pixels fx0 + 2 and fx0 + 3 lie inside the crop, and rows hold whole groups --, 16
// contiguous bytes, 8-byte aligned.
MELF_P10_FN size_t v210_dial_off(int fy, size_t pitch, int fx0)
{
    return (size_t)fy * pitch + (size_t)v210_group(fx0) * V210_GROUP_BYTES + (v210_phase(fx0) == 4 ? 8u : 0u);
}
// the quad's eight fields U Y V Y U Y V Y are fields f0 .. f0 + 7 of the twelve the 16 loaded bytes hold
MELF_P10_FN int v210_dial_field0(int p) { return p == 0 ? 0 : (p == 2 ? 4 : 2); }
// Y210: two macropixels, 16 bytes, 8-byte aligned
MELF_P10_FN size_t y210_dial_off(int fy, size_t pitch, int fx0) { return (size_t)fy * pitch + (size_t)fx0 * 4; }

// ---- prep ----------------------------------------------------------------------------------------------------------------------
// A lane's 32 pixels: the window starts at the EVEN pixel xs at or left of its first one and holds 34 pixels, 17 pairs.
//
// v210: the 17 pairs from pair slot s = (xs / 2) % 3 on touch 6 groups (s 0, 1) or 7 (s 2).  A lane loads the groups that hold its
// OWN pixels xs .. xend - 1 (xend: one past the lane's last pixel of the crop) and no other: they lie inside the crop's row, whose
// groups are whole, so no load can leave the row, let alone the buffer; a trailing group of the window that holds none of the lane's
// pixels -- it may lie beyond the row's groups -- is not loaded (its pairs read as zero and feed only columns no map position uses).
// A lane of 32 pixels needs six groups, or seven when s == 2 and its first pixel is odd.
MELF_P10_FN size_t v210_prep_off(size_t fo, int row, size_t pitch, int xs) { return fo + (size_t)row * pitch + (size_t)v210_group(xs) * V210_GROUP_BYTES; }
constexpr int V210_PREP_GROUPS = 7;   // at most
// the lane's own test: how many groups from the window's first hold the lane's pixels, 1 .. 7
MELF_P10_FN int v210_prep_groups(int xs, int xend) { return v210_group(xend - 1) - v210_group(xs) + 1; }
// wave-uniform: every live lane of the row needs at least the first six groups (only the last live lane can be short of 32 pixels)
MELF_P10_FN bool v210_rows_safe(int x0, int cols, int nkb)
{
    const int kbl = (cols - 1) / 32 < nkb - 1 ? (cols - 1) / 32 : nkb - 1;   // the last live lane's block
    const int xbeg = 32 * kbl, npx = cols - xbeg < 32 ? cols - xbeg : 32;
    return v210_prep_groups((x0 + xbeg) & ~1, x0 + xbeg + npx) >= 6;
}
// Y210: 17 macropixels, 136 bytes = 34 aligned dwords from the macropixel of xs (8-byte aligned), as 16-byte loads.  The window may
// reach past the crop and the row (never used: masked) but must end inside the buffer; it cannot start before the base.
constexpr int Y210_PREP_BYTES = 136;
MELF_P10_FN size_t y210_prep_off(size_t fo, int row, size_t pitch, int xs) { return fo + (size_t)row * pitch + (size_t)xs * 4; }
MELF_P10_FN bool y210_rows_safe(int grp, int nframes, size_t frame_stride, int row, size_t pitch, int x0, int nkb, size_t readable)
{
    const int lastf = grp * 32 + 31 < nframes - 1 ? grp * 32 + 31 : nframes - 1;
    return y210_prep_off((size_t)lastf * frame_stride, row, pitch, (x0 & ~1) + 32 * (nkb - 1)) + Y210_PREP_BYTES <= readable;
}
MELF_P10_FN bool y210_lane_ok(size_t o, size_t readable) { return o + Y210_PREP_BYTES <= readable; }

}  // namespace p10
}  // namespace melf
