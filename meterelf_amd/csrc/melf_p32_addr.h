// Address arithmetic and bit selection of the kernels that read 32-bit packed 4:4:4 frames (melf_process_packed32*: AYUV / VUYA, Y410,
// X2RGB10 ..): one little-endian word per pixel, three 8-bit reads at the positions of Packed32Fields.  Plain C++, the sibling of
// melf_p10_addr.h: the dial source (DialWord32, melf_frame_src.h), the one-pixel loads of the dot4 matcher and the stage kernel compute
// their addresses with these functions, and tests/p32_bounds_main.cpp runs the same functions on the CPU against buffers of exact
// extent.  The prep arm (PX 28, 29, prep_lplane_body.inc) loads what k_lplane_px4 loads, with the functions of melf_prep_addr.h.
// Every offset counts BYTES from a frame's first byte; x counts pixels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "melf_frame_layout.h"

#if defined(__HIPCC__)
#define MELF_P32_FN __host__ __device__ __forceinline__
#else
#define MELF_P32_FN inline
#endif

namespace melf {
namespace p32 {

// one read: eight bits of the word from bit pos on (pos <= 24).  pos is the same for every lane: one v_bfe_u32 with a scalar offset
MELF_P32_FN uint32_t read8(uint32_t word, uint32_t pos) { return (word >> pos) & 255u; }
// the three reads of a word as r0 | r1 << 8 | r2 << 16 (Y U V / R G B from byte 0 on)
MELF_P32_FN uint32_t reads(uint32_t word, const Packed32Fields& f)
{
    return read8(word, f.pos[0]) | read8(word, f.pos[1]) << 8 | read8(word, f.pos[2]) << 16;
}
// the B G R dword of an RGB word: B in byte 0, as a load of a BGR frame's pixel gives it
MELF_P32_FN uint32_t rgb_bgr(uint32_t word, const Packed32Fields& f)
{
    return read8(word, f.pos[2]) | read8(word, f.pos[1]) << 8 | read8(word, f.pos[0]) << 16;
}
// one pixel: its word, 4 bytes, 4-byte aligned
constexpr int PX_BYTES = 4;
MELF_P32_FN size_t px_off(int fy, size_t pitch, int fx) { return (size_t)fy * pitch + (size_t)fx * 4; }
// a lane's four window pixels from pixel fx0 on: their four words, 16 bytes, 4-byte aligned, inside the row while the four pixels are
constexpr int DIAL_BYTES = 16;
MELF_P32_FN size_t dial_off(int fy, size_t pitch, int fx0) { return (size_t)fy * pitch + (size_t)fx0 * 4; }

}  // namespace p32
}  // namespace melf
