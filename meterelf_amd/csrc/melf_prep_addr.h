// Address arithmetic of the prep kernels' 8-bit arms (prep_lplane_body.inc: PX 3, 4, 20, 21, 22, 23, 24): the first byte and the
// length of every aligned window a lane loads, and the decisions that guard them -- the row's rows_safe, the lane's own test, and the
// launcher's prep_window_readable.  Plain C++, the sibling of melf_y16_addr.h (PX 25): the kernels compute their addresses with
// these functions, and tests/prep_bounds_main.cpp sweeps the same functions on the CPU against buffers of exact extent.
// Every offset counts BYTES from the caller's base; x counts pixels.  The expressions keep the order and the types they had in the
// kernel body, so that every kernel compiles to what it compiled to (profiles/load_bounds/device_code_diff.txt).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MELF_PREP_FN __host__ __device__ __forceinline__
#else
#define MELF_PREP_FN inline
#endif

namespace melf {
namespace prep {

// the last frame of frame group grp (32 frames a group)
MELF_PREP_FN int last_frame(int grp, int nframes) { return grp * 32 + 31 < nframes - 1 ? grp * 32 + 31 : nframes - 1; }

// ---- which arm a launch takes, and what it may read as windows --------------------------------------------------------------------
enum Arm { ARM_PLANE = 1, ARM_PX3 = 3, ARM_PX4 = 4, ARM_YUV420 = 20, ARM_P422 = 22, ARM_PLANAR = 23, ARM_YUVP = 24, ARM_Y16 = 25 };
// The arms of 3-byte pixels and of 4:2:0 frames test their windows against the buffer's END only (the planar arms and the 16-bit arm
// test the start as well).  Both layouts may start at any byte, and with a base that is not 4-byte aligned the aligned window of the
// buffer's very first samples -- frame 0, row 0, a window that starts within 3 bytes of the base: 3-byte pixels from column 0; 4:2:0,
// whose windows start at even pixels, from a column below 4 -- would start 1 .. 3 bytes before the base.  For a crop that holds such
// a window the launcher tells the kernel that NOTHING is readable as a window: rows_safe and every lane's own test fail, in every
// row and frame of that launch, and every lane loads the crop's own samples one by one.  (A corner case -- the meter in the frame's
// first row at its first columns and an unaligned base -- that costs the common one nothing: the kernels' text has no test for it.)
MELF_PREP_FN size_t prep_window_readable(Arm arm, size_t base_phase, int x0, int y0, size_t readable)
{
    const int cols = arm == ARM_PX3 ? 1 : (arm == ARM_YUV420 ? 4 : 0);   // columns from which a first-row window reaches the base's dword
    return (base_phase & 3) != 0 && y0 == 0 && x0 < cols ? 0 : readable;
}

// ---- PX 3 / PX 4: packed pixels ------------------------------------------------------------------------------------------------------
// A lane's 32 pixels: PX 3 25 aligned dwords (100 bytes) from the dword that holds its first byte, PX 4 eight 16-byte loads (128
// bytes) from its first pixel (4-byte aligned like everything of that layout).
constexpr int packed_pb(int px) { return px == 4 ? 4 : 3; }
constexpr int packed_win(int px) { return px == 4 ? 128 : 100; }
MELF_PREP_FN bool packed_rows_safe(int grp, int nframes, size_t frame_stride, int row, int row_stride, int x0, int nkb, int pb, int win, size_t readable)
{
    return (size_t)last_frame(grp, nframes) * frame_stride + (size_t)row * row_stride + (size_t)(x0 + 32 * (nkb - 1)) * pb + win <= readable;
}
MELF_PREP_FN size_t packed_x_off(int x, int pb) { return (size_t)x * pb; }   // from the row's first byte
MELF_PREP_FN bool packed_lane_ok(int f, size_t frame_stride, int row, int row_stride, size_t o, int win, size_t readable)
{
    return (size_t)f * frame_stride + (size_t)row * row_stride + o + win <= readable;
}

// ---- PX 20 / PX 21: NV12, I420 ---------------------------------------------------------------------------------------------------------
// The window starts at the even pixel at or left of the lane's first: 34 Y bytes and the 17 chroma pairs under them (NV12 34
// interleaved bytes, I420 17 + 17), as aligned dwords: 10 for 34 bytes at any phase, 6 for 17.
constexpr int YUV420_Y_SPAN = 40;
constexpr int yuv420_c_span(bool nv12) { return nv12 ? 40 : 24; }
MELF_PREP_FN size_t yuv420_crow(int row, int c_pitch) { return (size_t)(row >> 1) * (size_t)c_pitch; }
MELF_PREP_FN int yuv420_xlast(int x0, int nkb) { return (x0 & ~1) + 32 * (nkb - 1); }
MELF_PREP_FN bool yuv420_rows_safe(size_t last, int row, int row_stride, int xlast, int64_t u_off, int64_t v_off, size_t crow, bool nv12, size_t readable)
{
    return last + (size_t)row * row_stride + (size_t)xlast + 40 <= readable &&
           last + (size_t)(u_off > v_off ? u_off : v_off) + crow + (size_t)(nv12 ? xlast : xlast >> 1) + 40 <= readable;
}
MELF_PREP_FN size_t yuv420_y_off(size_t fo, int row, int row_stride, int xs) { return fo + (size_t)row * row_stride + (size_t)xs; }
MELF_PREP_FN size_t yuv420_c_off(size_t fo, int64_t plane_off, size_t crow, int xs, bool interleaved)
{
    return fo + (size_t)plane_off + crow + (size_t)(interleaved ? xs : xs >> 1);
}
MELF_PREP_FN bool yuv420_lane_ok(size_t yo, size_t uo, size_t vo, bool nv12, size_t readable)
{
    return yo + 40 <= readable && uo + (nv12 ? 40 : 24) <= readable && (nv12 || vo + 24 <= readable);
}

// ---- PX 22: packed 4:2:2 ------------------------------------------------------------------------------------------------------------------
// The same even-pixel window is 17 consecutive aligned macropixel dwords: 68 bytes from the macropixel of the window's first pixel.
constexpr int P422_SPAN = 68;
MELF_PREP_FN bool p422_rows_safe(int grp, int nframes, size_t frame_stride, int row, int row_stride, int x0, int nkb, size_t readable)
{
    return (size_t)last_frame(grp, nframes) * frame_stride + (size_t)row * row_stride + (size_t)((x0 & ~1) + 32 * (nkb - 1)) * 2 + 68 <= readable;
}
MELF_PREP_FN size_t p422_x_off(int xs) { return (size_t)xs * 2; }
MELF_PREP_FN bool p422_lane_ok(int f, size_t frame_stride, int row, int row_stride, size_t o, size_t readable)
{
    return (size_t)f * frame_stride + (size_t)row * row_stride + o + 68 <= readable;
}

// ---- PX 23: planar RGB ----------------------------------------------------------------------------------------------------------------------
// A lane's 32 bytes of each plane: nine aligned dwords (36 bytes) from the dword that holds the first, at that plane's own phase.
constexpr int PLANAR_SPAN = 36;
MELF_PREP_FN size_t planar_row(int row, int row_stride, int x0) { return (size_t)row * row_stride + (size_t)x0; }
MELF_PREP_FN bool planar_rows_safe(uint32_t bm, int grp, int nframes, size_t frame_stride, size_t lo, size_t hi, size_t row, int nkb, size_t readable)
{
    return (bm == 0 || (size_t)grp * 32 * frame_stride + lo + row >= 3) &&
           (size_t)last_frame(grp, nframes) * frame_stride + hi + row + (size_t)(32 * (nkb - 1)) + 36 <= readable;
}
MELF_PREP_FN size_t planar_lane_off(int f, size_t frame_stride, int row, int row_stride, int x) { return (size_t)f * frame_stride + (size_t)row * row_stride + (size_t)x; }
MELF_PREP_FN bool planar_lane_ok(size_t ob, uint32_t mb, size_t og, uint32_t mg, size_t orr, uint32_t mr, size_t readable)
{
    return ob >= mb && og >= mg && orr >= mr && ob - mb + 36 <= readable && og - mg + 36 <= readable && orr - mr + 36 <= readable;
}

// ---- PX 24: planar / semi-planar YUV of any subsampling ---------------------------------------------------------------------------------------
// The even-pixel window of 34 Y bytes (40 as aligned dwords) and the chroma under it: 34 >> subx samples, cstep bytes apart.
constexpr int yuvp_nc(int subx) { return 34 >> subx; }                               // chroma samples under a window
constexpr int yuvp_cb(int subx, int cstep) { return yuvp_nc(subx) * cstep; }         // bytes of a chroma window
constexpr int yuvp_cwin(int subx, int cstep) { return (yuvp_cb(subx, cstep) + 6) / 4 * 4; }   // bytes its aligned dwords span
constexpr int YUVP_Y_SPAN = 40;
MELF_PREP_FN bool yuvp_rows_safe(uint32_t bm, size_t first, size_t last, size_t yrow, size_t crow, size_t c0, size_t c1, int x0e, int xlast, int subx, int cstep,
                                 int cwin, size_t readable)
{
    return (bm == 0 || (first + yrow + (size_t)x0e >= 3 && first + c0 + crow + (size_t)((x0e >> subx) * cstep) >= 3)) &&
           last + yrow + (size_t)xlast + 40 <= readable &&
           last + (cstep == 2 ? c0 : c1) + crow + (size_t)((xlast >> subx) * cstep) + cwin <= readable;
}
MELF_PREP_FN size_t yuvp_cx(int xs, int subx, int cstep) { return (size_t)((xs >> subx) * cstep); }
MELF_PREP_FN bool yuvp_lane_ok(size_t yo, uint32_t my, size_t uo, uint32_t mu, size_t vo, uint32_t mv, int cstep, int cwin, size_t readable)
{
    return yo >= my && uo >= mu && yo - my + 40 <= readable && uo - mu + cwin <= readable && (cstep == 2 || (vo >= mv && vo - mv + cwin <= readable));
}

}  // namespace prep
}  // namespace melf
