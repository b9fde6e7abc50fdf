// Address arithmetic of the kernels that read 16-bit YUV planes (melf_process_yuv16*): the first byte and the length of every load of
// the dial source's window fetch (DialYuv16, melf_frame_src.h) and of the prep arm (PX 25, prep_lplane_body.inc), and the decisions
// that guard them (the dial window's quads, the prep row's rows_safe and a lane's own test).  Plain C++: the kernels compute their
// addresses with these functions, and tests/y16_bounds_main.cpp sweeps the same functions on the CPU against buffers of exact extent.
// Every offset counts BYTES from the caller's base (prep) or from a frame's first byte (dials); x counts pixels = samples.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MELF_Y16_FN __host__ __device__ __forceinline__
#else
#define MELF_Y16_FN inline
#endif

namespace melf {
namespace y16 {

// the 8-bit sample of a 16-bit one: the low `shift` bits dropped, clamped (include/meterelf_hip.h)
MELF_Y16_FN uint32_t reduce(uint32_t s, uint32_t shift)
{
    const uint32_t v = s >> shift;
    return v < 255u ? v : 255u;
}

// ---- dial window -------------------------------------------------------------------------------------------------------------
// A lane fetches four pixels of a window row: four Y samples (8 bytes) and the two chroma pairs under them (CSTEP 1: one dword of
// each plane, CSTEP 2: 8 bytes of the interleaved plane) -- 16 bytes, when the four start at an EVEN pixel of the frame.  So the
// lanes' quads start at the even pixel at or left of the window's first column: shift = parity of that column in the frame
// (wave-uniform), the window's column k is pixel k + shift of the quads, and a window of ws columns takes (ws + shift + 3) / 4 quads.
MELF_Y16_FN int quad_shift(int fx_m, int wx0) { return (fx_m + wx0) & 1; }
MELF_Y16_FN int quad_count(int ws, int shift) { return (ws + shift + 3) >> 2; }
// wave-uniform: the quads (from crop column qx0 = wx0 - shift on) lie inside the crop's columns, sixteen lanes hold them
MELF_Y16_FN bool quads_inside(int qx0, int npiece, int tw) { return qx0 >= 0 && qx0 + 4 * npiece <= tw && npiece <= 16; }
// the lane's first pixel in the frame (even when the quads are used)
MELF_Y16_FN int lane_fx0(int fx_m, int qx0, int npiece, int pc) { return fx_m + qx0 + 4 * (pc < npiece - 1 ? pc : npiece - 1); }
// the lane's loads for frame row fy, from the frame's first byte: 8 bytes of Y ...
MELF_Y16_FN size_t dial_y_off(int fy, size_t y_pitch, int fx0) { return (size_t)fy * y_pitch + (size_t)fx0 * 2; }
// ... and from a chroma plane's offset (CSTEP 2: from the lower of the two): 4 bytes of each plane (CSTEP 1), 8 bytes (CSTEP 2)
MELF_Y16_FN size_t dial_c_off(int fy, int sub_y, size_t c_pitch, int fx0, int cstep) { return (size_t)(fy >> sub_y) * c_pitch + (size_t)(fx0 >> 1) * 2 * (size_t)cstep; }
constexpr int DIAL_Y_BYTES = 8;
MELF_Y16_FN int dial_c_bytes(int cstep) { return 4 * cstep; }
// one pixel (the colour core, the exact path): its Y sample and its chroma samples, 2 bytes each
MELF_Y16_FN size_t px_y_off(int fy, size_t y_pitch, int fx) { return (size_t)fy * y_pitch + (size_t)fx * 2; }
MELF_Y16_FN size_t px_c_off(int fy, int sub_y, size_t c_pitch, int fx, int cstep) { return (size_t)(fy >> sub_y) * c_pitch + (size_t)(fx >> 1) * 2 * (size_t)cstep; }

// ---- prep ----------------------------------------------------------------------------------------------------------------------
// A lane's 32 pixels: the window starts at the EVEN pixel at or left of its first one, 34 Y samples (68 bytes) and the 17 chroma
// pairs under them (CSTEP 1: 34 bytes of each plane, CSTEP 2: 68 bytes of the interleaved plane), as aligned dwords from the dword
// that holds the first sample (phase m = 0 or 2 bytes: everything is 2-byte aligned).
constexpr int PREP_Y_BYTES = 68;
MELF_Y16_FN int prep_c_bytes(int cstep) { return 34 * cstep; }
// bytes the aligned dwords of an NB-byte window span, from its first dword (load_window, k_match_mfma.hip)
MELF_Y16_FN int span(int nb) { return (nb + 6) / 4 * 4; }

struct PrepRow {          // one image row of one frame group (wave-uniform)
    size_t first, last;   // the group's first and last frame
    size_t yrow, crow;    // the row in the Y plane and in a chroma plane
    size_t c0, c1;        // the lower and the higher chroma offset
    int x0e, xlast;       // the first window's first pixel (even), the last window's
    uint32_t bm;          // byte phase of the base (0 or 2)
};
MELF_Y16_FN PrepRow prep_row(size_t base_phase, size_t frame_stride, size_t row_stride, int x0, int y0, int y, int grp, int nframes, int nkb,
                             int64_t u_off, int64_t v_off, size_t c_pitch, int sub_y)
{
    PrepRow r;
    const int lastf = grp * 32 + 31 < nframes - 1 ? grp * 32 + 31 : nframes - 1;
    r.first = (size_t)grp * 32 * frame_stride;
    r.last = (size_t)lastf * frame_stride;
    r.yrow = (size_t)(y0 + y) * row_stride;
    r.crow = (size_t)((y0 + y) >> sub_y) * c_pitch;
    r.c0 = (size_t)(u_off < v_off ? u_off : v_off);
    r.c1 = (size_t)(u_off < v_off ? v_off : u_off);
    r.x0e = x0 & ~1;
    r.xlast = r.x0e + 32 * (nkb - 1);
    r.bm = (uint32_t)(base_phase & 3);
    return r;
}
// the first byte of a lane's windows, window's first pixel xs (even), frame at byte fo
MELF_Y16_FN size_t prep_y_off(const PrepRow& r, size_t fo, int xs) { return fo + r.yrow + (size_t)xs * 2; }
MELF_Y16_FN size_t prep_c_off(const PrepRow& r, size_t fo, size_t plane_off, int xs, int cstep) { return fo + plane_off + r.crow + (size_t)(xs >> 1) * 2 * (size_t)cstep; }
// wave-uniform: every window of this row, in every frame of the group, starts at or behind the base and ends inside the buffer
MELF_Y16_FN bool prep_rows_safe(const PrepRow& r, int cstep, size_t readable)
{
    const bool head = r.bm == 0 || (prep_y_off(r, r.first, r.x0e) >= 2 && prep_c_off(r, r.first, r.c0, r.x0e, cstep) >= 2);
    return head && prep_y_off(r, r.last, r.xlast) + (size_t)span(PREP_Y_BYTES) <= readable &&
           prep_c_off(r, r.last, cstep == 2 ? r.c0 : r.c1, r.xlast, cstep) + (size_t)span(prep_c_bytes(cstep)) <= readable;
}
// one aligned window of nb bytes at byte o (phase m): inside the buffer at both ends
MELF_Y16_FN bool prep_window_ok(size_t o, uint32_t m, int nb, size_t readable) { return o >= m && o - m + (size_t)span(nb) <= readable; }

}  // namespace y16
}  // namespace melf
