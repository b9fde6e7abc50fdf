// The layout vocabulary of the frames the reading kernels take: the pixel codes, the plane descriptions and FrameLayout.  No HIP:
// melf_internal.h includes this where the text used to stand, melf_frame_checks.h (the descriptor checks) and the host-compiled
// test programs include it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/meterelf_hip.h"

namespace melf {

// Pixel layout of the images the reading kernels take: MELF_PIX_* (include/meterelf_hip.h) for camera frames, PIX_PLANE for
// the stage entry points' packed single-channel images (melf_match_ccoeff) and HLS dials crops (melf_read_dials).
constexpr int PIX_PLANE = -1;
inline int pix_bytes(int pix) { return pix == MELF_PIX_BGRA || pix == MELF_PIX_RGBA ? 4 : 3; }
// YUV 4:2:0 frames (melf_process_yuv*): the launch's pix, beside the MELF_PIX_* codes.  The Y plane is described like a
// single-channel image (base, frame_stride, row_stride of MatchSrc / DialsSrc), the chroma planes by YuvPlanes.
constexpr int PIX_NV12 = 16, PIX_I420 = 17;
inline bool pix_yuv(int pix) { return pix == PIX_NV12 || pix == PIX_I420; }
struct YuvPlanes {
    int64_t u_off, v_off;  // bytes from a frame's first byte to its U / V samples (NV12: v_off == u_off + 1)
    int c_pitch;           // bytes between chroma rows
    int pad;
};
// The colour conversion of YUV frames, 4:2:0 and 4:2:2 alike: the offset and the five coefficients of melf_device.h's yuv_chroma /
// yuv_luma (include/meterelf_hip.h states the formula).  A by-value kernel argument of every kernel that converts, the same for
// every lane: the compiler keeps it in SGPRs.  The four constants below are the single statement of the numbers: row 0 the
// three-decimal constants of cv2, the others round(2^20 c) of the standards' exact coefficients (derivation: include/meterelf_hip.h).
struct YuvMatrix {
    int yoff;                 // 16 (limited range) or 0 (full range)
    int cy;                   // luma gain
    int crv, cgv, cgu, cbu;   // R from v; G from v and from u; B from u
};
// Every coefficient fits a signed 24-bit operand (|c| < 2^23): the kernels multiply with v_mul_i32_i24 / v_mad_i32_i24, which read
// the low 24 bits of an operand as a signed number, and yuv_chroma's two forms of the G term (melf_device.h) stay equal only then.
constexpr bool yuv_matrix_fits24(const YuvMatrix& m)
{
    constexpr int lim = 1 << 23;
    return (m.yoff == 0 || m.yoff == 16) && m.cy > -lim && m.cy < lim && m.crv > -lim && m.crv < lim && m.cgv > -lim && m.cgv < lim &&
           m.cgu > -lim && m.cgu < lim && m.cbu > -lim && m.cbu < lim;
}
constexpr YuvMatrix YUV_BT601_LIMITED_MATRIX = {16, 1220542, 1673527, -852492, -409993, 2116026};
constexpr YuvMatrix YUV_BT601_FULL_MATRIX = {0, 1048576, 1470104, -748826, -360853, 1858077};
constexpr YuvMatrix YUV_BT709_LIMITED_MATRIX = {16, 1220945, 1879825, -558796, -223607, 2215014};
constexpr YuvMatrix YUV_BT709_FULL_MATRIX = {0, 1048576, 1651297, -490864, -196424, 1945738};
static_assert(yuv_matrix_fits24(YUV_BT601_LIMITED_MATRIX) && yuv_matrix_fits24(YUV_BT601_FULL_MATRIX) &&
                  yuv_matrix_fits24(YUV_BT709_LIMITED_MATRIX) && yuv_matrix_fits24(YUV_BT709_FULL_MATRIX),
              "a YUV coefficient does not fit the 24-bit multiply");
// the matrix of a descriptor's code (MELF_YUV_BT*); NULL: not a code (1 is never assigned)
inline const YuvMatrix* yuv_matrix(int code)
{
    static const YuvMatrix table[4] = {YUV_BT601_LIMITED_MATRIX, YUV_BT601_FULL_MATRIX, YUV_BT709_LIMITED_MATRIX,
                                       YUV_BT709_FULL_MATRIX};
    switch (code) {
    case MELF_YUV_BT601_LIMITED: return &table[0];
    case MELF_YUV_BT601_FULL: return &table[1];
    case MELF_YUV_BT709_LIMITED: return &table[2];
    case MELF_YUV_BT709_FULL: return &table[3];
    default: return nullptr;
    }
}
// Packed YUV 4:2:2 frames (melf_process_yuv422*): the launch's pix.  Two pixels per 4-byte macropixel; base, frame_stride and
// row_stride (bytes, all 4-byte aligned) describe the frames as for any packed layout, x0 and cols count pixels.  The formats
// differ in a byte permute only, which the kernels take as a runtime value (v_perm_b32 selector): macropixel -> Y0 U Y1 V.
constexpr int PIX_YUYV = 24, PIX_UYVY = 25, PIX_YVYU = 26;
inline bool pix_p422(int pix) { return pix >= PIX_YUYV && pix <= PIX_YVYU; }
inline uint32_t p422_sel(int pix) { return pix == PIX_UYVY ? 0x02030001u : (pix == PIX_YVYU ? 0x01020300u : 0x03020100u); }
// Planar frames (melf_process_planes*): the launch's pix.  Three planes of one byte per sample; base, frame_stride and row_stride
// (bytes, any alignment) describe a frame and the rows of each of its planes, PlanarPlanes where the planes start inside a frame
// (which gives the channel order), x0 and cols count pixels.  `readable` counts from base to the last sample of the last frame's
// last plane: no load may start before base or end behind base + readable.
constexpr int PIX_PLANAR = 32;
struct PlanarPlanes {
    int64_t b_off, g_off, r_off;  // bytes from a frame's first byte to the first sample of its B / G / R plane
};
// Planar and semi-planar YUV frames of any of the four chroma subsamplings (melf_process_yuv_planar*): the launch's pix.  The Y
// plane is described like a single-channel image (base, frame_stride, row_stride of MatchSrc / DialsSrc, any byte alignment), the
// chroma by YuvPlanarPlanes: U of pixel (x, y) at frame + u_off + (y >> sub_y) * c_pitch + (x >> sub_x) * c_step, V the same from
// v_off.  c_step 2: the two are the bytes of one interleaved pair (|u_off - v_off| == 1; which comes first is a runtime, wave-uniform
// matter).  A by-value kernel argument of its own: YuvPlanes and the kernels that take it stay as they are.  The hot kernels are
// instantiated per (sub_x, c_step) -- the four forms of the chroma fetch -- and take sub_y as the runtime shift of the chroma row.
constexpr int PIX_YUVP = 40;
struct YuvPlanarPlanes {
    int64_t u_off, v_off;  // bytes from a frame's first byte to its first U / V sample
    int c_pitch;           // bytes between chroma rows
    int sub_x, sub_y;      // log2 of the chroma subsampling, 0 or 1 each
    int c_step;            // bytes from one sample of a chroma plane to the next in its row: 1 planar, 2 semi-planar
};
// Planar and semi-planar YUV frames of 16-bit little-endian samples, chroma subsampled horizontally (melf_process_yuv16*): the
// launch's pix.  The Y plane is described by base, frame_stride and row_stride of MatchSrc / DialsSrc in BYTES (all 2-byte aligned),
// x0 and cols count pixels (samples); the chroma by Yuv16Planes: U of pixel (x, y) is the sample at byte frame + u_off + (y >> sub_y)
// * c_pitch + (x >> 1) * c_step * 2, V the same from v_off.  A sample s is read as min(s >> shift, 255) (melf_y16_addr.h: reduce),
// and from there on the arithmetic is that of PIX_YUVP.  A by-value kernel argument of its own; the hot kernels are instantiated
// per c_step and take sub_y, shift and the order of a pair's samples as runtime, wave-uniform values.
constexpr int PIX_YUV16 = 48;
struct Yuv16Planes {
    int64_t u_off, v_off;  // bytes from a frame's first byte to its first U / V sample
    int c_pitch;           // bytes between chroma rows
    int sub_y;             // log2 of the vertical chroma subsampling, 0 or 1
    int c_step;            // samples from one sample of a chroma plane to the next in its row: 1 planar, 2 semi-planar
    int shift;             // low bits dropped from a sample, 0 .. 8
};
// Packed 10-bit YUV 4:2:2 frames (melf_process_yuv422_10*): the launch's pix.  PIX_V210: rows of whole 16-byte groups, four
// little-endian words of three 10-bit fields each, six pixels a group in the order U Y V Y ..; base, frame_stride and row_stride
// (bytes) are multiples of 16, so a group is one aligned 16-byte load.  PIX_Y210 (Y210, Y212, Y216): macropixels of four MSB-aligned
// little-endian 16-bit words Y0 U Y1 V, 8 bytes for two pixels; base and strides are multiples of 8.  x0 and cols count pixels.  A
// field / word is read as its top 8 bits (melf_p10_addr.h: field8, the high bytes), and from there on the arithmetic is that of the
// packed 8-bit 4:2:2 frames.  Nothing travels with the pix but the matrix.
constexpr int PIX_V210 = 56, PIX_Y210 = 57;
inline bool pix_p10(int pix) { return pix == PIX_V210 || pix == PIX_Y210; }
// 32-bit packed 4:4:4 frames (melf_process_packed32*: AYUV / VUYA, Y410, X2RGB10 ..): the launch's pix.  A pixel is one little-endian
// 32-bit word; base, frame_stride and row_stride (bytes) are multiples of 4, x0 and cols count pixels.  The word holds three 8-bit
// reads, read k = (word >> pos[k]) & 255 (Packed32Fields: the same for every lane, so the kernels keep it in SGPRs and a read is one
// v_bfe_u32 with a scalar offset); every other bit is ignored.  PIX_P32_YUV: the reads are Y, U, V, converted under the matrix like
// the samples of an 8-bit 4:4:4 frame; PIX_P32_RGB: they are R, G, B, and nothing is converted.
constexpr int PIX_P32_YUV = 64, PIX_P32_RGB = 65;
inline bool pix_p32(int pix) { return pix == PIX_P32_YUV || pix == PIX_P32_RGB; }
struct Packed32Fields {
    uint32_t pos[3];       // low bit of the 8 bits read of Y, U, V / R, G, B: 0 .. 24
};

// How the frames of one launch lie in memory, beside the base, the strides and the rectangle of MatchSrc / DialsSrc: the pixel
// layout and what goes with it.  Host side only: the launchers hand the kernels the members by value.  Made by the makers below
// and by nothing else, so that which member means something for which pix is settled where the value is made, not at every use.
struct FrameLayout {
    int pix;
    YuvPlanes yuv;         // pix_yuv(pix): the chroma planes
    PlanarPlanes planes;   // PIX_PLANAR: where the three planes start
    const YuvMatrix* mx;   // pix_yuv(pix), pix_p422(pix), pix_p10(pix), PIX_YUVP, PIX_YUV16, PIX_P32_YUV: the frames' colour conversion, never NULL there
    size_t extent;         // bytes a kernel may read of the LAST frame, from its first byte (the others: frame_stride)
    YuvPlanarPlanes yuvp;  // PIX_YUVP: the chroma planes and their subsampling (mx: the conversion, as above)
    Yuv16Planes y16;       // PIX_YUV16: the chroma planes of 16-bit samples and the reduction (mx: the conversion, as above)
    Packed32Fields p32;    // pix_p32(pix): where the three reads sit in a pixel's word (PIX_P32_YUV: mx the conversion; _RGB: mx NULL)

    static FrameLayout packed(int pix /* MELF_PIX_* */, size_t extent) { return FrameLayout{pix, {}, {}, nullptr, extent}; }
    static FrameLayout yuv420(int pix /* PIX_NV12, PIX_I420 */, const YuvPlanes& yp, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{pix, yp, {}, &mx, extent};
    }
    static FrameLayout yuv422(int pix /* PIX_YUYV, PIX_UYVY, PIX_YVYU */, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{pix, {}, {}, &mx, extent};
    }
    static FrameLayout yuv_planar(const YuvPlanarPlanes& yp, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{PIX_YUVP, {}, {}, &mx, extent, yp};
    }
    static FrameLayout yuv16(const Yuv16Planes& yp, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{PIX_YUV16, {}, {}, &mx, extent, {}, yp};
    }
    static FrameLayout yuv422_10(int pix /* PIX_V210, PIX_Y210 */, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{pix, {}, {}, &mx, extent};
    }
    static FrameLayout packed32(int pix /* PIX_P32_YUV, PIX_P32_RGB */, const Packed32Fields& fields, const YuvMatrix* mx /* NULL for _RGB */,
                                size_t extent)
    {
        return FrameLayout{pix, {}, {}, mx, extent, {}, {}, fields};
    }
    static FrameLayout planar(const PlanarPlanes& pl, size_t extent) { return FrameLayout{PIX_PLANAR, {}, pl, nullptr, extent}; }
    static FrameLayout plane(size_t extent) { return FrameLayout{PIX_PLANE, {}, {}, nullptr, extent}; }
};

}  // namespace melf
