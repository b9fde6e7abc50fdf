// YUV 4:2:0 -> BGR alone: the stage kernel behind melf_yuv_to_bgr (include/meterelf_hip.h), under the descriptor's matrix (mx;
// MELF_YUV_BT601_LIMITED: what cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420) makes of a decoder's frame) before the reference's
// get_bgr_image hands it on (meterelf/_image.py:46-51).  The arithmetic is melf_device.h's yuv_chroma / yuv_bgr, the functions the
// reading kernels (k_lplane_yuv, k_match_yuv, k_yneedle) convert with in place: this kernel pins it for every (Y, U, V).
//
// Mapping: one thread per 2 x 2 block of pixels, which shares one chroma pair: two byte loads of chroma, two 2-byte loads of
// Y, two 6-byte rows of B G R out.  A parity and debugging aid, not a hot path: the hot path never forms the BGR frame.
#include "melf_device.h"
#include "melf_internal.h"
#include "melf_y16_addr.h"
#include "melf_p10_addr.h"
#include "melf_p32_addr.h"

namespace melf {

template <bool PLANAR>
__global__ __launch_bounds__(256) void k_yuv2bgr(const uint8_t* __restrict__ src, int H, int W, int y_pitch, size_t frame_stride,
                                                 YuvPlanes yuv, YuvMatrix mx, uint8_t* __restrict__ dst)
{
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y, f = blockIdx.z;
    if (bx >= (W >> 1) || by >= (H >> 1)) return;
    const uint8_t* frame = src + (size_t)f * frame_stride;
    const size_t co = (size_t)by * (size_t)yuv.c_pitch + (size_t)(PLANAR ? bx : 2 * bx);
    const YuvChroma c = yuv_chroma(frame[(size_t)yuv.u_off + co], frame[(size_t)yuv.v_off + co], mx);
    uint8_t* out = dst + ((size_t)f * H + 2 * by) * (size_t)W * 3 + (size_t)bx * 6;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint8_t* yrow = frame + (size_t)(2 * by + r) * (size_t)y_pitch + 2 * bx;
        const uint32_t p0 = yuv_bgr(yrow[0], c, mx), p1 = yuv_bgr(yrow[1], c, mx);
        uint8_t* o = out + (size_t)r * W * 3;
        o[0] = (uint8_t)p0; o[1] = (uint8_t)(p0 >> 8); o[2] = (uint8_t)(p0 >> 16);
        o[3] = (uint8_t)p1; o[4] = (uint8_t)(p1 >> 8); o[5] = (uint8_t)(p1 >> 16);
    }
}

void launch_yuv2bgr(const uint8_t* d_src, int pix, int n, int H, int W, int y_pitch, size_t frame_stride, const YuvPlanes& yuv,
                    const YuvMatrix& mx, uint8_t* d_dst, hipStream_t stream)
{
    // at most 65 535 frames per launch (grid z)
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int m = n - f0 < 65535 ? n - f0 : 65535;
        dim3 grid(((W >> 1) + 255) / 256, H >> 1, m), block(256);
        const uint8_t* s = d_src + (size_t)f0 * frame_stride;
        uint8_t* d = d_dst + (size_t)f0 * H * W * 3;
        if (pix == PIX_I420) hipLaunchKernelGGL(k_yuv2bgr<true>, grid, block, 0, stream, s, H, W, y_pitch, frame_stride, yuv, mx, d);
        else hipLaunchKernelGGL(k_yuv2bgr<false>, grid, block, 0, stream, s, H, W, y_pitch, frame_stride, yuv, mx, d);
    }
}

// Packed YUV 4:2:2 -> BGR alone: the stage kernel behind melf_yuv422_to_bgr, what cv2.cvtColor(COLOR_YUV2BGR_YUY2 / _UYVY / _YVYU)
// makes of a capture frame.  One thread per macropixel: one aligned dword in, permuted to Y0 U Y1 V by the runtime selector the
// reading kernels (k_p422_lplane, k_p422_match, k_p422_needle) use, two B G R pixels out.  This kernel pins the fetch and the
// arithmetic for every (Y, U, V) at both pixels of a macropixel; like k_yuv2bgr it is no hot path.
__global__ __launch_bounds__(256) void k_p422_to_bgr(const uint8_t* __restrict__ src, int H, int W, int row_pitch, size_t frame_stride,
                                                     uint32_t psel, YuvMatrix mx, uint8_t* __restrict__ dst)
{
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.z;
    if (bx >= (W >> 1)) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const uint32_t m = __builtin_amdgcn_perm(0u, *(const uint32_t*)(src + (size_t)f * frame_stride + (size_t)y * (size_t)row_pitch + (size_t)bx * 4), psel);
        const YuvChroma c = yuv_chroma((int)((m >> 8) & 255u), (int)(m >> 24), mx);
        const uint32_t p0 = yuv_bgr((int)(m & 255u), c, mx), p1 = yuv_bgr((int)((m >> 16) & 255u), c, mx);
        uint8_t* o = dst + ((size_t)f * H + y) * (size_t)W * 3 + (size_t)bx * 6;
        o[0] = (uint8_t)p0; o[1] = (uint8_t)(p0 >> 8); o[2] = (uint8_t)(p0 >> 16);
        o[3] = (uint8_t)p1; o[4] = (uint8_t)(p1 >> 8); o[5] = (uint8_t)(p1 >> 16);
    }
}

void launch_p422_to_bgr(const uint8_t* d_src, int pix, int n, int H, int W, int row_pitch, size_t frame_stride, const YuvMatrix& mx,
                        uint8_t* d_dst, hipStream_t stream)
{
    // at most 65 535 frames per launch (grid z); a workgroup row takes every 65 535th image row (grid y)
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int m = n - f0 < 65535 ? n - f0 : 65535;
        dim3 grid(((W >> 1) + 255) / 256, H < 65535 ? H : 65535, m), block(256);
        hipLaunchKernelGGL(k_p422_to_bgr, grid, block, 0, stream, d_src + (size_t)f0 * frame_stride, H, W, row_pitch, frame_stride,
                           p422_sel(pix), mx, d_dst + (size_t)f0 * H * W * 3);
    }
}

// Planar / semi-planar YUV of any subsampling -> BGR alone: the stage kernel behind melf_yuv_planar_to_bgr.  One thread per pixel:
// its Y byte and the chroma bytes at (y >> sub_y, x >> sub_x), the address formula of include/meterelf_hip.h as it stands (sub_x,
// sub_y and c_step are runtime scalars here), three bytes out.  This kernel pins the addressing and the arithmetic for every
// (Y, U, V) at every position inside a chroma block; like k_yuv2bgr it is no hot path.
__global__ __launch_bounds__(256) void k_yp_to_bgr(const uint8_t* __restrict__ src, int H, int W, int y_pitch, size_t frame_stride,
                                                     YuvPlanarPlanes yp, YuvMatrix mx, uint8_t* __restrict__ dst)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.z;
    if (x >= W) return;
    const uint8_t* frame = src + (size_t)f * frame_stride;
    const size_t cx = (size_t)(x >> yp.sub_x) * (size_t)yp.c_step;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const size_t co = (size_t)(y >> yp.sub_y) * (size_t)yp.c_pitch + cx;
        const YuvChroma c = yuv_chroma(frame[(size_t)yp.u_off + co], frame[(size_t)yp.v_off + co], mx);
        const uint32_t p = yuv_bgr(frame[(size_t)y * (size_t)y_pitch + (size_t)x], c, mx);
        uint8_t* o = dst + (((size_t)f * H + y) * (size_t)W + (size_t)x) * 3;
        o[0] = (uint8_t)p; o[1] = (uint8_t)(p >> 8); o[2] = (uint8_t)(p >> 16);
    }
}

void launch_yuvp_to_bgr(const uint8_t* d_src, int n, int H, int W, int y_pitch, size_t frame_stride, const YuvPlanarPlanes& yp,
                        const YuvMatrix& mx, uint8_t* d_dst, hipStream_t stream)
{
    // at most 65 535 frames per launch (grid z); a workgroup row takes every 65 535th image row (grid y)
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int m = n - f0 < 65535 ? n - f0 : 65535;
        dim3 grid((W + 255) / 256, H < 65535 ? H : 65535, m), block(256);
        hipLaunchKernelGGL(k_yp_to_bgr, grid, block, 0, stream, d_src + (size_t)f0 * frame_stride, H, W, y_pitch, frame_stride, yp, mx,
                           d_dst + (size_t)f0 * H * W * 3);
    }
}

// 16-bit planar / semi-planar YUV -> BGR alone: the stage kernel behind melf_yuv16_to_bgr.  One thread per pixel: its Y sample and
// the chroma samples at (y >> sub_y, x >> 1), 2-byte loads at the address formula of include/meterelf_hip.h as it stands, each
// reduced to 8 bits (y16::reduce: the statement of min(s >> shift, 255) every reading kernel shares), three bytes out.  This kernel
// pins the addressing, the reduction and the arithmetic for every sample value; like k_yuv2bgr it is no hot path.
__global__ __launch_bounds__(256) void k_y16_to_bgr(const uint8_t* __restrict__ src, int H, int W, int y_pitch, size_t frame_stride,
                                                    Yuv16Planes yp, YuvMatrix mx, uint8_t* __restrict__ dst)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.z;
    if (x >= W) return;
    const uint8_t* frame = src + (size_t)f * frame_stride;
    const uint32_t sh = (uint32_t)yp.shift;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const size_t co = y16::px_c_off(y, yp.sub_y, (size_t)yp.c_pitch, x, yp.c_step);
        const uint32_t u = *(const uint16_t*)(frame + (size_t)yp.u_off + co), v = *(const uint16_t*)(frame + (size_t)yp.v_off + co);
        const uint32_t ys = *(const uint16_t*)(frame + y16::px_y_off(y, (size_t)y_pitch, x));
        const YuvChroma c = yuv_chroma((int)y16::reduce(u, sh), (int)y16::reduce(v, sh), mx);
        const uint32_t p = yuv_bgr((int)y16::reduce(ys, sh), c, mx);
        uint8_t* o = dst + (((size_t)f * H + y) * (size_t)W + (size_t)x) * 3;
        o[0] = (uint8_t)p; o[1] = (uint8_t)(p >> 8); o[2] = (uint8_t)(p >> 16);
    }
}

void launch_y16_to_bgr(const uint8_t* d_src, int n, int H, int W, int y_pitch, size_t frame_stride, const Yuv16Planes& yp,
                       const YuvMatrix& mx, uint8_t* d_dst, hipStream_t stream)
{
    // at most 65 535 frames per launch (grid z); a workgroup row takes every 65 535th image row (grid y)
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int m = n - f0 < 65535 ? n - f0 : 65535;
        dim3 grid((W + 255) / 256, H < 65535 ? H : 65535, m), block(256);
        hipLaunchKernelGGL(k_y16_to_bgr, grid, block, 0, stream, d_src + (size_t)f0 * frame_stride, H, W, y_pitch, frame_stride, yp, mx,
                           d_dst + (size_t)f0 * H * W * 3);
    }
}

// Packed 10-bit YUV 4:2:2 -> BGR alone: the stage kernels behind melf_yuv422_10_to_bgr.  One thread per pixel: the two words of its
// group that hold its three fields (v210) or the two dwords of its macropixel (Y210), at the offsets and with the bit selection of
// melf_p10_addr.h that every reading kernel shares, three bytes out.  They pin the addressing, the selection and the arithmetic for
// every sample value at every position of a group; like k_yuv2bgr no hot path.
template <bool V210>
__device__ __forceinline__ void p10_to_bgr(const uint8_t* __restrict__ src, int H, int W, int row_pitch, size_t frame_stride, const YuvMatrix& mx,
                                           uint8_t* __restrict__ dst)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.z;
    if (x >= W) return;
    const uint8_t* frame = src + (size_t)f * frame_stride;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        uint32_t s;
        if constexpr (V210) {
            const uint32_t* w = (const uint32_t*)(frame + p10::v210_px_off(y, (size_t)row_pitch, x));
            const int ph = p10::v210_phase(x);
            s = p10::v210_px_yuv(w[0], w[1], ph >> 1, ph & 1);
        } else {
            const uint32_t* w = (const uint32_t*)(frame + p10::y210_px_off(y, (size_t)row_pitch, x));
            s = p10::y210_px_yuv(w[0], w[1], x & 1);
        }
        const uint32_t p = yuv_bgr((int)(s & 255u), yuv_chroma((int)((s >> 8) & 255u), (int)(s >> 16), mx), mx);
        uint8_t* o = dst + (((size_t)f * H + y) * (size_t)W + (size_t)x) * 3;
        o[0] = (uint8_t)p; o[1] = (uint8_t)(p >> 8); o[2] = (uint8_t)(p >> 16);
    }
}
__global__ __launch_bounds__(256) void k_v210_to_bgr(const uint8_t* __restrict__ src, int H, int W, int row_pitch, size_t frame_stride, YuvMatrix mx,
                                                     uint8_t* __restrict__ dst)
{
    p10_to_bgr<true>(src, H, W, row_pitch, frame_stride, mx, dst);
}
__global__ __launch_bounds__(256) void k_y210_to_bgr(const uint8_t* __restrict__ src, int H, int W, int row_pitch, size_t frame_stride, YuvMatrix mx,
                                                     uint8_t* __restrict__ dst)
{
    p10_to_bgr<false>(src, H, W, row_pitch, frame_stride, mx, dst);
}

void launch_p10_to_bgr(const uint8_t* d_src, int pix, int n, int H, int W, int row_pitch, size_t frame_stride, const YuvMatrix& mx,
                       uint8_t* d_dst, hipStream_t stream)
{
    // at most 65 535 frames per launch (grid z); a workgroup row takes every 65 535th image row (grid y)
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int m = n - f0 < 65535 ? n - f0 : 65535;
        dim3 grid((W + 255) / 256, H < 65535 ? H : 65535, m), block(256);
        const uint8_t* s = d_src + (size_t)f0 * frame_stride;
        uint8_t* d = d_dst + (size_t)f0 * H * W * 3;
        if (pix == PIX_V210) hipLaunchKernelGGL(k_v210_to_bgr, grid, block, 0, stream, s, H, W, row_pitch, frame_stride, mx, d);
        else hipLaunchKernelGGL(k_y210_to_bgr, grid, block, 0, stream, s, H, W, row_pitch, frame_stride, mx, d);
    }
}

// 32-bit packed 4:4:4 -> BGR alone: the stage kernels behind melf_packed32_to_bgr.  One thread per pixel: its word, the three reads at
// the positions every reading kernel takes (melf_p32_addr.h), YUV: the conversion under mx, else R G B as they are; three bytes out.
// They pin the addressing and the selection for every value at every position; like k_yuv2bgr no hot path.
template <bool YUV>
__global__ __launch_bounds__(256) void k_p32_to_bgr(const uint8_t* __restrict__ src, int H, int W, int row_pitch, size_t frame_stride, Packed32Fields fields,
                                                    YuvMatrix mx, uint8_t* __restrict__ dst)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.z;
    if (x >= W) return;
    const uint8_t* frame = src + (size_t)f * frame_stride;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const uint32_t wd = *(const uint32_t*)(frame + p32::px_off(y, (size_t)row_pitch, x));
        uint32_t p;
        if constexpr (YUV)
            p = yuv_bgr((int)p32::read8(wd, fields.pos[0]), yuv_chroma((int)p32::read8(wd, fields.pos[1]), (int)p32::read8(wd, fields.pos[2]), mx), mx);
        else
            p = p32::rgb_bgr(wd, fields);
        uint8_t* o = dst + (((size_t)f * H + y) * (size_t)W + (size_t)x) * 3;
        o[0] = (uint8_t)p; o[1] = (uint8_t)(p >> 8); o[2] = (uint8_t)(p >> 16);
    }
}

void launch_p32_to_bgr(const uint8_t* d_src, int pix, int n, int H, int W, int row_pitch, size_t frame_stride, const Packed32Fields& fields,
                       const YuvMatrix* mx, uint8_t* d_dst, hipStream_t stream)
{
    // at most 65 535 frames per launch (grid z); a workgroup row takes every 65 535th image row (grid y)
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int m = n - f0 < 65535 ? n - f0 : 65535;
        dim3 grid((W + 255) / 256, H < 65535 ? H : 65535, m), block(256);
        const uint8_t* s = d_src + (size_t)f0 * frame_stride;
        uint8_t* d = d_dst + (size_t)f0 * H * W * 3;
        if (pix == PIX_P32_YUV) hipLaunchKernelGGL(k_p32_to_bgr<true>, grid, block, 0, stream, s, H, W, row_pitch, frame_stride, fields, *mx, d);
        else hipLaunchKernelGGL(k_p32_to_bgr<false>, grid, block, 0, stream, s, H, W, row_pitch, frame_stride, fields, YuvMatrix{}, d);
    }
}

}  // namespace melf
