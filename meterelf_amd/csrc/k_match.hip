// K2 -- cv2.matchTemplate(L, template, TM_CCOEFF) + cv2.minMaxLoc
// (reference: meterelf/_utils.py:91-97, called from meterelf/_image.py:57-66).
//
// Exact integer formulation: cc[y,x] = sum_ij T[i,j] * I[y+i,x+j] in u32, window
// sum in u32, then OpenCV's own post-pass
//   R = float32( double(cc) - double(winsum) * mean(T) ).
// cc < 2^32, UNSIGNED: it passes 2^31 on bright frames for templates beyond 33 026
// pixels.  Nothing in this kernel bounds th * tw; the context's rule for the LDS
// tile below (setup_device_tables: (17 + ceil(tw / 4)) * (43 + th) * 4 <= 64 KiB)
// does -- it admits at most 159 x 256 = 40 704 pixels, cc <= 2.65e9 -- and that is
// what keeps the u32 accumulator from wrapping (tests/test_match_limits.py).
// OpenCV reaches cc through a float32 DFT; the exact value is what that
// approximates.
//
// Mapping (gfx950, wave64): one workgroup = 4 waves = a 44-row x 64-col tile of
// the correlation map.  The needed image rows (L plane, computed on the fly from
// the BGR frame) are staged once into LDS.  Lane = output column; each lane
// keeps MATCH_R = 11 consecutive output rows in registers, so one 4-byte image
// window (one LDS dword read + one v_alignbit) feeds 11 v_dot4_u32_u8 against
// wave-uniform template dwords that arrive through the scalar cache.  The window
// sum rides along as one extra dot4 with 0x01010101 per window.
#include <limits.h>

#include "melf_device.h"
#include "melf_internal.h"
#include "melf_y16_addr.h"
#include "melf_p10_addr.h"
#include "melf_p32_addr.h"

namespace melf {

__device__ inline bool better(float v, int i, float bv, int bi)
{
    // minMaxLoc: first maximum in raster order
    return i != INT_MAX && (bi == INT_MAX || v > bv || (v == bv && i < bi));
}

// The body of k_match and k_match_px4.  PX: 1 = packed single-channel u8 images, 3 = 3-byte pixels (BGR / RGB: L = (max + min) / 2
// does not depend on the channel order), 4 = 4-byte pixels (BGRA / RGBA, 4-byte aligned, the 4th byte ignored); 20 / 21 = NV12 /
// I420 frames (src: the Y plane, yuv: the chroma planes; a Y byte and the chroma pair under it per pixel, byte loads); 22 = packed
// YUV 4:2:2 frames (yuv: P422Sel, the byte permute to Y0 U Y1 V; a pixel's macropixel as one aligned dword load); 23 = planar
// frames (melf_process_planes*; yuv: PlanarPlanes, where the B, G and R planes start in a frame; three byte loads per pixel);
// 24 = planar / semi-planar YUV of any subsampling (melf_process_yuv_planar*; yuv: YuvPlanarPlanes; a Y byte and the chroma bytes
// at (y >> sub_y, x >> sub_x) per pixel, byte loads: the shifts and the sample step are wave-uniform scalars); 25 = 16-bit planar /
// semi-planar YUV (melf_process_yuv16*; yuv: Yuv16Planes; a Y sample and the chroma samples at (y >> sub_y, x >> 1) per pixel, 2-byte
// loads, each reduced to 8 bits by y16::reduce); 26 / 27 = packed 10-bit YUV 4:2:2, v210 / Y210 (melf_process_yuv422_10*; no yuv: the
// two words of the pixel's group / the two dwords of its macropixel, melf_p10_addr.h); 28 / 29 = 32-bit packed 4:4:4, Y U V / R G B
// (melf_process_packed32*; yuv: Packed32Fields, where the three reads sit; the pixel's word, one aligned dword, melf_p32_addr.h).
struct NoYuv {};
struct P422Sel { uint32_t sel; };
template <int PX, class YUV = NoYuv>
__device__ __forceinline__ void match_tile(MatchSrc src, MatchGeom g, const uint32_t* __restrict__ tplT,
                                           int rh, int rw, int nrb, float* __restrict__ result_map,
                                           MatchPartial* __restrict__ partials, int nparts, YUV yuv = YUV{},
                                           [[maybe_unused]] YuvMatrix mx = YuvMatrix{} /* PX 20 .. 22, 24: the frames' colour conversion */)
{
    constexpr int R = MATCH_R;
    extern __shared__ uint32_t lds[];
    __shared__ float s_v[MATCH_WAVES];
    __shared__ int s_i[MATCH_WAVES];

    const int tile = blockIdx.x, f = blockIdx.y;
    const int rb = tile % nrb, cb = tile / nrb;
    const int yb = rb * MATCH_RBLK, xb = cb * MATCH_CBLK;
    const uint8_t* img = src.base + (size_t)f * src.frame_stride;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // ---- stage the tile's image rows into LDS as packed u8 (zero outside) ----
    for (int row = wave; row < g.lds_rows; row += MATCH_WAVES) {
        const int y = yb + row;
        const uint8_t* prow = img + (size_t)(src.y0 + y) * src.row_stride;
        [[maybe_unused]] const uint8_t* urow = nullptr;
        [[maybe_unused]] const uint8_t* vrow = nullptr;
        if constexpr (PX == 20 || PX == 21) {
            urow = img + (size_t)yuv.u_off + (size_t)((src.y0 + y) >> 1) * (size_t)yuv.c_pitch;
            vrow = img + (size_t)yuv.v_off + (size_t)((src.y0 + y) >> 1) * (size_t)yuv.c_pitch;
        }
        if constexpr (PX == 24) {
            urow = img + (size_t)yuv.u_off + (size_t)((src.y0 + y) >> yuv.sub_y) * (size_t)yuv.c_pitch;
            vrow = img + (size_t)yuv.v_off + (size_t)((src.y0 + y) >> yuv.sub_y) * (size_t)yuv.c_pitch;
        }
        if constexpr (PX == 25) {
            urow = img + (size_t)yuv.u_off;
            vrow = img + (size_t)yuv.v_off;
        }
        for (int c4 = lane; c4 < g.ldsw; c4 += 64) {
            uint32_t packed = 0;
            if (y < src.rows) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = xb + c4 * 4 + k;
                    uint32_t v = 0;
                    if (x < src.cols) {
                        if constexpr (PX == 20 || PX == 21) {
                            const int cx = (src.x0 + x) >> 1, ci = PX == 20 ? 2 * cx : cx;
                            const YuvChroma c = yuv_chroma(urow[ci], vrow[ci], mx);
                            v = (uint32_t)yuv_lightness(prow[src.x0 + x], yuv_cmax(c), yuv_cmin(c), mx);
                        } else if constexpr (PX == 24) {
                            const int ci = ((src.x0 + x) >> yuv.sub_x) << (yuv.c_step - 1);
                            const YuvChroma c = yuv_chroma(urow[ci], vrow[ci], mx);
                            v = (uint32_t)yuv_lightness(prow[src.x0 + x], yuv_cmax(c), yuv_cmin(c), mx);
                        } else if constexpr (PX == 25) {
                            const size_t co = y16::px_c_off(src.y0 + y, yuv.sub_y, (size_t)yuv.c_pitch, src.x0 + x, yuv.c_step);
                            const uint32_t sft = (uint32_t)yuv.shift;
                            const YuvChroma c = yuv_chroma((int)y16::reduce(*(const uint16_t*)(urow + co), sft), (int)y16::reduce(*(const uint16_t*)(vrow + co), sft), mx);
                            v = (uint32_t)yuv_lightness((int)y16::reduce(*(const uint16_t*)(prow + (size_t)(src.x0 + x) * 2), sft), yuv_cmax(c), yuv_cmin(c), mx);
                        } else if constexpr (PX == 26 || PX == 27) {
                            const int fx = src.x0 + x;
                            uint32_t s;
                            if constexpr (PX == 26) {
                                const uint32_t* w = (const uint32_t*)(img + p10::v210_px_off(src.y0 + y, (size_t)src.row_stride, fx));
                                const int ph = p10::v210_phase(fx);
                                s = p10::v210_px_yuv(w[0], w[1], ph >> 1, ph & 1);
                            } else {
                                const uint32_t* w = (const uint32_t*)(img + p10::y210_px_off(src.y0 + y, (size_t)src.row_stride, fx));
                                s = p10::y210_px_yuv(w[0], w[1], fx & 1);
                            }
                            const YuvChroma c = yuv_chroma((int)((s >> 8) & 255u), (int)(s >> 16), mx);
                            v = (uint32_t)yuv_lightness((int)(s & 255u), yuv_cmax(c), yuv_cmin(c), mx);
                        } else if constexpr (PX == 28 || PX == 29) {
                            const uint32_t wd = *(const uint32_t*)(img + p32::px_off(src.y0 + y, (size_t)src.row_stride, src.x0 + x));
                            if constexpr (PX == 28) {
                                const YuvChroma c = yuv_chroma((int)p32::read8(wd, yuv.pos[1]), (int)p32::read8(wd, yuv.pos[2]), mx);
                                v = (uint32_t)yuv_lightness((int)p32::read8(wd, yuv.pos[0]), yuv_cmax(c), yuv_cmin(c), mx);
                            } else {
                                v = (uint32_t)hls_lightness((int)p32::read8(wd, yuv.pos[2]), (int)p32::read8(wd, yuv.pos[1]), (int)p32::read8(wd, yuv.pos[0]));
                            }
                        } else if constexpr (PX == 22) {
                            const int fx = src.x0 + x;
                            const uint32_t m = __builtin_amdgcn_perm(0u, *(const uint32_t*)(prow + (size_t)(fx >> 1) * 4), yuv.sel);
                            const YuvChroma c = yuv_chroma((int)((m >> 8) & 255u), (int)(m >> 24), mx);
                            v = (uint32_t)yuv_lightness((int)((fx & 1 ? m >> 16 : m) & 255u), yuv_cmax(c), yuv_cmin(c), mx);
                        } else if constexpr (PX == 23) {
                            const uint8_t* p = prow + (size_t)(src.x0 + x);
                            v = (uint32_t)hls_lightness(p[yuv.b_off], p[yuv.g_off], p[yuv.r_off]);
                        } else if (PX == 3) {
                            const uint8_t* p = prow + (size_t)(src.x0 + x) * 3;
                            v = (uint32_t)hls_lightness(p[0], p[1], p[2]);
                        } else if (PX == 4) {
                            const uint32_t px = *(const uint32_t*)(prow + (size_t)(src.x0 + x) * 4);
                            v = (uint32_t)hls_lightness(px & 255, (px >> 8) & 255, (px >> 16) & 255);
                        } else {
                            v = prow[src.x0 + x];
                        }
                    }
                    packed |= v << (8 * k);
                }
            }
            lds[row * g.ldsw + c4] = packed;
        }
    }
    __syncthreads();

    // ---- sliding-window correlation ----
    const int q = lane >> 2;
    const uint32_t sh = (uint32_t)(lane & 3) * 8u;
    const int yr0 = wave * R;
    uint32_t acc[R], ws[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = ws[r] = 0;

    const int T = g.th + R - 1;
    const int last = g.tw4 - 1;
    for (int t = 0; t < T; ++t) {
        const uint32_t* row = lds + (yr0 + t) * g.ldsw + q;
        const uint32_t* tp = tplT + (t + R - 1);  // tplT[jj][padded_row], padded_row = (t - r) + R - 1
        uint32_t d0 = row[0];
        uint32_t rsum = 0;
        for (int jj = 0; jj < last; ++jj) {
            const uint32_t d1 = row[jj + 1];
            const uint32_t w = __builtin_amdgcn_alignbit(d1, d0, sh);
            d0 = d1;
            rsum = __builtin_amdgcn_udot4(w, 0x01010101u, rsum, false);
            const uint32_t* tq = tp + jj * g.trows;
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_amdgcn_udot4(w, tq[-r], acc[r], false);
        }
        {
            const uint32_t d1 = row[last + 1];
            const uint32_t w = __builtin_amdgcn_alignbit(d1, d0, sh);
            rsum = __builtin_amdgcn_udot4(w, g.last_ones, rsum, false);
            const uint32_t* tq = tp + last * g.trows;
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_amdgcn_udot4(w, tq[-r], acc[r], false);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if ((unsigned)(t - r) < (unsigned)g.th) ws[r] += rsum;
    }

    // ---- OpenCV post-pass + first-max reduction ----
    float bestv = 0.f;
    int besti = INT_MAX;
    const int x = xb + lane;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int y = yb + yr0 + r;
        if (y < rh && x < rw) {
            double num = (double)acc[r];
            num -= (double)ws[r] * g.tmean;
            const float v = (float)num;
            const int idx = y * rw + x;
            if (result_map) result_map[(size_t)f * rh * rw + idx] = v;
            if (better(v, idx, bestv, besti)) { bestv = v; besti = idx; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bestv, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (better(ov, oi, bestv, besti)) { bestv = ov; besti = oi; }
    }
    if (lane == 0) { s_v[wave] = bestv; s_i[wave] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MATCH_WAVES; ++w)
            if (better(s_v[w], s_i[w], bestv, besti)) { bestv = s_v[w]; besti = s_i[w]; }
        MatchPartial p;
        p.val = bestv;
        p.idx = besti;
        partials[(size_t)f * nparts + tile] = p;
    }
}

template <bool FROM_BGR>
__global__ __launch_bounds__(256) void k_match(MatchSrc src, MatchGeom g, const uint32_t* __restrict__ tplT,
                                               int rh, int rw, int nrb, float* __restrict__ result_map,
                                               MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<FROM_BGR ? 3 : 1>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts);
}

// BGRA / RGBA frames (melf_process_frames*)
__global__ __launch_bounds__(256) void k_match_px4(MatchSrc src, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                   int rh, int rw, int nrb, float* __restrict__ result_map,
                                                   MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<4>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts);
}

// NV12 / I420 frames (melf_process_yuv*); mx: the frames' colour conversion (wave-uniform: SGPRs)
template <bool PLANAR>
__global__ __launch_bounds__(256) void k_match_yuv(MatchSrc src, YuvPlanes yuv, YuvMatrix mx, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                   int rh, int rw, int nrb, float* __restrict__ result_map,
                                                   MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<PLANAR ? 21 : 20, YuvPlanes>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts, yuv, mx);
}

// packed YUV 4:2:2 frames (melf_process_yuv422*); psel: macropixel -> Y0 U Y1 V
__global__ __launch_bounds__(256) void k_p422_match(MatchSrc src, uint32_t psel, YuvMatrix mx, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                    int rh, int rw, int nrb, float* __restrict__ result_map,
                                                    MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<22, P422Sel>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts, P422Sel{psel}, mx);
}

// planar frames (melf_process_planes*): the dot4 matcher with three byte loads per pixel, one from each plane
__global__ __launch_bounds__(256) void k_planar_match(MatchSrc src, PlanarPlanes planes, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                      int rh, int rw, int nrb, float* __restrict__ result_map,
                                                      MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<23, PlanarPlanes>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts, planes);
}

// planar / semi-planar YUV of any subsampling (melf_process_yuv_planar*): the dot4 matcher with a Y byte and two chroma bytes per pixel
__global__ __launch_bounds__(256) void k_yp_match(MatchSrc src, YuvPlanarPlanes yuv, YuvMatrix mx, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                    int rh, int rw, int nrb, float* __restrict__ result_map,
                                                    MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<24, YuvPlanarPlanes>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts, yuv, mx);
}

// 16-bit planar / semi-planar YUV (melf_process_yuv16*): the dot4 matcher with a Y sample and two chroma samples per pixel
__global__ __launch_bounds__(256) void k_y16_match(MatchSrc src, Yuv16Planes yuv, YuvMatrix mx, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                   int rh, int rw, int nrb, float* __restrict__ result_map,
                                                   MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<25, Yuv16Planes>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts, yuv, mx);
}

// packed 10-bit YUV 4:2:2 (melf_process_yuv422_10*): the dot4 matcher with the pixel's two words (v210) / its macropixel (Y210)
__global__ __launch_bounds__(256) void k_v210_match(MatchSrc src, YuvMatrix mx, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                    int rh, int rw, int nrb, float* __restrict__ result_map,
                                                    MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<26, NoYuv>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts, NoYuv{}, mx);
}

__global__ __launch_bounds__(256) void k_y210_match(MatchSrc src, YuvMatrix mx, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                    int rh, int rw, int nrb, float* __restrict__ result_map,
                                                    MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<27, NoYuv>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts, NoYuv{}, mx);
}

// 32-bit packed 4:4:4 (melf_process_packed32*): the dot4 matcher with the pixel's word, one aligned dword; YUV: the reads are Y, U, V
// under mx, else R, G, B (mx is not looked at)
template <bool YUV>
__global__ __launch_bounds__(256) void k_p32_match(MatchSrc src, Packed32Fields fields, YuvMatrix mx, MatchGeom g, const uint32_t* __restrict__ tplT,
                                                   int rh, int rw, int nrb, float* __restrict__ result_map,
                                                   MatchPartial* __restrict__ partials, int nparts)
{
    match_tile<YUV ? 28 : 29, Packed32Fields>(src, g, tplT, rh, rw, nrb, result_map, partials, nparts, fields, mx);
}

int match_parts(const MatchGeom& g, int rows, int cols)
{
    const int rh = rows - g.th + 1, rw = cols - g.tw + 1;
    if (rh <= 0 || rw <= 0) return 0;
    const int nrb = (rh + MATCH_RBLK - 1) / MATCH_RBLK, ncb = (rw + MATCH_CBLK - 1) / MATCH_CBLK;
    return nrb * ncb;
}

void launch_match(const MatchSrc& src, const FrameLayout& lay, int n, const MatchGeom& g, const uint32_t* d_tplT,
                  float* d_result_map, MatchPartial* d_partials, int* nparts_out, hipStream_t stream)
{
    const int pix = lay.pix;
    const int rh = src.rows - g.th + 1, rw = src.cols - g.tw + 1;
    const int nrb = (rh + MATCH_RBLK - 1) / MATCH_RBLK, ncb = (rw + MATCH_CBLK - 1) / MATCH_CBLK;
    const int nparts = nrb * ncb;
    if (nparts_out) *nparts_out = nparts;
    const size_t shmem = (size_t)g.lds_rows * g.ldsw * sizeof(uint32_t);
    dim3 grid(nparts, n), block(256);
    if (pix == PIX_YUV16)
        hipLaunchKernelGGL(k_y16_match, grid, block, shmem, stream, src, lay.y16, *lay.mx, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
    else if (pix == PIX_YUVP)
        hipLaunchKernelGGL(k_yp_match, grid, block, shmem, stream, src, lay.yuvp, *lay.mx, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
    else if (pix == PIX_V210)
        hipLaunchKernelGGL(k_v210_match, grid, block, shmem, stream, src, *lay.mx, g, d_tplT, rh, rw, nrb, d_result_map, d_partials, nparts);
    else if (pix == PIX_Y210)
        hipLaunchKernelGGL(k_y210_match, grid, block, shmem, stream, src, *lay.mx, g, d_tplT, rh, rw, nrb, d_result_map, d_partials, nparts);
    else if (pix == PIX_P32_YUV)
        hipLaunchKernelGGL(k_p32_match<true>, grid, block, shmem, stream, src, lay.p32, *lay.mx, g, d_tplT, rh, rw, nrb, d_result_map, d_partials, nparts);
    else if (pix == PIX_P32_RGB)
        hipLaunchKernelGGL(k_p32_match<false>, grid, block, shmem, stream, src, lay.p32, YuvMatrix{}, g, d_tplT, rh, rw, nrb, d_result_map, d_partials, nparts);
    else if (pix == PIX_PLANAR)
        hipLaunchKernelGGL(k_planar_match, grid, block, shmem, stream, src, lay.planes, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
    else if (pix_p422(pix))
        hipLaunchKernelGGL(k_p422_match, grid, block, shmem, stream, src, p422_sel(pix), *lay.mx, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
    else if (pix == PIX_NV12)
        hipLaunchKernelGGL(k_match_yuv<false>, grid, block, shmem, stream, src, lay.yuv, *lay.mx, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
    else if (pix == PIX_I420)
        hipLaunchKernelGGL(k_match_yuv<true>, grid, block, shmem, stream, src, lay.yuv, *lay.mx, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
    else if (pix == PIX_PLANE)
        hipLaunchKernelGGL(k_match<false>, grid, block, shmem, stream, src, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
    else if (pix_bytes(pix) == 4)
        hipLaunchKernelGGL(k_match_px4, grid, block, shmem, stream, src, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
    else
        hipLaunchKernelGGL(k_match<true>, grid, block, shmem, stream, src, g, d_tplT, rh, rw, nrb, d_result_map,
                           d_partials, nparts);
}

}  // namespace melf
