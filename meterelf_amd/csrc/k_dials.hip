// K3 -- per-dial needle reading + digit combine
// (reference: meterelf/_reading.py:19-115 get_meter_value, :118-151
// get_needle_points, :154-160 get_dial_color, :163-182
// determine_value_by_dial_positions; meterelf/_utils.py:18-42
// get_angle_by_vector; meterelf/_colors.py:38-50 get_range).
//
// Mapping (gfx950, wave64): one workgroup per frame, one wave per dial.
// Everything a dial needs lives inside its disk mask (radius R <= 29) plus the
// 2-px halo of the 3x3 closing, i.e. a window of at most 64 x 64 pixels, so a
// binary image is ONE 64-bit register per lane (lane = window row, bit = window
// column).  inRange masks come out of __ballot, the closing / flood fills / 8-
// connected labelling are shifts within the register plus neighbour-lane reads,
// contour areas are popcounts.  No pixel of the HLS image is ever written to
// memory: the window's BGR pixels are converted on the fly.
//
// cv2 semantics restated here:
//  * external contours of M = closed_mask & disk: the 8-connected components of
//    G = M u {pixels not 4-connected to the outside through ~M}; a component
//    inside another one's hole is not external and is swallowed by it;
//  * contourArea of an outer border = Q4(F) + Q3(F)/2 over the hole-filled
//    component F (2x2 blocks with 4 resp. 3 pixels set) -- tests/ check this
//    identity against a traced shoelace area;
//  * drawContours(thickness=-1) paints F.
#include <limits.h>
#include <stdlib.h>

#include <type_traits>

#include "melf_device.h"
#include "melf_internal.h"
#include "melf_frame_src.h"

namespace melf {

__device__ inline double py_fmod(double a, double b)
{
    // CPython float_rem
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0) != (m < 0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// get_angle_by_vector, meterelf/_utils.py:18-42; false = None
__device__ inline bool angle_by_vector(double x, double y, double& out)
{
    if (y == 0) {
        if (x > 0) { out = 0.25; return true; }
        if (x < 0) { out = 0.75; return true; }
        return false;
    }
    const double at = atan(x / y) / (2 * 3.141592653589793);
    // CPython's float % 1.0 without the library's fmod: v - trunc(v) IS fmod(v, 1.0) (the subtraction is exact), sign included
    // except at the zeros, which float_rem replaces by +0.0 anyway
    const double v = -at + (y > 0 ? 0.5 : 0.0);
    double m = v - trunc(v);
    if (m != 0.0) { if (m < 0) m += 1.0; } else { m = 0.0; }
    out = m;
    return true;
}

// determine_value_by_dial_positions, meterelf/_reading.py:163-182
__device__ inline double value_by_positions(double r4, double r3, double r2, double r1)
{
    int d3 = (int)r3 + ((py_fmod(r3, 1.0) > 0.55 && r4 <= 2) ? 1 : 0) - ((py_fmod(r3, 1.0) < 0.45 && r4 >= 8) ? 1 : 0);
    d3 = ((d3 % 10) + 10) % 10;
    int d2 = (int)r2 + ((py_fmod(r2, 1.0) > 0.55 && d3 <= 2) ? 1 : 0) - ((py_fmod(r2, 1.0) < 0.45 && d3 >= 8) ? 1 : 0);
    d2 = ((d2 % 10) + 10) % 10;
    int d1 = (int)r1 + ((py_fmod(r1, 1.0) > 0.55 && d2 <= 2) ? 1 : 0) - ((py_fmod(r1, 1.0) < 0.45 && d2 >= 8) ? 1 : 0);
    d1 = ((d1 % 10) + 10) % 10;
    return (d1 * 100.0) + (d2 * 10.0) + (d3 * 1.0) + r4 / 10.0;
}

struct Key {
    double a, d;
};
__device__ inline bool key_lt(const Key& p, const Key& q) { return p.a < q.a || (p.a == q.a && p.d < q.d); }
// One trimming round: the smallest of the lanes' `lo` keys and the largest of their `hi` keys.  The angle's extreme first (the two
// scans interleave); the lane that holds it is nearly always alone, and its distance is then a v_readlane away.
__device__ inline void wave_min_max_key(const Key& lo, const Key& hi, Key& klo, Key& khi)
{
    klo.a = wave_min_f64(lo.a);
    khi.a = wave_max_f64(hi.a);
    const uint64_t blo = __builtin_amdgcn_ballot_w64(lo.a == klo.a), bhi = __builtin_amdgcn_ballot_w64(hi.a == khi.a);
    if (__popcll(blo) == 1 && __popcll(bhi) == 1) {
        const int jl = __builtin_ctzll(blo), jh = __builtin_ctzll(bhi);
        const uint64_t dl = __double_as_longlong(lo.d), dh = __double_as_longlong(hi.d);
        klo.d = __longlong_as_double((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)dl, jl) |
                                     ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(dl >> 32), jl) << 32));
        khi.d = __longlong_as_double((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)dh, jh) |
                                     ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(dh >> 32), jh) << 32));
    } else {
        klo.d = wave_min_f64(lo.a == klo.a ? lo.d : 1e300);
        khi.d = wave_max_f64(hi.a == khi.a ? hi.d : -1e300);
    }
}

// Visits the ring points that the reference keeps (meterelf/_reading.py:53-69):
// set bits of `outer` (lane = row), angle within 0.25 turn of the momentum angle.
template <class F>
__device__ inline void for_each_kept(uint64_t outer, int lane, int wx0, int wy0, double cx, double cy,
                                     bool have_mom, double mom, F&& fn)
{
    const double dy = (double)(wy0 + lane) - cy;
    uint64_t bits = outer;
    while (bits) {
        const int x = __builtin_ctzll(bits);
        bits &= bits - 1;
        const double dx = (double)(wx0 + x) - cx;
        double a;
        if (angle_by_vector(dx, dy, a) && have_mom) {
            double dist = fabs(a - mom);
            const double dist2 = fabs(fabs(a - mom) - 1);
            if (dist2 < dist) dist = dist2;
            if (dist < 0.25) fn(a, dx * dx + dy * dy);
        }
    }
}

constexpr int DIAL_LIST_CAP = 768;   // candidate pixels of a dial window that take the exact float path
// Ring points (needle pixels inside the annulus) whose angles the angle phase caches.  512 since round 5: with 256 the timed
// workloads had a wave or two per batch just above it (257, 262 points), and the uncached path (an arctangent per point and pass,
// serially along the rows) cost such a wave 60 000 cycles instead of 14 000 -- and the launch, which ends with its slowest wave,
// 58 us instead of 38.  The squared distances are recomputed from the positions now (six instructions) instead of cached.
constexpr int RING_CAP = 512;
constexpr int RING_CAP_REGS = 1024;   // ... beyond the LDS cache: angles in registers, 16 per lane (positions: 2 KiB of the same LDS)
// LDS of one dial (one wave), carved from the kernel's dynamic block: the ring arrays of the angle phase re-use the
// candidate list and the in-range bits of the pixel phase (all of them dead by then).
//   [0, 4096) ra double[RING_CAP]          | pixel phase: [0, 3072) list_px u32[CAP], [3072, 4608) list_pos u16[CAP]
//   [4096, 5120) ring list u16[RING_CAP]   |              [4608, 5120) exact in-range bits, two dwords per window row
constexpr int DIAL_LDS_BYTES = 5120;
static_assert(DIAL_LIST_CAP * 4 + DIAL_LIST_CAP * 2 <= 4608 && RING_CAP * 8 + RING_CAP * 2 <= DIAL_LDS_BYTES, "dial LDS layout");

// packed 16-bit arithmetic on two values per register (v_pk_*_u16)
typedef unsigned short u16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2v, a), __builtin_bit_cast(u16x2v, b)));
}
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2v, a), __builtin_bit_cast(u16x2v, b)));
}
__device__ __forceinline__ uint32_t pk_add_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (u16x2v)(__builtin_bit_cast(u16x2v, a) + __builtin_bit_cast(u16x2v, b)));
}
__device__ __forceinline__ uint32_t pk_sub_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (u16x2v)(__builtin_bit_cast(u16x2v, a) - __builtin_bit_cast(u16x2v, b)));
}
__device__ __forceinline__ uint32_t pk_mul_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (u16x2v)(__builtin_bit_cast(u16x2v, a) * __builtin_bit_cast(u16x2v, b)));
}

// A frame's record, written by one wave: lanes 0 .. MELF_MAX_DIALS - 1 store pos[lane] / angle[lane] (zero beyond the
// context's dials), lane 0 the scalars.  Every byte of the record is written (no padding in melf_result).
__device__ __forceinline__ void write_record(melf_result* __restrict__ out, int lane, int status, int mx, int my, float mv, int failed_dial,
                                             uint32_t unreadable, double value, double pos_lane, double angle_lane)
{
    if (lane < MELF_MAX_DIALS) {
        out->pos[lane] = pos_lane;
        out->angle[lane] = angle_lane;
    }
    if (lane == 0) {
        out->status = status;
        out->match_x = mx; out->match_y = my;
        out->failed_dial = failed_dial;
        out->unreadable_mask = unreadable;
        out->match_val = mv;
        out->value = value;
    }
}
static_assert(sizeof(melf_result) == 24 + 16 * MELF_MAX_DIALS + 8, "melf_result has padding: write_record must fill it");

#ifdef MELF_DIALS_STAMP
// Diagnostic build only: shader-clock stamps at the phase boundaries of each wave (tools/dials_clock.py).
__device__ uint64_t g_dials_stamps[8 * 8192];
extern "C" __attribute__((visibility("default"))) int melf_debug_dials_stamps(uint64_t* out, int nwaves)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dials_stamps), sizeof(uint64_t) * 8 * (size_t)(nwaves < 8192 ? nwaves : 8192)) == hipSuccess ? 0 : -1;
}
// ... and the 100 MHz real-time counter at four of them (the shader-clock counters of different CUs cannot be compared) + HW_ID
__device__ uint64_t g_dials_real[8 * 8192];
extern "C" __attribute__((visibility("default"))) int melf_debug_dials_real(uint64_t* out, int nwaves)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dials_real), sizeof(uint64_t) * 8 * (size_t)(nwaves < 8192 ? nwaves : 8192)) == hipSuccess ? 0 : -1;
}
// ... and shader-clock stamps inside the closing / labelling and the momentum / angle phases
__device__ uint64_t g_dials_fine[16 * 8192];
extern "C" __attribute__((visibility("default"))) int melf_debug_dials_fine(uint64_t* out, int nwaves)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dials_fine), sizeof(uint64_t) * 16 * (size_t)(nwaves < 8192 ? nwaves : 8192)) == hipSuccess ? 0 : -1;
}
#define FSTAMPD(k) do { if (lane == 0 && (int)(blockIdx.x * (blockDim.x >> 6) + wv) < 8192) g_dials_fine[16 * (blockIdx.x * (blockDim.x >> 6) + wv) + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define DSTAMP(k) do { if (lane == 0 && (int)(blockIdx.x * (blockDim.x >> 6) + wv) < 8192) { \
        g_dials_stamps[8 * (blockIdx.x * (blockDim.x >> 6) + wv) + (k)] = __builtin_amdgcn_s_memtime(); \
        if ((k) < 6) g_dials_real[8 * (blockIdx.x * (blockDim.x >> 6) + wv) + (k)] = __builtin_amdgcn_s_memrealtime(); \
        if ((k) == 0) { uint32_t hw_; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_)); uint32_t xc_; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xc_)); \
                        g_dials_real[8 * (blockIdx.x * (blockDim.x >> 6) + wv) + 6] = hw_; g_dials_real[8 * (blockIdx.x * (blockDim.x >> 6) + wv) + 7] = xc_ & 15u; } } } while (0)
#else
#define DSTAMP(k) do { } while (0)
#define FSTAMPD(k) do { } while (0)
#endif

// Register budget: 128 of the SIMD's 512 ("amdgpu-num-vgpr" is doubled by the backend for gfx90a+'s unified file): four waves
// per SIMD, i.e. all 4 096 waves of a 1024-frame batch resident at once.  (Round 2 held it at 104 so that a wave fitted beside
// a register-capped match wave of the other caller stream; that variant is gone, and at 128 nothing spills and -- since round 4,
// tests/test_host_logic.py reads the code object's notes -- the kernel has no private segment at all.)
constexpr int DIALS_VGPRS = 64;
// NR: window rows whose pixels a lane requests up front (the largest dial window of the context, rounded up to 8)
template <bool FROM_HLS, int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_dials(DialsSrc src, melf_params P,
                                                              const DialGeom* __restrict__ geom,
                                                              const uint64_t* __restrict__ rowmasks,
                                                              const MatchPartial* __restrict__ partials,
                                                              int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialPacked<3, false, FROM_HLS>; const typename Src::Args sargs{0u};
#include "k_dials_body.inc"
}

// The other frame layouts (melf_process_frames*): RGB (BPP 3) and BGRA / RGBA (BPP 4), the channel order a runtime selector
// (swap_rb: R G B order) so that the formats share NR instantiations.
template <int BPP, int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_needles(DialsSrc src, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results, int swap_rb)
{
    using Src = DialPacked<BPP, true>; const typename Src::Args sargs{swap_rb ? 0x00020002u : 0u};
#include "k_dials_body.inc"
}

// NV12 / I420 frames (melf_process_yuv*): src describes the Y plane, yuv the chroma planes; PLANAR: separate U and V planes
// (I420, YV12) instead of interleaved pairs (NV12).  Past its loads the body is the one of 4-byte B G R pixels.  ymat: the frames'
// colour conversion, the same for every lane (SGPRs), so that the matrices share the NR instantiations.
template <bool PLANAR, int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_yneedle(DialsSrc src, YuvPlanes yuv, YuvMatrix ymat, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialYuv420<PLANAR>; const typename Src::Args sargs{yuv, ymat};
#include "k_dials_body.inc"
}

// Packed YUV 4:2:2 frames (melf_process_yuv422*): two pixels per aligned macropixel dword; psel: the byte permute that brings the
// frames' order (YUYV, UYVY, YVYU) to Y0 U Y1 V, a runtime value, so that the formats share the NR instantiations.
template <int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_p422_needle(DialsSrc src, uint32_t psel, YuvMatrix ymat, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialP422; const Src::Args sargs{psel, ymat};
#include "k_dials_body.inc"
}

// Planar / semi-planar YUV frames of any subsampling (melf_process_yuv_planar*): src describes the Y plane, yuv the chroma.  One
// instantiation per form of the chroma fetch (SUBX: log2 of the horizontal subsampling, CSTEP: bytes between the samples of a
// chroma plane) and NR; sub_y, the order of a pair's bytes and the matrix are runtime, wave-uniform values.
template <int SUBX, int CSTEP, int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_yp_needle(DialsSrc src, YuvPlanarPlanes yuv, YuvMatrix ymat, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialYuvPlanar<SUBX, CSTEP>; const typename Src::Args sargs{yuv, ymat};
#include "k_dials_body.inc"
}

// Planar / semi-planar YUV frames of 16-bit samples (melf_process_yuv16*): src describes the Y plane (strides in bytes), yuv the
// chroma and the reduction to 8 bits.  One instantiation per CSTEP (samples between the samples of a chroma plane) and NR; sub_y,
// shift, the order of a pair's samples and the matrix are runtime, wave-uniform values.
template <int CSTEP, int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_y16_needle(DialsSrc src, Yuv16Planes yuv, YuvMatrix ymat, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialYuv16<CSTEP>; const typename Src::Args sargs{yuv, ymat};
#include "k_dials_body.inc"
}

// Packed 10-bit YUV 4:2:2 frames (melf_process_yuv422_10*): v210, rows of whole 16-byte groups of six pixels, and Y210 / Y212 /
// Y216, macropixels of four 16-bit words.  Nothing but the matrix travels with the frames; one instantiation per format and NR.
template <int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_v210_needle(DialsSrc src, YuvMatrix ymat, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialV210; const Src::Args sargs{ymat};
#include "k_dials_body.inc"
}

template <int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_y210_needle(DialsSrc src, YuvMatrix ymat, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialY210; const Src::Args sargs{ymat};
#include "k_dials_body.inc"
}

// 32-bit packed 4:4:4 frames (melf_process_packed32*): one word per pixel, three 8-bit reads at the positions of `fields`; YUV: the
// reads are Y, U, V under ymat, else R, G, B (ymat is not looked at).  The positions and the matrix are the same for every lane
// (SGPRs), so that the formats of a colour kind share its NR instantiations.
template <bool YUV, int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_p32_needle(DialsSrc src, Packed32Fields fields, YuvMatrix ymat, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialWord32<YUV>; const typename Src::Args sargs{fields, ymat};
#include "k_dials_body.inc"
}

// Planar frames (melf_process_planes*): the B, G and R planes at `planes` in a frame.  Past its loads the body is the one of 4-byte
// B G R pixels.
template <int NR>
__global__ __launch_bounds__(64 * MELF_MAX_DIALS, 4) __attribute__((amdgpu_num_vgpr(DIALS_VGPRS))) void k_planar_needle(DialsSrc src, PlanarPlanes planes, melf_params P,
                                                                const DialGeom* __restrict__ geom,
                                                                const uint64_t* __restrict__ rowmasks,
                                                                const MatchPartial* __restrict__ partials,
                                                                int nparts, int rw, melf_result* __restrict__ results)
{
    using Src = DialPlanarRgb; const Src::Args sargs{planes};
#include "k_dials_body.inc"
}

// f(std::integral_constant<int, NR>) for the instantiated NR that holds ws_max window rows
template <class F>
static void with_nr(int ws_max, F&& f)
{
    if (ws_max <= 32) f(std::integral_constant<int, 32>{});
    else if (ws_max <= 40) f(std::integral_constant<int, 40>{});
    else if (ws_max <= 48) f(std::integral_constant<int, 48>{});
    else if (ws_max <= 52) f(std::integral_constant<int, 52>{});
    else if (ws_max <= 56) f(std::integral_constant<int, 56>{});
    else f(std::integral_constant<int, 64>{});
}

DialsLaunch launch_dials(const DialsSrc& src, const FrameLayout& lay, int n, const melf_params& P, const DialGeom* d_geom,
                         const uint64_t* d_rowmasks, const MatchPartial* d_partials, int nparts, int rw,
                         melf_result* d_results, hipStream_t stream, int ws_max)
{
    DialsLaunch ran = {0, -1};   // host-side note of the instantiation picked below (melf_ctx_last_dials)
    dim3 grid(n), block(64 * P.ndials);
    const size_t shmem = (size_t)P.ndials * DIAL_LDS_BYTES;
    const int pix = lay.pix;
    with_nr(ws_max, [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        ran.nr = NR;
        // lead: a kernel family's own arguments, which stand between src and P
        auto go = [&](auto kernel, auto... lead) {
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, src, lead..., P, d_geom, d_rowmasks, d_partials, nparts, rw, d_results);
        };
        auto go_needles = [&](auto kernel) {
            const int swap_rb = pix == MELF_PIX_RGB || pix == MELF_PIX_RGBA;
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, src, P, d_geom, d_rowmasks, d_partials, nparts, rw, d_results, swap_rb);
        };
        if (pix == PIX_YUV16) {
            if (lay.y16.c_step == 1) { ran.family = MELF_DIALS16_STEP1; go(k_y16_needle<1, NR>, lay.y16, *lay.mx); }
            else { ran.family = MELF_DIALS16_STEP2; go(k_y16_needle<2, NR>, lay.y16, *lay.mx); }
        }
        else if (pix == PIX_YUVP) {
            const YuvPlanarPlanes& yp = lay.yuvp;
            if (yp.sub_x == 0) {
                if (yp.c_step == 1) { ran.family = MELF_DIALS_YP_SUB0_STEP1; go(k_yp_needle<0, 1, NR>, yp, *lay.mx); }
                else { ran.family = MELF_DIALS_YP_SUB0_STEP2; go(k_yp_needle<0, 2, NR>, yp, *lay.mx); }
            } else {
                if (yp.c_step == 1) { ran.family = MELF_DIALS_YP_SUB1_STEP1; go(k_yp_needle<1, 1, NR>, yp, *lay.mx); }
                else { ran.family = MELF_DIALS_YP_SUB1_STEP2; go(k_yp_needle<1, 2, NR>, yp, *lay.mx); }
            }
        }
        else if (pix == PIX_V210) { ran.family = MELF_DIALS10_V210; go(k_v210_needle<NR>, *lay.mx); }
        else if (pix == PIX_Y210) { ran.family = MELF_DIALS10_Y210; go(k_y210_needle<NR>, *lay.mx); }
        else if (pix == PIX_P32_YUV) { ran.family = MELF_DIALS32_YUV; go(k_p32_needle<true, NR>, lay.p32, *lay.mx); }
        else if (pix == PIX_P32_RGB) { ran.family = MELF_DIALS32_RGB; go(k_p32_needle<false, NR>, lay.p32, YuvMatrix{}); }
        else if (pix == PIX_PLANAR) { ran.family = MELF_DIALS_PLANAR; go(k_planar_needle<NR>, lay.planes); }
        else if (pix_p422(pix)) { ran.family = MELF_DIALS_P422; go(k_p422_needle<NR>, p422_sel(pix), *lay.mx); }
        else if (pix == PIX_NV12) { ran.family = MELF_DIALS_NV12; go(k_yneedle<false, NR>, lay.yuv, *lay.mx); }
        else if (pix == PIX_I420) { ran.family = MELF_DIALS_I420; go(k_yneedle<true, NR>, lay.yuv, *lay.mx); }
        else if (pix == PIX_PLANE) { ran.family = MELF_DIALS_HLS; go(k_dials<true, NR>); }
        else if (pix == MELF_PIX_BGR) { ran.family = MELF_DIALS_BGR; go(k_dials<false, NR>); }
        else if (pix == MELF_PIX_RGB) { ran.family = MELF_DIALS_PACKED3; go_needles(k_needles<3, NR>); }
        else { ran.family = MELF_DIALS_PACKED4; go_needles(k_needles<4, NR>); }
    });
    return ran;
}

}  // namespace melf
