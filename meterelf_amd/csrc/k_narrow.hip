// k_narrow_rows: writes the meter crop of frames of WIDE samples (melf_process_wide_dev: 16-bit words, float16, bfloat16, float32)
// into a staged batch of bytes in HBM, which the reading kernels then take as one contiguous 8-bit batch -- the third sibling of
// k_gather_rows and k_orient_tiles: the same staged frames, from a source whose every sample is narrowed on the way (melf_narrow.h:
// the rule, shared with the host packer).  The launch shape is k_gather_rows': one wave per (frame, run, block of ROWS_PER_WAVE
// rows), a lane per aligned 16-byte piece of a staged row.  A piece is 16 consecutive samples, 32 or 64 source bytes, fetched with
// two or four 16-byte loads at the caller's alignment (a multiple of the sample size, no more), converted in registers and written
// with one 16-byte store; the last piece of a row takes its 1 .. 15 samples one by one.  Every address comes from
// melf_narrow_addr.h, which says what is loaded and why nothing behind a row's last sample or outside a frame's extent is.  No LDS.
// Two siblings with the same launch shape and the same per-wave body (narrow_wave_rows) take their source from a pointer table:
// k_narrow_list_rows from one pointer per frame (melf_process_wide_list_dev), k_narrow_plane_rows from one pointer per plane
// (melf_process_wide_plane_list_dev) -- what k_gather_rows and k_plane_rows are to a copy.
//
// TYPE: MELF_WIDE_*.  C: the samples of a packed pixel, 3 or 4, or 1 for planes.  Which scale and offset a sample takes follows from
// its position in the pixel: for C == 4 that is the sample's index in the piece mod 4, a constant of the unrolled loop; for C == 3
// the piece's phase (16 piece mod 3) rotates the three values once per piece, after which it is a constant too; for C == 1 it is the
// run's index, the same for the whole wave.
#include "melf_internal.h"
#include "melf_narrow_addr.h"

namespace melf {

typedef const __attribute__((address_space(1))) uint8_t* global_wide;

template <class T>
static __device__ __forceinline__ T load_wide(global_wide p)
{
    T v;
    __builtin_memcpy(&v, p, sizeof(T));   // any alignment: the source rows have the caller's
    return v;
}

// the three values v[(phase + i) % 3], i = 0 .. 2, without indexing an array by a runtime value
static __device__ __forceinline__ void rotate3(const uint32_t phase, const float a, const float b, const float c, float out[3])
{
    out[0] = phase == 0 ? a : (phase == 1 ? b : c);
    out[1] = phase == 0 ? b : (phase == 1 ? c : a);
    out[2] = phase == 0 ? c : (phase == 1 ? a : b);
}

// The rows of one wave, shared by the three kernels: lane by lane the 16-sample pieces of rows [wr.row0, wr.row0 + wr.nrows) of wr.run
// from src (wr.run.src_off counts samples from it; `extent` samples of it are readable) into the staged frame at dst.  plane: the
// run's index, the position of every sample for C == 1.
template <int TYPE, int C>
static __device__ __forceinline__ void narrow_wave_rows(const global_wide src, uint8_t* __restrict__ dst, const gather::WaveRows& wr,
                                                        const uint32_t plane, const uint64_t extent, const narrow::Rule& rule)
{
    constexpr int SS = TYPE == MELF_WIDE_F32 ? 4 : 2;          // bytes of a sample
    constexpr int SPW = 4 / SS;                                 // samples of a loaded dword
    constexpr int WORDS = narrow::PIECE / SPW;                  // dwords of a piece's samples: 8 or 16
    const int shift = rule.shift;
    const bool floor_ = rule.floor_ != 0;
    const float s0 = rule.scale[0], s1 = rule.scale[1], s2 = rule.scale[2];
    const float o0 = rule.offset[0], o1 = rule.offset[1], o2 = rule.offset[2];
    // C == 1: the plane's values, the same for the wave
    const float sp = plane == 0 ? s0 : (plane == 1 ? s1 : s2), op = plane == 0 ? o0 : (plane == 1 ? o1 : o2);

    const uint32_t ppr = gather::row_pieces(wr.run.row_bytes), total = ppr * wr.nrows;
    for (uint32_t i = threadIdx.x & 63; i < total; i += 64) {
        const uint32_t r = i / ppr, piece = i - r * ppr;
        const narrow::Samples p = narrow::samples_of(wr.run, wr.row0 + r, piece);
        if (!narrow::samples_readable(p, extent)) continue;
        const global_wide s = src + p.sample * (uint64_t)SS;
        float sc[3], of[3];   // by (sample index in the piece) % 3 for C == 3; [c] = position c for C == 4
        if (C == 3) {
            const uint32_t phase = narrow::piece_phase(piece, 3);
            rotate3(phase, s0, s1, s2, sc);
            rotate3(phase, o0, o1, o2, of);
        } else {
            sc[0] = s0; sc[1] = s1; sc[2] = s2;
            of[0] = o0; of[1] = o1; of[2] = o2;
        }
        uint32_t out[4] = {0, 0, 0, 0};
        if (p.count == (uint32_t)narrow::PIECE) {
            uint32_t w[WORDS];
#pragma unroll
            for (int q = 0; q < WORDS / 4; ++q) {
                const uint4 v = load_wide<uint4>(s + 16 * q);
                w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < narrow::PIECE; ++j) {
                if (C == 4 && (j & 3) == 3) continue;   // the 4th sample is never converted: its byte is 0
                const uint32_t bits = SS == 4 ? w[j] : (w[j / 2] >> (16 * (j & 1))) & 0xffffu;
                const int c = C == 4 ? (j & 3) : j % 3;
                const uint32_t b = narrow::narrow_sample<TYPE>(bits, shift, C == 1 ? sp : sc[c], C == 1 ? op : of[c], floor_);
                out[j / 4] |= b << (8 * (j & 3));
            }
        } else {
#pragma unroll
            for (int j = 0; j < narrow::PIECE - 1; ++j) {
                if (C == 4 && (j & 3) == 3) continue;
                if ((uint32_t)j < p.count) {
                    const uint32_t bits = SS == 4 ? load_wide<uint32_t>(s + 4 * j) : (uint32_t)load_wide<uint16_t>(s + 2 * j);
                    const int c = C == 4 ? (j & 3) : j % 3;
                    const uint32_t b = narrow::narrow_sample<TYPE>(bits, shift, C == 1 ? sp : sc[c], C == 1 ? op : of[c], floor_);
                    out[j / 4] |= b << (8 * (j & 3));
                }
            }
        }
        *(uint4*)(dst + p.dst_off) = uint4{out[0], out[1], out[2], out[3]};   // 16-byte aligned: dst_off, dst_pitch and staged_stride are multiples of 64 (+ 128)
    }
}

// One batch: frame f at frames + f * frame_stride (melf_process_wide_dev)
template <int TYPE, int C>
__global__ void __launch_bounds__(64 * gather::WAVES_PER_BLOCK)
k_narrow_rows(const uint8_t* __restrict__ frames, const size_t frame_stride, const RowRuns runs, const narrow::Rule rule,
              uint8_t* __restrict__ staged, const size_t staged_stride, const size_t extent, const uint32_t waves_per_frame)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * gather::WAVES_PER_BLOCK + threadIdx.x / 64);
    if (wave >= waves_per_frame) return;
    const uint32_t f = blockIdx.y;
    const gather::WaveRows wr = gather::wave_rows(runs, wave);
    const uint32_t plane = gather::wave_run(runs, wave);
    const global_wide src = (global_wide)(frames + (size_t)f * frame_stride);
    narrow_wave_rows<TYPE, C>(src, staged + (size_t)f * staged_stride, wr, plane, extent, rule);
}

// Frames in separate allocations (melf_process_wide_list_dev): frame f at frames[f], a table of n device pointers in HBM.  f is the
// same for the whole wave -- a scalar load --, and the pointer is cast to global memory as k_gather_rows does it, so that the
// samples are fetched with global, not flat, loads.  extent: one frame's, in samples.
template <int TYPE, int C>
__global__ void __launch_bounds__(64 * gather::WAVES_PER_BLOCK)
k_narrow_list_rows(const uint8_t* const* __restrict__ frames, const RowRuns runs, const narrow::Rule rule, uint8_t* __restrict__ staged,
                   const size_t staged_stride, const size_t extent, const uint32_t waves_per_frame)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * gather::WAVES_PER_BLOCK + threadIdx.x / 64);
    if (wave >= waves_per_frame) return;
    const uint32_t f = blockIdx.y;
    const gather::WaveRows wr = gather::wave_rows(runs, wave);
    const uint32_t plane = gather::wave_run(runs, wave);
    const global_wide src = (global_wide)frames[f];
    narrow_wave_rows<TYPE, C>(src, staged + (size_t)f * staged_stride, wr, plane, extent, rule);
}

// A frame's planes in separate allocations (melf_process_wide_plane_list_dev): three pointers per frame, frame-major; run k of the
// plan is plane slot k (B / G / R), so a wave takes its source from planes[f * 3 + k] -- f and k are the same for the whole wave: a
// scalar load --, counts its samples from that plane's own pointer and tests its pieces against the samples readable from it
// (split, in samples: melf_narrow_addr.h).  Scale and offset are those of position k.  C is 1.
template <int TYPE>
__global__ void __launch_bounds__(64 * gather::WAVES_PER_BLOCK)
k_narrow_plane_rows(const uint8_t* const* __restrict__ planes, const RowRuns runs, const PlaneSplit split, const narrow::Rule rule,
                    uint8_t* __restrict__ staged, const size_t staged_stride, const uint32_t waves_per_frame)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * gather::WAVES_PER_BLOCK + threadIdx.x / 64);
    if (wave >= waves_per_frame) return;
    const uint32_t f = blockIdx.y;
    const gather::PlaneRows pr = gather::plane_rows(runs, split, wave);
    const global_wide src = (global_wide)planes[(size_t)f * 3 + pr.k];
    narrow_wave_rows<TYPE, 1>(src, staged + (size_t)f * staged_stride, pr.wr, pr.k, pr.extent, rule);
}

template <int TYPE>
static void launch_narrow_type(const dim3 grid, hipStream_t stream, const uint8_t* frames, size_t frame_stride, const RowRuns& runs,
                               const narrow::Rule& rule, uint8_t* d_staged, size_t staged_stride, size_t extent, uint32_t waves)
{
    const dim3 block(64 * gather::WAVES_PER_BLOCK);
    switch (rule.channels) {
    case 1: hipLaunchKernelGGL((k_narrow_rows<TYPE, 1>), grid, block, 0, stream, frames, frame_stride, runs, rule, d_staged, staged_stride, extent, waves); break;
    case 3: hipLaunchKernelGGL((k_narrow_rows<TYPE, 3>), grid, block, 0, stream, frames, frame_stride, runs, rule, d_staged, staged_stride, extent, waves); break;
    default: hipLaunchKernelGGL((k_narrow_rows<TYPE, 4>), grid, block, 0, stream, frames, frame_stride, runs, rule, d_staged, staged_stride, extent, waves); break;
    }
}

void launch_narrow_rows(const void* d_frames, size_t frame_stride, int n, const RowRuns& runs, const narrow::Rule& rule, uint8_t* d_staged,
                        size_t staged_stride, size_t extent, hipStream_t stream)
{
    const uint32_t waves = gather::frame_waves(runs);
    if (n <= 0 || waves == 0) return;
    const dim3 grid((waves + gather::WAVES_PER_BLOCK - 1) / gather::WAVES_PER_BLOCK, (uint32_t)n);
    const uint8_t* frames = (const uint8_t*)d_frames;
    switch (rule.type) {
    case MELF_WIDE_U16: launch_narrow_type<MELF_WIDE_U16>(grid, stream, frames, frame_stride, runs, rule, d_staged, staged_stride, extent, waves); break;
    case MELF_WIDE_F16: launch_narrow_type<MELF_WIDE_F16>(grid, stream, frames, frame_stride, runs, rule, d_staged, staged_stride, extent, waves); break;
    case MELF_WIDE_BF16: launch_narrow_type<MELF_WIDE_BF16>(grid, stream, frames, frame_stride, runs, rule, d_staged, staged_stride, extent, waves); break;
    default: launch_narrow_type<MELF_WIDE_F32>(grid, stream, frames, frame_stride, runs, rule, d_staged, staged_stride, extent, waves); break;
    }
}

template <int TYPE>
static void launch_narrow_list_type(const dim3 grid, hipStream_t stream, const uint8_t* const* frames, const RowRuns& runs, const narrow::Rule& rule,
                                    uint8_t* d_staged, size_t staged_stride, size_t extent, uint32_t waves)
{
    const dim3 block(64 * gather::WAVES_PER_BLOCK);
    switch (rule.channels) {
    case 1: hipLaunchKernelGGL((k_narrow_list_rows<TYPE, 1>), grid, block, 0, stream, frames, runs, rule, d_staged, staged_stride, extent, waves); break;
    case 3: hipLaunchKernelGGL((k_narrow_list_rows<TYPE, 3>), grid, block, 0, stream, frames, runs, rule, d_staged, staged_stride, extent, waves); break;
    default: hipLaunchKernelGGL((k_narrow_list_rows<TYPE, 4>), grid, block, 0, stream, frames, runs, rule, d_staged, staged_stride, extent, waves); break;
    }
}

// d_frames: n device pointers in HBM; extent: samples readable from each
void launch_narrow_list_rows(const void* const* d_frames, int n, const RowRuns& runs, const narrow::Rule& rule, uint8_t* d_staged, size_t staged_stride,
                             size_t extent, hipStream_t stream)
{
    const uint32_t waves = gather::frame_waves(runs);
    if (n <= 0 || waves == 0) return;
    const dim3 grid((waves + gather::WAVES_PER_BLOCK - 1) / gather::WAVES_PER_BLOCK, (uint32_t)n);
    const uint8_t* const* frames = (const uint8_t* const*)d_frames;
    switch (rule.type) {
    case MELF_WIDE_U16: launch_narrow_list_type<MELF_WIDE_U16>(grid, stream, frames, runs, rule, d_staged, staged_stride, extent, waves); break;
    case MELF_WIDE_F16: launch_narrow_list_type<MELF_WIDE_F16>(grid, stream, frames, runs, rule, d_staged, staged_stride, extent, waves); break;
    case MELF_WIDE_BF16: launch_narrow_list_type<MELF_WIDE_BF16>(grid, stream, frames, runs, rule, d_staged, staged_stride, extent, waves); break;
    default: launch_narrow_list_type<MELF_WIDE_F32>(grid, stream, frames, runs, rule, d_staged, staged_stride, extent, waves); break;
    }
}

// d_planes: n * 3 device pointers in HBM, frame-major; split: in samples (narrow::wide_plane_split)
void launch_narrow_plane_rows(const void* const* d_planes, int n, const RowRuns& runs, const PlaneSplit& split, const narrow::Rule& rule,
                              uint8_t* d_staged, size_t staged_stride, hipStream_t stream)
{
    const uint32_t waves = gather::frame_waves(runs);
    // runs.count != 3 or packed samples do not happen: the plan of a wide plane list is a planar one, three runs of one sample a
    // pixel.  The test stays as the bound of the table read: run index < 3.
    if (n <= 0 || waves == 0 || runs.count != 3 || rule.channels != 1) return;
    const dim3 grid((waves + gather::WAVES_PER_BLOCK - 1) / gather::WAVES_PER_BLOCK, (uint32_t)n), block(64 * gather::WAVES_PER_BLOCK);
    const uint8_t* const* planes = (const uint8_t* const*)d_planes;
    switch (rule.type) {
    case MELF_WIDE_U16: hipLaunchKernelGGL((k_narrow_plane_rows<MELF_WIDE_U16>), grid, block, 0, stream, planes, runs, split, rule, d_staged, staged_stride, waves); break;
    case MELF_WIDE_F16: hipLaunchKernelGGL((k_narrow_plane_rows<MELF_WIDE_F16>), grid, block, 0, stream, planes, runs, split, rule, d_staged, staged_stride, waves); break;
    case MELF_WIDE_BF16: hipLaunchKernelGGL((k_narrow_plane_rows<MELF_WIDE_BF16>), grid, block, 0, stream, planes, runs, split, rule, d_staged, staged_stride, waves); break;
    default: hipLaunchKernelGGL((k_narrow_plane_rows<MELF_WIDE_F32>), grid, block, 0, stream, planes, runs, split, rule, d_staged, staged_stride, waves); break;
    }
}

}  // namespace melf
