// k_gather_rows: the device-side twin of the host-fed path's packer.  Copies the row runs of a staging plan (melf_stage_plan.h) from
// n separately allocated frames -- a table of n device pointers -- into a staged batch in HBM, which the reading kernels then take
// as one contiguous batch.  Purely a copy: no byte is converted or reordered.  One wave per (frame, run, block of ROWS_PER_WAVE
// rows): a crop row is 250 to 1000 bytes, so a wave's loads are a few contiguous rows of one frame, and its lanes walk the block's
// 16-byte pieces row after row.  Every address comes from melf_gather_addr.h, which says what is loaded and why nothing outside a
// frame's `extent` bytes is.  k_plane_rows, below it, is the same copy from a table of one pointer per PLANE.
#include "melf_internal.h"
#include "melf_gather_addr.h"

namespace melf {

// A frame's pointer comes out of the table in memory, so the compiler cannot see that it points to global memory and would load
// through it with flat instructions: say so.
typedef const __attribute__((address_space(1))) uint8_t* global_bytes;

template <class T>
static __device__ __forceinline__ T load_at(global_bytes p)
{
    T v;
    __builtin_memcpy(&v, p, sizeof(T));   // any alignment: the source rows have the caller's
    return v;
}

// The rows of one wave, shared by the two kernels: lane by lane the 16-byte pieces of rows [wr.row0, wr.row0 + wr.nrows) of wr.run, from
// src (wr.run.src_off counts from it; `extent` bytes of it are readable) into the staged frame at dst
static __device__ __forceinline__ void copy_wave_rows(const global_bytes src, uint8_t* __restrict__ dst, const gather::WaveRows& wr, const uint64_t extent)
{
    const uint32_t ppr = gather::row_pieces(wr.run.row_bytes), total = ppr * wr.nrows;
    for (uint32_t i = threadIdx.x & 63; i < total; i += 64) {
        const uint32_t r = i / ppr, piece = i - r * ppr;
        const gather::Piece p = gather::piece_of(wr.run, wr.row0 + r, piece);
        if (!gather::piece_readable(p, extent)) continue;
        const global_bytes s = src + p.src_off;
        uint4 v = {0, 0, 0, 0};
        if (p.bytes == (uint32_t)gather::PIECE) {
            v = load_at<uint4>(s);
        } else {
            // 1 .. 15 bytes: exactly the row's, by the binary digits of the count
            uint64_t lo = 0;     // bytes 0 .. 7 of the piece
            uint64_t hi = 0;     // bytes 8 .. 15
            if (gather::tail_has(p.bytes, 8)) lo = load_at<uint64_t>(s);
            uint64_t rest = 0;   // up to 7 bytes behind the 8-byte load, if any
            if (gather::tail_has(p.bytes, 4)) rest = load_at<uint32_t>(s + gather::tail_at(p.bytes, 4));
            if (gather::tail_has(p.bytes, 2)) rest |= (uint64_t)load_at<uint16_t>(s + gather::tail_at(p.bytes, 2)) << (8 * (gather::tail_at(p.bytes, 2) & 7));
            if (gather::tail_has(p.bytes, 1)) rest |= (uint64_t)load_at<uint8_t>(s + gather::tail_at(p.bytes, 1)) << (8 * (gather::tail_at(p.bytes, 1) & 7));
            if (gather::tail_has(p.bytes, 8)) hi = rest; else lo = rest;
            v = uint4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
        }
        *(uint4*)(dst + p.dst_off) = v;   // 16-byte aligned: dst_off, dst_pitch and staged_stride are multiples of 64 (+ 128)
    }
}

__global__ void __launch_bounds__(64 * gather::WAVES_PER_BLOCK)
k_gather_rows(const uint8_t* const* __restrict__ frames, const RowRuns runs, uint8_t* __restrict__ staged, const size_t staged_stride,
              const size_t extent, const uint32_t waves_per_frame)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * gather::WAVES_PER_BLOCK + threadIdx.x / 64);
    if (wave >= waves_per_frame) return;
    const uint32_t f = blockIdx.y;
    const gather::WaveRows wr = gather::wave_rows(runs, wave);
    const global_bytes src = (global_bytes)frames[f];
    uint8_t* __restrict__ dst = staged + (size_t)f * staged_stride;
    copy_wave_rows(src, dst, wr, extent);
}

void launch_gather_rows(const void* const* d_frames, int n, const RowRuns& runs, uint8_t* d_staged, size_t staged_stride, size_t extent,
                        hipStream_t stream)
{
    const uint32_t waves = gather::frame_waves(runs);
    if (n <= 0 || waves == 0) return;
    const dim3 grid((waves + gather::WAVES_PER_BLOCK - 1) / gather::WAVES_PER_BLOCK, (uint32_t)n);
    hipLaunchKernelGGL(k_gather_rows, grid, dim3(64 * gather::WAVES_PER_BLOCK), 0, stream, (const uint8_t* const*)d_frames, runs, d_staged,
                       staged_stride, extent, waves);
}

// k_plane_rows: the same copy for frames whose planes lie in separate allocations (melf_process_plane_list_dev).  The table holds
// nplanes pointers per frame, frame-major; run k of the plan is plane slot k (melf_stage_plan.h: plane_split), so a wave takes its
// source from planes[f * nplanes + k] -- f and k are the same for the whole wave: a scalar load -- and tests its pieces against the
// bytes readable from that plane's own pointer.  One launch for all planes, the launch shape of k_gather_rows.
__global__ void __launch_bounds__(64 * gather::WAVES_PER_BLOCK)
k_plane_rows(const uint8_t* const* __restrict__ planes, const uint32_t nplanes, const RowRuns runs, const PlaneSplit split,
             uint8_t* __restrict__ staged, const size_t staged_stride, const uint32_t waves_per_frame)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * gather::WAVES_PER_BLOCK + threadIdx.x / 64);
    if (wave >= waves_per_frame) return;
    const uint32_t f = blockIdx.y;
    const gather::PlaneRows pr = gather::plane_rows(runs, split, wave);
    const global_bytes src = (global_bytes)planes[(size_t)f * nplanes + pr.k];
    uint8_t* __restrict__ dst = staged + (size_t)f * staged_stride;
    copy_wave_rows(src, dst, pr.wr, pr.extent);
}

void launch_plane_rows(const void* const* d_planes, int nplanes, int n, const RowRuns& runs, const PlaneSplit& split, uint8_t* d_staged,
                       size_t staged_stride, hipStream_t stream)
{
    const uint32_t waves = gather::frame_waves(runs);
    // nplanes != runs.count does not happen: a plan of a plane list has one run per plane, and both callers (melf_api.hip) return
    // MELF_ERR_INVALID with a message before they get here.  The test stays as the bound of the table read: run index < nplanes.
    if (n <= 0 || waves == 0 || nplanes != runs.count) return;
    const dim3 grid((waves + gather::WAVES_PER_BLOCK - 1) / gather::WAVES_PER_BLOCK, (uint32_t)n);
    hipLaunchKernelGGL(k_plane_rows, grid, dim3(64 * gather::WAVES_PER_BLOCK), 0, stream, (const uint8_t* const*)d_planes, (uint32_t)nplanes, runs,
                       split, d_staged, staged_stride, waves);
}

}  // namespace melf
