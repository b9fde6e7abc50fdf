// k_orient_tiles: writes the meter crop of frames that are stored mirrored or transposed (EXIF orientations 2-8) upright into a
// staged batch in HBM, which the reading kernels then take as one contiguous batch -- the staged frames of the frame lists, from a
// source that is a permutation of the crop's elements.  One workgroup per (frame, run, tile of TILE x TILE elements): it loads the
// tile's source rectangle along the STORED rows, so that the loads are contiguous, into LDS, synchronises, reads LDS in destination
// order and writes the destination rows in aligned 16-byte pieces.  Every address comes from melf_orient_addr.h, which says what is
// loaded and stored and why nothing outside a frame's `extent` bytes is read.
//
// Load widths: a stored row of the tile is 64 to 256 contiguous bytes at whatever alignment the family's check leaves (any, for
// byte planes and 3-byte pixels), so it is fetched as the frame lists' rows are: 16-byte loads from the rectangle's first byte,
// which the memory system takes unaligned, and the last 1 .. 15 bytes by the binary digits of their count.  They go into LDS as
// four dwords (the rows of the LDS tile start on 4-byte, not 16-byte boundaries: the pitch is an odd number of dwords).  The read
// side is element-granular -- a byte, a 16-bit or a 32-bit LDS read per element, byte reads for 3-byte pixels --: the launch moves
// twice the crop's bytes through HBM, and that, not LDS issue, is its bound.
//
// EB: the bytes of an element of the frame's FIRST run.  The chroma runs of a semi-planar frame have elements twice that size (the
// interleaved pair); which of the two a tile has is the same for the whole workgroup.
#include "melf_internal.h"
#include "melf_orient_addr.h"

namespace melf {

typedef const __attribute__((address_space(1))) uint8_t* global_src;

template <class T>
static __device__ __forceinline__ T load_src(global_src p)
{
    T v;
    __builtin_memcpy(&v, p, sizeof(T));   // any alignment: the stored rows have the caller's
    return v;
}

// the 1 .. 16 bytes of a load piece, the others zero
static __device__ __forceinline__ uint4 load_piece(global_src s, const uint32_t bytes)
{
    if (bytes == (uint32_t)orient::PIECE) return load_src<uint4>(s);
    uint64_t lo = 0, hi = 0, rest = 0;   // bytes 0 .. 7, 8 .. 15; up to 7 bytes behind the 8-byte load, if any
    if (orient::tail_has(bytes, 8)) lo = load_src<uint64_t>(s);
    if (orient::tail_has(bytes, 4)) rest = load_src<uint32_t>(s + orient::tail_at(bytes, 4));
    if (orient::tail_has(bytes, 2)) rest |= (uint64_t)load_src<uint16_t>(s + orient::tail_at(bytes, 2)) << (8 * (orient::tail_at(bytes, 2) & 7));
    if (orient::tail_has(bytes, 1)) rest |= (uint64_t)load_src<uint8_t>(s + orient::tail_at(bytes, 1)) << (8 * (orient::tail_at(bytes, 1) & 7));
    if (orient::tail_has(bytes, 8)) hi = rest; else lo = rest;
    return uint4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

// One tile of elements of E bytes: src the stored frame, dst its staged frame, lds the workgroup's tile
template <int E>
static __device__ __forceinline__ void orient_tile(const global_src src, uint8_t* __restrict__ dst, const orient::Tile& t, const int code,
                                                   const uint64_t extent, uint8_t* lds)
{
    const uint32_t lpr = orient::load_pieces(t), loads = lpr * t.srows;
    for (uint32_t i = threadIdx.x; i < loads; i += orient::THREADS) {
        const uint32_t s = i / lpr, piece = i - s * lpr;
        const orient::Load l = orient::load_of(t, s, piece);
        uint4 v = {0, 0, 0, 0};
        if (orient::load_readable(l, extent)) v = load_piece(src + l.src_off, l.bytes);
        uint32_t* w = (uint32_t*)(lds + l.lds_off);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __syncthreads();
    const orient::LdsMap m = orient::lds_map(t, code);
    const uint32_t spr = orient::store_pieces(t), stores = spr * t.nr;
    for (uint32_t i = threadIdx.x; i < stores; i += orient::THREADS) {
        const uint32_t r = i / spr, piece = i - r * spr;
        const orient::Store st = orient::store_of(t, r, piece);
        uint32_t w[4] = {0, 0, 0, 0};
        if constexpr (E == 4) {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t e = piece * 4 + j;
                if (e < t.nc) w[j] = *(const uint32_t*)(lds + orient::lds_elem(m, r, e));
            }
        } else if constexpr (E == 2) {
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t e = piece * 8 + j;
                if (e < t.nc) w[j / 2] |= (uint32_t)*(const uint16_t*)(lds + orient::lds_elem(m, r, e)) << (16 * (j & 1));
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t d = piece * 16 + j, e = E == 1 ? d : d / 3, q = E == 1 ? 0 : d - 3 * e;   // byte q of element e
                if (e < t.nc) w[j / 4] |= (uint32_t)lds[orient::lds_elem(m, r, e) + q] << (8 * (j & 3));
            }
        }
        *(uint4*)(dst + st.dst_off) = uint4{w[0], w[1], w[2], w[3]};   // 16-byte aligned: dst_off, dst_pitch, staged_stride are multiples of 64 (+ 128)
    }
}

template <int EB>
__global__ void __launch_bounds__(orient::THREADS)
k_orient_tiles(const uint8_t* __restrict__ frames, const size_t frame_stride, const orient::Runs runs, uint8_t* __restrict__ staged,
               const size_t staged_stride)
{
    constexpr int EMAX = EB <= 2 ? 2 * EB : EB;
    __shared__ __attribute__((aligned(16))) uint8_t lds[orient::TILE * (orient::TILE * EMAX + 4)];
    const orient::Tile t = orient::tile_of(runs, blockIdx.x);
    const uint32_t f = blockIdx.y;
    const global_src src = (global_src)(frames + (size_t)f * frame_stride);
    uint8_t* __restrict__ dst = staged + (size_t)f * staged_stride;
    if (EB <= 2 && t.run.eb != (uint32_t)EB)
        orient_tile<EMAX>(src, dst, t, runs.code, runs.extent, lds);
    else
        orient_tile<EB>(src, dst, t, runs.code, runs.extent, lds);
}

void launch_orient_tiles(const void* d_frames, size_t frame_stride, int n, const orient::Runs& runs, uint8_t* d_staged, size_t staged_stride,
                         hipStream_t stream)
{
    const uint32_t tiles = orient::frame_tiles(runs);
    if (n <= 0 || tiles == 0) return;
    const dim3 grid(tiles, (uint32_t)n), block(orient::THREADS);
    const uint8_t* frames = (const uint8_t*)d_frames;
    switch (runs.run[0].eb) {
    case 1: hipLaunchKernelGGL(k_orient_tiles<1>, grid, block, 0, stream, frames, frame_stride, runs, d_staged, staged_stride); break;
    case 2: hipLaunchKernelGGL(k_orient_tiles<2>, grid, block, 0, stream, frames, frame_stride, runs, d_staged, staged_stride); break;
    case 3: hipLaunchKernelGGL(k_orient_tiles<3>, grid, block, 0, stream, frames, frame_stride, runs, d_staged, staged_stride); break;
    default: hipLaunchKernelGGL(k_orient_tiles<4>, grid, block, 0, stream, frames, frame_stride, runs, d_staged, staged_stride); break;
    }
}

}  // namespace melf
