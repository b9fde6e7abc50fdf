// Baseline JPEG files without restart markers whose scan is longer than k_jpeg_huff addresses (melf_ctx_set_jpeg_long_scans),
// host-only arithmetic: the chapter plan that k_jpeg_chapters (k_jpeg.hip), the host half of a batch and tests/jpeg_long_main.cpp share.
//
// k_jpeg_huff gives every lane one segment of the stream and keeps bit positions inside a segment in 16 bits: a segment holds at most
// MAX_SEG_BITS bits, a scan at most T segments.  k_jpeg_chapters cuts the scan into consecutive CHAPTERS of T segments of S bits each
// and takes them one after the other; a chapter is to it what the whole scan is to k_jpeg_huff.
//   seg_dwords()      S / 32 for a wanted chapter length, by k_jpeg_huff's rule: a multiple of 32 bits with an odd dword count (the
//                     lanes' stream reads then fall into different banks), at least 9 dwords, at most 999 (S <= 32 000)
//   chapter_bytes()   the chapter length that S gives
//   chapters()        how many chapters a stream of `bits` bits has
//   chapter()         chapter c's bit range [bit0, bit1) and its segments
//   seg_end()         where segment i of a chapter stops being decoded
//   MAX_SCAN_BYTES    the longest scan that is taken
// All positions are 32-bit, as in the kernels.  What may be computed without wrapping:
//   * bits = 8 n, and the decoders' stop 32 bits into the zero padding, bits + 32; a symbol that begins below the stop ends below
//     bits + 63 (a step consumes fewer than 32 bits);
//   * the nominal end of a segment, bit0 + (i + 1) S, before it is clamped to bits + 32: at most the end of the last chapter,
//     bit0 + T S < bits + T S.
// So 8 n + T * MAX_SEG_BITS + 64 <= 2^32 keeps every such sum below 2^32: n <= (2^32 - 1024 * 32 000 - 64) / 8 = 532 774 904 bytes.
// (Byte offsets into a batch's scan area are 32-bit too: a batch beyond 2^32 bytes is refused as ever, MELF_ERR_TOO_LARGE.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MELF_LONG_HD __host__ __device__ __forceinline__
#else
#define MELF_LONG_HD inline
#endif

namespace melf {
namespace jpeg_long {

constexpr uint32_t T = 1024;                 // segments of a chapter: the lanes of k_jpeg_chapters's workgroup
constexpr uint32_t MAX_SEG_BITS = 32000;     // the state-only decoder's 16-bit positions (k_jpeg.hip: jpeg_state_segment)
constexpr uint32_t MIN_SEG_DWORDS = 9;       // 8 | 1
constexpr uint32_t MAX_SEG_DWORDS = 999;     // the largest odd d with 32 d <= MAX_SEG_BITS
constexpr uint64_t MAX_SCAN_BYTES = ((1ull << 32) - (uint64_t)T * MAX_SEG_BITS - 64u) / 8u;
static_assert(MAX_SCAN_BYTES == 532774904ull, "the derivation above");
static_assert(32u * MAX_SEG_DWORDS <= MAX_SEG_BITS && 32u * (MAX_SEG_DWORDS + 2u) > MAX_SEG_BITS && (MAX_SEG_DWORDS & 1u), "largest odd dword count");

// Dwords per segment for chapters of (at least) `want` bytes: max(8, ceil(bits / (32 T))) | 1, capped at the largest the kernel addresses.
MELF_LONG_HD uint32_t seg_dwords(const uint64_t want)
{
    uint64_t d = (want * 8u + 32u * T - 1u) / (32u * T);
    if (d < 8u) d = 8u;
    d |= 1u;
    return d > MAX_SEG_DWORDS ? MAX_SEG_DWORDS : (uint32_t)d;
}
MELF_LONG_HD uint32_t chapter_bytes(const uint32_t d) { return T * 4u * d; }   // T segments of 32 d bits
constexpr uint32_t PRODUCTION_CHAPTER_BYTES = T * 4u * MAX_SEG_DWORDS;        // 4 091 904

MELF_LONG_HD bool taken(const uint64_t n) { return n <= MAX_SCAN_BYTES; }

// Chapters of a stream of `bits` bits (bits = 8 n, n taken) with segments of d dwords.
MELF_LONG_HD uint32_t chapters(const uint32_t bits, const uint32_t d)
{
    const uint32_t cb = T * 32u * d;
    return bits / cb + (bits % cb ? 1u : 0u);
}

struct Chapter {
    uint32_t bit0, bit1;   // [bit0, bit1): bit1 = min(bit0 + T S, bits)
    uint32_t nseg;         // segments that hold a bit of it: ceil((bit1 - bit0) / S), 1..T
};
MELF_LONG_HD Chapter chapter(const uint32_t bits, const uint32_t d, const uint32_t c)
{
    const uint32_t S = 32u * d, cb = T * S;
    Chapter k;
    k.bit0 = c * cb;                                        // c < chapters(): below bits
    k.bit1 = bits - k.bit0 > cb ? k.bit0 + cb : bits;
    k.nseg = (k.bit1 - k.bit0 + S - 1u) / S;
    return k;
}
// Segment i of a chapter that begins at bit0 is decoded up to here: its nominal end, or 32 bits into the zero padding behind the stream.
MELF_LONG_HD uint32_t seg_end(const uint32_t bits, const uint32_t d, const uint32_t bit0, const uint32_t i)
{
    const uint32_t e = bit0 + (i + 1u) * 32u * d, stop = bits + 32u;
    return e < stop ? e : stop;
}

}  // namespace jpeg_long
}  // namespace melf
