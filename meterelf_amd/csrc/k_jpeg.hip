// Baseline JPEG decode on the GPU: replaces the host decode behind
// cv2.imread (meterelf/_image.py:49) for the files the meter cameras write -- baseline sequential
// DCT, 8 bit, Huffman, one interleaved scan, YCbCr 4:2:0 / 4:2:2 / 4:4:4 or greyscale (and 4:4:0 / 4:1:1 for a caller that asked for
// them: melf_ctx_set_jpeg_samplings; and three scans of one component each instead of the interleaved one for a caller that asked
// for those: melf_ctx_set_jpeg_multiscan, melf_jpeg_scans.h).  Within that: SOF0 or SOF1, Huffman
// table ids 0 and 1 in any assignment to the components, quantisation tables 0..3 with 8- or 16-bit entries, any component
// ids, any order and packing of the header segments.  Everything else is reported unsupported (the caller's host decoder
// takes it), including a file that refers to a Huffman table it does not define (libjpeg-turbo falls back to the Annex K
// tables there, and so does the parser for a caller that asked for it: melf_ctx_set_jpeg_default_tables) or to one libjpeg rejects (over-subscribed, using the all-ones code, a DC category above 15).
//
// The result must be the bytes libjpeg(-turbo) produces with its defaults (what cv2.imread and
// Pillow both use): JDCT_ISLOW inverse DCT, "fancy" triangle-filter chroma upsampling, the
// 16-bit fixed-point YCbCr->RGB tables.  All of that is integer arithmetic, restated here from
// the algorithm descriptions in the libjpeg documentation (jidctint / jdsample / jdcolor) and
// pinned bit-for-bit against Pillow on the reference's 304 fixture files plus synthetic files.
//
//   host   parse markers (melf_jpeg_parse.h), canonical Huffman data, strip byte stuffing / RSTn markers (recording where the
//          restart intervals begin)
//   J1     k_jpeg_huff      one workgroup per image, one lane per bit-stream segment (speculative decode until
//                           the segments' exit states reach a fixed point) -> int16 coefficient blocks in decode order
//          k_jpeg_huff_rst  streams with restart intervals: one lane per interval, no speculation needed
//          k_jpeg_prog_scan progressive files (SOF2), for a caller that asked for them (melf_ctx_set_jpeg_progressive): every scan
//                           accumulated into the same coefficient blocks, one wave per (file, scan, restart interval), one launch
//                           per level of scans that depend on each other (melf_jpeg_prog.h); J2 and J3 then run as for any file
//          (multi-scan sequential files: each scan is a one-component record of its own through k_jpeg_clean and the two kernels above,
//          k_jpeg_scan_status then gives the file the worst of its scans' statuses)
//   J2     k_jpeg_idct      one thread per 8x8 block: dequantise + ISLOW IDCT -> u8 planes
//   J3     k_jpeg_color420  8 pixels per thread: fancy upsample + YCC->BGR -> NHWC frame (k_jpeg_color: other modes)
//          k_jpeg_color_exif  files with an EXIF orientation 2-8 (when the caller asked for them): the same conversion in
//                           stored geometry, each pixel written where the upright frame has it
#include "melf_internal.h"
#include "melf_jpeg_cut.h"
#include "melf_jpeg_long.h"
#include "melf_jpeg_orient_addr.h"
#include "melf_jpeg_parse.h"
#include "melf_jpeg_prog.h"
#include "melf_jpeg_scans.h"
#include "melf_threads.h"

#include <emmintrin.h>

#include <algorithm>
#include <climits>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace melf {

// ------------------------------------------------------------ device-side records ----
struct JpegImageDev {
    uint32_t scan_off, scan_len;  // clean entropy-coded bytes (no stuffing, no markers) in the scan area
    uint32_t coef_blk[3];         // first coefficient block of each component (units of 64 int16)
    uint32_t plane_off[3];        // byte offset of each component's sample plane
    uint16_t blocks_x[3], blocks_y[3];
    uint16_t mcus_x, mcus_y;
    uint16_t restart_interval;
    uint8_t ncomp, hs0, vs0, ok;
    uint8_t tq[3], td[3], ta[3];
    uint8_t orient;               // EXIF orientation the colour stage applies (1..8); the other stages work in stored geometry
    uint8_t planar;               // a multi-scan sequential file (ok = 4): every component's blocks in an area of its own, coef_blk[c], the
                                  // REAL blocks in raster order, written by the one-component records of its scans (melf_jpeg_scans.h)
    uint8_t end_marker;           // written by k_jpeg_clean: the byte behind the FF that ended the scan (D9 = EOI), 0 when the bytes ended first
    uint32_t rst_off, rst_cnt;    // restart intervals: table of their byte offsets in the clean scan (relative to the
                                  // scan area), number of intervals.  A planar file's record has no scan of its own and keeps its
                                  // real block grids here: rst_off = luma, rst_cnt = chroma, columns | rows << 16
    // Filled by the host; scan_len and rst_cnt (and the bytes they describe) by k_jpeg_clean on the GPU (round 4):
    uint32_t scan_cap;            // bytes of the scan area reserved for this file's clean scan (zero-filled behind scan_len)
    uint32_t raw_off, raw_len;    // the file's entropy-coded segment as it is in the file (stuffing, fill bytes, RSTn, EOI and
                                  // whatever follows), in the raw area
};
static_assert(sizeof(JpegImageDev) % 4 == 0, "record must stay dword aligned");

// ------------------------------------------------------------ J0: scan cleaning ----
// The entropy-coded segment without byte stuffing (FF 00 -> FF), fill bytes and RSTn markers, up to the first other marker
// (normally EOI) -- on the GPU since round 4 (rounds 1-3: a host pass, clean_scan): the host no longer touches the entropy-coded bytes except to copy them (or, for
// the file-name entry points, not at all: the files are read straight into the pinned buffer the upload starts from).
// One workgroup per file, 16 KiB per round, 16 consecutive bytes per thread.  In entropy-coded data every FF is special and
// the byte behind it says how: 00 = a stuffed FF (keep the FF, drop the 00), FF = fill (drop this one, look at the next),
// D0..D7 = RSTn (drop both, the next restart interval begins at the clean offset reached), anything else -- or the end of
// the data -- ends the scan.  Per round: (1) the first scan-ending FF of the round (minimum over the workgroup), (2) keep
// flags and restart markers below it, one packed prefix scan of both counts, (3) byte stores of the kept bytes at their
// clean offsets, restart offsets into the table behind the scan.  Leaves scan_len / rst_cnt in the file's record and the
// rest of the file's scan region zeroed, exactly what the host pass left.
constexpr int CLEAN_T = 1024;   // threads of k_jpeg_clean: 16 KiB per round, a camera frame's scan in two or three
// 0x80 in every byte of x that is zero (exact: no borrow between bytes), and such flags gathered into a nibble
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
__device__ __forceinline__ uint32_t flag_nibble(uint32_t f)
{
    const uint32_t y = f >> 7;   // bits 0, 8, 16, 24
    return (y | (y >> 7) | (y >> 14) | (y >> 21)) & 15u;
}
__global__ __launch_bounds__(CLEAN_T) void k_jpeg_clean(JpegImageDev* __restrict__ imgs, const uint8_t* __restrict__ raw,
                                                        uint8_t* __restrict__ scan)
{
    __shared__ int s_end;
    __shared__ uint32_t s_wsum[CLEAN_T / 64];
    JpegImageDev* R = imgs + blockIdx.x;
    if (!R->ok) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint8_t* __restrict__ s = raw + R->raw_off;
    const int n = (int)R->raw_len;
    uint8_t* __restrict__ out = scan + R->scan_off;
    const bool has_rst = R->restart_interval != 0;
    uint32_t* __restrict__ rst = (uint32_t*)(scan + R->rst_off);
    const int rst_cap = has_rst ? (int)R->rst_cnt + 1 : 0;   // the host left the EXPECTED number of intervals here
    int o_base = 0, r_base = 0;   // clean bytes written, restart markers seen, before this round
    bool ended = false;
    int endpos = -1;   // where the FF that ended the scan stands (uniform), -1: none, the bytes ended first
    for (int base = 0; base < n && !ended; base += CLEAN_T * 16) {
        if (tid == 0) s_end = INT_MAX;
        const int my = base + tid * 16;
        // bytes my - 1 .. my + 16 (the raw area is padded: reads past n stay inside it; their values are masked below)
        uint32_t w[5] = {0, 0, 0, 0, 0};
        uint32_t prev = 0;
        if (my < n) {
#pragma unroll
            for (int q = 0; q < 5; ++q) __builtin_memcpy(&w[q], s + my + 4 * q, 4);
            if (my > 0) prev = s[my - 1];
        }
        // One bit per byte 0 .. 16 of the thread's window: is it FF (F), 00 (Z), D0..D7 (D)?  The whole classification then
        // is a handful of 17-bit mask operations (the per-byte form of this loop was 2 000 instructions per round).
        uint32_t F = 0, Z = 0, D = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            F |= flag_nibble(zero_bytes(~w[q])) << (4 * q);
            Z |= flag_nibble(zero_bytes(w[q])) << (4 * q);
            D |= flag_nibble(zero_bytes((w[q] & 0xF8F8F8F8u) ^ 0xD0D0D0D0u)) << (4 * q);
        }
        {
            const uint32_t b16 = w[4] & 255u;
            F |= (uint32_t)(b16 == 0xFFu) << 16;
            Z |= (uint32_t)(b16 == 0x00u) << 16;
            D |= (uint32_t)((b16 & 0xF8u) == 0xD0u) << 16;
        }
        const int left = n - my;                                                         // bytes of the data from `my` on (may be <= 0)
        const uint32_t Vm = left >= 16 ? 0xFFFFu : (left > 0 ? (1u << left) - 1u : 0u);   // byte j exists
        const uint32_t NV = left >= 17 ? 0xFFFFu : (left > 1 ? (1u << (left - 1)) - 1u : 0u);   // byte j + 1 exists
        const uint32_t Fn = F >> 1, Zn = Z >> 1, Dn = D >> 1;
        const uint32_t Fp = ((F << 1) | (uint32_t)(prev == 0xFFu)) & 0xFFFFu;
        const uint32_t F16 = F & 0xFFFFu;
        // an FF that ends the scan: no byte behind it, or one that is neither 00 nor FF nor D0..D7
        const uint32_t endmask = F16 & Vm & ~((Zn | Fn | Dn) & NV);
        __syncthreads();
        if (endmask) atomicMin(&s_end, my + (int)__builtin_ctz(endmask));
        __syncthreads();
        const int se = s_end;
        const int end = min(se, n);
        if (se != INT_MAX) endpos = se;
        const int live = end - my;
        const uint32_t Lm = live >= 16 ? 0xFFFFu : (live > 0 ? (1u << live) - 1u : 0u);
        // kept: a stuffed FF (FF 00), and every other byte that is not the second byte of a stuffed pair or of a marker
        const uint32_t keep = Lm & ((F16 & Zn & NV) | (~F16 & ~(Fp & (Z | D)) & 0xFFFFu));
        const uint32_t mark = Lm & F16 & Dn & NV;
        // exclusive prefix of (kept bytes | markers << 16) over the workgroup
        const uint32_t cnt = (uint32_t)__popc(keep);
        const uint32_t mine = cnt | ((uint32_t)__popc(mark) << 16);
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wsum[wv] = incl;
        __syncthreads();
        uint32_t before = incl - mine, total = 0;
#pragma unroll
        for (int q = 0; q < CLEAN_T / 64; ++q) {
            const uint32_t t = s_wsum[q];
            if (q < wv) before += t;
            total += t;
        }
        const int ko = o_base + (int)(before & 0xffffu);
        // restart markers (rare: only files with restart intervals have any): the interval behind marker k begins at the
        // clean offset reached where the marker stood
        if (__builtin_amdgcn_ballot_w64(mark != 0u) != 0ull) {
            int ro = r_base + (int)(before >> 16);
            uint32_t m = mark;
            while (m) {
                const int j = __builtin_ctz(m);
                m &= m - 1u;
                ++ro;
                if (ro < rst_cap) rst[ro] = (uint32_t)(ko + __popc(keep & ((1u << j) - 1u)));
            }
        }
        // the kept bytes moved together: a dropped byte below the highest kept one is squeezed out of the 16-byte value, highest
        // first (typically none or one per thread; the loop runs as often as the wave's worst lane needs)
        uint32_t v0 = w[0], v1 = w[1], v2 = w[2], v3 = w[3];
        uint32_t drop = keep ? (~keep & ((2u << (31 - __builtin_clz(keep))) - 1u)) : 0u;
        while (__builtin_amdgcn_ballot_w64(drop != 0u) != 0ull) {
            if (drop) {
                const int q = 31 - __builtin_clz(drop);   // the byte to squeeze out
                drop &= ~(1u << q);
                const int dq = q >> 2;
                const uint32_t lm = (1u << (8 * (q & 3))) - 1u;   // bytes of dword dq below it
                const uint32_t s0 = __builtin_amdgcn_alignbit(v1, v0, 8), s1 = __builtin_amdgcn_alignbit(v2, v1, 8),
                               s2 = __builtin_amdgcn_alignbit(v3, v2, 8), s3 = v3 >> 8;
                v0 = dq == 0 ? ((v0 & lm) | (s0 & ~lm)) : v0;
                v1 = dq == 1 ? ((v1 & lm) | (s1 & ~lm)) : (dq < 1 ? s1 : v1);
                v2 = dq == 2 ? ((v2 & lm) | (s2 & ~lm)) : (dq < 2 ? s2 : v2);
                v3 = dq == 3 ? ((v3 & lm) | (s3 & ~lm)) : s3;
            }
        }
        {   // cnt bytes at out + ko: whole dwords (any alignment), then up to three single bytes
            uint8_t* o = out + ko;
            if (cnt >= 4u) __builtin_memcpy(o, &v0, 4);
            if (cnt >= 8u) __builtin_memcpy(o + 4, &v1, 4);
            if (cnt >= 12u) __builtin_memcpy(o + 8, &v2, 4);
            if (cnt >= 16u) __builtin_memcpy(o + 12, &v3, 4);
            const uint32_t full = cnt >> 2;
            const uint32_t tailw = full == 0u ? v0 : (full == 1u ? v1 : (full == 2u ? v2 : v3));
            const uint32_t r = cnt & 3u;
            uint8_t* t = o + 4 * full;
            if (r >= 1u) t[0] = (uint8_t)tailw;
            if (r >= 2u) t[1] = (uint8_t)(tailw >> 8);
            if (r >= 3u) t[2] = (uint8_t)(tailw >> 16);
        }
        o_base += (int)(total & 0xffffu);
        r_base += (int)(total >> 16);
        ended = end < base + CLEAN_T * 16;   // uniform: the scan ended inside this round (or the data did)
        __syncthreads();                      // s_end and s_wsum are rewritten by the next round
    }
    const int cap = (int)R->scan_cap;
    for (int i = o_base + tid; i < cap; i += CLEAN_T) out[i] = 0;
    if (tid == 0) {
        R->scan_len = (uint32_t)o_base;
        R->end_marker = endpos >= 0 && endpos + 1 < n ? s[endpos + 1] : (uint8_t)0;   // (never 00: FF 00 is a stuffed FF)
        if (has_rst) {
            rst[0] = 0;
            R->rst_cnt = (uint32_t)(r_base + 1);
        }
    }
}

// Stage entry point (include/meterelf_hip.h, melf_jpeg_clean_segment; tests/test_jpeg.py): k_jpeg_clean on ONE byte string as if it were a file's
// entropy-coded segment -- arbitrary bytes, so that the tests can feed it every FF pattern, legal or not, and compare with the
// sequential rule.  restart_expected > 0: a file with restart intervals, table of restart_expected + 1 entries.
extern "C" __attribute__((visibility("default"))) int melf_jpeg_clean_segment(const uint8_t* raw, int n, int restart_expected, uint8_t* out,
                                                                            int32_t* out_len, uint32_t* rst, int32_t* rst_cnt)
{
    if (n < 0 || !out || !out_len || (n > 0 && !raw)) return -1;
    const size_t scan_cap = ((size_t)n + 128 + 63) / 64 * 64, table = restart_expected > 0 ? ((size_t)restart_expected + 1) * 4 + 64 : 0;
    JpegImageDev rec;
    memset(&rec, 0, sizeof(rec));
    rec.ok = restart_expected > 0 ? 2 : 1;
    rec.restart_interval = restart_expected > 0 ? 1 : 0;
    rec.rst_cnt = (uint32_t)std::max(restart_expected, 0);
    rec.rst_off = (uint32_t)scan_cap;
    rec.scan_cap = (uint32_t)scan_cap;
    rec.raw_len = (uint32_t)n;
    uint8_t *d_rec = nullptr, *d_raw = nullptr, *d_scan = nullptr;
    int rc = -1;
    if (hipMalloc((void**)&d_rec, sizeof(rec)) == hipSuccess && hipMalloc((void**)&d_raw, (size_t)n + 64) == hipSuccess &&
        hipMalloc((void**)&d_scan, scan_cap + table + 64) == hipSuccess &&
        hipMemset(d_raw, 0xFF, (size_t)n + 64) == hipSuccess &&   // what lies behind the data must not matter: make it hostile
        hipMemset(d_scan, 0xEE, scan_cap + table + 64) == hipSuccess &&
        hipMemcpy(d_rec, &rec, sizeof(rec), hipMemcpyHostToDevice) == hipSuccess &&
        (n == 0 || hipMemcpy(d_raw, raw, (size_t)n, hipMemcpyHostToDevice) == hipSuccess)) {
        hipLaunchKernelGGL(k_jpeg_clean, dim3(1), dim3(CLEAN_T), 0, 0, (JpegImageDev*)d_rec, d_raw, d_scan);
        std::vector<uint8_t> back(scan_cap + table);
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(&rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(back.data(), d_scan, back.size(), hipMemcpyDeviceToHost) == hipSuccess) {
            *out_len = (int32_t)rec.scan_len;
            memcpy(out, back.data(), scan_cap);   // the caller's buffer holds n + 192 bytes: clean bytes, then the zero fill
            if (restart_expected > 0 && rst && rst_cnt) {
                *rst_cnt = (int32_t)rec.rst_cnt;
                memcpy(rst, back.data() + scan_cap, ((size_t)restart_expected + 1) * 4);
            }
            rc = 0;
        }
    }
    (void)hipFree(d_rec); (void)hipFree(d_raw); (void)hipFree(d_scan);
    return rc;
}

// ------------------------------------------------------------------ J1: Huffman ----
__device__ __constant__ uint8_t c_zz2nat[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ------------------------------------------------- J1: Huffman, segment-parallel ----
// One workgroup per image, one lane per bit-stream segment.  A Huffman stream can only be decoded from
// a known state (bit position, block within the MCU, coefficient index), but decoders started from a
// wrong state fall into step with the true one by themselves (self-synchronisation), so:
//   round 0   every lane walks its segment from a guessed state (state only: no values) and publishes its exit state;
//   round r   a lane whose predecessor's exit state changed walks again from that state (the changed segments
//             compacted onto the first lanes); the true state of lane 0 propagates at least one lane per round; the
//             fixtures need 8-19 rounds (fixed point: exit[i] = F_i(exit[i-1]) for all i);
//   scan      blocks completed per segment -> exclusive prefix over the lanes = each segment's first block;
//   output    one more decode that writes the coefficients, DC predictors starting at zero in every segment;
//   fix-up    prefix over the lanes of the segments' DC-difference sums -> the predictors at each segment's entry,
//             added to the DC coefficients the segment stored.
// The decode tables of the image sit in LDS, the stream is read through L1 a dword ahead.  What bounds the kernel is
// the number of INSTRUCTIONS per decode step (tools/ubench/wave_latency.hip: a lone wave issues one per ~6 cycles
// whatever it is, four waves on a SIMD one per ~4 between them), so both decoders are written to be short.
struct SegState {
    uint32_t p;      // bit position
    int blk, k;      // block within the MCU, coefficient index (0 = DC symbol comes next)
};
// First-level lookup of the Huffman kernels, built in LDS by the kernels themselves: four tables (DC 0, DC 1, AC 0,
// AC 1) of 2^TAB_BITS dwords.  An entry says what the next TAB_BITS bits of the stream start with -- ONE symbol, or
// TWO when the second code also lies wholly inside the window.  A symbol is the pair (bits it occupies: code +
// magnitude bits, the symbol alone fixes their number; coefficients it advances: DC 1, AC run + 1, ZRL 16, end of block
// 64 = k leaves the block), packed so that ONE addition advances the state-only decoder's packed position
// (bit position in bits 0..15, coefficient index from bit 16):
//   bits  0.. 4  bits1        bits 16..22  adv1       the first symbol
//   bits  7..11  bits2        bits 23..29  adv2       both symbols together (adv2 = 64 when the second ends the block);
//                                                      an entry WITHOUT a second symbol repeats the first here, so that
//                                                      the decoder need not ask whether there is one
//   bits 12..15  sbits        magnitude bits of the first symbol (the last sbits of its bits1)
// Bit 31 set: the first code is longer than the window.  For the AC tables the entry then carries (bits 0..11) where
// the window's 2^6 continuations start in `longtab`, a direct table over the 16-bit windows that begin with a long code
// (LONG_N of them per AC table; their Kraft sum is small: 319 for the standard tables); bit 30: not covered (a DC table,
// or a code set with more long-code space) -- canonical compares from `slow`.  A full wave meets a long code in most of
// its steps, so what it costs is paid by every step: one more lookup instead of ~40 instructions.
// The second symbol of a DC entry is the block's first AC symbol, decoded with the AC table that goes with that DC
// table; a DC table whose blocks do not all use that AC table gets no second symbols (McuLayout::pair_dc).  The
// coefficient-writing decoder reads the first symbol only; the state-only decoder of the speculative pass and of the
// synchronisation rounds takes both: a flat block (DC difference + end of block, 4-6 bits) is one step, most short AC
// symbols go two at a time.
constexpr uint32_t SYM_MASK = 0x007f001fu;  // bits | adv << 16 of the first symbol; the second sits 7 bits higher
constexpr int TAB_BITS = 10;
constexpr int LONG_N = 512;  // entries of the long-code table per AC table
// k_jpeg_huff keeps bit positions inside a segment in 16 bits: segments of at most 32 000 bits, i.e. scans of at most
// 4 MB with 1024 lanes (2 MB with the usual 512); larger baseline files without restart markers go to the host decoder,
// or, in a context with melf_ctx_set_jpeg_long_scans, to k_jpeg_chapters
constexpr size_t JPEG_MAX_PAR_SCAN = 4000000;
constexpr uint32_t TAB_MASK = (1u << TAB_BITS) - 1u;

// Per-MCU-position tables packed into registers: 1 bit of DC table id, 1 bit of AC table id and 2 bits
// of component per block position (an MCU has at most 6 blocks here: 4:2:0 and 4:1:1 have 6, 4:2:2 and 4:4:0 have 4).
// The pixel window the decoder produces (x0, y0 multiples of 16): the whole frame, or -- when the caller only
// reads the meter_rect crop -- that crop plus 16 pixels of context for the chroma filter.  Coefficients outside it
// are neither zeroed nor stored, J2 / J3 do not run there.
// The window is in PIXELS and knows nothing of the file's MCU (a run's files may differ in sampling).  Every stage turns it into
// the file's own MCUs the same way -- floor(x0 / mw) .. ceil(x1 / mw), floor(y0 / mh) .. ceil(y1 / mh) with mw x mh = 8 hs0 x 8 vs0:
// jpeg_zero_window for J1, k_jpeg_idct for J2 -- so the MCUs that are zeroed, stored and inverse-transformed are exactly those that
// hold a pixel of the window, whatever the MCU: 8 x 8, 16 x 8, 16 x 16, and 8 x 16 (4:4:0) and 32 x 8 (4:1:1) just the same.  For the
// MCUs up to 16 x 16 the 16-aligned origin is an MCU corner; for a 32-wide MCU x0 may lie 16 pixels inside its first MCU, which is
// then decoded whole (16 more columns than asked for, never fewer).  What the 16 pixels of margin are for is the chroma filter's
// reach, at most one chroma sample = 2 luma pixels in the filtered direction (4:1:1 is not filtered at all); it is not an MCU count.
struct JpegWindow {
    int x0, y0, x1, y1;
};
struct McuWindow {  // the same in MCUs of one image
    int mx0, mx1, my0, my1;
};

struct McuLayout {
    uint32_t dc_bits, ac_bits, comp_bits;
    uint32_t tsel5;      // per block, 5 bits: DC table id | (2 + AC table id) << 2 (the state-only decoder's table choice)
    uint32_t nxt5;       // per block, 5 bits: 5 * index of the block that follows it in the MCU
    uint32_t oh0, oh1, oh2;  // per block, at bit 5 * block: the block belongs to component 0 / 1 / 2
    uint32_t pair_dc;    // bit t: every block with DC table t uses the AC table its entries' second symbols come from
    int ac_of_dc0, ac_of_dc1;  // that AC table, per DC table
    int bpm, yblocks;
};

__device__ __forceinline__ McuLayout jpeg_mcu_layout(const JpegImageDev* R)
{
    const int ncomp = R->ncomp;
    McuLayout L;
    L.yblocks = ncomp == 1 ? 1 : R->hs0 * R->vs0;
    L.bpm = ncomp == 1 ? 1 : L.yblocks + 2;
    L.dc_bits = L.ac_bits = L.comp_bits = L.tsel5 = L.nxt5 = 0;
    L.oh0 = L.oh1 = L.oh2 = 0;
    L.pair_dc = 3;
    int a0 = -1, a1 = -1;
    for (int b = 0; b < L.bpm; ++b) {
        const int c = b < L.yblocks ? 0 : 1 + b - L.yblocks;
        const int td = R->td[c] & 1, ta = R->ta[c] & 1;
        L.dc_bits |= (uint32_t)td << b;
        L.ac_bits |= (uint32_t)ta << b;
        L.comp_bits |= (uint32_t)c << (2 * b);
        L.tsel5 |= ((uint32_t)td | (2u + (uint32_t)ta) << 2) << (5 * b);
        L.nxt5 |= (uint32_t)(5 * (b + 1 == L.bpm ? 0 : b + 1)) << (5 * b);
        L.oh0 |= (c == 0 ? 1u : 0u) << (5 * b);
        L.oh1 |= (c == 1 ? 1u : 0u) << (5 * b);
        L.oh2 |= (c == 2 ? 1u : 0u) << (5 * b);
        if (td == 0 && a0 < 0) a0 = ta;
        if (td == 1 && a1 < 0) a1 = ta;
        if ((td == 0 ? a0 : a1) != ta) L.pair_dc &= ~(1u << td);
    }
    L.ac_of_dc0 = a0 < 0 ? 0 : a0;
    L.ac_of_dc1 = a1 < 0 ? 0 : a1;
    return L;
}

// the entry of a single symbol (the second-symbol fields repeat it)
__device__ __forceinline__ uint32_t huff_step(const bool dc, const int len, const int sym)
{
    const int sbits = sym & 15, run = sym >> 4;
    const int adv = dc ? 1 : (sbits ? run + 1 : (run == 15 ? 16 : 64));
    const uint32_t one = (uint32_t)(len + sbits) | (uint32_t)adv << 16;
    return one | one << 7 | (uint32_t)sbits << 12;
}

// Canonical decode of the code at the top of the nb-bit window x, looking at its first `avail` bits only: the symbol's
// step, or 0 when the code is longer than that.  sl: the table's HuffSlow in LDS.
template <int NB>
__device__ __forceinline__ uint32_t huff_window_step(const uint32_t* __restrict__ sl, const bool dc, const uint32_t x, const int avail)
{
    int len = 1;
#pragma unroll
    for (int l = 1; l <= NB; ++l) len += (l <= avail && (x >> (NB - l)) >= sl[l - 1]) ? 1 : 0;
    if (len > avail) return 0;
    const int idx = (int)sl[16 + len - 1] + (int)(x >> (NB - len));
    return huff_step(dc, len, ((const uint8_t*)(sl + 32))[idx & 255]);
}

__device__ __forceinline__ uint32_t huff_long_step(const uint32_t* __restrict__ sl, const bool dc, const uint32_t w, bool& invalid);

// The four tables and the long-code table, by all T threads of the workgroup (slow[] complete; a barrier must follow).
template <int T>
__device__ __forceinline__ void jpeg_build_tables(uint32_t* __restrict__ tab, uint32_t* __restrict__ longtab, const uint32_t* __restrict__ slow,
                                                  const McuLayout L, const int tid)
{
    for (int i = tid; i < (4 << TAB_BITS); i += T) {
        const int t = i >> TAB_BITS;
        const bool dc = t < 2;
        const uint32_t x = (uint32_t)i & TAB_MASK;
        uint32_t e = huff_window_step<TAB_BITS>(slow + t * SLOW_DW, dc, x, TAB_BITS);
        const int bits1 = (int)(e & 31u), adv1 = (int)((e >> 16) & 127u);
        if (e && adv1 != 64 && bits1 < TAB_BITS && (!dc || ((L.pair_dc >> t) & 1u))) {  // a second code may lie wholly inside the window
            const int t2 = dc ? 2 + (t == 0 ? L.ac_of_dc0 : L.ac_of_dc1) : t;
            const uint32_t e2 = huff_window_step<TAB_BITS>(slow + t2 * SLOW_DW, false, (x << bits1) & TAB_MASK, TAB_BITS - bits1);
            if (e2) {
                const int a2 = (int)((e2 >> 16) & 127u);
                const uint32_t both = (uint32_t)(bits1 + (int)(e2 & 31u)) | (uint32_t)(a2 == 64 ? 64 : adv1 + a2) << 16;
                e = (e & ~(SYM_MASK << 7)) | both << 7;
            }
        }
        if (!e) {  // a long code: where its 16-bit windows start in longtab, if they are there
            const uint32_t first = slow[t * SLOW_DW + TAB_BITS - 1] << (16 - TAB_BITS);  // the first 16-bit window with a long code
            const uint32_t off = (x << (16 - TAB_BITS)) - first;
            e = (!dc && off + (1u << (16 - TAB_BITS)) <= (uint32_t)LONG_N) ? 0x80000000u | ((uint32_t)(t - 2) * LONG_N + off) : 0xC0000000u;
        }
        tab[i] = e;
    }
    for (int i = tid; i < 2 * LONG_N; i += T) {
        const uint32_t* sl = slow + (2 + i / LONG_N) * SLOW_DW;
        const uint32_t w16 = (sl[TAB_BITS - 1] << (16 - TAB_BITS)) + (uint32_t)(i % LONG_N);
        uint32_t e = 0;
        if (w16 <= 0xffffu) {
            bool invalid = false;
            e = huff_long_step(sl, false, w16 << 16, invalid);
            if (invalid) e |= 0x80000000u;
        }
        longtab[i] = e;
    }
}

// The first symbol when its code is longer than the window: the canonical compares for the remaining lengths.
// A window that starts with no code at all (only a speculative decode or a corrupt file gets there) counts as a
// 16-bit end of block / zero DC difference and sets `invalid`.
__device__ __forceinline__ uint32_t huff_long_step(const uint32_t* __restrict__ sl, const bool dc, const uint32_t w, bool& invalid)
{
    const uint32_t code16 = w >> 16;
    int len = TAB_BITS + 1, sym = 0;
#pragma unroll
    for (int l = TAB_BITS + 1; l <= 16; ++l) len += (code16 >> (16 - l)) >= sl[l - 1] ? 1 : 0;
    if (len > 16) {
        invalid = true;
        len = 16;
    } else {
        const int idx = (int)sl[16 + len - 1] + (int)(code16 >> (16 - len));
        sym = ((const uint8_t*)(sl + 32))[idx & 255];
    }
    return huff_step(dc, len, sym);
}

// An entry with bit 31 set: the first symbol's code is longer than the window (w: the next 32 bits).  Returns the
// symbol's entry; bit 31 of the result: no code at all (see huff_long_step).
__device__ __forceinline__ uint32_t huff_long_entry(const uint32_t e, const uint32_t* __restrict__ longtab, const uint32_t* __restrict__ slow,
                                                    const uint32_t t, const bool dc, const uint32_t w)
{
    if (e & 0x40000000u) {
        bool invalid = false;
        const uint32_t r = huff_long_step(slow + t * SLOW_DW, dc, w, invalid);
        return invalid ? r | 0x80000000u : r;
    }
    return longtab[(e & 0xfffu) + ((w >> 16) & ((1u << (16 - TAB_BITS)) - 1u))];
}

// The coefficient blocks of an image are stored in DECODE ORDER (block n of the scan at n * 64 coefficients: MCU after
// MCU, the MCU's blocks in scan order), so that the decoders' "next block" is the next 128 bytes and the IDCT kernel does
// the little arithmetic of finding a plane position's block.  Where block n of MCU (mx, my) lives, or NULL outside the
// window (such blocks are decoded -- the DC predictors need them -- but not stored):
struct CoefBlocks {
    int16_t* base;
    McuWindow mw;
};
__device__ __forceinline__ int16_t* coef_block_ptr(const CoefBlocks& cp, const int mx, const int my, const int n)
{
    const bool inside = (unsigned)(mx - cp.mw.mx0) < (unsigned)(cp.mw.mx1 - cp.mw.mx0) && (unsigned)(my - cp.mw.my0) < (unsigned)(cp.mw.my1 - cp.mw.my0);
    return inside ? cp.base + (size_t)n * 64 : nullptr;
}

// One segment, symbol by symbol, writing the coefficients of the blocks inside the window.  pred0..2: the DC predictors
// at the segment's entry (in), at its exit (out); ndc: DC symbols decoded.  Every lane of a full wave is at another
// place of its block, so whatever any symbol kind needs is executed in every step: the loop is written for the UNION --
// one value extraction, one store (DC: predictor sum at index 0; AC: the value at its natural position), predictor sums
// by multiply-add with a one-hot component vector that changes with the block, the stream window of the state-only
// decoder -- and only the block change (next block's pointer, tables, component) sits behind a branch.
__device__ __forceinline__ void jpeg_decode_segment(
    const uint32_t* __restrict__ W, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ longtab, const uint32_t* __restrict__ slow,
    const uint8_t* __restrict__ nat, const McuLayout L, SegState& s, const uint32_t p_end, int& nblk,
    int nb, const int total_blocks, int& pred0, int& pred1, int& pred2, int& ndc, const int mcus_x, const CoefBlocks& cp, int& bad)
{
    uint32_t p = s.p;
    int blk = s.blk, k = s.k;
    int mx, my;
    {
        const int mcu = nb / L.bpm;
        my = mcu / mcus_x;
        mx = mcu - my * mcus_x;
    }
    int16_t* cb = coef_block_ptr(cp, mx, my, nb);
    int nbl = 0, nd = 0;
    int a0 = pred0, a1 = pred1, a2 = pred2;
    uint32_t bs = 5u * (uint32_t)blk;
    int c0 = (int)__builtin_amdgcn_ubfe(L.oh0, bs, 1), c1 = (int)__builtin_amdgcn_ubfe(L.oh1, bs, 1), c2 = (int)__builtin_amdgcn_ubfe(L.oh2, bs, 1);
    // the stream: three byte-swapped dwords that rotate when the position crosses a dword, the next one requested a step ahead
    const uint32_t* __restrict__ Wp = W + (p >> 5);
    uint32_t Xs = p << 27;
    uint32_t d0 = __builtin_bswap32(Wp[0]), d1 = __builtin_bswap32(Wp[1]), d2 = __builtin_bswap32(Wp[2]);
    uint32_t off = 3;
    uint32_t nraw = Wp[3];
    uint32_t t = __builtin_amdgcn_ubfe(L.tsel5, bs + (k == 0 ? 0u : 2u), 2);
    uint32_t b0 = (uint32_t)(((((uint64_t)d0 << 32) | d1) << (Xs >> 27)) >> 32);
    while (p < p_end && nb < total_blocks) {
        uint32_t e = tab[__builtin_amdgcn_alignbit(t, b0, 32 - TAB_BITS)];
        if (__builtin_amdgcn_sicmp((int32_t)e, 0, 40 /* < */) != 0ull) {  // some lane met a long code
            asm volatile("");
            if ((int32_t)e < 0) {
                e = huff_long_entry(e, longtab, slow, t, k == 0, b0);
                if ((int32_t)e < 0) bad = 1;
            }
        }
        const int used = (int)(e & 31u), adv = (int)((e >> 16) & 127u), sbits = (int)((e >> 12) & 15u);
        const int raw = (int)__builtin_amdgcn_ubfe(b0, 32 - used, sbits);  // width 0 -> 0
        const int m = 1 << sbits;
        const int v = 2 * raw < m ? raw - m + 1 : raw;  // EXTEND (F.2.2.1); sbits = 0 -> 0
        const bool isdc = k == 0;
        const int vd = isdc ? v : 0;
        a0 = __mul24(vd, c0) + a0;
        a1 = __mul24(vd, c1) + a1;
        a2 = __mul24(vd, c2) + a2;
        const int pr = c0 ? a0 : c1 ? a1 : a2;
        nd += isdc ? 1 : 0;
        k += adv;  // DC: 0 -> 1
        const int pos = k - 1;  // run zeros, then this coefficient
        const int zz = nat[pos & 63];
        const bool st = cb != nullptr && (isdc || (sbits != 0 && pos < 64));
        if (st) cb[isdc ? 0 : zz] = (int16_t)(isdc ? pr : v);
        p += (uint32_t)used;
        const bool rot = __builtin_uadd_overflow(Xs, (uint32_t)used << 27, &Xs);
        d0 = rot ? d1 : d0;
        d1 = rot ? d2 : d1;
        d2 = rot ? __builtin_bswap32(nraw) : d2;
        off += rot ? 1u : 0u;
        // only the lanes that moved on ask for their next dword: with eight full waves per image a load in EVERY step kept
        // the stream's lines the most recently used ones of the L2 and pushed the coefficient lines out between two
        // stores to the same block (WRITE_SIZE 449 -> 290 MB per 512 files, same kernel time)
        if (rot) nraw = Wp[off];
        __builtin_amdgcn_sched_barrier(0);
        if (k >= 64) {
            k = 0;
            ++nbl;
            ++nb;
            if (++blk == L.bpm) {
                blk = 0;
                if (++mx == mcus_x) { mx = 0; ++my; }
            }
            bs = 5u * (uint32_t)blk;
            cb = coef_block_ptr(cp, mx, my, nb);
            c0 = (int)__builtin_amdgcn_ubfe(L.oh0, bs, 1);
            c1 = (int)__builtin_amdgcn_ubfe(L.oh1, bs, 1);
            c2 = (int)__builtin_amdgcn_ubfe(L.oh2, bs, 1);
        }
        t = __builtin_amdgcn_ubfe(L.tsel5, bs + (k == 0 ? 0u : 2u), 2);
        b0 = (uint32_t)(((((uint64_t)d0 << 32) | d1) << (Xs >> 27)) >> 32);
    }
    s.p = p; s.blk = blk; s.k = k;
    pred0 = a0; pred1 = a1; pred2 = a2;
    nblk = nbl;
    ndc = nd;
}

// What a segment's decode does to the decoder STATE, without coefficients or DC values: exit state and blocks completed.
// The same walk as jpeg_decode_segment (same tables, same treatment of impossible codes, same stop at p_end; the second
// symbol of an entry is taken only where the one-at-a-time decoder would decode it next: same block, before p_end), so a
// segment entered in the true state leaves in the true state.
// The synchronisation rounds are a chain of dependent steps of ONE wave, and a lone wave pays ~6 cycles per instruction
// whatever it is, ~20 more per VALU -> SALU -> VALU hop, 20-55 per branch (tools/ubench/wave_latency.hip): what counts
// is the number of instructions per step.  Hence: no data-dependent branches but the rare long code; bit position
// (relative to `base`, 16 bits) and coefficient index packed into one register X that an entry's symbol advances with one
// addition; both conditions for the second symbol from one packed 16-bit subtraction; the stream as three byte-swapped
// dwords d0 d1 d2 that rotate when the position crosses a dword, the dword after them requested a step ahead; table
// id and next block from 5-bit-per-block lookup words in scalar registers.  No DC values here: the output pass sums
// them per segment and a fix-up adds the predictors (k_jpeg_huff).
typedef short melf_s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void jpeg_state_segment(
    const uint32_t* __restrict__ W, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ longtab, const uint32_t* __restrict__ slow, const McuLayout L,
    SegState& s, const uint32_t p_end, int& nblk, int* diag = nullptr)
{
    const uint32_t base = s.p & ~31u;
    const uint32_t* __restrict__ Wp = W + (base >> 5);
    uint32_t X = (s.p - base) | (uint32_t)s.k << 16;           // position | coefficient index << 16
    uint32_t Xs = X << 27;                                      // the position's low five bits on top: their carry = "next dword"
    const uint32_t C = (p_end - base) | 64u << 16;             // their limits (p_end - base < 32768: checked by the kernel)
    uint32_t bs = 5u * (uint32_t)s.blk;
    int nb = 0;
    uint32_t d0 = __builtin_bswap32(Wp[0]), d1 = __builtin_bswap32(Wp[1]), d2 = __builtin_bswap32(Wp[2]);
    uint32_t off = 3;
    uint32_t nraw = Wp[3];
    uint32_t t = __builtin_amdgcn_ubfe(L.tsel5, bs + (s.k == 0 ? 0u : 2u), 2);
    uint32_t b0 = (uint32_t)(((((uint64_t)d0 << 32) | d1) << (Xs >> 27)) >> 32);
    while ((X & 0xffffu) < (C & 0xffffu)) {
        uint32_t e = tab[__builtin_amdgcn_alignbit(t, b0, 32 - TAB_BITS)];  // (t << TAB_BITS) | (b0 >> (32 - TAB_BITS))
#ifdef MELF_JPEG_ROUNDS
        if (diag) ++diag[0];
#endif
        if (__builtin_amdgcn_sicmp((int32_t)e, 0, 40 /* < */) != 0ull) {  // some lane met a long code (one compare + scalar branch)
            asm volatile("");  // keeps the compiler from folding the two conditions into one divergent branch
            if ((int32_t)e < 0) e = huff_long_entry(e, longtab, slow, t, (X >> 16) == 0u, b0);
        }
        const uint32_t sym1 = e & SYM_MASK, sym2 = (e >> 7) & SYM_MASK;
        const uint32_t Y = X + sym1;  // after the first symbol
        const melf_s16x2 z = __builtin_bit_cast(melf_s16x2, Y) - __builtin_bit_cast(melf_s16x2, C);
        // both still inside: position < p_end and coefficient index < 64 -> the second symbol is the decoder's next
        const bool two = (__builtin_bit_cast(uint32_t, z) & 0x80008000u) == 0x80008000u;
#ifdef MELF_JPEG_ROUNDS
        if (diag && two && sym1 != sym2) ++diag[1];
#endif
        const uint32_t sel = two ? sym2 : sym1;
        uint32_t Xn = X + sel;
        const bool rot = __builtin_uadd_overflow(Xs, sel << 27, &Xs);  // crossed into the next dword (a step consumes < 32 bits)
        d0 = rot ? d1 : d0;
        d1 = rot ? d2 : d1;
        d2 = rot ? __builtin_bswap32(nraw) : d2;
        off += rot ? 1u : 0u;
        nraw = Wp[off];  // requested here, consumed a whole step later (an L1 hit takes most of a step)
        __builtin_amdgcn_sched_barrier(0);
        const bool end = Xn >= (64u << 16);       // the block is complete
        Xn = end ? (Xn & 0xffffu) : Xn;
        nb += end ? 1 : 0;
        const uint32_t nxt = __builtin_amdgcn_ubfe(L.nxt5, bs, 5);
        bs = end ? nxt : bs;
        t = __builtin_amdgcn_ubfe(L.tsel5, bs + (end ? 0u : 2u), 2);
        X = Xn;
        b0 = (uint32_t)(((((uint64_t)d0 << 32) | d1) << (Xs >> 27)) >> 32);
    }
    s.p = base + (X & 0xffffu);
    s.k = (int)(X >> 16);
    s.blk = (int)((bs * 13u) >> 6);  // bs / 5 for bs <= 25
    nblk = nb;
}

// the three 16-bit lanes of a packed DC-difference sum (each true sum fits: it is a difference of two DC values)
__device__ __forceinline__ void unpack_dsum(int64_t d, int& a, int& b, int& c)
{
    a = (int)(int16_t)(d & 0xffff);
    d = (d - a) >> 16;
    b = (int)(int16_t)(d & 0xffff);
    d = (d - b) >> 16;
    c = (int)(int16_t)(d & 0xffff);
}

#ifdef MELF_JPEG_ROUNDS
__device__ uint64_t g_jpeg_stamps[8 * 8192];  // per image: start, tables built, round 0 done, rounds done, scan done, output pass done, end
extern "C" __attribute__((visibility("default"))) int melf_debug_jpeg_stamps(uint64_t* out, int n)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_jpeg_stamps), sizeof(uint64_t) * 8 * (size_t)(n < 8192 ? n : 8192)) == hipSuccess ? 0 : -1;
}
#define JSTAMP(k) do { if (tid == 0 && img < 8192) g_jpeg_stamps[8 * img + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
__device__ uint32_t g_jpeg_rounds[8192];
// images 0..7, rounds 1..32: segments decoded again, cycles, loop iterations of the slowest lane, of all lanes, two-symbol steps
__device__ uint32_t g_jpeg_round_log[8 * 32 * 5];
extern "C" __attribute__((visibility("default"))) int melf_debug_jpeg_round_log(uint32_t* out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_jpeg_round_log), sizeof(g_jpeg_round_log)) == hipSuccess ? 0 : -1;
}
extern "C" __attribute__((visibility("default"))) int melf_debug_jpeg_rounds(uint32_t* out, int n)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_jpeg_rounds), sizeof(uint32_t) * (size_t)(n < 8192 ? n : 8192)) == hipSuccess ? 0 : -1;
}
#endif

// Zeroes the coefficient blocks of the image's window (the rest of the buffer is never read) and returns the
// window in MCUs.  Called by all threads of the image's workgroup; a __syncthreads() must follow before stores.
template <int T>
__device__ __forceinline__ McuWindow jpeg_zero_window(const JpegImageDev* R, const JpegWindow win, int16_t* __restrict__ coefs, int tid)
{
    const int hs0 = R->hs0, vs0 = R->vs0, ncomp = R->ncomp;
    const int mwid = 8 * hs0, mhei = 8 * vs0;
    McuWindow m;
    m.mx0 = win.x0 / mwid; m.mx1 = min((win.x1 + mwid - 1) / mwid, (int)R->mcus_x);
    m.my0 = win.y0 / mhei; m.my1 = min((win.y1 + mhei - 1) / mhei, (int)R->mcus_y);
    // (floor and ceiling in the file's own MCU, 8 x 16 and 32 x 8 included: 0 <= mx0 < mx1 <= mcus_x because 0 <= x0 < x1 <= W, same for y)
    // decode order: the window's MCUs of one MCU row are one run of bpm * 128 bytes each
    const int bpm = ncomp == 1 ? 1 : hs0 * vs0 + 2;
    const int run16 = (m.mx1 - m.mx0) * bpm * 8, rows = m.my1 - m.my0;  // uint4s per row of MCUs
    uint4* base = (uint4*)(coefs + (size_t)R->coef_blk[0] * 64);
    for (int i = tid; i < rows * run16; i += T) {
        const int r = i / run16, q = i - r * run16;
        base[((size_t)(m.my0 + r) * R->mcus_x + m.mx0) * bpm * 8 + q] = make_uint4(0u, 0u, 0u, 0u);
    }
    return m;
}

#ifndef MELF_JPEG_ROUNDS
#define JSTAMP(k) do { } while (0)
#endif

// Files that end early (melf_ctx_set_jpeg_truncated, melf_jpeg_cut.h).  The Huffman kernels of a context that takes such files get a
// table of two JpegCutRec per file (NULL otherwise: everything as ever).  A file whose stream holds no impossible code but runs
// out before the frame's last block is then not reported corrupt: its status becomes JPEG_ST_CUT, and k_jpeg_cut_tail, one wave per
// file behind the Huffman kernels, finishes the cut MCU from an exact decoder state, zeroes what lies behind it and settles the status
// (JPEG_ST_CUT stays for a file completed under the rule -- J2 and J3 treat it as 0, the host maps it to 0 and counts it -- and 2
// for one that is corrupt after all).  k_jpeg_huff leaves that state: the entry states of its last two segments (block index and
// DC predictors included), of which the tail takes the later one that does not lie behind the stream's last real bit.
// k_jpeg_huff_rst needs no record: the last interval found starts in a known state.
struct JpegCutRec {
    uint32_t p;           // bit position
    int32_t nb;           // block in decode order
    int32_t blk_k;        // block within the MCU << 8 | coefficient index
    int32_t pred[3];      // DC predictors there
};
__device__ __forceinline__ bool jpeg_status_ok(const int32_t st) { return st == 0 || st == JPEG_ST_CUT; }

// At most 80 SGPRs per wave, VCC and the other implicit ones included: one more 16-register granule and a SIMD holds
// 7 waves instead of 8, i.e. three workgroups of 512 per CU instead of four and a 1024-image batch in two passes
// (measured in round 2: 73 -> 75 numbered SGPRs took the kernel from 1.07 to 1.47 ms with the same cycles per workgroup).
template <int T>
__global__ __launch_bounds__(T) __attribute__((amdgpu_num_sgpr(80))) void k_jpeg_huff(const JpegImageDev* __restrict__ imgs, const HuffSlow* __restrict__ g_slow,
                                                 const uint8_t* __restrict__ scan, int16_t* __restrict__ coefs,
                                                 int32_t* __restrict__ status, JpegWindow win, JpegCutRec* __restrict__ cutrec)
{
    __shared__ uint32_t tab[4 << TAB_BITS];
    __shared__ uint32_t longtab[2 * LONG_N];
    __shared__ uint32_t slow[4 * SLOW_DW];
    __shared__ uint8_t nat[64];
    __shared__ uint32_t e_p[T], e_s[T];  // exit state of each segment: bit position, blk << 8 | k
    __shared__ uint32_t n_p[T], n_s[T];  // entry state its last decode started from
    __shared__ int sc_n[T];              // blocks completed in the segment (then: prefix sums)
    __shared__ int64_t sc_d[T];          // packed DC-difference sums of the output pass (then: prefix sums)
    __shared__ uint16_t todo[T];         // segments to decode again this round, compacted
    __shared__ int wcount[T / 64];
#ifdef MELF_JPEG_ROUNDS
    __shared__ int s_diag[3];
#endif
    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    const JpegImageDev* R = imgs + img;
    if (R->ok != 1) return;
    const uint32_t* W = (const uint32_t*)(scan + R->scan_off);  // zero-padded by 128 bytes; read through L1/L2
    JSTAMP(0);
    const McuWindow mwin = jpeg_zero_window<T>(R, win, coefs, tid);  // visible to the output pass: barriers in between
    const uint32_t scan_len = R->scan_len;
    const uint32_t bits = scan_len * 8u;
    // segment length: a multiple of 32 bits with an odd dword count, so that the lanes' stream reads fall into
    // different LDS banks
    const uint32_t S = 32u * (max(8u, (bits + 32u * T - 1) / (32u * T)) | 1u);
    const int nseg = (int)((bits + S - 1) / S);
    if (S > 32000u) {  // the state-only decoder keeps positions inside a segment in 16 bits (host: a larger T, or its own decoder)
        if (tid == 0) status[img] = 2;
        return;
    }
    {
        const uint32_t* ssrc = (const uint32_t*)(g_slow + (size_t)img * 4);
        for (int i = tid; i < 4 * SLOW_DW; i += T) slow[i] = ssrc[i];
        for (int i = tid; i < 64; i += T) nat[i] = c_zz2nat[i];
    }
    __syncthreads();
    const McuLayout L = jpeg_mcu_layout(R);
    jpeg_build_tables<T>(tab, longtab, slow, L, tid);
    const int mcus_x = R->mcus_x;
    const int total_blocks = mcus_x * (int)R->mcus_y * L.bpm;
    const CoefBlocks cp = {coefs + (size_t)R->coef_blk[0] * 64, mwin};
    __syncthreads();

    JSTAMP(1);
    // Per-segment state lives in LDS (entry used by the segment's last decode, exit state, blocks completed, DC
    // sums): in the synchronisation rounds the few segments whose entry changed are COMPACTED onto the first lanes,
    // so that a round occupies one or two waves instead of a lane here and there in all of them (a wave64
    // instruction costs the same issue slot however few lanes are active, and five workgroups share the SIMDs).
    const bool mine = tid < nseg;
    int bad = 0;
    {
        SegState ex = {(uint32_t)tid * S, 0, 0};
        int nblk = 0;
        if (mine) jpeg_state_segment(W, tab, longtab, slow, L, ex, min((uint32_t)(tid + 1) * S, bits + 32u), nblk);
        n_p[tid] = (uint32_t)tid * S;  // entry of the last decode
        n_s[tid] = 0;
        e_p[tid] = ex.p;
        e_s[tid] = (uint32_t)(ex.blk << 8 | ex.k);
        sc_n[tid] = mine ? nblk : 0;
    }
    __syncthreads();
    JSTAMP(2);
    // Window-limited convergence (round 4).  When only a window of the frame is wanted (melf_jpeg_process_batch: the
    // meter_rect crop, MCU rows 9-27 of 40 on the fixtures), nothing behind the window's last MCU row is ever read: not
    // the coefficients, not the DC predictors.  The synchronisation rounds then only have to settle the segments up to the
    // one that holds the window's end, and the output pass skips the segments behind it.  Where that segment lies is
    // estimated from the speculative pass's block counts (a wrongly-phased decoder still counts blocks almost right: a
    // block too many or too few per segment at worst, i.e. a random walk of a few dozen blocks over 512 segments) with a
    // margin of one and a half MCU rows, and CHECKED against the exact counts once the rounds are over: if the settled
    // prefix does not reach the window's end after all, the rounds go on over every segment.  What is given up: a stream
    // damaged only BEHIND the window is no longer reported corrupt (libjpeg would decode the window just the same).
    // All of it counts in BLOCKS of the file's own MCU row (mcus_x * bpm), so it holds for every MCU shape: a 4:1:1 row is
    // ceil(W / 32) MCUs of 6 blocks and 8 pixels tall, a 4:4:0 row ceil(W / 8) MCUs of 4 blocks and 16 tall; the margin is an
    // estimate's slack, the exact check behind the rounds is what the result rests on.
    const int wend = min(total_blocks, mwin.my1 * mcus_x * L.bpm);   // first block behind the window
    int cut = nseg - 1;                                               // last segment the rounds have to settle
    if (wend < total_blocks) {
        const int mine_n = sc_n[tid];
        __syncthreads();
        for (int off = 1; off < T; off <<= 1) {
            const int a = tid >= off ? sc_n[tid - off] : 0;
            __syncthreads();
            sc_n[tid] += a;
            __syncthreads();
        }
        // segments whose (estimated) first block lies behind the window's end + margin: not needed
        const int first_blk = sc_n[tid] - mine_n;
        const int need = mine && first_blk < wend + (3 * mcus_x * L.bpm) / 2 ? 1 : 0;
        const int nneed = __syncthreads_count(need);                  // the needed segments are a prefix: their number
        cut = max(0, min(nseg, nneed) - 1);
        sc_n[tid] = mine_n;                                            // back to per-segment counts for the rounds
        __syncthreads();
    }
    int rounds = 0, redone = 0;  // reported by the diagnostic build only
    (void)rounds;
    (void)redone;
    int nblk = 0, done_blocks = 0;
    for (;;) {   // rounds over the segments up to `cut`, then the exact block counts; once more over all segments if they fall short
    for (;;) {
        // which segments see a new entry state?
        uint32_t np = 0, ns = 0;
        if (tid > 0) { np = e_p[tid - 1]; ns = e_s[tid - 1]; }
        const bool ch = mine && tid <= cut && (np != n_p[tid] || ns != n_s[tid]);
        // compact them: position = number of changed segments before this one
        const uint64_t bal = __ballot(ch);
        const int wave = tid >> 6, lane = tid & 63;
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < T / 64; ++w) {
            const int c = wcount[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (total == 0) break;
        ++rounds;
#ifdef MELF_JPEG_ROUNDS
        const uint64_t round_t0 = __builtin_amdgcn_s_memtime();
        if (tid < 3) s_diag[tid] = 0;
#endif
        if (ch) {
            const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
            todo[pos] = (uint16_t)tid;
            n_p[tid] = np;  // the entry this segment is about to be decoded from
            n_s[tid] = ns;
        }
        __syncthreads();
        for (int q = tid; q < total; q += T) {
            const int i = todo[q];
            ++redone;
            SegState ex = {n_p[i], (int)(n_s[i] >> 8), (int)(n_s[i] & 255u)};
            int nblk;
#ifdef MELF_JPEG_ROUNDS
            int diag[2] = {0, 0};
            jpeg_state_segment(W, tab, longtab, slow, L, ex, min((uint32_t)(i + 1) * S, bits + 32u), nblk, diag);
            atomicMax(&s_diag[0], diag[0]);
            atomicAdd(&s_diag[1], diag[0]);
            atomicAdd(&s_diag[2], diag[1]);
#else
            jpeg_state_segment(W, tab, longtab, slow, L, ex, min((uint32_t)(i + 1) * S, bits + 32u), nblk);
#endif
            e_p[i] = ex.p;  // nobody reads exit states before the next barrier
            e_s[i] = (uint32_t)(ex.blk << 8 | ex.k);
            sc_n[i] = nblk;
        }
        __syncthreads();
#ifdef MELF_JPEG_ROUNDS
        if (tid == 0 && img < 8 && rounds <= 32) {
            uint32_t* lg = g_jpeg_round_log + (img * 32 + rounds - 1) * 5;
            lg[0] = (uint32_t)total;
            lg[1] = (uint32_t)(__builtin_amdgcn_s_memtime() - round_t0);
            lg[2] = (uint32_t)s_diag[0];
            lg[3] = (uint32_t)s_diag[1];
            lg[4] = (uint32_t)s_diag[2];
        }
#endif
    }
    JSTAMP(3);
    // exclusive prefix over the segments: blocks completed
    nblk = sc_n[tid];
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
        const int a = tid >= off ? sc_n[tid - off] : 0;
        __syncthreads();
        sc_n[tid] += a;
        __syncthreads();
    }
    done_blocks = sc_n[T - 1];
    // the settled prefix must reach the window's end (it always does unless the estimate above was off by more than its margin)
    if (cut >= nseg - 1 || sc_n[cut] >= wend) break;
    __syncthreads();
    sc_n[tid] = nblk;
    cut = nseg - 1;
    __syncthreads();
    }
    const bool limited = cut < nseg - 1;
    if (tid == 0) wcount[0] = nseg;   // (free since the rounds ended; read at the kernel's end, barriers in between)
    const SegState entry = {n_p[tid], (int)(n_s[tid] >> 8), (int)(n_s[tid] & 255u)};
    const uint32_t p_end = min((uint32_t)(tid + 1) * S, bits + 32u);
    JSTAMP(4);
    const int nb_in = sc_n[tid] - (mine ? nblk : 0);
    // output pass: every segment from its true entry state and first block, DC predictors starting at ZERO -- the DC
    // coefficients it stores are sums of the segment's own differences; what they lack is known only after a prefix sum
    // over the segments of those sums (three 16-bit lanes of one 64-bit word), and a fix-up pass adds it
    const bool ran = mine && tid <= cut && nb_in < wend;   // (wend = total_blocks when the whole frame is wanted)
    int q0 = 0, q1 = 0, q2 = 0, ndc = 0;
    if (ran) {
        if (entry.blk != nb_in % L.bpm) bad = 1;  // the propagated state and the block count disagree: corrupt stream
        SegState st = entry;
        int n2;
        jpeg_decode_segment(W, tab, longtab, slow, nat, L, st, p_end, n2, nb_in, total_blocks, q0, q1, q2, ndc, mcus_x, cp, bad);
        // where the frame's last block ended, if this segment completed it (e_p is free since the rounds ended): behind the
        // stream's end when it was completed on the zero bits of the scan area's padding alone -- a file that ends early all
        // the same, which a caller that takes such files is told about (at the kernel's end)
        e_p[tid] = nb_in + n2 >= total_blocks ? st.p : 0u;
    }
    const int64_t dsum = (int64_t)q0 + ((int64_t)q1 << 16) + ((int64_t)q2 << 32);
    sc_d[tid] = dsum;
    __syncthreads();
    JSTAMP(5);
    for (int off = 1; off < T; off <<= 1) {
        const int64_t b = tid >= off ? sc_d[tid - off] : 0;
        __syncthreads();
        sc_d[tid] += b;
        __syncthreads();
    }
    if (ran && ndc > 0) {
        int pr0, pr1, pr2;
        unpack_dsum(sc_d[tid] - dsum, pr0, pr1, pr2);  // the predictors at the segment's entry
        if ((pr0 | pr1 | pr2) != 0) {
            // the blocks whose DC symbol this segment decoded: from the first block that BEGINS here
            const int b0 = nb_in + (entry.k != 0 ? 1 : 0);
            const int mcu = b0 / L.bpm;
            int blk = b0 - mcu * L.bpm, my = mcu / mcus_x, mx = mcu - (mcu / mcus_x) * mcus_x;
            // four blocks at a time: their loads are in flight together (a load that follows the lane's own store misses L1)
            for (int i = 0; i < ndc; i += 4) {
                int16_t* cb[4];
                int add[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    cb[u] = i + u < ndc ? coef_block_ptr(cp, mx, my, b0 + i + u) : nullptr;
                    const int comp = (int)((L.comp_bits >> (2 * blk)) & 3u);
                    add[u] = comp == 0 ? pr0 : comp == 1 ? pr1 : pr2;
                    if (++blk == L.bpm) {
                        blk = 0;
                        if (++mx == mcus_x) { mx = 0; ++my; }
                    }
                }
                int16_t v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = cb[u] ? cb[u][0] : (int16_t)0;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (cb[u]) cb[u][0] = (int16_t)(v[u] + add[u]);
            }
        }
    }
    const int anybad = __syncthreads_or(bad);
    JSTAMP(6);
#ifdef MELF_JPEG_ROUNDS  // diagnostic build: rounds and re-decoded segments per image (tools/jpeg_rounds.py)
    {
        __shared__ int s_redone;
        if (tid == 0) s_redone = 0;
        __syncthreads();
        atomicAdd(&s_redone, redone);
        __syncthreads();
        if (tid == 0 && img < 8192) g_jpeg_rounds[img] = ((uint32_t)rounds << 16) | (uint32_t)min(s_redone * 100 / max(nseg, 1), 65535);
    }
#endif
    // the whole scan settled: it must hold every block of the frame; a window-limited decode: the settled prefix reached the
    // window's end (checked above) and the segments it decoded were consistent
    int32_t st = (anybad || (!limited && done_blocks < total_blocks)) ? 2 : 0;
    // (uniform conditions: the barrier inside is reached by all threads or by none)
    if (cutrec != nullptr && !anybad && !limited && (st != 0 || __syncthreads_or(ran && e_p[tid] > R->scan_len * 8u))) {
        // no impossible code, but the stream runs out before the frame's last block (or holds it only thanks to the zero padding):
        // a cut file for k_jpeg_cut_tail.  The entry
        // states of the last two segments (exact: the rounds settled them), with the block and the predictors there -- all of it
        // still in LDS (the prefix sums are inclusive: segment j's first block and predictors are its predecessor's sums), so
        // that nothing of this lives in a register while the decoders run
        const int j = wcount[0] - 2 + tid;
        if (tid < 2 && j >= 0) {
            JpegCutRec r;
            r.p = n_p[j]; r.blk_k = (int32_t)n_s[j]; r.nb = j > 0 ? sc_n[j - 1] : 0;
            unpack_dsum(j > 0 ? sc_d[j - 1] : (int64_t)0, r.pred[0], r.pred[1], r.pred[2]);
            cutrec[2 * img + tid] = r;
        }
        st = JPEG_ST_CUT;
    }
    if (tid == 0) status[img] = st;
}

// Scans longer than T segments of the length k_jpeg_huff can address (melf_ctx_set_jpeg_long_scans; records with ok = 5): the scan in
// CHAPTERS of T segments of S = 32 seg_dw bits (melf_jpeg_long.h has the plan and its bounds).  One workgroup still owns one file and
// works through the chapters in order; a chapter takes k_jpeg_huff's three phases -- the speculative state-only pass over its
// segments, the synchronisation rounds, the output pass with the DC prefix sum and fix-up -- with the same two segment decoders.
// What carries over from chapter to chapter (uniform values, every lane reads them from the LDS arrays before the chapter's last barrier):
//   c_p, c_s     the entry state of the next chapter's first segment: the settled exit state of this chapter's last one, so it is
//                EXACT (chapter 0: the stream's first bit).  Segment 0 of a chapter therefore never sees a new entry, after round r
//                segments 0..r are settled, and the rounds of a chapter end after at most nseg - 1 of them;
//   c_nb         blocks completed so far: a segment's first block is c_nb + the exclusive prefix of the chapter's counts;
//   c_pr0..2     the DC predictors: the carried ones + the inclusive end of the chapter's DC-difference sums.
// The loop ends after the chapter in which the completed blocks reach the window's end (wend), or after the last chapter.  Chapters in
// front of the window run all three phases (the predictors and block counts come from them); coef_block_ptr filters their stores as
// ever.  Inside a chapter every segment is settled: no estimated cut.  Loop bounds: nchap chapters, nseg + 1 rounds per chapter.
// No workgroup waits for another and nothing waits on memory.  A file that runs out of data is corrupt here (no JpegCutRec, no tail).
template <int T>
__global__ __launch_bounds__(T) void k_jpeg_chapters(const JpegImageDev* __restrict__ imgs, const HuffSlow* __restrict__ g_slow,
                                                      const uint8_t* __restrict__ scan, int16_t* __restrict__ coefs,
                                                      int32_t* __restrict__ status, JpegWindow win, const uint32_t seg_dw)
{
    static_assert(T == (int)jpeg_long::T, "the plan's segments per chapter");
    __shared__ uint32_t tab[4 << TAB_BITS];
    __shared__ uint32_t longtab[2 * LONG_N];
    __shared__ uint32_t slow[4 * SLOW_DW];
    __shared__ uint8_t nat[64];
    __shared__ uint32_t e_p[T], e_s[T];  // exit state of each segment of the chapter: bit position, blk << 8 | k
    __shared__ uint32_t n_p[T], n_s[T];  // entry state its last decode started from
    __shared__ int sc_n[T];              // blocks completed in the segment (then: prefix sums)
    __shared__ int64_t sc_d[T];          // packed DC-difference sums of the output pass (then: prefix sums)
    __shared__ uint16_t todo[T];         // segments to decode again this round, compacted
    __shared__ int wcount[T / 64];
    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    const JpegImageDev* R = imgs + img;
    if (R->ok != 5) return;
    const uint32_t* W = (const uint32_t*)(scan + R->scan_off);  // zero-padded by 128 bytes
    const McuWindow mwin = jpeg_zero_window<T>(R, win, coefs, tid);
    const uint32_t scan_len = R->scan_len;
    if (!jpeg_long::taken(scan_len) || seg_dw < jpeg_long::MIN_SEG_DWORDS || seg_dw > jpeg_long::MAX_SEG_DWORDS) {  // (the host sends neither)
        if (tid == 0) status[img] = 2;
        return;
    }
    const uint32_t bits = scan_len * 8u;
    const uint32_t S = 32u * seg_dw;
    const uint32_t nchap = jpeg_long::chapters(bits, seg_dw);
    {
        const uint32_t* ssrc = (const uint32_t*)(g_slow + (size_t)img * 4);
        for (int i = tid; i < 4 * SLOW_DW; i += T) slow[i] = ssrc[i];
        for (int i = tid; i < 64; i += T) nat[i] = c_zz2nat[i];
    }
    __syncthreads();
    const McuLayout L = jpeg_mcu_layout(R);
    jpeg_build_tables<T>(tab, longtab, slow, L, tid);
    const int mcus_x = R->mcus_x;
    const int total_blocks = mcus_x * (int)R->mcus_y * L.bpm;
    const CoefBlocks cp = {coefs + (size_t)R->coef_blk[0] * 64, mwin};
    const int wend = min(total_blocks, mwin.my1 * mcus_x * L.bpm);   // first block behind the window (the frame's end when all is wanted)
    __syncthreads();

    uint32_t c_p = 0, c_s = 0;
    int c_nb = 0, c_pr0 = 0, c_pr1 = 0, c_pr2 = 0;
    int bad = 0, anybad = 0;
    for (uint32_t chap = 0; chap < nchap; ++chap) {
        const jpeg_long::Chapter C = jpeg_long::chapter(bits, seg_dw, chap);
        const int nseg = (int)C.nseg;
        const bool mine = tid < nseg;
        const uint32_t p_end = jpeg_long::seg_end(bits, seg_dw, C.bit0, (uint32_t)tid);
        {   // speculative pass: segment 0 from the carried state, the others from a guess
            SegState ex = {C.bit0 + (uint32_t)tid * S, 0, 0};
            if (tid == 0) { ex.p = c_p; ex.blk = (int)(c_s >> 8); ex.k = (int)(c_s & 255u); }
            n_p[tid] = ex.p;
            n_s[tid] = (uint32_t)(ex.blk << 8 | ex.k);
            int nblk = 0;
            if (mine) jpeg_state_segment(W, tab, longtab, slow, L, ex, p_end, nblk);
            e_p[tid] = ex.p;
            e_s[tid] = (uint32_t)(ex.blk << 8 | ex.k);
            sc_n[tid] = mine ? nblk : 0;
        }
        __syncthreads();
        int round = 0;
        for (; round <= nseg; ++round) {
            uint32_t np = 0, ns = 0;
            if (tid > 0) { np = e_p[tid - 1]; ns = e_s[tid - 1]; }
            const bool ch = mine && tid > 0 && (np != n_p[tid] || ns != n_s[tid]);
            const uint64_t bal = __ballot(ch);
            const int wave = tid >> 6, lane = tid & 63;
            if (lane == 0) wcount[wave] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < T / 64; ++w) {
                const int c = wcount[w];
                before += w < wave ? c : 0;
                total += c;
            }
            if (total == 0) break;
            if (ch) {
                const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
                todo[pos] = (uint16_t)tid;
                n_p[tid] = np;
                n_s[tid] = ns;
            }
            __syncthreads();
            for (int q = tid; q < total; q += T) {
                const int i = todo[q];
                SegState ex = {n_p[i], (int)(n_s[i] >> 8), (int)(n_s[i] & 255u)};
                int nblk;
                jpeg_state_segment(W, tab, longtab, slow, L, ex, jpeg_long::seg_end(bits, seg_dw, C.bit0, (uint32_t)i), nblk);
                e_p[i] = ex.p;  // nobody reads exit states before the next barrier
                e_s[i] = (uint32_t)(ex.blk << 8 | ex.k);
                sc_n[i] = nblk;
            }
            __syncthreads();
        }
        if (round > nseg) bad = 1;   // (cannot happen: see above; the bound is what ends the loop whatever the stream holds)
        // exclusive prefix over the segments: blocks completed
        const int nblk = sc_n[tid];
        __syncthreads();
        for (int off = 1; off < T; off <<= 1) {
            const int a = tid >= off ? sc_n[tid - off] : 0;
            __syncthreads();
            sc_n[tid] += a;
            __syncthreads();
        }
        const SegState entry = {n_p[tid], (int)(n_s[tid] >> 8), (int)(n_s[tid] & 255u)};
        const int nb_in = c_nb + sc_n[tid] - nblk;
        // output pass: DC predictors starting at zero in every segment, then the prefix sum of the segments' DC-difference sums
        const bool ran = mine && nb_in < wend;
        int q0 = 0, q1 = 0, q2 = 0, ndc = 0;
        if (ran) {
            if (entry.blk != nb_in % L.bpm) bad = 1;  // the propagated state and the block count disagree: corrupt stream
            SegState st = entry;
            int n2;
            jpeg_decode_segment(W, tab, longtab, slow, nat, L, st, p_end, n2, nb_in, total_blocks, q0, q1, q2, ndc, mcus_x, cp, bad);
        }
        const int64_t dsum = (int64_t)q0 + ((int64_t)q1 << 16) + ((int64_t)q2 << 32);
        sc_d[tid] = dsum;
        __syncthreads();
        for (int off = 1; off < T; off <<= 1) {
            const int64_t b = tid >= off ? sc_d[tid - off] : 0;
            __syncthreads();
            sc_d[tid] += b;
            __syncthreads();
        }
        if (ran && ndc > 0) {
            int pr0, pr1, pr2;
            unpack_dsum(sc_d[tid] - dsum, pr0, pr1, pr2);  // the chapter's differences in front of the segment
            pr0 += c_pr0; pr1 += c_pr1; pr2 += c_pr2;      // the predictors at the segment's entry
            if ((pr0 | pr1 | pr2) != 0) {
                const int b0 = nb_in + (entry.k != 0 ? 1 : 0);   // the first block that BEGINS here
                const int mcu = b0 / L.bpm;
                int blk = b0 - mcu * L.bpm, my = mcu / mcus_x, mx = mcu - (mcu / mcus_x) * mcus_x;
                for (int i = 0; i < ndc; ++i) {
                    int16_t* cb = coef_block_ptr(cp, mx, my, b0 + i);
                    const int comp = (int)((L.comp_bits >> (2 * blk)) & 3u);
                    if (cb) cb[0] = (int16_t)(cb[0] + (comp == 0 ? pr0 : comp == 1 ? pr1 : pr2));
                    if (++blk == L.bpm) {
                        blk = 0;
                        if (++mx == mcus_x) { mx = 0; ++my; }
                    }
                }
            }
        }
        // what the next chapter starts from (read before the barrier; the arrays are rewritten behind it)
        c_p = e_p[nseg - 1];
        c_s = e_s[nseg - 1];
        c_nb += sc_n[T - 1];
        {
            int d0, d1, d2;
            unpack_dsum(sc_d[T - 1], d0, d1, d2);
            c_pr0 += d0; c_pr1 += d1; c_pr2 += d2;
        }
        anybad = __syncthreads_or(bad);
        if (anybad || c_nb >= wend) break;
    }
    // an impossible code or an inconsistent state on the way, or the stream ran out before the window's (the frame's) last block
    if (tid == 0) status[img] = (anybad || c_nb < wend) ? 2 : 0;
}

// Streams with restart intervals need no speculation: every interval starts byte aligned with the DC
// predictors at zero.  One workgroup per image, lanes stride over the intervals (the host recorded where
// each begins while stripping the markers) and write their coefficients directly.
template <int T>
__global__ __launch_bounds__(T) void k_jpeg_huff_rst(const JpegImageDev* __restrict__ imgs, const HuffSlow* __restrict__ g_slow,
                                                     const uint8_t* __restrict__ scan, int16_t* __restrict__ coefs,
                                                     int32_t* __restrict__ status, JpegWindow win, const int take_cut)
{
    __shared__ uint32_t tab[4 << TAB_BITS];
    __shared__ uint32_t longtab[2 * LONG_N];
    __shared__ uint32_t slow[4 * SLOW_DW];
    __shared__ uint8_t nat[64];
    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    const JpegImageDev* R = imgs + img;
    if (R->ok != 2) return;
    const uint32_t* W = (const uint32_t*)(scan + R->scan_off);
    const uint32_t* rst = (const uint32_t*)(scan + R->rst_off);
    const McuWindow mwin = jpeg_zero_window<T>(R, win, coefs, tid);
    {
        const uint32_t* ssrc = (const uint32_t*)(g_slow + (size_t)img * 4);
        for (int i = tid; i < 4 * SLOW_DW; i += T) slow[i] = ssrc[i];
        for (int i = tid; i < 64; i += T) nat[i] = c_zz2nat[i];
    }
    __syncthreads();
    const McuLayout L = jpeg_mcu_layout(R);
    jpeg_build_tables<T>(tab, longtab, slow, L, tid);
    const int mcus_x = R->mcus_x;
    const int total_blocks = mcus_x * (int)R->mcus_y * L.bpm;
    const int per_interval = (int)R->restart_interval * L.bpm;
    const int nint = (int)R->rst_cnt;
    const int expected = (total_blocks + per_interval - 1) / per_interval;
    const uint32_t p_stop = R->scan_len * 8u + 32u;   // where a walk stops at the latest: 32 bits into the zero padding
    const CoefBlocks cp = {coefs + (size_t)R->coef_blk[0] * 64, mwin};
    __syncthreads();
    // markers missing or surplus: corrupt stream -- unless the caller takes files that end early (take_cut): then intervals may be
    // missing at the end, and the last one found may be short; both are bit 1 of `bad`, for k_jpeg_cut_tail to settle
    int bad = nint == expected ? 0 : (take_cut && nint < expected ? 2 : 1);
    for (int it = tid; it < min(nint, expected); it += T) {
        SegState st = {rst[it] * 8u, 0, 0};
        const int nb0 = it * per_interval, nb1 = min(nb0 + per_interval, total_blocks);
        int n2, ndc, q0 = 0, q1 = 0, q2 = 0;  // every interval starts with zero predictors
        jpeg_decode_segment(W, tab, longtab, slow, nat, L, st, p_stop, n2, nb0, nb1, q0, q1, q2, ndc, mcus_x, cp, bad);
        if (n2 < nb1 - nb0) bad |= take_cut && it == nint - 1 ? 2 : 1;  // ran out of data before the interval's last block
        else if (take_cut && it == nint - 1 && st.p + 32u > p_stop) bad |= 2;   // complete, but only on zero bits behind the stream's end
    }
    // (the barrier tells whether ANY lane's value is non-zero, not which bits: a second one, for the files that need it, tells corrupt from cut)
    const int any = __syncthreads_or(bad);
    const int anybad = any ? __syncthreads_or(bad & 1) : 0;
    if (tid == 0) status[img] = anybad ? 2 : any ? JPEG_ST_CUT : 0;
}

// ------------------------------------------------- J1, files that end early: the cut MCU ----
// One wave per file behind the Huffman kernels of a run; a file that is not cut (status other than JPEG_ST_CUT) leaves at once.
// The first lane walks on from an exact state (melf_jpeg_cut.h: finish) over the MASKED stream -- the real bits, then zeros that are
// produced, not read -- and stores the coefficients of the blocks inside the window exactly as the output pass would have (the blocks
// the Huffman kernel already wrote there hold the same values: it decoded the same bits followed by the scan area's zero padding).
// Then the wave zeroes the 64 blocks behind the cut MCU: the Huffman kernels stop at bits + 32, not at bits, so a segment's walk
// may have completed blocks of LATER MCUs on zero bits -- fewer than 32 of them, since a symbol ends below bits + 63 and a block
// takes two bits at the least.  Blocks further on were zeroed by jpeg_zero_window and never written.
// Bounds: a block index nb < total_blocks is stored only when its MCU lies inside the window, as coef_block_ptr has it.
// Refused here (status 2): a scan ended by a marker other than EOI, an impossible code met on the way, a state that does not reach
// the stream's end.
static_assert(sizeof(jpeg_cut::Huff) == sizeof(HuffSlow) && offsetof(jpeg_cut::Huff, valoff) == offsetof(HuffSlow, valoff) &&
              offsetof(jpeg_cut::Huff, huffval) == offsetof(HuffSlow, huffval), "melf_jpeg_cut.h restates HuffSlow");
__global__ __launch_bounds__(64) void k_jpeg_cut_tail(const JpegImageDev* __restrict__ imgs, const HuffSlow* __restrict__ g_slow,
                                                      const uint8_t* __restrict__ scan, int16_t* __restrict__ coefs,
                                                      int32_t* __restrict__ status, const JpegCutRec* __restrict__ cutrec, JpegWindow win)
{
    __shared__ uint32_t sl[4 * SLOW_DW];
    __shared__ uint8_t nat[64];
    __shared__ int s_res[2];
    const int img = blockIdx.x, lane = threadIdx.x;
    if (status[img] != JPEG_ST_CUT) return;
    const JpegImageDev* R = imgs + img;
    {
        const uint32_t* ssrc = (const uint32_t*)(g_slow + (size_t)img * 4);
        for (int i = lane; i < 4 * SLOW_DW; i += 64) sl[i] = ssrc[i];
        nat[lane] = c_zz2nat[lane];
    }
    __syncthreads();
    const int hs0 = R->hs0, vs0 = R->vs0, ncomp = R->ncomp, mcus_x = R->mcus_x;
    const int mwid = 8 * hs0, mhei = 8 * vs0;
    const int bpm = ncomp == 1 ? 1 : hs0 * vs0 + 2;
    const int total_blocks = mcus_x * (int)R->mcus_y * bpm;
    // the window in MCUs, as jpeg_zero_window gave it to the Huffman kernels
    const int mx0 = win.x0 / mwid, mx1 = min((win.x1 + mwid - 1) / mwid, mcus_x);
    const int my0 = win.y0 / mhei, my1 = min((win.y1 + mhei - 1) / mhei, (int)R->mcus_y);
    int16_t* const base = coefs + (size_t)R->coef_blk[0] * 64;
    auto inside = [&](const int32_t nb) {
        const int mcu = nb / bpm, my = mcu / mcus_x, mx = mcu - my * mcus_x;
        return nb < total_blocks && mx >= mx0 && mx < mx1 && my >= my0 && my < my1;
    };
    if (lane == 0) {
        int res = jpeg_cut::INVALID_CODE;
        jpeg_cut::State st = {0u, 0, 0, 0, 0, 0, 0};
        const uint32_t m = R->end_marker;
        if (m == 0u || m == 0xD9u) {   // the bytes ended, or EOI: what libjpeg's data source ends a short scan with
            jpeg_cut::Layout L = {bpm, 0u, 0u, 0u};
            for (int b = 0; b < bpm; ++b) {
                const int c = b < bpm - 2 || ncomp == 1 ? 0 : 1 + b - (bpm - 2);
                L.comp_bits |= (uint32_t)c << (2 * b);
                L.dc_bits |= (uint32_t)(R->td[c] & 1) << b;
                L.ac_bits |= (uint32_t)(R->ta[c] & 1) << b;
            }
            const uint8_t* s = scan + R->scan_off;
            const uint32_t bits = R->scan_len * 8u;
            const jpeg_cut::Huff* tabs = (const jpeg_cut::Huff*)sl;
            auto sink = [&](const int32_t nb, const int idx, const int v) {
                if (inside(nb)) base[(size_t)nb * 64 + idx] = (int16_t)v;
            };
            if (R->ok == 1) {
                // the later of the two states k_jpeg_huff left that is not behind the stream's end (a slot it did not write
                // holds zeros: the state at the stream's first bit)
                JpegCutRec r = cutrec[2 * img + 1];
                if (r.p > bits) r = cutrec[2 * img];
                if (r.p <= bits) {
                    st = {r.p, r.blk_k >> 8, r.blk_k & 255, r.nb, r.pred[0], r.pred[1], r.pred[2]};
                    res = jpeg_cut::finish(s, bits, tabs, nat, L, st, total_blocks, sink);
                }
            } else {
                // restart intervals: the last one found from its first bit; if it turns out complete and intervals are still
                // owing, the first MCU of the next one, from zero bits
                const uint32_t* rst = (const uint32_t*)(scan + R->rst_off);
                const int per_interval = (int)R->restart_interval * bpm;
                const int nint = (int)R->rst_cnt, expected = (total_blocks + per_interval - 1) / per_interval;
                if (nint >= 1 && nint <= expected && rst[nint - 1] * 8u <= bits) {
                    st = {rst[nint - 1] * 8u, 0, 0, (nint - 1) * per_interval, 0, 0, 0};
                    res = jpeg_cut::finish(s, bits, tabs, nat, L, st, min(st.nb + per_interval, total_blocks), sink);
                    if (res == jpeg_cut::NOT_CUT && nint < expected) {
                        st = {bits, 0, 0, nint * per_interval, 0, 0, 0};
                        res = jpeg_cut::finish(s, bits, tabs, nat, L, st, min(st.nb + per_interval, total_blocks), sink);
                    }
                }
            }
        }
        s_res[0] = res;
        s_res[1] = st.nb;
    }
    __syncthreads();
    if (s_res[0] != jpeg_cut::CUT) {
        if (lane == 0) status[img] = 2;
        return;
    }
    const int32_t after = s_res[1];
    for (int i = lane; i < 64 * 8; i += 64) {
        const int32_t nb = after + (i >> 3);
        if (inside(nb)) ((uint4*)(base + (size_t)nb * 64))[i & 7] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// ------------------------------------------------- J1, progressive files: one scan ----
// The scans of one LEVEL of every progressive file of a run (melf_jpeg_prog.h has the decoder and what it rests on).  One wave per
// work item (file, scan, restart interval of that scan); an item whose file has no such scan, whose scan is of another level, or
// whose file an earlier level found corrupt, leaves at once.  A scan's level is one more than the highest level among the earlier
// scans of its file that send a coefficient it sends too (same component, overlapping band): levels are launched in order, one
// launch each, so a scan finds what the scans it builds on left, and the scans of a level -- the first DC scan and the first AC
// scans of all bands and components, say -- run side by side.  Inside a launch no wave waits for another: the intervals of a
// scan touch different blocks, the scans of a level different coefficients.  The wave brings the records, the scan's tables and
// their first-level lookup tables into LDS together; the decode itself is one sequential chain (a bit position that depends on
// every symbol before it) and runs on the first lane, which is why melf_jpeg_prog.h keeps memory out of that chain.
__global__ __launch_bounds__(64) void k_jpeg_prog_scan(const jpeg_prog::File* __restrict__ files, const jpeg_prog::Scan* __restrict__ scans,
                                                       const jpeg_prog::Huff* __restrict__ tabs, const uint32_t* __restrict__ rst,
                                                       const uint8_t* __restrict__ raw, int16_t* __restrict__ coefs,
                                                       int32_t* __restrict__ status, const int level)
{
    __shared__ uint32_t sl[4 * SLOW_DW];
    __shared__ uint16_t look[4 * jpeg_prog::LOOK_N];
    __shared__ uint8_t nat[64];
    __shared__ __attribute__((aligned(16))) int16_t stage[64];
    __shared__ uint32_t recs[(sizeof(jpeg_prog::File) + sizeof(jpeg_prog::Scan)) / 4];
    const int img = blockIdx.y, lane = threadIdx.x, s = blockIdx.z;
    if ((uint32_t)s >= files[img].scan_count || scans[files[img].scan_first + (uint32_t)s].level != level || status[img] != 0) return;
    {   // the two records, so that the decoder's loops read them from LDS (nothing it stores can alias them there)
        constexpr int FD = sizeof(jpeg_prog::File) / 4, SD = sizeof(jpeg_prog::Scan) / 4;
        if (lane < FD) recs[lane] = ((const uint32_t*)(files + img))[lane];
        else if (lane < FD + SD) recs[lane] = ((const uint32_t*)(scans + files[img].scan_first + (uint32_t)s))[lane - FD];
    }
    __syncthreads();
    const jpeg_prog::File& F = *(const jpeg_prog::File*)recs;
    const jpeg_prog::Scan& sc = *(const jpeg_prog::Scan*)(recs + sizeof(jpeg_prog::File) / 4);
    const uint32_t expected = jpeg_prog::scan_intervals(F, sc), it = blockIdx.x;
    if (sc.rst_count != expected) {   // restart markers missing or surplus
        if (it == 0 && lane == 0) status[img] = 2;
        return;
    }
    if (it >= expected) return;
    for (int i = lane; i < 4 * SLOW_DW; i += 64) {
        const int t = i / SLOW_DW;
        const int id = t < 3 ? sc.dc_tab[t] : sc.ac_tab;
        sl[i] = id == jpeg_prog::NO_TABLE ? 0u : ((const uint32_t*)(tabs + F.tab_first + id))[i - t * SLOW_DW];
    }
    nat[lane] = c_zz2nat[lane];
    __syncthreads();
    for (int i = lane; i < 4 * jpeg_prog::LOOK_N; i += 64)
        look[i] = jpeg_prog::look_entry((const jpeg_prog::Huff*)sl + i / jpeg_prog::LOOK_N, (uint32_t)(i % jpeg_prog::LOOK_N));
    __syncthreads();
    if (lane != 0) return;
    const uint8_t* d = raw + F.raw_off + sc.off;
    const uint32_t begin = rst[F.rst_first + sc.rst_first + it];
    const uint32_t units = jpeg_prog::scan_units(F, sc);
    const uint32_t u0 = sc.restart_interval ? it * sc.restart_interval : 0u;
    const uint32_t nu = sc.restart_interval ? min(units - u0, (uint32_t)sc.restart_interval) : units;
    int bad = begin > sc.len || (it > 0 && (begin < 2 || d[begin - 1] != 0xD0u + ((it - 1u) & 7u)));   // an RSTn out of sequence
    if (!bad)
        bad = jpeg_prog::decode_interval(F, sc, d, begin, sc.len, u0, nu, (const jpeg_prog::Huff*)sl, look, nat, coefs + (size_t)F.coef_first * 64, stage);
    if (bad) status[img] = 2;
}

// ------------------------------------------------------------------ J2: IDCT ----
// The "accurate integer" inverse DCT (libjpeg jidctint: Loeffler-Ligtenberg-Moschytz, 13-bit
// constants, 2 extra bits kept between the passes).  Every shift below is part of the result.
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

__device__ __forceinline__ void idct_1d(const int in[8], int out[8], const int shift, const bool pass1)
{
    constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633,
                  F1_501 = 12299, F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    (void)pass1;
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * F0_541;
    int tmp2 = z1 + z3 * (-F1_847);
    int tmp3 = z1 + z2 * F0_765;
    z2 = in[0]; z3 = in[4];
    int tmp0 = (z2 + z3) << 13;
    int tmp1 = (z2 - z3) << 13;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F1_175;
    tmp0 *= F0_298; tmp1 *= F2_053; tmp2 *= F3_072; tmp3 *= F1_501;
    z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = descale(tmp10 + tmp3, shift); out[7] = descale(tmp10 - tmp3, shift);
    out[1] = descale(tmp11 + tmp2, shift); out[6] = descale(tmp11 - tmp2, shift);
    out[2] = descale(tmp12 + tmp1, shift); out[5] = descale(tmp12 - tmp1, shift);
    out[3] = descale(tmp13 + tmp0, shift); out[4] = descale(tmp13 - tmp0, shift);
}

__global__ __launch_bounds__(256) void k_jpeg_idct(const JpegImageDev* __restrict__ imgs, const uint16_t* __restrict__ g_qt,
                                                   const int16_t* __restrict__ coefs, const int32_t* __restrict__ status,
                                                   uint8_t* __restrict__ planes, JpegWindow win)
{
    const int img = blockIdx.y;
    const JpegImageDev& I = imgs[img];   // a reference: a local copy indexed by the component lives in scratch
    if (!I.ok || !jpeg_status_ok(status[img])) return;
    // blocks of the MCUs that overlap the pixel window: floor / ceiling in the file's own MCU, the very MCUs jpeg_zero_window gave
    // the Huffman stage (the window's origin is 16-aligned: an MCU corner for MCUs up to 16 x 16, and for the 32 x 8 MCU of 4:1:1
    // possibly the middle of one, which the floor takes whole).  Stores: bx < blocks_x[c], by < blocks_y[c] since mx1 <= mcus_x,
    // my1 <= mcus_y, so a block's 8 x 8 samples lie inside the component's plane of blocks_x * 8 x blocks_y * 8 bytes.
    const int mw = 8 * I.hs0, mh = 8 * I.vs0;
    const int mx0 = win.x0 / mw, mx1 = min((win.x1 + mw - 1) / mw, (int)I.mcus_x);
    const int my0 = win.y0 / mh, my1 = min((win.y1 + mh - 1) / mh, (int)I.mcus_y);
    const int w0 = (mx1 - mx0) * I.hs0, h0 = (my1 - my0) * I.vs0, wc = mx1 - mx0, hc = my1 - my0;
    const int nb0 = w0 * h0;
    const int nbc = I.ncomp == 3 ? wc * hc : 0;
    int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nb0 + 2 * nbc) return;
    int c = 0;
    if (j >= nb0) { j -= nb0; c = 1; if (j >= nbc) { j -= nbc; c = 2; } }
    const int ww = c == 0 ? w0 : wc;
    const int by = (c == 0 ? my0 * I.vs0 : my0) + j / ww, bx = (c == 0 ? mx0 * I.hs0 : mx0) + j % ww;
    // the block's place in decode order (CoefBlocks): its MCU, then its index among the MCU's blocks
    const int fx = c == 0 ? I.hs0 : 1, fy = c == 0 ? I.vs0 : 1, bpm = I.ncomp == 1 ? 1 : I.hs0 * I.vs0 + 2;
    const int mcu = (by / fy) * I.mcus_x + bx / fx;
    const int inb = c == 0 ? (by % fy) * I.hs0 + bx % fx : I.hs0 * I.vs0 + c - 1;
    const int16_t* src = coefs + ((size_t)I.coef_blk[0] + (size_t)mcu * bpm + inb) * 64;
    if (I.planar) {
        // a multi-scan file: the component's real blocks in raster order in its own area.  No scan sends the MCU-padding blocks:
        // they come out as zero blocks (flat 128), and no pixel of the frame reads them
        const uint32_t grid = c == 0 ? I.rst_off : I.rst_cnt;
        const int rbx = (int)(grid & 0xffffu), rby = (int)(grid >> 16);
        if (bx >= rbx || by >= rby) {
            const int pstride = I.blocks_x[c] * 8;
            uint8_t* pad = planes + I.plane_off[c] + (size_t)(by * 8) * pstride + bx * 8;
#pragma unroll
            for (int y = 0; y < 8; ++y) *(uint2*)(pad + (size_t)y * pstride) = make_uint2(0x80808080u, 0x80808080u);
            return;
        }
        src = coefs + ((size_t)I.coef_blk[c] + (size_t)by * rbx + bx) * 64;
    }
    const uint16_t* q = g_qt + ((size_t)img * 4 + I.tq[c]) * 64;
    int ws[64];
    // pass 1: columns
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        int in[8], out[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) in[y] = (int)src[y * 8 + x] * (int)q[y * 8 + x];
        idct_1d(in, out, 13 - 2, true);
#pragma unroll
        for (int y = 0; y < 8; ++y) ws[y * 8 + x] = out[y];
    }
    // pass 2: rows, descale by 2^(13+2+3), level shift and clamp
    const int stride = I.blocks_x[c] * 8;
    uint8_t* dst = planes + I.plane_off[c] + (size_t)(by * 8) * stride + bx * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int out[8];
        idct_1d(ws + y * 8, out, 13 + 2 + 3, false);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            lo |= (uint32_t)min(max(out[x] + 128, 0), 255) << (8 * x);
            hi |= (uint32_t)min(max(out[x + 4] + 128, 0), 255) << (8 * x);
        }
        *(uint2*)(dst + (size_t)y * stride) = make_uint2(lo, hi);
    }
}

// A multi-scan file's status is the worst of its scans' statuses (0 or 2 each): map holds, per such file, the index of its record and
// of its three scans' records.  Runs behind the scans' Huffman kernels; the IDCT and colour stages read the file's combined status.
__global__ __launch_bounds__(64) void k_jpeg_scan_status(const uint32_t* __restrict__ map, const int files, int32_t* __restrict__ status)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= files) return;
    const uint32_t* m = map + 4 * (size_t)f;
    status[m[0]] = max(status[m[1]], max(status[m[2]], status[m[3]]));
}

// ------------------------------------------------------ J3: upsample + colour ----
// "Fancy" upsampling (libjpeg jdsample): a triangle filter, 3/4 nearer sample + 1/4 further one in
// each direction, with the rounding constant alternating 8, 7 (or 1, 2) so that the bias cancels;
// at the image border the missing neighbour is the edge sample itself.
__device__ __forceinline__ int chroma_h2v2(const uint8_t* P, int stride, int cw, int ch, int x, int y)
{
    const int cy = y >> 1, cx = x >> 1;
    const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    const uint8_t* near = P + (size_t)cy * stride;
    const uint8_t* far = P + (size_t)fy * stride;
    if (cw <= 2) return near[cx];  // libjpeg falls back to plain replication for very narrow components
    const int t = 3 * near[cx] + far[cx];
    if (x & 1) return cx == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}
__device__ __forceinline__ int chroma_h2v1(const uint8_t* P, int stride, int cw, int x, int y)
{
    const uint8_t* row = P + (size_t)y * stride;
    const int cx = x >> 1, v = row[cx];
    if (cw <= 2) return v;
    if (x & 1) return cx == cw - 1 ? v : (3 * v + row[cx + 1] + 2) >> 2;
    return cx == 0 ? v : (3 * v + row[cx - 1] + 1) >> 2;
}
// 4:4:0 (libjpeg's h1v2 fancy upsampling): the triangle filter down the columns only, 3/4 the nearer chroma row + 1/4 the further one,
// rounding 1 for the even and 2 for the odd output row; the missing neighbour at the top and bottom is the edge row itself, the last
// REAL row (ch = ceil(H / 2)), not the MCU padding.  No narrow-image fallback: libjpeg has that for the horizontal filters only.
__device__ __forceinline__ int chroma_h1v2(const uint8_t* P, int stride, int ch, int x, int y)
{
    const int cy = y >> 1;
    const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    return (3 * P[(size_t)cy * stride + x] + P[(size_t)fy * stride + x] + 1 + (y & 1)) >> 2;
}

// YCbCr -> RGB with libjpeg's 16-bit fixed-point tables (jdcolor): the rounding term sits in the
// Cb part of the green sum, right shifts are arithmetic.
__device__ __forceinline__ uint32_t ycc_to_bgr(int y, int cb, int cr)
{
    cb -= 128; cr -= 128;
    const int r = y + ((91881 * cr + 32768) >> 16);
    const int g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int b = y + ((116130 * cb + 32768) >> 16);
    return (uint32_t)min(max(b, 0), 255) | ((uint32_t)min(max(g, 0), 255) << 8) | ((uint32_t)min(max(r, 0), 255) << 16);
}

// 4:2:0 fast path (W % 8 == 0, even window rows): one thread per 8 output pixels of TWO rows (2 cy, 2 cy + 1) = 4 chroma
// columns of chroma row cy, which both rows weigh 3/4, plus the row above for the even and the row below for the odd
// output row: three chroma rows fetched for two output rows instead of four, and the work items of a window are packed
// into the workgroups (a 272-pixel window has 34 items per row: one row per 256-thread workgroup left 87 % of the lanes
// idle).  The border cases of the triangle filter are the general formula with the missing neighbour replaced by the
// sample itself ((4t + 8) >> 4 == (3t + t + 8) >> 4), i.e. clamped indices.
__global__ __launch_bounds__(256) void k_jpeg_color420(const JpegImageDev* __restrict__ imgs, const int32_t* __restrict__ status,
                                                       const uint8_t* __restrict__ planes, int H, int W,
                                                       uint8_t* __restrict__ frames, JpegWindow win)
{
    const int img = blockIdx.y;
    const int gx = (win.x1 - win.x0 + 7) / 8;                 // groups of 8 pixels per window row
    const int item = blockIdx.x * 256 + threadIdx.x;
    const int pr = item / gx, g = win.x0 / 8 + (item - pr * gx);
    const int y = win.y0 + 2 * pr;                            // even (win.y0 is a multiple of 16)
    if (y >= win.y1 || g * 8 >= win.x1) return;
    const bool two = y + 1 < win.y1;
    // the record and the status in one round trip (field by field, each && waited for its own load)
    const JpegImageDev rec = imgs[img];
    const int32_t st = status[img];
    const JpegImageDev* R = &rec;
    if (!(rec.ok && rec.ncomp == 3 && rec.hs0 == 2 && rec.vs0 == 2)) return;  // the generic kernel's image
    uint8_t* const orow = frames + ((size_t)img * H + y) * W * 3 + (size_t)g * 24;
    if (!jpeg_status_ok(st)) {  // failed in the entropy decoder: zero frame
        uint2* z = (uint2*)orow;
        z[0] = z[1] = z[2] = make_uint2(0u, 0u);
        if (two) {
            uint2* z2 = (uint2*)(orow + (size_t)W * 3);
            z2[0] = z2[1] = z2[2] = make_uint2(0u, 0u);
        }
        return;
    }
    const int ys = R->blocks_x[0] * 8, cs = R->blocks_x[1] * 8;
    const int cw = (W + 1) >> 1, ch = (H + 1) >> 1;
    const int cy = y >> 1, fu = max(cy - 1, 0), fd = min(cy + 1, ch - 1);
    const int cx0 = g * 4;
    const int cl = max(cx0 - 1, 0), cr = min(cx0 + 4, cw - 1);
    int te[2][6], to[2][6];   // 3 * near + far for the even / the odd output row
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint8_t* P = planes + R->plane_off[1 + c];
        const uint8_t* near = P + (size_t)cy * cs;
        const uint8_t* up = P + (size_t)fu * cs;
        const uint8_t* dn = P + (size_t)fd * cs;
        const uint32_t n4 = *(const uint32_t*)(near + cx0), u4 = *(const uint32_t*)(up + cx0), d4 = *(const uint32_t*)(dn + cx0);
        const int nl = near[cl], nr = near[cr];
        te[c][0] = 3 * nl + up[cl]; te[c][5] = 3 * nr + up[cr];
        to[c][0] = 3 * nl + dn[cl]; to[c][5] = 3 * nr + dn[cr];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nj = 3 * (int)((n4 >> (8 * j)) & 255u);
            te[c][1 + j] = nj + (int)((u4 >> (8 * j)) & 255u);
            to[c][1 + j] = nj + (int)((d4 >> (8 * j)) & 255u);
        }
    }
    const uint8_t* yrow = planes + R->plane_off[0] + (size_t)y * ys + g * 8;
    const uint2 yy0 = *(const uint2*)yrow;
    const uint2 yy1 = two ? *(const uint2*)(yrow + ys) : yy0;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        if (row == 1 && !two) break;
        const int (*t)[6] = row ? to : te;
        const uint2 yy = row ? yy1 : yy0;
        uint32_t px[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cbe = (3 * t[0][1 + j] + t[0][j] + 8) >> 4, cbo = (3 * t[0][1 + j] + t[0][2 + j] + 7) >> 4;
            const int cre = (3 * t[1][1 + j] + t[1][j] + 8) >> 4, cro = (3 * t[1][1 + j] + t[1][2 + j] + 7) >> 4;
            const uint32_t ysrc = j < 2 ? yy.x : yy.y;
            px[2 * j] = ycc_to_bgr((int)((ysrc >> (16 * (j & 1))) & 255u), cbe, cre);
            px[2 * j + 1] = ycc_to_bgr((int)((ysrc >> (16 * (j & 1) + 8)) & 255u), cbo, cro);
        }
        uint32_t* o = (uint32_t*)(orow + (size_t)row * W * 3);
        uint32_t d[6];
        d[0] = px[0] | (px[1] << 24); d[1] = (px[1] >> 8) | (px[2] << 16); d[2] = (px[2] >> 16) | (px[3] << 8);
        d[3] = px[4] | (px[5] << 24); d[4] = (px[5] >> 8) | (px[6] << 16); d[5] = (px[6] >> 16) | (px[7] << 8);
        *(uint2*)(o) = make_uint2(d[0], d[1]);
        *(uint2*)(o + 2) = make_uint2(d[2], d[3]);
        *(uint2*)(o + 4) = make_uint2(d[4], d[5]);
    }
}

// One pixel of any sampling the decoder takes, as 0x00RRGGBB: the general colour stage, shared by the upright kernel below and by
// the oriented one.  H and W are the STORED frame's (the chroma planes' sizes and border rules follow from them).
struct PlaneSrc {
    const uint8_t *Y, *Cb, *Cr;
    int ys, cs, cw, ch;
    int mode;   // 0 grey, 1 4:4:4, 2 4:2:2 (h2v1), 3 4:2:0 (h2v2), 4 4:4:0 (h1v2), 5 4:1:1 (h4v1: plain replication)
};
// Bounds of the two chroma reads melf_ctx_set_jpeg_samplings adds, for a pixel (x, y) of the window, 0 <= x < W, 0 <= y < H (the
// window lies inside the stored frame), in a chroma plane of cs = 8 * blocks_x[1] bytes a row and 8 * blocks_y[1] rows:
//   4:1:1  column x >> 2 <= (W - 1) / 4 < cw = ceil(W / 4) <= 8 * ceil(W / 32) = 8 * blocks_x[1], row y < H <= 8 * blocks_y[1].  The
//          sample's MCU is the one that holds pixel (x, y) (an MCU is 32 pixels = 8 chroma columns wide), so it overlaps the window
//          and was inverse-transformed for every window (k_jpeg_idct takes every MCU that holds a pixel of it).
//   4:4:0  column x < W <= 8 * blocks_x[1]; rows cy = y >> 1 <= (H - 1) / 2 < ch = ceil(H / 2) <= 8 * blocks_y[1], and cy - 1, cy + 1
//          clamped to [0, ch): inside the plane whatever the window.  Row cy is in the MCU of pixel (x, y); rows cy +- 1 are luma rows
//          y - 2 .. y + 3, so for the pixels a caller reads (at least 16 rows inside the window, or at a frame edge, where the clamp
//          applies) they are rows of the window and their MCU rows were inverse-transformed.  The window's own outermost two rows
//          may filter with a row from outside it -- memory of this file's plane, never read by the caller -- exactly as the first and
//          last rows of a 4:2:0 window always have.
__device__ __forceinline__ PlaneSrc plane_src(const JpegImageDev& I, const uint8_t* planes, int H, int W)
{
    PlaneSrc s;
    s.Y = planes + I.plane_off[0];
    s.ys = I.blocks_x[0] * 8;
    s.mode = I.ncomp == 1 ? 0 : (I.hs0 == 2 && I.vs0 == 2) ? 3 : I.hs0 == 2 ? 2 : I.vs0 == 2 ? 4 : I.hs0 == 4 ? 5 : 1;
    s.Cb = s.Cr = s.Y;
    s.cs = s.cw = s.ch = 0;
    if (I.ncomp != 1) {
        s.Cb = planes + I.plane_off[1];
        s.Cr = planes + I.plane_off[2];
        s.cs = I.blocks_x[1] * 8;
        s.cw = (W + I.hs0 - 1) / I.hs0; s.ch = (H + I.vs0 - 1) / I.vs0;
    }
    return s;
}
__device__ __forceinline__ uint32_t plane_bgr(const PlaneSrc& s, int x, int y)
{
    const int yy = s.Y[(size_t)y * s.ys + x];
    if (s.mode == 0) return (uint32_t)yy | ((uint32_t)yy << 8) | ((uint32_t)yy << 16);
    int cb, cr;
    if (s.mode == 3) { cb = chroma_h2v2(s.Cb, s.cs, s.cw, s.ch, x, y); cr = chroma_h2v2(s.Cr, s.cs, s.cw, s.ch, x, y); }
    else if (s.mode == 2) { cb = chroma_h2v1(s.Cb, s.cs, s.cw, x, y); cr = chroma_h2v1(s.Cr, s.cs, s.cw, x, y); }
    else if (s.mode == 4) { cb = chroma_h1v2(s.Cb, s.cs, s.ch, x, y); cr = chroma_h1v2(s.Cr, s.cs, s.ch, x, y); }
    else if (s.mode == 5) { cb = s.Cb[(size_t)y * s.cs + (x >> 2)]; cr = s.Cr[(size_t)y * s.cs + (x >> 2)]; }
    else { cb = s.Cb[(size_t)y * s.cs + x]; cr = s.Cr[(size_t)y * s.cs + x]; }
    return ycc_to_bgr(yy, cb, cr);
}

__global__ __launch_bounds__(256) void k_jpeg_color(const JpegImageDev* __restrict__ imgs, const int32_t* __restrict__ status,
                                                    const uint8_t* __restrict__ planes, int H, int W,
                                                    uint8_t* __restrict__ frames, int fast420, JpegWindow win)
{
    const int img = blockIdx.z, y = win.y0 + blockIdx.y;
    const int x0 = win.x0 + (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= win.x1) return;
    const JpegImageDev& I = imgs[img];   // a reference: a local copy indexed by the component lives in scratch
    if (fast420 && I.ok && I.ncomp == 3 && I.hs0 == 2 && I.vs0 == 2) return;  // k_jpeg_color420 did it
    uint8_t* out = frames + ((size_t)img * H + y) * W * 3 + (size_t)x0 * 3;
    const int npx = min(4, W - x0);
    if (!I.ok || !jpeg_status_ok(status[img])) {
        for (int k = 0; k < npx * 3; ++k) out[k] = 0;
        return;
    }
    const PlaneSrc src = plane_src(I, planes, H, W);
    uint32_t px[4] = {0, 0, 0, 0};
    for (int k = 0; k < npx; ++k) px[k] = plane_bgr(src, x0 + k, y);
    if (npx == 4 && ((W * 3) & 3) == 0) {  // 12 bytes, dword aligned
        uint32_t* o = (uint32_t*)out;
        o[0] = px[0] | (px[1] << 24);
        o[1] = (px[1] >> 8) | (px[2] << 16);
        o[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int k = 0; k < npx; ++k) { out[3 * k] = px[k] & 255; out[3 * k + 1] = (px[k] >> 8) & 255; out[3 * k + 2] = (px[k] >> 16) & 255; }
    }
}

// Colour stage of the files stored under an EXIF orientation 2-8 (every sampling, any size).  Decode first, permute afterwards, as
// cv2.imread does: the conversion above runs in STORED geometry (Hs x Ws, the chroma filter along the stored axes), and each pixel
// is written where the upright frame has it (melf_jpeg_orient_addr.h); the frames are n x H' x W' x 3 with H' x W' = Ws x Hs for
// codes 5-8.  Built like k_orient_tiles: a workgroup takes a tile of OT x OT pixels of the stored window, every thread converts
// pixels along the stored rows (the plane reads of a wave are contiguous) and parks them as one dword each in LDS; after the
// barrier the workgroup writes the tile's rows of the UPRIGHT frame, consecutive lanes consecutive dwords of a row.
// OT = 64, not 32: an upright row of a tile is then 192 contiguous bytes instead of 96 (the store side is what the kernel is bound
// by: W' * 3 has no alignment, so every row has ragged ends, and they are a 6th of the row's dwords at 32 and a 12th at 64), and the
// tile's 16.3 KiB of LDS still leave room for 9 workgroups on a CU, more than the 8 its wave slots hold at 256 threads.
// Row pitch 65 dwords: the transposed read (codes 5-8) walks a tile column, 65 dwords apart, i.e. one bank further per pixel (LDS
// dword reads bank over 32 dwords per 32-lane half); the row-wise write and the untransposed read are contiguous anyway.
// Bounds: win lies inside the stored frame (jpeg_orient::window clamps it), so sx < Ws <= 8 * blocks_x and sy < Hs <= 8 * blocks_y:
// no load leaves the file's own planes (the chroma filter clamps its neighbours itself); and the stored pixel (sx, sy) of the frame
// goes to one pixel (x, y) of H' x W': no store leaves bytes [0, H' * W' * 3) of the file's frame.
constexpr int OT = 64, OT_PITCH = OT + 1;
__global__ __launch_bounds__(256) void k_jpeg_color_exif(const JpegImageDev* __restrict__ imgs, const int32_t* __restrict__ status,
                                                             const uint8_t* __restrict__ planes, int Hs, int Ws, int code,
                                                             uint8_t* __restrict__ frames, JpegWindow win)
{
    __shared__ uint32_t tile[OT * OT_PITCH];
    const int img = blockIdx.y;
    const int tiles_x = (win.x1 - win.x0 + OT - 1) / OT;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int sx0 = win.x0 + tx * OT, sy0 = win.y0 + ty * OT;
    const int tw = min(OT, win.x1 - sx0), th = min(OT, win.y1 - sy0);
    if (tw <= 0 || th <= 0) return;   // uniform: a launch with more tiles than the window has
    const JpegImageDev& I = imgs[img];
    if (I.ok && jpeg_status_ok(status[img])) {
        const PlaneSrc src = plane_src(I, planes, Hs, Ws);
        for (int i = threadIdx.x; i < th * OT; i += 256) {
            const int ly = i / OT, lx = i % OT;
            if (lx < tw) tile[ly * OT_PITCH + lx] = plane_bgr(src, sx0 + lx, sy0 + ly);
        }
    } else {   // not decoded, or failed in the entropy decoder: zeros over its oriented window
        for (int i = threadIdx.x; i < th * OT; i += 256) tile[(i / OT) * OT_PITCH + i % OT] = 0;
    }
    __syncthreads();
    // the tile in the upright frame: nr rows of nc pixels from (x0, y0); element e of row r sits at tile[base + r * sr + e * se]
    const bool t = jpeg_orient::transposed(code), fx = jpeg_orient::flips_x(code), fy = jpeg_orient::flips_y(code);
    const int u0 = fx ? Ws - sx0 - tw : sx0, v0 = fy ? Hs - sy0 - th : sy0;
    const int step_x = fx ? -1 : 1, step_y = fy ? -OT_PITCH : OT_PITCH;
    const int base = (fx ? tw - 1 : 0) + (fy ? (th - 1) * OT_PITCH : 0);
    const int nr = t ? tw : th, nc = t ? th : tw, x0 = t ? v0 : u0, y0 = t ? u0 : v0;
    const int sr = t ? step_x : step_y, se = t ? step_y : step_x;
    const int Hup = t ? Ws : Hs, Wup = t ? Hs : Ws;
    uint8_t* const out = frames + (size_t)img * Hup * Wup * 3;
    const int nb = nc * 3;              // bytes of a row of the tile
    const int slots = (nb + 6) / 4;     // aligned dwords a row can touch, whatever its first byte's alignment
    for (int i = threadIdx.x; i < nr * slots; i += 256) {
        const int r = i / slots, k = i - r * slots;
        uint8_t* const row = out + ((size_t)(y0 + r) * Wup + x0) * 3;
        const int j0 = 4 * k - (int)((uintptr_t)row & 3);   // the slot's first byte, counted from the row's first
        if (j0 >= nb) continue;
        const int li = base + r * sr;
        if (j0 >= 0 && j0 + 4 <= nb) {   // a whole dword of the row: the bytes of two neighbouring pixels
            const int e = j0 / 3, q = j0 - 3 * e;
            const uint64_t two = (uint64_t)tile[li + e * se] | ((uint64_t)tile[li + min(e + 1, nc - 1) * se] << 24);
            *(uint32_t*)(row + j0) = (uint32_t)(two >> (8 * q));
        } else {                         // a ragged end: byte stores
            for (int b = max(j0, 0); b < min(j0 + 4, nb); ++b) {
                const int e = b / 3, q = b - 3 * e;
                row[b] = (uint8_t)(tile[li + e * se] >> (8 * q));
            }
        }
    }
}

// ------------------------------------------------------------------ workspace ----
struct JpegWorkspace {
    uint8_t* h_stage = nullptr;  // pinned: records and tables of one batch
    size_t h_cap = 0;
    uint8_t* d_stage = nullptr;  // the same on the device, and behind them the clean scans (written by k_jpeg_clean)
    size_t d_cap = 0;
    uint8_t* h_raw = nullptr;    // pinned: the files' entropy-coded segments as they are in the files
    size_t h_raw_cap = 0;
    uint8_t* d_raw = nullptr;
    size_t d_raw_cap = 0;
    size_t raw_total = 0;        // bytes of the raw area in use
    const uint8_t* raw_src = nullptr;  // where the upload of the raw area starts: h_raw, or the caller's own pinned buffer
    int16_t* d_coefs = nullptr;
    size_t coef_cap = 0;  // int16 elements
    uint8_t* d_planes = nullptr;
    size_t plane_cap = 0;
    int32_t* d_status = nullptr;
    size_t status_cap = 0;
    bool cut = false;            // the batch's context takes files that end early (TAKE_TRUNCATED): the Huffman kernels leave states
    uint8_t* d_cut = nullptr;    // in two JpegCutRec per file here, and k_jpeg_cut_tail runs behind them
    size_t cut_cap = 0;
    // layout of the current batch inside the stage buffers
    size_t off_imgs = 0, off_qt = 0, off_slow = 0, off_scan = 0, total = 0;   // total: what is uploaded (records + tables)
    size_t off_pfile = 0, off_pscan = 0, off_ptab = 0, off_prst = 0;          // progressive files: their records, scans, tables, intervals
    size_t scan_bytes = 0;      // device-only scan area behind them
    size_t coef_elems = 0, plane_bytes = 0;
    int max_blocks = 0;
    int n_par = 0, n_seq = 0;   // images for the segment-parallel / the restart-interval Huffman kernel
    int n_420 = 0;              // three-component 4:2:0 images (fast colour kernel)
    int n_long = 0;             // images for k_jpeg_chapters (melf_ctx_set_jpeg_long_scans)
    uint32_t long_dw = 0;       // its segment length in dwords (melf_jpeg_long.h)
    size_t max_par_scan = 0;    // longest clean scan among the former (bytes)
    // The batch as runs of consecutive files of one orientation code: J1..J3 are launched once per run, on the run's window of
    // the stored frame.  A batch without oriented files is one run of code 1 whose counts are the five above.
    // A run of progressive files (prog) is decoded level by level (k_jpeg_prog_scan): prog_items[l] = the most restart intervals any
    // scan of level l of its files has, prog_scans the most scans of a file; its files' coefficient blocks (prog_coef0, prog_coefs of them, in blocks) are zeroed in front of the first scan.
    struct Run {
        int first, n, code;
        int n_par, n_seq, n_420, max_blocks;
        size_t max_par_scan;
        bool prog = false;
        size_t prog_coef0 = 0, prog_coefs = 0;
        std::vector<uint32_t> prog_items;
        uint32_t prog_scans = 0;
        int n_long = 0;   // files for k_jpeg_chapters (ok = 5)
    };
    std::vector<Run> runs;
    // Multi-scan sequential files (melf_jpeg_scans.h): their scans are one-component records of their own behind the batch's n file
    // records (n_scan_recs of them, with tables and clean-scan regions of their own), grouped by what fixes a scan's window -- the
    // file's orientation code and sampling, and whether the component is luma or chroma -- each group one launch of the Huffman kernels
    // on its own window.  ms_files: such files in the batch; off_msmap: per file the indices of its record and of its three scans'
    // records (k_jpeg_scan_status).  A batch without such a file has none of this and launches what it launched before.
    struct ScanGroup {
        int first, n, code, hs0, vs0, chroma;   // first: index among the scan records
        int n_par, n_seq;
        size_t max_par_scan;
    };
    std::vector<ScanGroup> scan_groups;
    int n_scan_recs = 0, ms_files = 0;
    size_t off_msmap = 0;
};

void jpeg_workspace_free(JpegWorkspace* w)
{
    if (!w) return;
    if (w->h_stage) (void)hipHostFree(w->h_stage);
    if (w->d_stage) (void)hipFree(w->d_stage);
    if (w->h_raw) (void)hipHostFree(w->h_raw);
    if (w->d_raw) (void)hipFree(w->d_raw);
    if (w->d_coefs) (void)hipFree(w->d_coefs);
    if (w->d_planes) (void)hipFree(w->d_planes);
    if (w->d_status) (void)hipFree(w->d_status);
    if (w->d_cut) (void)hipFree(w->d_cut);
    delete w;
}

template <class T>
static hipError_t grow_dev(T** p, size_t* cap, size_t need)
{
    if (need <= *cap) return hipSuccess;
    if (*p) {
        // With several chunks (and up to three calls) in flight the kernels of an older chunk may still read this workspace:
        // the caller has only waited for the slot's UPLOAD event.  hipFree happens to synchronise, but nothing promises it
        // (melf_api.hip's grow() does the same); growth is rare.
        (void)hipDeviceSynchronize();
        (void)hipFree(*p);
    }
    *p = nullptr; *cap = 0;
    const size_t want = need + need / 4;
    hipError_t e = hipMalloc((void**)p, want * sizeof(T));
    if (e == hipSuccess) *cap = want;
    return e;
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Header parse of n files in one parallel pass (a chunked caller parses the whole call's files once and prepares chunk
// by chunk): status[i] 0 = for the GPU, 1 = valid but unsupported, 2 = unreadable, 3 = other size.
struct JpegParsed {
    std::vector<JpegHeader> hdr;
    std::vector<HuffSlow> slow;   // 4 per file (DC 0, DC 1, AC 0, AC 1), when built with the headers; else empty
};
static void build_slow4(const JpegHeader& h, HuffSlow* slow)
{
    for (int t = 0; t < 2; ++t) {
        if (h.dc[t].set) build_huff(h.dc[t], slow + t); else memset(slow + t, 0, sizeof(HuffSlow));
        if (h.ac[t].set) build_huff(h.ac[t], slow + 2 + t); else memset(slow + 2 + t, 0, sizeof(HuffSlow));
    }
}
JpegParsed* jpeg_parsed_new(int n, bool with_tables)
{
    JpegParsed* p = new JpegParsed();
    p->hdr.resize(n);
    if (with_tables) p->slow.resize((size_t)n * 4);
    return p;
}
void jpeg_parsed_resize(JpegParsed* p, int n)   // keeps what it has allocated: entries are reset by jpeg_parse_one
{
    if ((int)p->hdr.size() < n) p->hdr.resize(n);
    if (!p->slow.empty() && p->slow.size() < (size_t)n * 4) p->slow.resize((size_t)n * 4);
}
// take_orient: files with an orientation tag are taken, and H, W are then the UPRIGHT size (what a caller groups files by).
void jpeg_parse_one(JpegParsed* p, int i, const uint8_t* data, size_t size, int* H, int* W, int* supported, int take)
{
    JpegHeader& h = p->hdr[i];
    h = JpegHeader();   // the object may be a previous call's
    if (!data || parse_headers(data, size, h, take) != 0) { h.progressive = false; *H = *W = 0; *supported = 0; return; }
    *H = jpeg_orient::swapped_h(h.orient, h.H, h.W); *W = jpeg_orient::swapped_w(h.orient, h.H, h.W); *supported = h.why ? 0 : 1;
    if (!h.why && !h.progressive && !p->slow.empty()) build_slow4(h, p->slow.data() + (size_t)i * 4);   // (a progressive file's tables go with its scans)
}
void jpeg_parsed_free(JpegParsed* p) { delete p; }
int jpeg_parsed_orientation(const JpegParsed* p, int i) { return p->hdr[i].orient; }
int jpeg_parsed_progressive(const JpegParsed* p, int i) { return p->hdr[i].progressive ? 1 : 0; }

// Host half of a batch: parse every file (unless `parsed` holds the headers already: files first .. first + n - 1 of that
// pass, host_status filled), lay the batch out, fill the pinned stage buffer.
// host_status[i]: 0 = handed to the GPU, 1 = valid but unsupported, 2 = unreadable, 3 = other size.
// take_orient: files with an EXIF orientation 2..8 are handed to the GPU too; H and W are the UPRIGHT size, which such a file's
// stored size gives after the swap its code asks for, and everything laid out here for it follows its STORED size.
int jpeg_prepare_batch(JpegWorkspace** pws, const uint8_t* const* data, const size_t* sizes, int n, int H, int W,
                       int32_t* host_status, std::string* err, const JpegParsed* parsed, int first, const int* pidx,
                       const uint8_t* pin_base, size_t pin_len, int take)
{
    if (!*pws) *pws = new JpegWorkspace();
    JpegWorkspace* w = *pws;
    w->cut = (take & TAKE_TRUNCATED) != 0;
    // long scans (melf_ctx_set_jpeg_long_scans): the segment length of the chapters, and from which raw length on a restart-less
    // baseline scan is k_jpeg_chapters's -- beyond what k_jpeg_huff addresses, or beyond one chapter where the caller chose a length
    const bool long_on = (take & TAKE_LONG) != 0;
    const uint32_t long_choice = ((uint32_t)take >> JPEG_TAKE_LONG_DW_SHIFT) & JPEG_TAKE_LONG_DW_MASK;
    w->long_dw = long_choice ? long_choice : jpeg_long::MAX_SEG_DWORDS;
    const size_t long_from = long_choice ? jpeg_long::chapter_bytes(long_choice) : JPEG_MAX_PAR_SCAN;
    static const bool trace = diag_env("MELF_JPEG_TRACE") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    std::vector<JpegHeader> own;
    std::vector<size_t> scan_off(n + 1, 0), raw_off(n + 1, 0);
    const int nthreads = host_pool().size() + 1;
    auto par_for = [&](const std::function<void(int)>& fn) { host_pool().run(n, fn); };
    if (!parsed) {
        own.resize(n);
        par_for([&](int i) {
            JpegHeader& h = own[i];
            if (!data[i] || parse_headers(data[i], sizes[i], h, take) != 0) { host_status[i] = 2; return; }
            if (h.why) { host_status[i] = 1; return; }
            if (jpeg_orient::swapped_h(h.orient, h.H, h.W) != H || jpeg_orient::swapped_w(h.orient, h.H, h.W) != W) { host_status[i] = 3; return; }
            host_status[i] = 0;
        });
    }
    auto hidx = [&](int i) { return parsed ? (pidx ? pidx[first + i] : first + i) : i; };
    const JpegHeader* const hbase = parsed ? parsed->hdr.data() : own.data();
    // Every file of the batch already in the caller's pinned buffer: the upload starts there (one span from the first file's
    // first byte to the last one's last; what lies between the files travels along), no byte is copied here.
    bool direct = pin_base != nullptr && n > 0;
    const uint8_t* span_lo = nullptr;
    const uint8_t* span_hi = nullptr;
    size_t bytes_sum = 0;
    if (direct) {
        for (int i = 0; i < n && direct; ++i) {
            if (host_status[i] != 0) continue;
            if (data[i] < pin_base || data[i] + sizes[i] + 64 > pin_base + pin_len) { direct = false; break; }
            if (!span_lo || data[i] < span_lo) span_lo = data[i];
            if (!span_hi || data[i] + sizes[i] > span_hi) span_hi = data[i] + sizes[i];
            bytes_sum += sizes[i];
        }
        // a batch picked from all over the buffer (the flat files that go first, a second frame size): copy after all
        if (direct && (!span_lo || (size_t)(span_hi - span_lo) > 2 * bytes_sum + (1u << 20))) direct = false;
    }
    const auto tp1 = std::chrono::steady_clock::now();
    // layout
    size_t coef_blocks = 0, plane_bytes = 0;
    int max_blocks = 0;
    std::vector<JpegImageDev> rec(n);
    std::vector<int> ms_files;            // multi-scan sequential files handed to the GPU
    std::vector<jpeg_prog::File> pfile;   // one per file once the batch has a progressive file
    size_t pscans = 0, ptabs = 0, prsts = 0;
    for (int i = 0; i < n; ++i)
        if (host_status[i] == 0 && hbase[hidx(i)].progressive) { pfile.resize(n); memset(pfile.data(), 0, (size_t)n * sizeof(jpeg_prog::File)); break; }
    for (int i = 0; i < n; ++i) {
        JpegImageDev& r = rec[i];
        memset(&r, 0, sizeof(r));
        scan_off[i + 1] = scan_off[i];
        raw_off[i + 1] = raw_off[i];
        if (host_status[i] != 0) continue;
        const JpegHeader& h = hbase[hidx(i)];
        if (h.multiscan) {   // each scan has the 1024-segment allowance of a file's one scan
            for (const JpegHeader::MScan& sc : h.ms)
                if (!sc.restart_interval && sc.len > JPEG_MAX_PAR_SCAN) host_status[i] = 1;   // valid, but for the host decoder
            if (host_status[i] != 0) continue;
            ms_files.push_back(i);
        }
        if (h.progressive) {
            jpeg_prog::File& f = pfile[i];
            f = prog_file_geometry(h);
            f.scan_first = (uint32_t)pscans; f.scan_count = (uint32_t)h.pscans.size();
            f.tab_first = (uint32_t)ptabs; f.rst_first = (uint32_t)prsts;
            f.coef_first = (uint32_t)coef_blocks;
            pscans += h.pscans.size(); ptabs += h.ptabs.size(); prsts += h.prst.size();
        }
        r.ok = 1;
        r.orient = (uint8_t)h.orient;
        r.ncomp = (uint8_t)h.ncomp; r.hs0 = (uint8_t)h.hs[0]; r.vs0 = (uint8_t)h.vs[0];
        r.restart_interval = (uint16_t)h.restart_interval;
        r.mcus_x = (uint16_t)((h.W + 8 * h.hs[0] - 1) / (8 * h.hs[0]));   // the stored size: (W, H), swapped for codes 5-8
        r.mcus_y = (uint16_t)((h.H + 8 * h.vs[0] - 1) / (8 * h.vs[0]));
        int blocks = 0;
        for (int c = 0; c < h.ncomp; ++c) {
            r.tq[c] = (uint8_t)h.tq[c]; r.td[c] = (uint8_t)h.td[c]; r.ta[c] = (uint8_t)h.ta[c];
            r.blocks_x[c] = (uint16_t)(r.mcus_x * (c == 0 ? h.hs[0] : 1));
            r.blocks_y[c] = (uint16_t)(r.mcus_y * (c == 0 ? h.vs[0] : 1));
            r.coef_blk[c] = (uint32_t)coef_blocks;
            r.plane_off[c] = (uint32_t)plane_bytes;
            const size_t nb = (size_t)r.blocks_x[c] * r.blocks_y[c];
            coef_blocks += nb;
            plane_bytes += nb * 64;
            blocks += (int)nb;
        }
        max_blocks = std::max(max_blocks, blocks);
        const size_t raw_len = sizes[i] - h.scan_begin;
        r.raw_off = direct ? (uint32_t)(data[i] + h.scan_begin - span_lo) : (uint32_t)raw_off[i];
        r.raw_len = (uint32_t)raw_len;
        raw_off[i + 1] = raw_off[i] + align_up(raw_len + 32, 64);   // k_jpeg_clean reads up to 20 bytes past the end
        // (a progressive file is decoded from its raw bytes: no clean scan, no restart table in the scan area)
        size_t region = (h.progressive || h.multiscan) ? 128 : align_up(raw_len + 128, 64);
        if (h.restart_interval && !h.progressive && !h.multiscan) {  // room for the table of interval offsets behind the scan
            const size_t mcus = (size_t)r.mcus_x * r.mcus_y;
            r.rst_cnt = (uint32_t)((mcus + h.restart_interval - 1) / h.restart_interval);  // expected; replaced by the number found
            r.rst_off = (uint32_t)region;                                                   // relative for now
            region += align_up(((size_t)r.rst_cnt + 1) * sizeof(uint32_t), 64);
        }
        scan_off[i + 1] = scan_off[i] + region;
    }
    // The scans of the multi-scan files: one-component records behind the n file records, in groups of one window
    struct ScanEntry { int file, comp; uint32_t key; };
    std::vector<ScanEntry> ms_scans;
    for (const int i : ms_files)
        for (int c = 0; c < 3; ++c)
            ms_scans.push_back({i, c, (uint32_t)rec[i].orient << 16 | (uint32_t)rec[i].hs0 << 8 | (uint32_t)rec[i].vs0 << 4 | (c ? 1u : 0u)});
    std::stable_sort(ms_scans.begin(), ms_scans.end(), [](const ScanEntry& a, const ScanEntry& b) { return a.key < b.key; });
    const int extra = (int)ms_scans.size();
    w->scan_groups.clear();
    w->n_scan_recs = extra;
    w->ms_files = (int)ms_files.size();
    if (extra) {
        rec.resize((size_t)n + extra);
        scan_off.resize((size_t)n + extra + 1);
        for (int k = 0; k < extra; ++k) {
            const ScanEntry& se = ms_scans[k];
            const JpegHeader& h = hbase[hidx(se.file)];
            const JpegHeader::MScan& sc = h.ms[se.comp];
            const jpeg_scans::Comp comp = jpeg_scans::component(h.W, h.H, h.hs[0], h.vs[0], se.comp);
            JpegImageDev& r = rec[(size_t)n + k];
            memset(&r, 0, sizeof(r));
            r.ok = sc.restart_interval ? 2 : 1;
            r.orient = 1;
            r.ncomp = 1; r.hs0 = 1; r.vs0 = 1;
            r.restart_interval = (uint16_t)sc.restart_interval;
            r.mcus_x = r.blocks_x[0] = (uint16_t)comp.rbx;   // one block is an MCU: the component's real blocks in raster order
            r.mcus_y = r.blocks_y[0] = (uint16_t)comp.rby;
            r.coef_blk[0] = rec[se.file].coef_blk[se.comp];
            r.raw_off = rec[se.file].raw_off + (uint32_t)sc.off;   // inside the file's bytes, which are uploaded once
            r.raw_len = (uint32_t)sc.len;
            size_t region = align_up(sc.len + 128, 64);
            r.scan_cap = (uint32_t)region;
            r.scan_off = (uint32_t)scan_off[(size_t)n + k];
            if (sc.restart_interval) {
                const size_t blocks = (size_t)comp.rbx * comp.rby;
                r.rst_cnt = (uint32_t)((blocks + sc.restart_interval - 1) / sc.restart_interval);   // expected; replaced by the number found
                r.rst_off = (uint32_t)(scan_off[(size_t)n + k] + region);
                region += align_up(((size_t)r.rst_cnt + 1) * sizeof(uint32_t), 64);
            }
            scan_off[(size_t)n + k + 1] = scan_off[(size_t)n + k] + region;
            if (w->scan_groups.empty() || ms_scans[k - 1].key != se.key)
                w->scan_groups.push_back({k, 0, (int)rec[se.file].orient, (int)rec[se.file].hs0, (int)rec[se.file].vs0, se.comp ? 1 : 0, 0, 0, 0});
            JpegWorkspace::ScanGroup& g = w->scan_groups.back();
            ++g.n;
            if (r.ok == 1) { ++g.n_par; g.max_par_scan = std::max(g.max_par_scan, sc.len); } else ++g.n_seq;
        }
    }
    const size_t nrec = (size_t)n + extra;
    if (coef_blocks >= (1ull << 32) / 64 || plane_bytes >= (1ull << 32) || scan_off[nrec] >= (1ull << 32) || raw_off[n] >= (1ull << 32)) {
        if (err) *err = "JPEG batch too large for 32-bit offsets; decode in smaller batches";
        return MELF_ERR_TOO_LARGE;
    }
    w->off_imgs = 0;
    w->off_qt = align_up(w->off_imgs + nrec * sizeof(JpegImageDev), 256);
    w->off_slow = align_up(w->off_qt + (size_t)n * 4 * 64 * sizeof(uint16_t), 256);
    w->off_pfile = align_up(w->off_slow + nrec * 4 * sizeof(HuffSlow), 256);
    w->off_pscan = align_up(w->off_pfile + pfile.size() * sizeof(jpeg_prog::File), 256);
    w->off_ptab = align_up(w->off_pscan + pscans * sizeof(jpeg_prog::Scan), 256);
    w->off_prst = align_up(w->off_ptab + ptabs * sizeof(jpeg_prog::Huff), 256);
    w->off_msmap = align_up(w->off_prst + prsts * sizeof(uint32_t), 256);
    w->off_scan = align_up(w->off_msmap + ms_files.size() * 4 * sizeof(uint32_t), 256);
    w->total = w->off_scan;                 // uploaded: records + tables
    w->scan_bytes = scan_off[nrec] + 64;    // device only
    w->raw_total = direct ? (size_t)(span_hi - span_lo) + 64 : raw_off[n] + 64;
    if (w->raw_total >= (1ull << 32)) {
        if (err) *err = "JPEG batch too large for 32-bit offsets; decode in smaller batches";
        return MELF_ERR_TOO_LARGE;
    }
    if (!direct && w->raw_total > w->h_raw_cap) {
        if (w->h_raw) (void)hipHostFree(w->h_raw);
        w->h_raw = nullptr; w->h_raw_cap = 0;
        const size_t want = w->raw_total + w->raw_total / 4;
        if (hipHostMalloc((void**)&w->h_raw, want, hipHostMallocDefault) != hipSuccess) {
            if (err) *err = "hipHostMalloc failed for the JPEG raw-scan buffer";
            return MELF_ERR_HIP;
        }
        w->h_raw_cap = want;
    }
    w->raw_src = direct ? span_lo : w->h_raw;
    w->coef_elems = coef_blocks * 64;
    w->plane_bytes = plane_bytes;
    w->max_blocks = max_blocks;
    if (w->total > w->h_cap) {
        if (w->h_stage) (void)hipHostFree(w->h_stage);
        w->h_stage = nullptr; w->h_cap = 0;
        const size_t want = w->total + w->total / 4;
        if (hipHostMalloc((void**)&w->h_stage, want, hipHostMallocDefault) != hipSuccess) {
            if (err) *err = "hipHostMalloc failed for the JPEG staging buffer";
            return MELF_ERR_HIP;
        }
        w->h_cap = want;
    }
    const auto tp2 = std::chrono::steady_clock::now();
    uint8_t* base = w->h_stage;
    const bool tables_ready = parsed && !parsed->slow.empty();
    auto fill = [&](int i) {
        JpegImageDev& r = rec[i];
        uint16_t* qt = (uint16_t*)(base + w->off_qt) + (size_t)i * 256;
        HuffSlow* slow = (HuffSlow*)(base + w->off_slow) + (size_t)i * 4;
        if (host_status[i] != 0) return;
        const JpegHeader& h = hbase[hidx(i)];
        for (int t = 0; t < 4; ++t) {
            if (h.qt_set[t]) memcpy(qt + t * 64, h.qt[t], 128); else memset(qt + t * 64, 0, 128);
        }
        if (h.progressive || h.multiscan) memset(slow, 0, 4 * sizeof(HuffSlow));   // its tables go with its scans, below
        else if (tables_ready) memcpy(slow, parsed->slow.data() + (size_t)hidx(i) * 4, 4 * sizeof(HuffSlow));
        else build_slow4(h, slow);
        // the entropy-coded segment as it is: stuffing, fill bytes and restart markers are taken out on the GPU (k_jpeg_clean),
        // which also writes the clean length and the restart table (r.rst_cnt: the EXPECTED number of intervals until then)
        if (!direct) {
            // streaming (non-temporal) stores: the pinned buffer is written once and read by the DMA engine, never by this core
            // (a plain memcpy reads every destination line before it writes it: a third of the copy's memory traffic)
            uint8_t* dst = w->h_raw + r.raw_off;   // 64-byte aligned
            const uint8_t* src = data[i] + h.scan_begin;
            const size_t whole = (size_t)r.raw_len & ~(size_t)15;
            for (size_t o = 0; o < whole; o += 16) _mm_stream_si128((__m128i*)(dst + o), _mm_loadu_si128((const __m128i*)(src + o)));
            memcpy(dst + whole, src + whole, r.raw_len - whole);
            _mm_sfence();
        }
        r.scan_cap = (uint32_t)(h.restart_interval ? r.rst_off : scan_off[i + 1] - scan_off[i]);
        r.scan_off = (uint32_t)scan_off[i];
        r.scan_len = 0;
        if (h.restart_interval) r.rst_off = (uint32_t)(scan_off[i] + r.rst_off);
        r.ok = h.restart_interval != 0 ? 2 : 1;
        if (h.multiscan) {
            // The Huffman kernels pass this record by (ok = 4) and k_jpeg_clean only zeroes its 128 bytes of the scan area: the file's
            // scans have records of their own.  What the record keeps is what J2 and J3 need: geometry, quantisation, the planar mark
            // and the real block grids.
            const jpeg_scans::Comp y = jpeg_scans::component(h.W, h.H, h.hs[0], h.vs[0], 0), cc = jpeg_scans::component(h.W, h.H, h.hs[0], h.vs[0], 1);
            r.raw_len = 0; r.restart_interval = 0;
            r.rst_off = (uint32_t)y.rbx | (uint32_t)y.rby << 16;
            r.rst_cnt = (uint32_t)cc.rbx | (uint32_t)cc.rby << 16;
            r.scan_cap = (uint32_t)(scan_off[i + 1] - scan_off[i]);
            r.ok = 4;
            r.planar = 1;
            return;
        }
        if (h.progressive) {
            // The baseline kernels must pass this file by: ok = 3 is neither k_jpeg_huff's nor k_jpeg_huff_rst's, and with no raw
            // bytes in the record k_jpeg_clean only zeroes the file's 128 bytes of the scan area.  Where the bytes are says the
            // progressive record; the scans' records, tables and interval tables are copied as the parser left them.
            jpeg_prog::File& f = pfile[i];
            f.raw_off = r.raw_off; f.raw_len = r.raw_len;
            r.raw_len = 0; r.restart_interval = 0; r.rst_off = 0; r.rst_cnt = 0;
            r.scan_cap = (uint32_t)(scan_off[i + 1] - scan_off[i]);
            r.ok = 3;
            memcpy((jpeg_prog::Scan*)(base + w->off_pscan) + f.scan_first, h.pscans.data(), h.pscans.size() * sizeof(jpeg_prog::Scan));
            memcpy((jpeg_prog::Huff*)(base + w->off_ptab) + f.tab_first, h.ptabs.data(), h.ptabs.size() * sizeof(jpeg_prog::Huff));
            memcpy((uint32_t*)(base + w->off_prst) + f.rst_first, h.prst.data(), h.prst.size() * sizeof(uint32_t));
            return;
        }
        // longer than 1024 lanes x the segment length k_jpeg_huff can address (the raw length: the clean one is only known on
        // the GPU and at most 1/128 shorter)
        if (!h.restart_interval && (r.raw_len > JPEG_MAX_PAR_SCAN || (long_on && r.raw_len > long_from))) {
            // with melf_ctx_set_jpeg_long_scans: a record kind of its own (ok = 5: k_jpeg_chapters's), up to the longest scan
            // 32-bit bit positions address (melf_jpeg_long.h)
            if (long_on && jpeg_long::taken(r.raw_len)) r.ok = 5;
            else {
                r.ok = 0;
                host_status[i] = 1;  // valid, but for the host decoder
            }
        }
    };
    // nothing but two small copies per file left to do: not worth waking the pool (whose threads the file reads of the next
    // call are using)
    if (direct && tables_ready) { for (int i = 0; i < n; ++i) fill(i); }
    else par_for(fill);
    w->n_par = w->n_seq = w->n_420 = w->n_long = 0;
    w->max_par_scan = 0;
    w->runs.clear();
    for (int i = 0; i < n; ++i) {
        // a file that is not decoded (zeros over the window) belongs to the run it stands in
        const int code = rec[i].ok ? rec[i].orient : (w->runs.empty() ? 1 : w->runs.back().code);
        const bool prog = rec[i].ok ? rec[i].ok == 3 : (w->runs.empty() ? false : w->runs.back().prog);
        if (w->runs.empty() || w->runs.back().code != code || w->runs.back().prog != prog) {
            w->runs.push_back({i, 0, code, 0, 0, 0, 0, 0});
            w->runs.back().prog = prog;
        }
        JpegWorkspace::Run& run = w->runs.back();
        ++run.n;
        if (rec[i].ok == 3) {
            const jpeg_prog::File& f = pfile[i];
            const JpegHeader& h = hbase[hidx(i)];
            if (run.prog_coefs == 0) run.prog_coef0 = f.coef_first;
            run.prog_coefs = f.coef_first + jpeg_prog::area_blocks(f) - run.prog_coef0;   // files lie in the area in batch order
            run.prog_scans = std::max(run.prog_scans, (uint32_t)h.pscans.size());
            for (const jpeg_prog::Scan& t : h.pscans) {
                if (run.prog_items.size() <= t.level) run.prog_items.resize((size_t)t.level + 1, 0);
                run.prog_items[t.level] = std::max(run.prog_items[t.level], jpeg_prog::scan_intervals(f, t));
            }
        }
        if (rec[i].ok == 1) { ++w->n_par; ++run.n_par; w->max_par_scan = std::max(w->max_par_scan, (size_t)rec[i].raw_len); run.max_par_scan = std::max(run.max_par_scan, (size_t)rec[i].raw_len); }
        else if (rec[i].ok == 2) { ++w->n_seq; ++run.n_seq; }
        else if (rec[i].ok == 5) { ++w->n_long; ++run.n_long; }
        if (rec[i].ok && rec[i].ncomp == 3 && rec[i].hs0 == 2 && rec[i].vs0 == 2) { ++w->n_420; ++run.n_420; }
        int blocks = 0;
        for (int c = 0; c < rec[i].ncomp; ++c) blocks += (int)rec[i].blocks_x[c] * rec[i].blocks_y[c];
        run.max_blocks = std::max(run.max_blocks, blocks);   // (a record that was not laid out has no components)
    }
    for (int k = 0; k < extra; ++k) {   // a scan's two tables, as they were at its SOS, in the slots DC 0 and AC 0 of its record
        const JpegHeader::MScan& sc = hbase[hidx(ms_scans[k].file)].ms[ms_scans[k].comp];
        HuffSlow* slow = (HuffSlow*)(base + w->off_slow) + ((size_t)n + k) * 4;
        memset(slow, 0, 4 * sizeof(HuffSlow));
        build_huff(sc.dc, slow);
        build_huff(sc.ac, slow + 2);
    }
    for (size_t f = 0; f < ms_files.size(); ++f) {
        uint32_t* m = (uint32_t*)(base + w->off_msmap) + 4 * f;
        m[0] = (uint32_t)ms_files[f];
        for (int k = 0; k < extra; ++k)
            if (ms_scans[k].file == ms_files[f]) m[1 + ms_scans[k].comp] = (uint32_t)(n + k);
    }
    memcpy(base + w->off_imgs, rec.data(), nrec * sizeof(JpegImageDev));
    if (!pfile.empty()) memcpy(base + w->off_pfile, pfile.data(), (size_t)n * sizeof(jpeg_prog::File));
    if (trace) {
        const auto tp3 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[melf jpeg] prepare: parse %.2f ms, layout %.2f ms, tables + scan copies %.2f ms (%d threads)\n", ms(tp0, tp1), ms(tp1, tp2),
                ms(tp2, tp3), nthreads);
    }
    return MELF_SUCCESS;
}

// Device half, in two steps so that a caller can pipeline batches: jpeg_upload_batch grows the device buffers and copies
// the stage buffer (on `copy_stream`), jpeg_decode_batch_kernels runs J1..J3 (on `stream`) and leaves the per-file status
// in w->d_status.  `timer(k)` brackets kernel k (0..2) when profiling.
#define JTRY(expr)                                                               \
    do {                                                                         \
        hipError_t e_ = (expr);                                                  \
        if (e_ != hipSuccess) {                                                  \
            if (err) *err = std::string(#expr) + ": " + hipGetErrorString(e_);   \
            return MELF_ERR_HIP;                                                 \
        }                                                                        \
    } while (0)
int jpeg_upload_batch(JpegWorkspace* w, int n, hipStream_t copy_stream, std::string* err)
{
    JTRY(grow_dev(&w->d_stage, &w->d_cap, w->total + w->scan_bytes));
    JTRY(grow_dev(&w->d_raw, &w->d_raw_cap, w->raw_total));
    JTRY(grow_dev(&w->d_coefs, &w->coef_cap, w->coef_elems + 64));
    JTRY(grow_dev(&w->d_planes, &w->plane_cap, w->plane_bytes + 64));
    JTRY(grow_dev(&w->d_status, &w->status_cap, (size_t)n + w->n_scan_recs));
    if (w->cut) JTRY(grow_dev(&w->d_cut, &w->cut_cap, (size_t)n * 2 * sizeof(JpegCutRec)));
    JTRY(hipMemcpyAsync(w->d_stage, w->h_stage, w->total, hipMemcpyHostToDevice, copy_stream));
    JTRY(hipMemcpyAsync(w->d_raw, w->raw_src, w->raw_total, hipMemcpyHostToDevice, copy_stream));
    return MELF_SUCCESS;
}

int jpeg_decode_batch_kernels(JpegWorkspace* w, int n, int H, int W, uint8_t* d_frames, hipStream_t stream, std::string* err,
                              void (*timer)(void*, int, int), void* timer_arg, const int* rect)
{
    // Per run of one orientation code: the caller's rectangle, taken back to the stored frame, grown by one MCU (chroma filter
    // context) and aligned to 16, or the frame (melf_jpeg_orient_addr.h).  A kernel of a run gets the run's first file as its file 0.
    struct RunGeo { int Hs, Ws; JpegWindow win; };
    std::vector<RunGeo> geo;
    for (const JpegWorkspace::Run& r : w->runs) {
        const int Hs = jpeg_orient::swapped_h(r.code, H, W), Ws = jpeg_orient::swapped_w(r.code, H, W);
        const jpeg_orient::Window ow = jpeg_orient::window(rect, r.code, Hs, Ws);
        geo.push_back({Hs, Ws, {ow.x0, ow.y0, ow.x1, ow.y1}});
    }
    JTRY(hipMemsetAsync(w->d_status, 0, ((size_t)n + w->n_scan_recs) * sizeof(int32_t), stream));
    const JpegImageDev* const imgs0 = (const JpegImageDev*)(w->d_stage + w->off_imgs);
    const uint16_t* const qt0 = (const uint16_t*)(w->d_stage + w->off_qt);
    const HuffSlow* const slow0 = (const HuffSlow*)(w->d_stage + w->off_slow);
    const uint8_t* scan = w->d_stage + w->off_scan;
    const size_t nruns = w->runs.size();
    // files that end early: a state k_jpeg_huff does not write reads as zeros, the state at the stream's first bit
    JpegCutRec* const cut0 = w->cut && w->n_par + w->n_seq > 0 ? (JpegCutRec*)w->d_cut : nullptr;
    if (cut0 && w->n_par > 0) JTRY(hipMemsetAsync(cut0, 0, (size_t)n * 2 * sizeof(JpegCutRec), stream));
    if (timer) timer(timer_arg, 0, 0);
    if (w->n_par + w->n_seq + w->n_long + w->n_scan_recs > 0)   // J0: stuffing, fill bytes and restart markers out of the uploaded segments
        hipLaunchKernelGGL(k_jpeg_clean, dim3(n + w->n_scan_recs), dim3(CLEAN_T), 0, stream, (JpegImageDev*)(w->d_stage + w->off_imgs), w->d_raw, w->d_stage + w->off_scan);
    for (size_t q = 0; q < nruns; ++q) {
        const JpegWorkspace::Run& r = w->runs[q];
        const JpegWindow win = geo[q].win;
        const JpegImageDev* imgs = imgs0 + r.first;
        const HuffSlow* slow = slow0 + (size_t)r.first * 4;
        int32_t* status = w->d_status + r.first;
        JpegCutRec* const cutrec = cut0 ? cut0 + 2 * (size_t)r.first : nullptr;
        if (r.n_par > 0) {  // one workgroup per image, one lane per stream segment
            // 512 lanes per image; a batch with a scan too long for 512 segments of the length the kernel can address takes 1024
            if (r.max_par_scan > JPEG_MAX_PAR_SCAN / 2)
                hipLaunchKernelGGL(k_jpeg_huff<1024>, dim3(r.n), dim3(1024), 0, stream, imgs, slow, scan, w->d_coefs, status, win, cutrec);
            else
                hipLaunchKernelGGL(k_jpeg_huff<512>, dim3(r.n), dim3(512), 0, stream, imgs, slow, scan, w->d_coefs, status, win, cutrec);
        }
        if (r.n_seq > 0) {  // streams with restart intervals: one lane per interval
            hipLaunchKernelGGL(k_jpeg_huff_rst<256>, dim3(r.n), dim3(256), 0, stream, imgs, slow, scan, w->d_coefs, status, win, cutrec ? 1 : 0);
        }
        if (r.n_long > 0)   // scans beyond k_jpeg_huff's reach, chapter by chapter (only runs that hold one)
            hipLaunchKernelGGL(k_jpeg_chapters<1024>, dim3(r.n), dim3(1024), 0, stream, imgs, slow, scan, w->d_coefs, status, win, w->long_dw);
        if (cutrec && r.n_par + r.n_seq > 0)   // one wave per file; a file that is not cut leaves at once
            hipLaunchKernelGGL(k_jpeg_cut_tail, dim3(r.n), dim3(64), 0, stream, imgs, slow, scan, w->d_coefs, status, cutrec, win);
        if (r.prog && !r.prog_items.empty()) {
            // Progressive files: the WHOLE coefficient area zeroed (a refinement scan reads one bit for every coefficient that is
            // non-zero, in every block of the image: where the stream goes depends on blocks outside the window too), then level
            // after level of scans.  IDCT and colour run on the window, as for every file.
            JTRY(hipMemsetAsync(w->d_coefs + r.prog_coef0 * 64, 0, r.prog_coefs * 64 * sizeof(int16_t), stream));
            const jpeg_prog::File* pf = (const jpeg_prog::File*)(w->d_stage + w->off_pfile) + r.first;
            for (size_t sidx = 0; sidx < r.prog_items.size(); ++sidx)
                hipLaunchKernelGGL(k_jpeg_prog_scan, dim3(r.prog_items[sidx], r.n, r.prog_scans), dim3(64), 0, stream, pf,
                                   (const jpeg_prog::Scan*)(w->d_stage + w->off_pscan), (const jpeg_prog::Huff*)(w->d_stage + w->off_ptab),
                                   (const uint32_t*)(w->d_stage + w->off_prst), w->d_raw, w->d_coefs, status, (int)sidx);
        }
    }
    // The scans of multi-scan files, group by group: a group's records share the window its component class has in its files
    // (melf_jpeg_scans.h), the way a run's files share theirs.  Then every such file's status from its scans'.
    for (const JpegWorkspace::ScanGroup& g : w->scan_groups) {
        const int Hs = jpeg_orient::swapped_h(g.code, H, W), Ws = jpeg_orient::swapped_w(g.code, H, W);
        const jpeg_orient::Window ow = jpeg_orient::window(rect, g.code, Hs, Ws);
        const jpeg_scans::Window sw = jpeg_scans::scan_window({ow.x0, ow.y0, ow.x1, ow.y1}, Ws, Hs, g.hs0, g.vs0, g.chroma);
        const JpegWindow win = {sw.x0, sw.y0, sw.x1, sw.y1};
        const JpegImageDev* imgs = imgs0 + n + g.first;
        const HuffSlow* slow = slow0 + ((size_t)n + g.first) * 4;
        int32_t* status = w->d_status + n + g.first;
        if (g.n_par > 0) {
            if (g.max_par_scan > JPEG_MAX_PAR_SCAN / 2)
                hipLaunchKernelGGL(k_jpeg_huff<1024>, dim3(g.n), dim3(1024), 0, stream, imgs, slow, scan, w->d_coefs, status, win, (JpegCutRec*)nullptr);
            else
                hipLaunchKernelGGL(k_jpeg_huff<512>, dim3(g.n), dim3(512), 0, stream, imgs, slow, scan, w->d_coefs, status, win, (JpegCutRec*)nullptr);
        }
        if (g.n_seq > 0)   // (a multi-scan file that ends inside a scan stays corrupt: no states, no tail)
            hipLaunchKernelGGL(k_jpeg_huff_rst<256>, dim3(g.n), dim3(256), 0, stream, imgs, slow, scan, w->d_coefs, status, win, 0);
    }
    if (w->ms_files > 0)
        hipLaunchKernelGGL(k_jpeg_scan_status, dim3((w->ms_files + 63) / 64), dim3(64), 0, stream, (const uint32_t*)(w->d_stage + w->off_msmap),
                           w->ms_files, w->d_status);
    if (timer) timer(timer_arg, 0, 1);
    JTRY(hipGetLastError());
    if (w->max_blocks > 0) {
        if (timer) timer(timer_arg, 1, 0);
        for (size_t q = 0; q < nruns; ++q) {
            const JpegWorkspace::Run& r = w->runs[q];
            if (r.max_blocks <= 0) continue;
            const JpegWindow win = geo[q].win;
            const int win_w = win.x1 - win.x0, win_h = win.y1 - win.y0;
            // at most (window / 8)^2 luma blocks + two chroma planes of up to the same count (4:4:4).  A 32-wide MCU (4:1:1) can add
            // up to 16 columns on EACH side of the 16-aligned window: w0 <= win_w / 8 + 6 luma blocks a row against the
            // win_w / 8 + 3 allowed for here, but its two chroma planes are a quarter of the luma each, 1.5 w0 h0 blocks in all, and
            // 1.5 (win_w / 8 + 6) <= 3 (win_w / 8 + 3); h0 = ceil(win_h / 8) as ever.  4:4:0 has MCUs of 8 x 16: nothing new.
            const int wblocks = 3 * ((win_w + 15) / 8 + 2) * ((win_h + 15) / 8 + 2);
            const int nblk = std::min(r.max_blocks, wblocks);
            hipLaunchKernelGGL(k_jpeg_idct, dim3((nblk + 255) / 256, r.n), dim3(256), 0, stream, imgs0 + r.first, qt0 + (size_t)r.first * 256, w->d_coefs,
                               w->d_status + r.first, w->d_planes, win);
        }
        if (timer) timer(timer_arg, 1, 1);
        JTRY(hipGetLastError());
    }
    if (timer) timer(timer_arg, 2, 0);
    for (size_t q = 0; q < nruns; ++q) {
        const JpegWorkspace::Run& r = w->runs[q];
        const JpegWindow win = geo[q].win;
        const int win_w = win.x1 - win.x0, win_h = win.y1 - win.y0;
        const JpegImageDev* imgs = imgs0 + r.first;
        const int32_t* status = w->d_status + r.first;
        uint8_t* frames = d_frames + (size_t)r.first * H * W * 3;
        if (r.code != 1) {   // every sampling through the one oriented kernel
            const int tiles = ((win_w + OT - 1) / OT) * ((win_h + OT - 1) / OT);
            hipLaunchKernelGGL(k_jpeg_color_exif, dim3(tiles, r.n), dim3(256), 0, stream, imgs, status, w->d_planes, geo[q].Hs, geo[q].Ws, r.code,
                               frames, win);
            continue;
        }
        const int fast420 = (W % 8 == 0 && r.n_420 > 0) ? 1 : 0;
        if (fast420) {
            const int items = ((win_w + 7) / 8) * ((win_h + 1) / 2);   // 8 pixels x 2 rows each
            hipLaunchKernelGGL(k_jpeg_color420, dim3((items + 255) / 256, r.n), dim3(256), 0, stream, imgs, status, w->d_planes, H, W, frames, win);
        }
        if (!fast420 || r.n_420 < r.n)
            hipLaunchKernelGGL(k_jpeg_color, dim3((win_w + 1023) / 1024, win_h, r.n), dim3(256), 0, stream, imgs, status, w->d_planes, H, W, frames, fast420, win);
    }
    if (timer) timer(timer_arg, 2, 1);
    JTRY(hipGetLastError());
    return MELF_SUCCESS;
}

const int32_t* jpeg_device_status(const JpegWorkspace* w) { return w->d_status; }

// One batch start to end on one stream (upload, J1..J3, status back, synchronised when status_out_host is given).
int jpeg_launch_batch(JpegWorkspace* w, int n, int H, int W, uint8_t* d_frames, int32_t* status_out_host,
                      hipStream_t stream, std::string* err, void (*timer)(void*, int, int), void* timer_arg, const int* rect)
{
    if (int rc = jpeg_upload_batch(w, n, stream, err)) return rc;
    if (int rc = jpeg_decode_batch_kernels(w, n, H, W, d_frames, stream, err, timer, timer_arg, rect)) return rc;
    if (status_out_host) {
        JTRY(hipMemcpyAsync(status_out_host, w->d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        JTRY(hipStreamSynchronize(stream));
    }
    return MELF_SUCCESS;
}
#undef JTRY

}  // namespace melf
