// Stand-alone program (its own main; compiled alone against melf_jpeg_long.h, plain and under the host sanitizers): sweeps the chapter
// plan of long baseline scans (melf_ctx_set_jpeg_long_scans) over scan lengths from 1 byte to the largest length that is taken and just
// beyond -- densely around every power of two and around every multiple of the production chapter, coarsely in between -- and over
// chapter lengths from 1 byte up.  It asserts, per scan length and chapter length:
//   * S is a multiple of 32 bits with an odd dword count, at least 9 dwords, and S <= 32 000; the chapter length in force is what was
//     asked for rounded up (or the production length where more was asked for);
//   * the chapters tile [0, bits) exactly, without gap or overlap, each with 1..T segments that tile it in turn, and only the last
//     chapter is short;
//   * no position the kernel computes in 32 bits wraps: every chapter's first bit, every segment's nominal end and its clamped end,
//     the decoders' stop bits + 32 and the furthest bit a symbol can reach, bits + 63, against the same sums in 64 bits;
//   * the length just beyond the bound is refused, and the bound is the one the derivation gives.
// Prints "ok <cases>" and returns 0, or the first violation and 1.
#include "melf_jpeg_long.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

using namespace melf;

static long g_cases = 0;

static int fail(const char* what, uint64_t n, uint64_t want, uint32_t d, uint32_t c)
{
    fprintf(stderr, "%s: scan of %llu bytes, chapters of %llu bytes wanted, %u dwords a segment, chapter %u\n", what, (unsigned long long)n,
            (unsigned long long)want, d, c);
    return 1;
}

// every chapter, or -- for scans of very many chapters -- the first and last few and a stride through the middle
static int check(const uint64_t n, const uint64_t want)
{
    ++g_cases;
    const uint32_t d = jpeg_long::seg_dwords(want);
    if (d < jpeg_long::MIN_SEG_DWORDS || d > jpeg_long::MAX_SEG_DWORDS || !(d & 1u) || 32u * d > jpeg_long::MAX_SEG_BITS) return fail("segment length", n, want, d, 0);
    const uint64_t cbytes = jpeg_long::chapter_bytes(d);
    if (cbytes != (uint64_t)jpeg_long::T * 4u * d) return fail("chapter length", n, want, d, 0);
    if (cbytes < want && d != jpeg_long::MAX_SEG_DWORDS) return fail("chapter shorter than asked for", n, want, d, 0);
    if (d > jpeg_long::MIN_SEG_DWORDS && (uint64_t)jpeg_long::T * 4u * (d - 2u) >= want) return fail("chapter rounded up further than the rule does", n, want, d, 0);
    if (!jpeg_long::taken(n)) return fail("a length below the bound refused", n, want, d, 0);
    const uint64_t bits64 = n * 8u, S = 32u * (uint64_t)d, cb = (uint64_t)jpeg_long::T * S;
    if (bits64 + 63u >= (1ull << 32)) return fail("bits + 63 wraps", n, want, d, 0);
    const uint32_t bits = (uint32_t)bits64;
    const uint32_t nchap = jpeg_long::chapters(bits, d);
    if ((uint64_t)nchap != (bits64 + cb - 1u) / cb) return fail("chapter count", n, want, d, 0);
    const uint32_t dense = 4;
    const uint32_t stride = nchap > 64u ? nchap / 29u : 1u;
    // (chapter c begins at c full chapters and ends at the next one's beginning or at the stream's end: that is the tiling; of a scan
    // of very many chapters the first and last few and a stride through the middle are looked at)
    uint64_t last_end = 0;
    for (uint32_t c = 0; c < nchap; c += (c < dense || c + dense + stride >= nchap) ? 1u : stride) {
        const jpeg_long::Chapter k = jpeg_long::chapter(bits, d, c);
        if ((uint64_t)k.bit0 != (uint64_t)c * cb || k.bit0 >= bits) return fail("a chapter does not begin where the one before ended", n, want, d, c);
        const uint64_t end64 = (uint64_t)c * cb + cb < bits64 ? (uint64_t)c * cb + cb : bits64;
        if ((uint64_t)k.bit1 != end64 || k.bit1 <= k.bit0) return fail("chapter end", n, want, d, c);
        if (c + 1u < nchap && (uint64_t)k.bit1 - k.bit0 != cb) return fail("a short chapter that is not the last", n, want, d, c);
        if (k.nseg < 1u || k.nseg > jpeg_long::T || (uint64_t)k.nseg != (end64 - k.bit0 + S - 1u) / S) return fail("segments of a chapter", n, want, d, c);
        // the segments: lane i's nominal end and clamped end for EVERY lane of the workgroup (lanes behind nseg compute theirs too)
        const uint32_t T = jpeg_long::T, q = k.nseg / 5u;
        const uint32_t lanes[] = {0u, 1u, 2u, q, 2u * q, 3u * q, 4u * q, k.nseg - 1u, k.nseg, k.nseg + 1u, T - 2u, T - 1u};
        for (const uint32_t i : lanes) {
            if (i >= T) continue;
            const uint64_t nominal = (uint64_t)k.bit0 + (uint64_t)(i + 1u) * S;
            if (nominal >= (1ull << 32)) return fail("a segment's nominal end wraps", n, want, d, c);
            const uint64_t e64 = nominal < bits64 + 32u ? nominal : bits64 + 32u;
            if ((uint64_t)jpeg_long::seg_end(bits, d, k.bit0, i) != e64) return fail("segment end", n, want, d, c);
            if (i + 1u == k.nseg && e64 < end64) return fail("the chapter's last segment ends before the chapter does", n, want, d, c);
            if (i + 1u < k.nseg && e64 != nominal) return fail("a segment inside a chapter is clamped", n, want, d, c);
        }
        if ((uint64_t)k.bit0 + (uint64_t)jpeg_long::T * S >= (1ull << 32)) return fail("the last lane's nominal end wraps", n, want, d, c);
        last_end = end64;
    }
    if (last_end != bits64) return fail("the chapters do not end at the stream's end", n, want, d, nchap - 1u);
    return 0;
}

int main()
{
    static_assert(jpeg_long::PRODUCTION_CHAPTER_BYTES == 4091904u, "production chapter");
    if (jpeg_long::MAX_SCAN_BYTES * 8u + (uint64_t)jpeg_long::T * jpeg_long::MAX_SEG_BITS + 64u > (1ull << 32) ||
        (jpeg_long::MAX_SCAN_BYTES + 1u) * 8u + (uint64_t)jpeg_long::T * jpeg_long::MAX_SEG_BITS + 64u <= (1ull << 32)) {
        fprintf(stderr, "MAX_SCAN_BYTES is not the largest length of the derivation\n");
        return 1;
    }
    if (jpeg_long::taken(jpeg_long::MAX_SCAN_BYTES + 1u) || jpeg_long::taken(1ull << 32) || jpeg_long::taken((1ull << 32) + 5u) || !jpeg_long::taken(jpeg_long::MAX_SCAN_BYTES)) {
        fprintf(stderr, "the length just beyond the bound is not refused\n");
        return 1;
    }
    // scan lengths
    std::set<uint64_t> lens;
    const uint64_t top = jpeg_long::MAX_SCAN_BYTES;
    for (uint64_t n = 1; n <= 300; ++n) lens.insert(n);
    for (int p = 1; p < 32; ++p)
        for (int64_t k = -6; k <= 6; ++k) {
            const int64_t n = (int64_t)(1ull << p) + k, nb = (int64_t)((1ull << p) / 8u) + k;   // powers of two in bytes and in bits
            if (n >= 1 && (uint64_t)n <= top) lens.insert((uint64_t)n);
            if (nb >= 1 && (uint64_t)nb <= top) lens.insert((uint64_t)nb);
        }
    for (uint64_t m = jpeg_long::PRODUCTION_CHAPTER_BYTES; m <= top + jpeg_long::PRODUCTION_CHAPTER_BYTES; m += jpeg_long::PRODUCTION_CHAPTER_BYTES)
        for (int64_t k = -5; k <= 5; ++k)
            if ((int64_t)m + k >= 1 && m + k <= top) lens.insert(m + k);
    for (uint64_t n = 1000; n <= top; n += n / 7u + 13u) lens.insert(n);
    for (int64_t k = 0; k <= 40; ++k) lens.insert(top - (uint64_t)k);
    // chapter lengths wanted: 1 byte up, every rounding step's neighbourhood, the production length and beyond
    std::vector<uint64_t> wants;
    for (uint64_t w = 1; w <= 64; ++w) wants.push_back(w);
    for (uint32_t d = 7; d <= jpeg_long::MAX_SEG_DWORDS + 4u; d += (d < 40u || d + 12u > jpeg_long::MAX_SEG_DWORDS) ? 1u : 37u)
        for (int64_t k = -2; k <= 2; ++k) wants.push_back((uint64_t)((int64_t)(4096u * (uint64_t)d) + k));
    wants.push_back(1ull << 31);
    wants.push_back((1ull << 31) - 1u);
    for (const uint64_t n : lens)
        for (const uint64_t w : wants)
            if (check(n, w)) return 1;
    printf("ok %ld\n", g_cases);
    return 0;
}
