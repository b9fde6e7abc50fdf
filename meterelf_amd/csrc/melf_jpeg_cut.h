// Baseline JPEG files that end early (melf_ctx_set_jpeg_truncated): the walk that finishes the cut MCU, compiled by both sides --
// k_jpeg_cut_tail (k_jpeg.hip) on the GPU and tests/jpeg_cut_main.cpp on the host.
//
// The rule (what libjpeg's data source makes of the end of the bytes: a fake EOI, zero bits from there on).  Let the STREAM be the
// entropy-coded bytes as k_jpeg_clean leaves them, followed by an endless run of zero bits, decoded MCU by MCU as ever.
//   the cut MCU   the MCU during whose decode a bit behind the real bytes is first required, by a Huffman code or by the value
//                 bits behind it.  It is decoded completely, from the zero bits, and it is the last MCU decoded.
//   behind it     every block of every later MCU is all zero, DC included: no predictor is applied.
//   a stream that ends exactly on an MCU boundary with MCUs still owing makes the NEXT MCU the cut MCU, decoded entirely from zeros.
// With restart intervals: the last interval found may be short (or empty); if it is complete and intervals are still owing, the first
// MCU of the next interval, predictors reset, is the cut MCU.
//
// finish() walks on from an exact decoder state at a symbol boundary not behind `bits` (the real bits of the stream), symbol by
// symbol, and hands every coefficient it decodes to a sink, until the cut MCU is complete.  It never reads a byte at or behind
// ceil(bits / 8): the zeros behind the stream are PRODUCED by window(), by masking, because finishing an MCU on zero bits can take
// far more than the 128 bytes of zero padding the scan area has (6 blocks x 63 symbols of code plus value bits).
//
// A run of zeros that overshoots the block (position above 63) stores its value at natural index 63, as libjpeg does (its
// zig-zag table has sixteen spare entries of 63); a valid stream never gets there, a zero-filled one can with tables whose
// all-zero AC code carries a run.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MELF_CUT_HD __host__ __device__ __forceinline__
#else
#define MELF_CUT_HD inline
#endif

namespace melf {
namespace jpeg_cut {

struct Huff {   // restates HuffSlow (melf_jpeg_parse.h): canonical decode data for code lengths 1..16
    uint32_t limit[16];
    int32_t valoff[16];
    uint8_t huffval[256];
};

struct Layout {   // the MCU: bpm <= 6 blocks; per block b its component (2 bits at 2 b) and its DC / AC table id (bit b)
    int bpm;
    uint32_t comp_bits, dc_bits, ac_bits;
};

struct State {
    uint32_t p;     // bit position of the next symbol
    int blk, k;     // block within the MCU, coefficient index (0: the DC symbol comes next)
    int32_t nb;     // index of the block in decode order
    int pred0, pred1, pred2;   // DC predictors of the three components (scalars: nothing here is indexed at run time)
};

constexpr int INVALID_CODE = -1, NOT_CUT = 0, CUT = 1;

// The 32 bits at bit position p of the stream: the real bits below `bits`, zeros from there on.  Bytes at or behind
// ceil(bits / 8) are not read.
MELF_CUT_HD uint32_t window(const uint8_t* s, const uint32_t bits, const uint32_t p)
{
    if (p >= bits) return 0u;
    const uint32_t nbytes = (bits + 7u) >> 3, b0 = p >> 3;
    uint64_t v = 0;
    for (uint32_t i = 0; i < 5u; ++i) v = (v << 8) | (b0 + i < nbytes ? (uint64_t)s[b0 + i] : 0ull);
    uint32_t w = (uint32_t)(v >> (8u - (p & 7u)));
    const uint32_t keep = bits - p;
    if (keep < 32u) w &= ~0u << (32u - keep);
    return w;
}

// Walks from st until the cut MCU is complete or block `limit` (the frame's or the restart interval's end) is reached.
// tabs: DC 0, DC 1, AC 0, AC 1; nat: zig-zag position -> natural index (64 entries).  sink(nb, natural index, value) receives
// every coefficient decoded, the DC ones with their predictor added.  Returns CUT (st.nb: the first block behind the cut MCU),
// NOT_CUT (the limit was reached on real bits alone) or INVALID_CODE (a code no table has).
template <class Sink>
MELF_CUT_HD int finish(const uint8_t* s, const uint32_t bits, const Huff* tabs, const uint8_t* nat, const Layout& L, State& st,
                       const int32_t limit, Sink&& sink)
{
    bool cut = false;
    while (st.nb < limit) {
        if (cut && st.blk == 0 && st.k == 0) break;
        const bool dc = st.k == 0;
        const Huff& T = tabs[dc ? (L.dc_bits >> st.blk) & 1u : 2u + ((L.ac_bits >> st.blk) & 1u)];
        const uint32_t w = window(s, bits, st.p);
        int len = 1;
        for (int l = 1; l <= 16; ++l) len += (w >> (32 - l)) >= T.limit[l - 1] ? 1 : 0;
        if (len > 16) return INVALID_CODE;
        const int sym = T.huffval[(T.valoff[len - 1] + (int32_t)(w >> (32 - len))) & 255];
        const int sbits = sym & 15, run = sym >> 4;
        const int raw = sbits ? (int)((w << len) >> (32 - sbits)) : 0;
        const int v = sbits && 2 * raw < (1 << sbits) ? raw - (1 << sbits) + 1 : raw;   // EXTEND (T.81 F.2.2.1)
        if (st.p + (uint32_t)(len + sbits) > bits) cut = true;
        st.p += (uint32_t)(len + sbits);
        if (dc) {
            const uint32_t c = (L.comp_bits >> (2 * st.blk)) & 3u;
            st.pred0 += c == 0u ? v : 0;
            st.pred1 += c == 1u ? v : 0;
            st.pred2 += c == 2u ? v : 0;
            sink(st.nb, 0, (int)(int16_t)(c == 0u ? st.pred0 : c == 1u ? st.pred1 : st.pred2));
            st.k = 1;
        } else if (sbits) {
            const int pos = st.k + run;
            sink(st.nb, (int)nat[pos < 63 ? pos : 63], v);
            st.k = pos + 1;
        } else {
            st.k = run == 15 ? st.k + 16 : 64;
        }
        if (st.k >= 64) {
            st.k = 0;
            ++st.nb;
            if (++st.blk == L.bpm) st.blk = 0;
        }
    }
    return cut ? CUT : NOT_CUT;
}

}  // namespace jpeg_cut
}  // namespace melf
