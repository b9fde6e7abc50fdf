// Progressive JPEG (SOF2, ITU-T T.81 Annex G): the scan decoder's body.  Host and device code share it: k_jpeg.hip's
// k_jpeg_prog_scan runs decode_interval on the GPU, its header parser uses walk_scan, and tests/jpeg_prog_main.cpp compiles the
// header alone (no HIP headers are needed) and runs the same functions on the CPU, plain and under the host sanitizers.
//
// A progressive file sends its coefficient blocks in several scans; every scan adds to the blocks the scans before it left:
//   DC first       Ss = 0, Ah = 0   the DC difference, as in a baseline scan, stored shifted left by Al
//   DC refinement  Ss = 0, Ah > 0   one bit per block: bit Al of the DC coefficient
//   AC first       Ss > 0, Ah = 0   run/size symbols for the band Ss..Se, values shifted left by Al; a symbol with size 0 and run
//                                   r < 15 is EOBr: this block's band ends here and so do the bands of the next
//                                   2^r + (r extra bits) - 1 blocks (runs of up to 32767 blocks); run 15 is ZRL, sixteen zeros
//   AC refinement  Ss > 0, Ah > 0   the same symbols, but a run counts only coefficients that are still ZERO: every coefficient
//                                   the scans before left non-zero ("history") is passed over and costs one correction bit (bit
//                                   Al of its magnitude) where it is passed; a new coefficient is +-(1 << Al), its sign bit comes
//                                   right behind the symbol, IN FRONT of the correction bits of the coefficients its run passes;
//                                   ZRL passes sixteen zero-history positions; under an EOB run the rest of the band only takes
//                                   the correction bits of its non-zero coefficients
//
// Where a scan's blocks are.  Two facts decide this:
//   1. An INTERLEAVED scan (more than one component; here only DC scans can be) visits the MCU-padded grid: mcus_x * mcus_y MCUs
//      in raster order, in each MCU the scan's components in order, of a component its vs x hs blocks row by row.
//   2. A NON-INTERLEAVED scan (one component, AC or DC) visits only the component's REAL blocks:
//      ceil(ceil(W * hs_c / hs_max) / 8) by ceil(ceil(H * vs_c / vs_max) / 8) of them, in raster order.  That grid is narrower and
//      shorter than the padded one whenever the size is not a whole number of MCUs, and restart intervals count in that order.
//      (The padded blocks such a scan never visits keep what the DC scans gave them and zeros elsewhere, as in libjpeg.)
// The blocks are stored in the baseline decoder's order (k_jpeg.hip: CoefBlocks): block `inb` of MCU `mcu` at
// (coef_blk[0] + mcu * bpm + inb) * 64 coefficients, an MCU's blocks being luma row by row, then Cb, then Cr.
//
// Every loop is bounded by construction: the byte position only moves forward and the scan's length ends it (behind the data the
// reader hands out zero bits and counts them: an interval that used any is corrupt); a block loop ends at the band's end; the
// block counter ends at the interval's block count; an EOB run longer than the blocks left is corrupt; every block index is
// checked against the file's coefficient area before anything is stored.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
// (inlined into the kernel: the compiler then knows which pointers are LDS, and the decoder needs no call frame in scratch)
#define MELF_JP_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define MELF_JP_FN inline
#endif

namespace melf {
namespace jpeg_prog {

constexpr int NO_TABLE = 255;

// Canonical Huffman decode data (T.81 F.2.2.3), the layout of melf_jpeg_parse.h's HuffSlow: limit[l - 1] is the code counter after the
// codes of length l (one past the largest l-bit code), valoff[l - 1] the value index of the first l-bit code minus that code.
struct Huff {
    uint32_t limit[16];
    int32_t valoff[16];
    uint8_t huffval[256];
};

struct Scan {                  // one scan of one file
    uint32_t off, len;         // its entropy-coded bytes as they are in the file (stuffing, fill bytes, RSTn), from the file's first scan
    uint32_t rst_first;        // first entry of the scan in the file's table of restart intervals: entry k = where interval k begins,
                               // relative to `off` (entry 0 = 0; behind an RSTn marker otherwise)
    uint32_t rst_count;        // intervals found in the bytes (counted up to one more than the scan should have)
    uint16_t restart_interval; // MCUs of THIS scan per interval (0: none) -- single blocks in a non-interleaved scan
    uint8_t ns, Ss, Se, Ah, Al;
    uint8_t ac_tab;            // the scan's tables: indices into the file's table list, NO_TABLE where the scan needs none
    uint8_t comp[3], dc_tab[3];
    uint8_t level;             // scans of one level touch no common coefficient and run side by side: 1 + the highest level among the
                               // earlier scans that share a component and a coefficient with this one (0: none does)
    uint8_t pad;
};
static_assert(sizeof(Scan) == 32, "scan records are uploaded as they are");

struct File {                  // one progressive file of a batch (scan_count = 0: not a progressive file)
    uint32_t raw_off, raw_len; // the file's bytes from its first scan on, in the raw area
    uint32_t scan_first, scan_count;
    uint32_t tab_first, rst_first;
    uint32_t coef_first;       // first coefficient block of the file; mcus_x * mcus_y * bpm blocks follow
    uint16_t mcus_x, mcus_y;
    uint16_t rbx0, rby0;       // REAL block grid of component 0
    uint16_t rbxc, rbyc;       // ... of the chroma components (both 1x1)
    uint8_t ncomp, hs0, vs0, pad;
};
static_assert(sizeof(File) == 44, "file records are uploaded as they are");

MELF_JP_FN int blocks_per_mcu(const File& f) { return f.ncomp == 1 ? 1 : f.hs0 * f.vs0 + 2; }
MELF_JP_FN uint32_t area_blocks(const File& f) { return (uint32_t)f.mcus_x * f.mcus_y * (uint32_t)blocks_per_mcu(f); }

// MCUs of a scan (the units restart intervals count) and blocks per such MCU
MELF_JP_FN uint32_t scan_units(const File& f, const Scan& s)
{
    if (s.ns > 1) return (uint32_t)f.mcus_x * f.mcus_y;
    return s.comp[0] == 0 ? (uint32_t)f.rbx0 * f.rby0 : (uint32_t)f.rbxc * f.rbyc;
}
MELF_JP_FN int unit_blocks(const File& f, const Scan& s)
{
    if (s.ns <= 1) return 1;
    int nb = 0;
    for (int k = 0; k < 3; ++k)
        if (k < s.ns) nb += s.comp[k] == 0 ? f.hs0 * f.vs0 : 1;
    return nb;
}
MELF_JP_FN uint32_t scan_intervals(const File& f, const Scan& s)
{
    const uint32_t u = scan_units(f, s);
    return s.restart_interval ? (u + s.restart_interval - 1u) / s.restart_interval : 1u;
}

// Block j of the scan's MCU `unit`: its place in the file's coefficient area (in blocks), and which of the scan's components (ci)
MELF_JP_FN uint32_t block_place(const File& f, const Scan& s, const uint32_t unit, int j, int* ci)
{
    const int yb = f.ncomp == 1 ? 1 : f.hs0 * f.vs0, bpm = blocks_per_mcu(f);
    if (s.ns > 1) {   // fact 1: the padded grid, MCU by MCU
        for (int k = 0; k < s.ns && k < 3; ++k) {
            const int c = s.comp[k];
            const int nb = c == 0 ? yb : 1;
            if (j < nb) {
                *ci = k;
                return unit * (uint32_t)bpm + (uint32_t)(c == 0 ? j : yb + c - 1);
            }
            j -= nb;
        }
        *ci = 0;
        return 0xFFFFFFFFu;   // no such block: outside every area
    }
    // fact 2: the component's real blocks in raster order
    const int c = s.comp[0];
    *ci = 0;
    const uint32_t bw = c == 0 ? f.rbx0 : f.rbxc;
    const uint32_t by = unit / (bw ? bw : 1u), bx = unit - by * bw;
    const uint32_t fx = c == 0 ? f.hs0 : 1u, fy = c == 0 ? f.vs0 : 1u;
    const uint32_t mcu = (by / fy) * f.mcus_x + bx / fx;
    const uint32_t inb = c == 0 ? (by % fy) * f.hs0 + bx % fx : (uint32_t)(yb + c - 1);
    return mcu * (uint32_t)bpm + inb;
}

// ---- the bit reader: raw bytes in, FF 00 -> FF, fill FFs dropped, stop at a marker (or a lone FF at the end) ----
// The GPU build reads the stream and the blocks of an AC refinement in another way than the plain host build (below: 16-byte
// lines, a staged copy of the block).  MELF_JP_HOST_STAGED makes a host build take those same paths, so that the test program can
// run them under the sanitizers on buffers laid out as jpeg_prepare_batch lays them out.
#if defined(__HIP_DEVICE_COMPILE__)
#define MELF_JP_STAGED 1
#define MELF_JP_UNROLL _Pragma("unroll")
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // a plain vector: the compiler keeps it in registers
MELF_JP_FN u32x4 load16(const void* p) { return *(const u32x4*)p; }
MELF_JP_FN void store16(void* p, const u32x4 v) { *(u32x4*)p = v; }
#elif defined(MELF_JP_HOST_STAGED)
#define MELF_JP_STAGED 1
#define MELF_JP_UNROLL
struct u32x4 { uint32_t x, y, z, w; };
inline u32x4 load16(const void* p) { u32x4 v; memcpy(&v, p, 16); return v; }
inline void store16(void* p, const u32x4 v) { memcpy(p, &v, 16); }
#else
#define MELF_JP_STAGED 0
#endif
struct Bits {
    const uint8_t* d;
    uint32_t pos, end;
    uint64_t buf;   // the next bits, from bit 63 down
    int n;          // how many of them
    int pad;        // zero bits handed out behind the data
    bool stop;
#if MELF_JP_STAGED
    // On the GPU one lane reads the stream, and a byte load from memory costs that lane a microsecond: the bytes come through two
    // 16-byte lines held in registers, the line behind the current one requested when the current one is entered.
    u32x4 c0, c1;
    uintptr_t line;   // address of c0's line (0: none yet)
#endif
};
#if MELF_JP_STAGED
// Reads whole aligned 16-byte lines around d[at], at < end: up to 15 bytes in front of d and 31 behind d[end - 1].  The raw area
// is allocated 256-byte aligned; a file's bytes (from its first scan on) begin 64-byte aligned with at least 32 spare bytes behind
// them (jpeg_prepare_batch: align_up(raw_len + 32, 64)), or lie in one uploaded span with 64 spare bytes behind it, so every line
// lies inside the area.  tests/jpeg_prog_main.cpp runs this on a buffer of exactly that shape under the address sanitizer.
MELF_JP_FN uint32_t stream_byte(Bits& b, const uint32_t at)
{
    const uintptr_t a = (uintptr_t)(b.d + at), line = a & ~(uintptr_t)15;
    if (line != b.line) {
        b.c0 = line == b.line + 16 ? b.c1 : load16((const void*)line);
        b.c1 = load16((const void*)(line + 16));
        b.line = line;
    }
    const uint32_t i = (uint32_t)(a & 15u), q = i >> 2;
    const uint32_t w = q == 0 ? b.c0.x : q == 1 ? b.c0.y : q == 2 ? b.c0.z : b.c0.w;
    return (w >> (8u * (i & 3u))) & 255u;
}
#define MELF_JP_BYTE(b, at) stream_byte(b, at)
#else
#define MELF_JP_BYTE(b, at) ((uint32_t)(b).d[at])
#endif
MELF_JP_FN void fill(Bits& b)
{
    while (b.n <= 56) {
        uint32_t byte = 0;
        while (!b.stop) {   // pos moves forward in every turn
            if (b.pos >= b.end) { b.stop = true; break; }
            byte = MELF_JP_BYTE(b, b.pos);
            if (byte != 0xFFu) { ++b.pos; break; }
            if (b.pos + 1 >= b.end) { b.stop = true; break; }
            const uint32_t nx = MELF_JP_BYTE(b, b.pos + 1);
            if (nx == 0u) { b.pos += 2; break; }
            if (nx == 0xFFu) { ++b.pos; continue; }
            b.stop = true;
        }
        if (b.stop) { byte = 0; b.pad += 8; }
        b.buf |= (uint64_t)byte << (56 - b.n);
        b.n += 8;
    }
}
MELF_JP_FN uint32_t get_bits(Bits& b, const int k)   // 0 <= k <= 16
{
    if (b.n < k) fill(b);
    if (k == 0) return 0;
    const uint32_t v = (uint32_t)(b.buf >> (64 - k));
    b.buf <<= k;
    b.n -= k;
    return v;
}
// First-level lookup of a table: for each 8-bit window (length << 8) | symbol of the code it starts with, 0 when that code is
// longer than 8 bits (or does not exist).
constexpr int LOOK_BITS = 8, LOOK_N = 1 << LOOK_BITS;
MELF_JP_FN uint16_t look_entry(const Huff* t, const uint32_t x)
{
    for (int l = 1; l <= LOOK_BITS; ++l) {
        const uint32_t p = x >> (LOOK_BITS - l);
        if (p < t->limit[l - 1]) return (uint16_t)((l << 8) | t->huffval[(uint32_t)(t->valoff[l - 1] + (int32_t)p) & 255u]);
    }
    return 0;
}
// the next symbol, or -1 when the bits start no code of the table.  look: the table's LOOK_N first-level entries, or NULL
MELF_JP_FN int get_symbol(Bits& b, const Huff* t, const uint16_t* look)
{
    if (b.n < 16) fill(b);
    const uint32_t c = (uint32_t)(b.buf >> 48);
    int l0 = 1;
    if (look) {
        const uint32_t e = look[c >> (16 - LOOK_BITS)];
        if (e) {
            b.buf <<= (e >> 8);
            b.n -= (int)(e >> 8);
            return (int)(e & 255u);
        }
        l0 = LOOK_BITS + 1;
    }
    for (int l = l0; l <= 16; ++l) {
        const uint32_t p = c >> (16 - l);
        if (p < t->limit[l - 1]) {
            b.buf <<= l;
            b.n -= l;
            return t->huffval[(uint32_t)(t->valoff[l - 1] + (int32_t)p) & 255u];
        }
    }
    return -1;
}
MELF_JP_FN int extend(const uint32_t v, const int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }   // F.2.2.1, s >= 1

// One restart interval (or a whole scan without restart markers): `nunits` MCUs of scan `s` from MCU `unit0` on, read from
// d[begin .. end), added to the file's coefficient area `area` (area_blocks(f) blocks).  nat: zigzag position -> place in the
// block.  tabs[0..2]: the DC tables of the scan's components (DC first scans), tabs[3]: its AC table (AC scans); look: their four
// first-level tables (LOOK_N entries each), or NULL.  0 = done, 1 = corrupt (the data ran out, a code that does not exist, a run
// that leaves the band or the interval).
// On the GPU the interval is one lane's chain of dependent steps, so what it waits for is memory.  DC first and AC first scans
// only store (the coefficients they send were zero: the parser has checked the script).  A DC refinement ORs its bit into the
// block with an atomic whose result nobody waits for.  An AC refinement must read the block: it reads a copy in `stage` (LDS,
// 128 bytes of the lane's own), stores every coefficient it changes to the copy AND to memory (single 16-bit stores: a scan of
// the same level may be writing other coefficients of the block), and asks for the NEXT block before it works on this one.
MELF_JP_FN int decode_interval(const File& f, const Scan& s, const uint8_t* d, const uint32_t begin, const uint32_t end, const uint32_t unit0,
                               const uint32_t nunits, const Huff* tabs, const uint16_t* look, const uint8_t* nat, int16_t* area, int16_t* stage)
{
    const Huff *dc0 = tabs, *dc1 = tabs + 1, *dc2 = tabs + 2, *ac = tabs + 3;
    const uint16_t *ldc0 = look, *ldc1 = look ? look + LOOK_N : look, *ldc2 = look ? look + 2 * LOOK_N : look, *lac = look ? look + 3 * LOOK_N : look;
    Bits b = {d, begin, end, 0, 0, 0, false};
#if MELF_JP_STAGED
    u32x4 nx[8];   // the next block of an AC refinement, on its way
    if (s.Ss > 0 && s.Ah > 0 && nunits > 0) {
        int c0;
        const uint32_t p0 = block_place(f, s, unit0, 0, &c0);
        if (p0 >= area_blocks(f)) return 1;
        const int16_t* src = area + (size_t)p0 * 64;
        MELF_JP_UNROLL
        for (int q = 0; q < 8; ++q) nx[q] = load16(src + 8 * q);
    }
#else
    (void)stage;
#endif
    const uint32_t nblocks = area_blocks(f);
    const int ub = unit_blocks(f, s);
    const int Ss = s.Ss, Se = s.Se > 63 ? 63 : s.Se, Al = s.Al;
    const int p1 = 1 << Al, m1 = -(1 << Al);
    int pred0 = 0, pred1 = 0, pred2 = 0;
    uint32_t eobrun = 0;
    for (uint32_t u = 0; u < nunits; ++u) {
        for (int j = 0; j < ub; ++j) {
            int ci = 0;
            const uint32_t place = block_place(f, s, unit0 + u, j, &ci);
            if (place >= nblocks) return 1;
            int16_t* B = area + (size_t)place * 64;
            if (Ss == 0) {
                if (s.Ah == 0) {   // DC first
                    const int sym = get_symbol(b, ci == 0 ? dc0 : ci == 1 ? dc1 : dc2, ci == 0 ? ldc0 : ci == 1 ? ldc1 : ldc2);
                    if (sym < 0 || sym > 15) return 1;
                    const int diff = sym ? extend(get_bits(b, sym), sym) : 0;
                    int pr = ci == 0 ? pred0 : ci == 1 ? pred1 : pred2;
                    pr += diff;
                    if (ci == 0) pred0 = pr; else if (ci == 1) pred1 = pr; else pred2 = pr;
                    B[0] = (int16_t)(pr * p1);
                } else if (get_bits(b, 1)) {   // DC refinement
#if defined(__HIP_DEVICE_COMPILE__)
                    // the block is 128-byte aligned and B[0] the low half of its first dword (p1 < 2^14)
                    (void)__hip_atomic_fetch_or((unsigned int*)B, (unsigned int)p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
                    B[0] = (int16_t)(B[0] | p1);
#endif
                }
                continue;
            }
            if (s.Ah == 0) {   // AC first
                if (eobrun > 0) { --eobrun; continue; }
                for (int k = Ss; k <= Se; ++k) {
                    const int sym = get_symbol(b, ac, lac);
                    if (sym < 0) return 1;
                    const int r = sym >> 4, sz = sym & 15;
                    if (sz) {
                        k += r;
                        if (k > Se) return 1;
                        B[nat[k]] = (int16_t)(extend(get_bits(b, sz), sz) * p1);
                    } else if (r == 15) {
                        k += 15;
                    } else {
                        eobrun = (1u << r) + (r ? get_bits(b, r) : 0u);
                        if (eobrun > nunits - u) return 1;   // the run leaves the interval
                        --eobrun;                            // this block's band ends here
                        break;
                    }
                }
                continue;
            }
            // AC refinement
#if MELF_JP_STAGED
            int16_t* const G = B;       // the block in memory
            int16_t* const R = stage;   // ... and the copy the scan reads
            MELF_JP_UNROLL
            for (int q = 0; q < 8; ++q) store16(stage + 8 * q, nx[q]);
            if (u + 1 < nunits) {
                int c1;
                const uint32_t pn = block_place(f, s, unit0 + u + 1, 0, &c1);
                if (pn >= nblocks) return 1;
                const int16_t* src = area + (size_t)pn * 64;
                MELF_JP_UNROLL
                for (int q = 0; q < 8; ++q) nx[q] = load16(src + 8 * q);
            }
#define MELF_JP_THROUGH(k) G[nat[k]] = R[nat[k]]
#else
            int16_t* const R = B;
#define MELF_JP_THROUGH(k) (void)0
#endif
            int k = Ss;
            if (eobrun == 0) {
                for (; k <= Se; ++k) {
                    const int sym = get_symbol(b, ac, lac);
                    if (sym < 0) return 1;
                    int r = sym >> 4;
                    const int sz = sym & 15;
                    int val = 0;
                    if (sz) {
                        if (sz != 1) return 1;   // a new coefficient is +-1 at this precision
                        val = get_bits(b, 1) ? p1 : m1;
                    } else if (r != 15) {
                        eobrun = (1u << r) + (r ? get_bits(b, r) : 0u);
                        if (eobrun > nunits - u) return 1;
                        break;   // the rest of the band is handled below
                    }
                    // pass r zero-history coefficients (ZRL: fifteen, and the sixteenth below), correcting the others on the way
                    for (; k <= Se; ++k) {
                        int16_t* q = R + nat[k];
                        if (*q != 0) {
                            if (get_bits(b, 1) && (*q & p1) == 0) { *q = (int16_t)(*q + (*q >= 0 ? p1 : m1)); MELF_JP_THROUGH(k); }
                        } else {
                            if (--r < 0) break;
                        }
                    }
                    if (val) {
                        if (k > Se) return 1;   // the run left the band
                        R[nat[k]] = (int16_t)val;
                        MELF_JP_THROUGH(k);
                    }
                }
            }
            if (eobrun > 0) {
                for (; k <= Se; ++k) {
                    int16_t* q = R + nat[k];
                    if (*q != 0 && get_bits(b, 1) && (*q & p1) == 0) { *q = (int16_t)(*q + (*q >= 0 ? p1 : m1)); MELF_JP_THROUGH(k); }
                }
                --eobrun;
            }
#undef MELF_JP_THROUGH
        }
    }
    return b.n < b.pad ? 1 : 0;   // bits from behind the data were used
}

// ---- host side ----
// Walks a scan's entropy-coded bytes d[i .. n): returns where the first marker that is not RSTn stands (the place of its FF), or
// n when the data end first.  Every RSTn met begins a new interval behind it: rst[k] = its first byte relative to i, for
// k < cap; *count = intervals met (rst[0] = 0 is the first), counted up to cap + 1.
inline size_t walk_scan(const uint8_t* d, size_t i, const size_t n, uint32_t* rst, const uint32_t cap, uint32_t* count)
{
    const size_t i0 = i;
    uint32_t cnt = 1;
    if (cap > 0) rst[0] = 0;
    while (i < n) {
        const uint8_t* p = (const uint8_t*)memchr(d + i, 0xFF, n - i);
        if (!p) { i = n; break; }
        i = (size_t)(p - d);
        if (i + 1 >= n) { i = n; break; }   // a lone FF at the end: the data ended
        const uint8_t nx = d[i + 1];
        if (nx == 0x00) { i += 2; continue; }
        if (nx == 0xFF) { i += 1; continue; }
        if (nx >= 0xD0 && nx <= 0xD7) {
            i += 2;
            if (cnt < cap) rst[cnt] = (uint32_t)(i - i0);
            if (cnt <= cap) ++cnt;
            continue;
        }
        break;
    }
    *count = cnt;
    return i;
}

// A scan as the host decodes it (the test program; the GPU takes one interval per wave): every interval in turn, with the checks
// the kernel makes -- as many intervals as the scan should have, each behind the RSTn the sequence asks for.
inline int decode_scan_host(const File& f, const Scan& s, const uint8_t* raw, const uint32_t* rst, const Huff* tabs, const uint8_t* nat,
                            int16_t* area)
{
    const uint32_t expected = scan_intervals(f, s), units = scan_units(f, s);
    if (s.rst_count != expected) return 1;
    const uint8_t* d = raw + s.off;
    for (uint32_t it = 0; it < expected; ++it) {
        const uint32_t begin = rst[s.rst_first + it];
        if (begin > s.len) return 1;
        if (it > 0 && (begin < 2 || d[begin - 1] != 0xD0u + ((it - 1u) & 7u))) return 1;
        const uint32_t u0 = s.restart_interval ? it * s.restart_interval : 0u;
        const uint32_t nu = s.restart_interval ? (units - u0 < s.restart_interval ? units - u0 : s.restart_interval) : units;
        // the scan's four tables side by side, as the kernel holds them, and their first-level tables
        Huff four[4];
        uint16_t look[4 * LOOK_N];
        for (int t = 0; t < 4; ++t) {
            const int id = t < 3 ? s.dc_tab[t] : s.ac_tab;
            if (id == NO_TABLE) memset(&four[t], 0, sizeof(Huff)); else four[t] = tabs[id];
            for (int x = 0; x < LOOK_N; ++x) look[t * LOOK_N + x] = look_entry(&four[t], (uint32_t)x);
        }
        int16_t stage[64];   // (used by the staged build only)
        if (decode_interval(f, s, d, begin, s.len, u0, nu, four, look, nat, area, stage)) return 1;
    }
    return 0;
}

}  // namespace jpeg_prog
}  // namespace melf
