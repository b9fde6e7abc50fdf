// The JPEG header parser, host-only: the one piece of the JPEG path that reads a file's bytes one by one before anything has judged
// them.  k_jpeg.hip (the decoder's host side) and melf_api.hip (the probes) include it; tests/jpeg_parse_main.cpp compiles it alone,
// plain and under the host sanitizers, and sweeps it over whole, cut and mutated files (tests/test_jpeg_parse.py).
//
//   next_segment()                 the one walk over marker segments (parse_headers and jpeg_file_orientation)
//   read_sof / _dqt / _dht / _app1_exif / _adobe   one function per kind of segment
//   sos_single / sos_component_scan / sos_progressive   one per scan grammar: the interleaved scan of a baseline file, the three
//                                  one-component scans of a multi-scan file (melf_jpeg_scans.h), a progressive script (melf_jpeg_prog.h)
//   frame_ready_for_scans()        what all three ask of the frame before a scan byte is looked at
//   parse_headers()                the loop that hands every segment to its function
//   jpeg_probe_flags()             what the decode calls would answer, from the headers alone
//
// What is taken: baseline sequential DCT (SOF0 / SOF1), 8 bit, Huffman, one interleaved scan, YCbCr 4:2:0 / 4:2:2 / 4:4:4 or greyscale,
// Huffman table ids 0 and 1, quantisation tables 0..3 -- and what the TAKE_* switches add.  Everything else is reported unsupported
// (JpegHeader::why), including a file that refers to a Huffman table it does not define or to one libjpeg rejects.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/meterelf_hip.h"
#include "melf_jpeg_prog.h"
#include "melf_jpeg_scans.h"
#include "melf_jpeg_std_tables.h"

namespace melf {

static const uint8_t ZIGZAG_TO_NATURAL[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffSpec {
    uint8_t bits[17];  // bits[l] = number of codes of length l
    uint8_t vals[256];
    int nvals;
    bool set;
};

// What the file is.  (What the parser keeps while it reads it: ParseState.)
struct JpegHeader {
    int H = 0, W = 0, ncomp = 0;
    int id[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    int restart_interval = 0;
    uint16_t qt[4][64];
    bool qt_set[4] = {false, false, false, false};
    HuffSpec dc[4], ac[4];      // ids 2 and 3: progressive and multi-scan files only
    size_t scan_begin = 0;
    bool saw_jfif = false, saw_adobe = false, saw_exif = false;
    int orient = 1;             // EXIF orientation of the first Exif APP1 (1 when absent, unreadable or outside 1..8)
    int orient_tag = 1;         // the same whether or not the caller takes oriented files
    int adobe_transform = 0;
    const char* why = nullptr;  // non-NULL: a valid-looking file this decoder does not handle
    // A progressive file (SOF2) that is taken: its scans (byte offsets relative to scan_begin, the first scan's first byte), the
    // distinct Huffman tables they use, and where their restart intervals begin
    bool progressive = false;
    std::vector<jpeg_prog::Scan> pscans;
    std::vector<jpeg_prog::Huff> ptabs;
    std::vector<uint32_t> prst;
    // A multi-scan sequential file that is taken (melf_jpeg_scans.h): per COMPONENT its scan -- the tables in force at its SOS, its
    // restart interval (in blocks of the component), and its entropy-coded bytes (offset relative to scan_begin, up to the next marker)
    struct MScan { HuffSpec dc, ac; int restart_interval; size_t off, len; };
    bool multiscan = false;
    std::vector<MScan> ms;      // three, once multiscan
};

// MELF_JPEG_TAKE_*: what a caller's switches make the parser accept.  TAKE_PROBE_FLAGS: all of them, the flags a probe may be given.
constexpr int TAKE_ORIENTED = MELF_JPEG_TAKE_ORIENTED, TAKE_PROGRESSIVE = MELF_JPEG_TAKE_PROGRESSIVE, TAKE_SAMPLINGS = MELF_JPEG_TAKE_SAMPLINGS,
              TAKE_DEFAULT_TABLES = MELF_JPEG_TAKE_DEFAULT_TABLES, TAKE_MULTISCAN = MELF_JPEG_TAKE_MULTISCAN;
constexpr int TAKE_PROBE_FLAGS = TAKE_ORIENTED | TAKE_PROGRESSIVE | TAKE_SAMPLINGS | TAKE_DEFAULT_TABLES | TAKE_MULTISCAN;
// Files that end early (melf_ctx_set_jpeg_truncated): the switch travels with the flags above as a bit of its own that no probe takes
// and the parser does not look at (truncation does not show in the headers); it is the Huffman stage's.
constexpr int JPEG_TAKE_TRUNCATED_INTERNAL = 256;
constexpr int TAKE_TRUNCATED = JPEG_TAKE_TRUNCATED_INTERNAL;
static_assert((TAKE_PROBE_FLAGS & TAKE_TRUNCATED) == 0 && TAKE_PROBE_FLAGS == 55, "the switches' bits");
// Long scans (melf_ctx_set_jpeg_long_scans): an internal bit too -- whether a scan is long does not show in what a probe reports -- and
// beside it the segment length a caller chose for the chapters, in dwords (melf_jpeg_long.h; 0: the production length).
constexpr int JPEG_TAKE_LONG_INTERNAL = 512;
constexpr int TAKE_LONG = JPEG_TAKE_LONG_INTERNAL;
constexpr int JPEG_TAKE_LONG_DW_SHIFT = 16;
constexpr uint32_t JPEG_TAKE_LONG_DW_MASK = 1023u;
static_assert((TAKE_PROBE_FLAGS & TAKE_LONG) == 0 && (TAKE_TRUNCATED & TAKE_LONG) == 0, "the switches' bits");

// What the parser keeps while it goes through a progressive file's scans (T.81 G.1.1.1.1 and libjpeg's progressive decoder).
struct ProgState {
    int8_t bits[3][64];   // per coefficient: -1 = not sent yet, else the precision (Al) it has been brought to
    int dc_idx[4], ac_idx[4];   // where table id t, as defined now, stands in h.ptabs (-1: not built)
    bool started = false;       // the first scan's SOS has been taken (the frame was judged then)
    ProgState() { memset(bits, -1, sizeof(bits)); for (int t = 0; t < 4; ++t) dc_idx[t] = ac_idx[t] = -1; }
};

// What the parser keeps while it goes through a file: the caller's switches, decoded, and where it is in the file's grammar.
struct ParseState {
    const bool take_orient, take_prog, take_samp, take_std_tables, take_multi;
    bool have_sof = false;      // a frame header (SOF0, SOF1, or SOF2 where taken) has been read
    // A DHT defined id 2 or 3 where that may still turn out to be allowed: in front of the frame header (a progressive file may), or
    // anywhere with take_multi (a multi-scan file may).  Decided at the SOF without take_multi, at the first SOS with it.
    bool high_table = false;
    unsigned ms_seen = 0;       // multi-scan sequential file: the components that have had their scan (bit c)
    ProgState ps;
    explicit ParseState(const int take)
        : take_orient((take & TAKE_ORIENTED) != 0), take_prog((take & TAKE_PROGRESSIVE) != 0), take_samp((take & TAKE_SAMPLINGS) != 0),
          take_std_tables((take & TAKE_DEFAULT_TABLES) != 0), take_multi((take & TAKE_MULTISCAN) != 0) {}
};

// What a segment's function answers.  SEG_STOP: parse_headers returns 0 -- h.why says why the file is not taken, or the file's last
// scan has been recorded.  A function may also set h.why and answer SEG_NEXT: the file is refused, the size is still wanted.
enum { SEG_BAD = -1, SEG_STOP = 0, SEG_NEXT = 1 };

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// SOFn: C0..CF without DHT (C4), JPG (C8) and DAC (CC)
inline bool is_frame_marker(const int m) { return m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC; }

// The next marker at or behind d[i], found as libjpeg's next_marker finds it: garbage in front of an FF is tolerated, fill FFs are
// skipped, and the parameterless markers (SOI, RSTn, TEM) are passed by.  False when the data end first.  Else *m is the marker and i
// stands behind its segment: EOI has none (*len = 0); for any other marker *payload, *len are the bytes behind its length field, or
// *len = -1 when the length field is cut off, below 2, or reaches past the data (i then stands behind the marker).
inline bool next_segment(const uint8_t* d, const size_t n, size_t& i, int* m, const uint8_t** payload, int* len)
{
    for (;;) {
        while (i < n && d[i] != 0xFF) ++i;
        while (i < n && d[i] == 0xFF) ++i;
        if (i >= n) return false;
        *m = d[i++];
        if (*m == 0xD8 || (*m >= 0xD0 && *m <= 0xD7) || *m == 0x01) continue;
        *payload = d + i;
        *len = *m == 0xD9 ? 0 : -1;
        if (*m == 0xD9 || i + 2 > n) return true;
        const int L = be16(d + i);
        if (L < 2 || i + L > n) return true;
        *payload = d + i + 2;
        *len = L - 2;
        i += L;
        return true;
    }
}

// The orientation tag (0x0112) of IFD0 of an EXIF block (TIFF header at `t`): 1..8, or 0 when absent / unreadable.
inline int exif_orientation(const uint8_t* t, int n)
{
    if (n < 8) return 0;
    const bool le = t[0] == 'I' && t[1] == 'I';
    if (!le && !(t[0] == 'M' && t[1] == 'M')) return 0;
    auto u16 = [&](int o) { return le ? (t[o] | t[o + 1] << 8) : (t[o] << 8 | t[o + 1]); };
    auto u32 = [&](int o) { return le ? ((uint32_t)t[o] | (uint32_t)t[o + 1] << 8 | (uint32_t)t[o + 2] << 16 | (uint32_t)t[o + 3] << 24)
                                      : ((uint32_t)t[o] << 24 | (uint32_t)t[o + 1] << 16 | (uint32_t)t[o + 2] << 8 | (uint32_t)t[o + 3]); };
    if (u16(2) != 42) return 0;
    const uint32_t ifd = u32(4);
    if (ifd > (uint32_t)n - 2) return 0;
    const int cnt = u16((int)ifd);
    for (int k = 0; k < cnt; ++k) {
        const long e = (long)ifd + 2 + 12L * k;
        if (e + 12 > n) return 0;
        if (u16((int)e) == 0x0112) {
            const int v = u16((int)e + 8);   // type SHORT, count 1: the value sits in the first two bytes of the value field
            return (v >= 1 && v <= 8) ? v : 0;
        }
    }
    return 0;
}

// What libjpeg checks when it builds the decoding table of a Huffman table the scan refers to (jdhuff, derived tables): the
// canonical code counter must stay below 2^l after the codes of every length l in use -- an over-subscribed code set fails
// that, and so does a complete one, whose last code is all ones -- and a DC table may only hold the categories 0..15.  A
// table that fails makes libjpeg refuse the file; the kernels would decode something from it, so it is refused here too.
inline const char* huff_spec_flaw(const HuffSpec& t, const bool dc)
{
    int last = 0;
    for (int l = 1; l <= 16; ++l) if (t.bits[l]) last = l;
    long code = 0;
    for (int l = 1; l <= last; ++l) {
        code += t.bits[l];
        if (code >= (1L << l)) return "Huffman table over-subscribed or using the all-ones code (libjpeg rejects it)";
        code <<= 1;
    }
    if (dc)
        for (int i = 0; i < t.nvals; ++i)
            if (t.vals[i] > 15) return "DC Huffman table with a category above 15 (libjpeg rejects it)";
    return nullptr;
}

struct HuffSlow {  // canonical decode data (JPEG spec F.2.2.3) for code lengths 1..16
    // limit[l - 1]: the canonical code counter after the codes of length l (one past the largest code of
    // length l, carried over from shorter lengths if there is none).  A bit window's l-bit prefix is
    // below limit[l - 1] exactly for l >= the code's length, so the length is 1 + the number of l with
    // prefix >= limit[l - 1]: independent compares, no data-dependent loop.
    uint32_t limit[16];
    int32_t valoff[16];  // huffval index of the first code of length l, minus that code
    uint8_t huffval[256];
};
constexpr int SLOW_DW = 96;
static_assert(sizeof(HuffSlow) == SLOW_DW * 4, "HuffSlow is copied to LDS as dwords");
static_assert(sizeof(jpeg_prog::Huff) == sizeof(HuffSlow) && offsetof(jpeg_prog::Huff, valoff) == offsetof(HuffSlow, valoff) &&
              offsetof(jpeg_prog::Huff, huffval) == offsetof(HuffSlow, huffval), "melf_jpeg_prog.h restates HuffSlow");

// Table: HuffSlow, or jpeg_prog::Huff, which restates it
template <class Table>
inline void build_huff(const HuffSpec& t, Table* slow)
{
    memset(slow, 0, sizeof(*slow));
    memcpy(slow->huffval, t.vals, t.nvals);
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        slow->valoff[l - 1] = p - code;
        p += t.bits[l];
        code += t.bits[l];
        slow->limit[l - 1] = (uint32_t)code;
        code <<= 1;
    }
}

// ------------------------------------------------------------------ the frame ----
// The rules on the frame header that do not depend on the kind of scan: sets h.why, and makes a greyscale frame 1x1.
// take_samp (TAKE_SAMPLINGS): luma 1x2 (4:4:0) and 4x1 (4:1:1) are taken too; 4:1:0 (4x2) has 10 blocks an MCU, McuLayout packs 6.
inline void frame_rules(JpegHeader& h, const bool take_samp)
{
    if (h.H <= 0 || h.W <= 0) { h.why = "empty image"; return; }
    if (h.ncomp == 3) {
        if (h.saw_adobe && h.adobe_transform != 1) h.why = "Adobe marker says the data are not YCbCr";
        else if (!h.saw_jfif && !h.saw_adobe && h.id[0] == 'R' && h.id[1] == 'G' && h.id[2] == 'B') h.why = "RGB component ids";
        else if (h.hs[1] != 1 || h.vs[1] != 1 || h.hs[2] != 1 || h.vs[2] != 1) h.why = "subsampled chroma with sampling factors above 1";
        else if (!((h.hs[0] == 1 && h.vs[0] == 1) || (h.hs[0] == 2 && h.vs[0] == 1) || (h.hs[0] == 2 && h.vs[0] == 2))) {
            if (!take_samp) h.why = "luma sampling other than 1x1, 2x1, 2x2";
            else if (h.hs[0] == 4 && h.vs[0] == 2) h.why = "4:1:0 (luma sampling 4x2): more than 6 blocks an MCU";
            else if (!((h.hs[0] == 1 && h.vs[0] == 2) || (h.hs[0] == 4 && h.vs[0] == 1))) h.why = "luma sampling other than 1x1, 2x1, 2x2, 1x2, 4x1";
        }
    } else {
        h.hs[0] = h.vs[0] = 1;  // a single-component scan is never interleaved: one block per MCU
    }
}

// libjpeg-turbo's std_huff_tables, for a caller that asked for it (TAKE_DEFAULT_TABLES): when the Huffman decoder starts -- behind the
// headers up to the first SOS -- each of the slots DC 0, AC 0, DC 1, AC 1 that no DHT has defined receives the table Annex K.3 prints
// for it (melf_jpeg_std_tables.h).  Slots 2 and 3 receive nothing; a slot a DHT defined keeps its definition, flawed or not.
inline void install_std_tables(JpegHeader& h)
{
    for (int cls = 0; cls < 2; ++cls)
        for (int id = 0; id < 2; ++id) {
            HuffSpec& t = cls ? h.ac[id] : h.dc[id];
            if (t.set) continue;
            const jpeg_std::Table& k = jpeg_std::TABLES[cls][id];
            t.bits[0] = 0;
            memcpy(t.bits + 1, k.counts, 16);
            memcpy(t.vals, k.vals, (size_t)k.nvals);
            t.nvals = k.nvals;
            t.set = true;
        }
}

// The frame must be one for the decoder before any scan byte is looked at: the first SOS of every scan grammar asks here, once, with
// h.why still clear.  The frame's rules; then per component its quantisation table -- and, for the single interleaved scan, whose SOS
// names every component's Huffman tables (h.td, h.ta), those too, so that the first thing missing or flawed in frame order gives the
// reason.  std_tables: a frame that passed receives the Annex K tables in its empty slots -- once, before the first scan, as libjpeg
// does.  False: h.why says why not.
inline bool frame_ready_for_scans(JpegHeader& h, const ParseState& st, const bool std_tables, const bool single_scan)
{
    frame_rules(h, st.take_samp);
    for (int c = 0; c < h.ncomp && !h.why; ++c) {
        if (!h.qt_set[h.tq[c]]) h.why = "missing quantisation table";
        else if (!single_scan) continue;
        else if (!h.dc[h.td[c]].set || !h.ac[h.ta[c]].set) h.why = "missing Huffman table";
        else if (const char* flaw = huff_spec_flaw(h.dc[h.td[c]], true)) h.why = flaw;
        else if (const char* flaw_ac = huff_spec_flaw(h.ac[h.ta[c]], false)) h.why = flaw_ac;
    }
    if (h.why) return false;
    if (std_tables) install_std_tables(h);
    return true;
}

// ------------------------------------------------------------------ one function per kind of segment ----
// SOFn.  Baseline / extended sequential Huffman (SOF0, SOF1) is read -- and progressive (SOF2) where the caller takes it and no frame
// header came before; every other process is unsupported, with the size where it can be read.  One frame header per file once a
// progressive frame is taken or a multi-scan file's first scan has been: any further SOFn (libjpeg: "duplicate SOF") makes the file
// unsupported -- the rules on the frame were applied to the first one, and the scans recorded so far rest on its geometry.
inline int read_sof(const int m, const uint8_t* s, const int len, JpegHeader& h, ParseState& st)
{
    if (h.progressive) { h.why = "second frame header in a progressive file (libjpeg rejects it)"; return SEG_STOP; }
    if (h.multiscan) { h.why = "second frame header behind a scan (libjpeg rejects it)"; return SEG_STOP; }
    if (!(m == 0xC0 || m == 0xC1 || (m == 0xC2 && st.take_prog && !st.have_sof))) {
        h.why = "not a baseline sequential Huffman JPEG (progressive / lossless / arithmetic)";
        if (len >= 6) { h.H = be16(s + 1); h.W = be16(s + 3); }
        return SEG_STOP;
    }
    if (len < 6) return SEG_BAD;
    if (s[0] != 8) { h.why = "sample precision is not 8 bits"; }   // (and on: the size is still wanted)
    h.H = be16(s + 1); h.W = be16(s + 3); h.ncomp = s[5];
    if (h.ncomp != 1 && h.ncomp != 3) { h.why = "neither greyscale nor three components"; h.ncomp = h.ncomp > 3 ? 3 : h.ncomp; }
    if (len < 6 + 3 * (int)s[5]) return SEG_BAD;
    for (int c = 0; c < h.ncomp; ++c) {
        h.id[c] = s[6 + 3 * c]; h.hs[c] = s[7 + 3 * c] >> 4; h.vs[c] = s[7 + 3 * c] & 15; h.tq[c] = s[8 + 3 * c] & 3;
    }
    st.have_sof = true;
    if (m == 0xC2) h.progressive = true;
    else if (st.high_table && !st.take_multi) h.why = "Huffman table id above 1";   // (take_multi: decided at the first SOS)
    return SEG_NEXT;
}

// DQT.  Behind the first scan of a progressive or a multi-scan file it is refused: the IDCT runs once, with one set of tables.
inline int read_dqt(const uint8_t* s, const int len, JpegHeader& h, const ParseState& st)
{
    if (h.multiscan) { h.why = "quantisation table defined after the first scan of a multi-scan file"; return SEG_STOP; }
    if (st.ps.started) { h.why = "quantisation table defined after the first scan of a progressive file"; return SEG_STOP; }
    int o = 0;
    while (o < len) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        ++o;
        if (tq > 3 || o + (pq ? 128 : 64) > len) return SEG_BAD;
        for (int k = 0; k < 64; ++k) {
            const int v = pq ? be16(s + o + 2 * k) : s[o + k];
            h.qt[tq][ZIGZAG_TO_NATURAL[k]] = (uint16_t)v;
        }
        h.qt_set[tq] = true;
        o += pq ? 128 : 64;
    }
    return SEG_NEXT;
}

// DHT.  Ids 2 and 3 are a progressive or a multi-scan file's to use; anywhere else they make the file unsupported, as ever -- at once
// where that is known, else through st.high_table.
inline int read_dht(const uint8_t* s, const int len, JpegHeader& h, ParseState& st)
{
    int o = 0;
    while (o < len) {
        if (o + 17 > len) return SEG_BAD;
        const int tc = s[o] >> 4, th = s[o] & 15;
        int total = 0;
        for (int l = 1; l <= 16; ++l) total += s[o + l];
        if (total > 256 || o + 17 + total > len || tc > 1) return SEG_BAD;
        if (th > 3 || (th > 1 && !st.take_prog && !st.take_multi)) { h.why = "Huffman table id above 1"; o += 17 + total; continue; }
        if (th > 1 && !h.progressive) { if (st.have_sof && !st.take_multi) h.why = "Huffman table id above 1"; else st.high_table = true; }
        (tc ? st.ps.ac_idx[th] : st.ps.dc_idx[th]) = -1;   // a scan after this one builds the new definition
        HuffSpec& t = tc ? h.ac[th] : h.dc[th];
        t.bits[0] = 0;
        for (int l = 1; l <= 16; ++l) t.bits[l] = s[o + l];
        memcpy(t.vals, s + o + 17, total);
        t.nvals = total;
        t.set = true;
        o += 17 + total;
    }
    return SEG_NEXT;
}

// APP1: cv2.imread (3.4) applies the EXIF orientation tag.  Unless the caller takes oriented files (k_jpeg_color_exif), a file that
// asks for it goes to the caller's host decoder (which rotates: meterelf_amd/_image.py).  Only the first Exif block counts; a later
// one that asks again is left to the host.
inline void read_app1_exif(const uint8_t* s, const int len, JpegHeader& h, const ParseState& st)
{
    if (len < 14 || memcmp(s, "Exif\0\0", 6)) return;
    const int o = exif_orientation(s + 6, len - 6);
    if (o > 1 && !h.saw_exif) h.orient_tag = o;
    if (o > 1 && (!st.take_orient || h.saw_exif)) h.why = "EXIF orientation other than top-left (decoded and rotated on the host)";
    else if (o > 1) h.orient = o;
    h.saw_exif = true;
}

inline void read_adobe(const uint8_t* s, const int len, JpegHeader& h)
{
    if (len >= 12 && !memcmp(s, "Adobe", 5)) { h.saw_adobe = true; h.adobe_transform = s[11]; }
}

// ------------------------------------------------------------------ one function per scan grammar ----
// Each is given the SOS parameters `s` (ns, then ns pairs of component id and table ids, then Ss, Se, Ah | Al: their length has been
// checked) and i, the scan's first entropy-coded byte; the two that go on to further scans leave i behind the scan's bytes.

// The single interleaved scan of a baseline file: the headers end here.
inline int sos_single(const uint8_t* s, const size_t i, JpegHeader& h, const ParseState& st)
{
    const int ns = s[0];
    if (ns != h.ncomp) { h.why = "more than one scan (non-interleaved components)"; return SEG_STOP; }
    if (st.take_multi && st.high_table && !h.why) h.why = "Huffman table id above 1";   // no multi-scan file after all
    for (int k = 0; k < ns; ++k) {
        const int cid = s[1 + 2 * k];
        int c = -1;
        for (int q = 0; q < h.ncomp; ++q) if (h.id[q] == cid) c = q;
        if (c != k) { h.why = "scan component order differs from the frame header"; return SEG_STOP; }
        h.td[c] = s[2 + 2 * k] >> 4; h.ta[c] = s[2 + 2 * k] & 15;
        if (h.td[c] > 1 || h.ta[c] > 1) h.why = "Huffman table id above 1";
    }
    const uint8_t* e = s + 1 + 2 * ns;
    if (e[0] != 0 || e[1] != 63 || e[2] != 0) { h.why = "not a full sequential scan"; return SEG_STOP; }
    h.scan_begin = i;
    if (h.why) return SEG_STOP;
    // the Annex K tables, here in front of the check, which judges the tables this scan names (so a frame that has a size keeps them
    // even when it is then refused for its sampling or a quantisation table)
    if (st.take_std_tables && h.H > 0 && h.W > 0) install_std_tables(h);
    frame_ready_for_scans(h, st, false, true);
    return SEG_STOP;
}

// A scan of a sequential file that sends its components in scans of their own (melf_jpeg_scans.h).  Ids 2 and 3 and redefinitions
// between the scans are free: every scan keeps a snapshot of the two tables in force at its SOS.
inline int sos_component_scan(const uint8_t* d, const size_t n, const uint8_t* s, size_t& i, JpegHeader& h, ParseState& st)
{
    if (h.why) return SEG_STOP;
    if (!h.multiscan) {
        if (!frame_ready_for_scans(h, st, st.take_std_tables, false)) return SEG_STOP;
        h.scan_begin = i;
        h.multiscan = true;
        h.ms.assign(3, JpegHeader::MScan());
    }
    const int ns = s[0];
    int c = -1;
    for (int q = 0; q < h.ncomp; ++q) if (h.id[q] == s[1]) c = q;
    const uint8_t* e = s + 1 + 2 * ns;
    if (const char* flaw = jpeg_scans::scan_rule(ns, c, st.ms_seen, e[0], e[1], e[2])) { h.why = flaw; return SEG_STOP; }
    const int td = s[2] >> 4, ta = s[2] & 15;
    if (td > 3 || ta > 3) { h.why = "Huffman table id above 3"; return SEG_STOP; }
    if (!h.dc[td].set || !h.ac[ta].set) { h.why = "missing Huffman table"; return SEG_STOP; }
    if (const char* flaw = huff_spec_flaw(h.dc[td], true)) { h.why = flaw; return SEG_STOP; }
    if (const char* flaw = huff_spec_flaw(h.ac[ta], false)) { h.why = flaw; return SEG_STOP; }
    JpegHeader::MScan& sc = h.ms[c];
    sc.dc = h.dc[td]; sc.ac = h.ac[ta];
    sc.restart_interval = h.restart_interval;
    sc.off = i - h.scan_begin;
    uint32_t found = 0;
    const size_t end = jpeg_prog::walk_scan(d, i, n, nullptr, 0, &found);   // the one pass over these files' bytes
    if (end >= n) return SEG_BAD;   // the data end inside a scan: a truncated file
    sc.len = end - i;
    st.ms_seen |= 1u << c;
    i = end;
    if (st.ms_seen != 7u) return SEG_NEXT;
    size_t j = end;   // behind the third scan: EOI (what lies behind that is ignored, as ever)
    while (j < n && d[j] == 0xFF) ++j;
    if (j >= n) return SEG_BAD;
    if (d[j] != 0xD9) h.why = "segment behind the third scan of a multi-scan file other than EOI";
    return SEG_STOP;
}

inline jpeg_prog::File prog_file_geometry(const JpegHeader& h)
{
    jpeg_prog::File f;
    memset(&f, 0, sizeof(f));
    f.ncomp = (uint8_t)h.ncomp; f.hs0 = (uint8_t)h.hs[0]; f.vs0 = (uint8_t)h.vs[0];
    f.mcus_x = (uint16_t)((h.W + 8 * h.hs[0] - 1) / (8 * h.hs[0]));
    f.mcus_y = (uint16_t)((h.H + 8 * h.vs[0] - 1) / (8 * h.vs[0]));
    f.rbx0 = (uint16_t)((h.W + 7) / 8); f.rby0 = (uint16_t)((h.H + 7) / 8);
    f.rbxc = (uint16_t)(((h.W + h.hs[0] - 1) / h.hs[0] + 7) / 8); f.rbyc = (uint16_t)(((h.H + h.vs[0] - 1) / h.vs[0] + 7) / 8);
    return f;
}

// One SOS of a progressive file (s: its parameters): the scan's record, or why the file is not taken.
inline const char* prog_scan_header(JpegHeader& h, ProgState& ps, const uint8_t* s, jpeg_prog::Scan& sc)
{
    memset(&sc, 0, sizeof(sc));
    sc.ac_tab = jpeg_prog::NO_TABLE;
    for (int k = 0; k < 3; ++k) sc.dc_tab[k] = jpeg_prog::NO_TABLE;
    const int ns = s[0];
    if (ns < 1 || ns > h.ncomp) return "progressive scan with a component count outside 1..components of the frame";
    const uint8_t* e = s + 1 + 2 * ns;
    const int Ss = e[0], Se = e[1], Ah = e[2] >> 4, Al = e[2] & 15;
    if (Ss == 0 ? Se != 0 : (ns != 1 || Se < Ss || Se > 63)) return "progressive scan whose band is not DC alone or Ss <= Se <= 63 of one component";
    if (Ah != 0 && Al != Ah - 1) return "progressive scan whose Al is not Ah - 1";
    if (Al > 13) return "progressive scan with Al above 13";
    sc.ns = (uint8_t)ns; sc.Ss = (uint8_t)Ss; sc.Se = (uint8_t)Se; sc.Ah = (uint8_t)Ah; sc.Al = (uint8_t)Al;
    sc.restart_interval = (uint16_t)h.restart_interval;
    int prev = -1;
    for (int k = 0; k < ns; ++k) {
        const int cid = s[1 + 2 * k];
        int c = -1;
        for (int q = 0; q < h.ncomp; ++q) if (h.id[q] == cid) c = q;
        if (c <= prev) return "progressive scan whose components are not in the frame header's order";
        prev = c;
        sc.comp[k] = (uint8_t)c;
        const int td = s[2 + 2 * k] >> 4, ta = s[2 + 2 * k] & 15;
        if (td > 3 || ta > 3) return "Huffman table id above 3";
        if (Ss > 0 && ps.bits[c][0] < 0) return "inconsistent progression: an AC scan before the component's first DC scan";
        for (int z = Ss; z <= Se; ++z) {
            if (Ah == 0 ? ps.bits[c][z] >= 0 : ps.bits[c][z] != Ah)
                return Ah == 0 ? "inconsistent progression: a first scan over coefficients already sent"
                               : "inconsistent progression: a refinement of coefficients whose precision is not Ah";
            ps.bits[c][z] = (int8_t)Al;
        }
        // the tables in force now: a DC first scan decodes with its DC tables, every AC scan with its AC table
        const bool need_dc = Ss == 0 && Ah == 0, need_ac = Ss > 0;
        if (need_dc || need_ac) {
            const HuffSpec& t = need_dc ? h.dc[td] : h.ac[ta];
            int& idx = need_dc ? ps.dc_idx[td] : ps.ac_idx[ta];
            if (!t.set) return "missing Huffman table";
            if (idx < 0) {
                if (const char* flaw = huff_spec_flaw(t, need_dc)) return flaw;
                if (h.ptabs.size() >= 255) return "too many Huffman tables";
                idx = (int)h.ptabs.size();
                h.ptabs.emplace_back();
                build_huff(t, &h.ptabs.back());
            }
            if (need_dc) sc.dc_tab[k] = (uint8_t)idx; else sc.ac_tab = (uint8_t)idx;
        }
    }
    return nullptr;
}

// A scan of a progressive file that is taken (SOF2 with TAKE_PROGRESSIVE): recorded in h.pscans with its tables, its bytes and
// where its restart intervals begin.
inline int sos_progressive(const uint8_t* d, const size_t n, const uint8_t* s, size_t& i, JpegHeader& h, ParseState& st)
{
    if (h.why) return SEG_STOP;   // refused by a segment in front of or between the scans: no further scan is looked at
    if (!st.ps.started) {
        if (!frame_ready_for_scans(h, st, false, false)) return SEG_STOP;
        h.scan_begin = i;
        st.ps.started = true;
    }
    if (h.pscans.size() >= (size_t)MELF_JPEG_PROG_SCANS_MAX) { h.why = "progressive file with more scans than MELF_JPEG_PROG_SCANS_MAX"; return SEG_STOP; }
    jpeg_prog::Scan sc;
    if (const char* flaw = prog_scan_header(h, st.ps, s, sc)) { h.why = flaw; return SEG_STOP; }
    // the scan's bytes, once: where it ends and where its restart intervals begin
    const jpeg_prog::File geo = prog_file_geometry(h);
    const uint32_t expected = jpeg_prog::scan_intervals(geo, sc);
    sc.off = (uint32_t)(i - h.scan_begin);
    sc.rst_first = (uint32_t)h.prst.size();
    h.prst.resize(h.prst.size() + expected);
    uint32_t found = 0;
    const size_t end = jpeg_prog::walk_scan(d, i, n, h.prst.data() + sc.rst_first, expected, &found);
    if (end >= n) return SEG_BAD;   // the data end inside a scan: a truncated file
    sc.len = (uint32_t)(end - i);
    sc.rst_count = found;
    for (uint32_t k = found; k < expected; ++k) h.prst[sc.rst_first + k] = 0;
    for (const jpeg_prog::Scan& t : h.pscans) {   // the level: behind every earlier scan that touches a coefficient of this one
        bool shared = false;
        for (int a = 0; a < sc.ns; ++a)
            for (int b = 0; b < t.ns; ++b) shared = shared || sc.comp[a] == t.comp[b];
        if (shared && sc.Ss <= t.Se && t.Ss <= sc.Se && t.level + 1 > sc.level) sc.level = (uint8_t)(t.level + 1);
    }
    h.pscans.push_back(sc);
    i = end;
    return SEG_NEXT;
}

// SOS: which grammar the file speaks is known by now.
inline int read_sos(const uint8_t* d, const size_t n, const uint8_t* s, const int len, size_t& i, JpegHeader& h, ParseState& st)
{
    if (!st.have_sof || len < 1) return SEG_BAD;
    const int ns = s[0];
    if (len < 1 + 2 * ns + 3) return SEG_BAD;
    if (h.progressive) return sos_progressive(d, n, s, i, h, st);
    if (h.multiscan || (st.take_multi && h.ncomp == 3 && (ns == 1 || ns == 2))) return sos_component_scan(d, n, s, i, h, st);
    return sos_single(s, i, h, st);
}

// EOI where a segment was looked for: the end of a progressive file's scans, else a file without (all of) its scans.
inline int end_of_image(JpegHeader& h, const ParseState& st)
{
    if (h.progressive && st.ps.started) {
        // libjpeg smooths blocks whose AC coefficients have not reached full precision (jdcoefct's block smoothing): the pixels are
        // those of the coefficient blocks only when every scan of the script has arrived
        for (int c = 0; c < h.ncomp; ++c)
            for (int z = 0; z < 64; ++z)
                if (st.ps.bits[c][z] != 0) { h.why = "progressive script incomplete: not every coefficient reaches full precision (libjpeg smooths such blocks)"; return 0; }
        return 0;
    }
    if (h.multiscan) { h.why = "sequential file that ends before every component has had its scan"; return 0; }
    return -1;   // EOI before SOS
}

// Returns 0 = parsed (check h.why for "unsupported"), -1 = not a JPEG / truncated headers.
// take: TAKE_ORIENTED -- a file with an orientation tag 2..8 is one for the GPU (h.orient says which); TAKE_PROGRESSIVE -- so is a
// progressive file of the subset include/meterelf_hip.h states (h.progressive, h.pscans); TAKE_SAMPLINGS -- and a 4:4:0 or 4:1:1
// file (frame_rules); TAKE_DEFAULT_TABLES -- and a sequential file that leaves Huffman tables 0 / 1 out (install_std_tables);
// TAKE_MULTISCAN -- and a sequential file of three one-component scans (h.multiscan, h.ms).  Otherwise they are unsupported, as ever.
inline int parse_headers(const uint8_t* d, size_t n, JpegHeader& h, const int take = 0)
{
    ParseState st(take);
    for (int t = 0; t < 4; ++t) { h.dc[t].set = false; h.ac[t].set = false; }
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return -1;
    size_t i = 2;
    for (;;) {
        int m = 0, len = 0;
        const uint8_t* s = nullptr;
        if (!next_segment(d, n, i, &m, &s, &len)) return -1;
        if (m == 0xD9) return end_of_image(h, st);
        if (len < 0) return -1;
        // between the scans of a multi-scan sequential file DHT and DRI count; COM and APPn are passed by
        if (h.multiscan && ((m >= 0xE0 && m <= 0xEF) || m == 0xFE)) continue;
        int next = SEG_NEXT;
        if (is_frame_marker(m)) next = read_sof(m, s, len, h, st);
        else if (m == 0xDB) next = read_dqt(s, len, h, st);
        else if (m == 0xC4) next = read_dht(s, len, h, st);
        else if (m == 0xDD) { if (len < 2) return -1; h.restart_interval = be16(s); }
        else if (m == 0xE0) { if (len >= 5 && !memcmp(s, "JFIF\0", 5)) h.saw_jfif = true; }
        else if (m == 0xE1) read_app1_exif(s, len, h, st);
        else if (m == 0xEE) read_adobe(s, len, h);
        else if (m == 0xDA) next = read_sos(d, n, s, len, i, h, st);
        if (next != SEG_NEXT) return next;
    }
}

// What the decode calls of a context with the switches `flags` (MELF_JPEG_TAKE_*) answer from the headers: the STORED size, whether
// the file is taken, and why not.  *orientation (may be NULL): the file's code whether or not files that carry one are taken
// (report_tag), or the code the decoder would apply (1 unless TAKE_ORIENTED is among the flags).
inline int jpeg_probe_flags(const uint8_t* data, size_t size, int flags, bool report_tag, int* H, int* W, int* orientation, int* supported,
                            std::string* why)
{
    JpegHeader h;
    const bool parsed = parse_headers(data, size, h, flags & TAKE_PROBE_FLAGS) == 0;
    *H = parsed ? h.H : 0; *W = parsed ? h.W : 0; *supported = parsed && !h.why ? 1 : 0;
    if (orientation) *orientation = !parsed ? 1 : report_tag ? h.orient_tag : h.orient;
    if (why) *why = !parsed ? "not a JPEG file or truncated headers" : h.why ? h.why : "";
    return 0;
}

// The orientation alone (1..8), from a walk over the marker segments in front of the frame header: what parse_headers records,
// for a caller that orders a call's files before they are parsed.  *progressive: the frame header is SOF2.
inline int jpeg_file_orientation(const uint8_t* d, size_t n, int* progressive = nullptr)
{
    if (progressive) *progressive = 0;
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return 1;
    size_t i = 2;
    for (;;) {
        int m = 0, len = 0;
        const uint8_t* s = nullptr;
        if (!next_segment(d, n, i, &m, &s, &len)) return 1;
        if (m == 0xC2 && progressive) *progressive = 1;
        if (m == 0xD9 || m == 0xDA || is_frame_marker(m) || len < 0) return 1;
        if (m == 0xE1 && len >= 14 && !memcmp(s, "Exif\0\0", 6)) {
            const int o = exif_orientation(s + 6, len - 6);
            return o > 1 ? o : 1;
        }
    }
}

}  // namespace melf
