// Host run of meterelf_amd/csrc/melf_jpeg_prog.h (tests/test_jpeg_progressive.py builds and runs it, plain and under the host
// sanitizers): the progressive scan decoder's body on whole files.  Usage: jpeg_prog_main <manifest>, one file per line,
//     <file.jpg> <expected.i16 | ->
// expected.i16: the coefficient area the file must decode to, int16, in the decoder's block order ((MCU * blocks per MCU + block
// in the MCU) * 64, natural order inside a block).  Prints per file "ok" (decoded, area equal where one was given), "MISMATCH",
// "corrupt" (the decoder or this program's marker walk gave up) and returns 1 on a mismatch.  The coefficient area is malloc'd to
// exactly its size, so a block index out of range is seen by the sanitizer.  The marker parser here is the test's own and takes
// nothing on trust: the damaged files it is given can hold anything behind the first scan.
// The scans are decoded from a copy of the file's bytes laid out as jpeg_prepare_batch lays a file out in the raw area: from the
// first scan's first byte on, 64-byte aligned, align_up(length + 32, 64) bytes and not one more.  Built with -DMELF_JP_HOST_STAGED
// the header takes the GPU build's paths (the stream through aligned 16-byte lines, AC refinement on a staged copy of the block
// with the next block read ahead), so the sanitizer sees the reads those paths make around the data and the area.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../meterelf_amd/csrc/melf_jpeg_prog.h"

using namespace melf::jpeg_prog;

static uint8_t NAT[64];
static void make_nat()
{
    int k = 0;
    for (int s = 0; s < 15; ++s)
        for (int i = 0; i <= s; ++i) {
            const int y = (s % 2) ? i : s - i, x = s - y;
            if (y < 8 && x < 8) NAT[k++] = (uint8_t)(y * 8 + x);
        }
}

struct Spec { uint8_t bits[17]; uint8_t vals[256]; bool set = false; };
static void build(const Spec& t, Huff* h)
{
    memset(h, 0, sizeof(*h));
    int n = 0;
    for (int l = 1; l <= 16; ++l) n += t.bits[l];
    memcpy(h->huffval, t.vals, n > 256 ? 256 : n);
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        h->valoff[l - 1] = p - code;
        p += t.bits[l];
        code += t.bits[l];
        h->limit[l - 1] = (uint32_t)code;
        code <<= 1;
    }
}

// 0 = decoded into area (allocated here), 1 = corrupt
static int decode_file(const std::vector<uint8_t>& v, std::vector<int16_t>* result)
{
    const uint8_t* d = v.data();
    const size_t n = v.size();
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return 1;
    File f;
    memset(&f, 0, sizeof(f));
    int W = 0, H = 0, cid[3] = {0, 0, 0}, ri = 0;
    bool sof = false;
    Spec dc[4], ac[4];
    std::vector<Huff> tabs;
    std::vector<uint32_t> rst;
    int16_t* area = nullptr;
    uint8_t* raw = nullptr;     // the bytes from the first scan on, as the raw area holds them
    size_t scan_begin = 0;
    size_t i = 2;
    int rc = 1;
    for (int scans = 0; scans <= 64;) {
        while (i < n && d[i] != 0xFF) ++i;
        while (i < n && d[i] == 0xFF) ++i;
        if (i >= n) break;
        const int m = d[i++];
        if (m == 0xD9) { rc = area ? 0 : 1; break; }
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (i + 2 > n) break;
        const int L = (d[i] << 8) | d[i + 1];
        if (L < 2 || i + L > n) break;
        const uint8_t* s = d + i + 2;
        const int len = L - 2;
        if (m == 0xC2) {
            if (sof || len < 6 || s[0] != 8 || (s[5] != 1 && s[5] != 3) || len < 6 + 3 * s[5]) break;
            H = (s[1] << 8) | s[2]; W = (s[3] << 8) | s[4];
            if (H <= 0 || W <= 0) break;
            f.ncomp = s[5];
            for (int c = 0; c < f.ncomp; ++c) cid[c] = s[6 + 3 * c];
            f.hs0 = f.ncomp == 1 ? 1 : s[7] >> 4; f.vs0 = f.ncomp == 1 ? 1 : s[7] & 15;
            if (f.hs0 < 1 || f.hs0 > 2 || f.vs0 < 1 || f.vs0 > 2) break;
            f.mcus_x = (uint16_t)((W + 8 * f.hs0 - 1) / (8 * f.hs0)); f.mcus_y = (uint16_t)((H + 8 * f.vs0 - 1) / (8 * f.vs0));
            f.rbx0 = (uint16_t)((W + 7) / 8); f.rby0 = (uint16_t)((H + 7) / 8);
            f.rbxc = (uint16_t)(((W + f.hs0 - 1) / f.hs0 + 7) / 8); f.rbyc = (uint16_t)(((H + f.vs0 - 1) / f.vs0 + 7) / 8);
            sof = true;
        } else if (m == 0xC4) {
            int o = 0;
            bool bad = false;
            while (o < len) {
                if (o + 17 > len) { bad = true; break; }
                const int tc = s[o] >> 4, th = s[o] & 15;
                int total = 0;
                for (int l = 1; l <= 16; ++l) total += s[o + l];
                if (tc > 1 || th > 3 || total > 256 || o + 17 + total > len) { bad = true; break; }
                Spec& t = tc ? ac[th] : dc[th];
                t.bits[0] = 0;
                memcpy(t.bits + 1, s + o + 1, 16);
                memcpy(t.vals, s + o + 17, total);
                t.set = true;
                o += 17 + total;
            }
            if (bad) break;
        } else if (m == 0xDD) {
            if (len < 2) break;
            ri = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!sof || len < 1) break;
            const int ns = s[0];
            if (ns < 1 || ns > f.ncomp || len < 1 + 2 * ns + 3) break;
            Scan sc;
            memset(&sc, 0, sizeof(sc));
            sc.ac_tab = NO_TABLE;
            sc.ns = (uint8_t)ns;
            const uint8_t* e = s + 1 + 2 * ns;
            sc.Ss = e[0]; sc.Se = e[1]; sc.Ah = e[2] >> 4; sc.Al = e[2] & 15;
            if (sc.Al > 13 || sc.Se > 63 || sc.Ss > sc.Se || (sc.Ss == 0 && sc.Se != 0) || (sc.Ss > 0 && ns != 1)) break;
            sc.restart_interval = (uint16_t)ri;
            tabs.clear();
            bool bad = false;
            for (int k = 0; k < 3; ++k) sc.dc_tab[k] = NO_TABLE;
            for (int k = 0; k < ns && !bad; ++k) {
                int c = -1;
                for (int q = 0; q < f.ncomp; ++q) if (cid[q] == s[1 + 2 * k]) c = q;
                const int td = s[2 + 2 * k] >> 4, ta = s[2 + 2 * k] & 15;
                if (c < 0 || td > 3 || ta > 3) { bad = true; break; }
                sc.comp[k] = (uint8_t)c;
                if (sc.Ss == 0 && sc.Ah == 0) {
                    if (!dc[td].set) { bad = true; break; }
                    sc.dc_tab[k] = (uint8_t)tabs.size();
                    tabs.emplace_back();
                    build(dc[td], &tabs.back());
                } else if (sc.Ss > 0) {
                    if (!ac[ta].set) { bad = true; break; }
                    sc.ac_tab = (uint8_t)tabs.size();
                    tabs.emplace_back();
                    build(ac[ta], &tabs.back());
                }
            }
            if (bad) break;
            if (tabs.empty()) tabs.emplace_back();   // a DC refinement: decode_scan_host wants a table to point at
            if (!area) {
                area = (int16_t*)malloc((size_t)area_blocks(f) * 64 * sizeof(int16_t));   // exactly its size
                if (!area) break;
                memset(area, 0, (size_t)area_blocks(f) * 64 * sizeof(int16_t));
            }
            const uint32_t expected = scan_intervals(f, sc);
            rst.assign(expected, 0);
            uint32_t found = 0;
            const size_t begin = i + L;
            if (!raw) {
                scan_begin = begin;
                const size_t raw_len = n - scan_begin, cap = (raw_len + 32 + 63) / 64 * 64;
                raw = (uint8_t*)aligned_alloc(64, cap);
                if (!raw) break;
                memcpy(raw, d + scan_begin, raw_len);
                memset(raw + raw_len, 0, cap - raw_len);
            }
            const size_t end = walk_scan(d, begin, n, rst.data(), expected, &found);
            if (end >= n) break;
            sc.off = 0; sc.len = (uint32_t)(end - begin);
            sc.rst_first = 0; sc.rst_count = found;
            if (decode_scan_host(f, sc, raw + (begin - scan_begin), rst.data(), tabs.data(), NAT, area)) break;
            ++scans;
            i = end;
            continue;
        }
        i += L;
    }
    if (rc == 0 && result) result->assign(area, area + (size_t)area_blocks(f) * 64);
    free(area);
    free(raw);
    return rc;
}

static bool read_file(const char* path, std::vector<uint8_t>* out)
{
    FILE* fp = fopen(path, "rb");
    if (!fp) return false;
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    out->resize(sz > 0 ? (size_t)sz : 0);
    const size_t got = sz > 0 ? fread(out->data(), 1, (size_t)sz, fp) : 0;
    fclose(fp);
    return got == out->size();
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s manifest\n", argv[0]); return 2; }
    make_nat();
    FILE* mf = fopen(argv[1], "r");
    if (!mf) return 2;
    char a[4096], b[4096];
    int mismatches = 0, files = 0, ok = 0, corrupt = 0;
    while (fscanf(mf, "%4095s %4095s", a, b) == 2) {
        std::vector<uint8_t> jpg, want;
        if (!read_file(a, &jpg)) { printf("%s unreadable\n", a); ++mismatches; continue; }
        std::vector<int16_t> got;
        const int rc = decode_file(jpg, &got);
        ++files;
        if (rc) { ++corrupt; printf("%s corrupt\n", a); if (strcmp(b, "-")) ++mismatches; continue; }
        if (strcmp(b, "-")) {
            if (!read_file(b, &want) || want.size() != got.size() * sizeof(int16_t) || memcmp(want.data(), got.data(), want.size())) {
                size_t at = 0;
                const int16_t* w = (const int16_t*)want.data();
                while (at < got.size() && at * 2 < want.size() && w[at] == got[at]) ++at;
                printf("%s MISMATCH (first difference at coefficient %zu of %zu, expected file holds %zu)\n", a, at, got.size(), want.size() / 2);
                ++mismatches;
                continue;
            }
        }
        ++ok;
        printf("%s ok\n", a);
    }
    fclose(mf);
    printf("files %d, ok %d, corrupt %d, mismatches %d\n", files, ok, corrupt, mismatches);
    return mismatches ? 1 : 0;
}
