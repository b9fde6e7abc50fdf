// The JPEG header parser (meterelf_amd/csrc/melf_jpeg_parse.h) as an ordinary host program: tests/test_jpeg_parse.py builds it plain
// and under the host sanitizers and holds what it prints against tests/golden/jpeg_parse/digests.json.
//
//   jpeg_parse_main LIST              LIST: one job per line, "MODE LIMIT PATH" (LIMIT 0: the whole file)
//   jpeg_parse_main --time REPS DIR.. parse every *.jpg given REPS times with mask 0 and with all five bits; prints microseconds
//
// Every parse runs with each of the 32 valid `take` masks (the subsets of {1, 2, 4, 16, 32}) on a heap copy of exactly the bytes
// parsed, so that a read behind them is an error the address sanitizer reports.
//   whole      one line per mask: "mask rc H W orient orient_tag supported why|digest", digest = a 64-bit digest of a canonical
//              serialisation of everything else in JpegHeader; then "orientation o progressive p" (jpeg_file_orientation)
//   cuts       the same for every prefix of the file's first LIMIT bytes, folded into one digest per mask (and one of the orientations)
//   mutations  the same for every byte before the end of the first SOS header replaced in turn by 00, FF and byte ^ 01, folded alike
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "melf_jpeg_parse.h"

using namespace melf;

namespace {

// a running 64-bit digest, eight bytes a step (a multiply-and-fold of each word into the state: the sweeps make millions of these)
struct Digest {
    uint64_t h = 1469598103934665603ull;
    void num(const int64_t v)
    {
        h = (h ^ (uint64_t)v) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    void bytes(const void* p, const size_t n)
    {
        const uint8_t* b = (const uint8_t*)p;
        num((int64_t)n);
        size_t i = 0;
        for (; i + 8 <= n; i += 8) {
            uint64_t w = 0;
            for (int k = 0; k < 8; ++k) w |= (uint64_t)b[i + k] << (8 * k);
            num((int64_t)w);
        }
        uint64_t w = 0;
        for (int k = 0; i + k < n; ++k) w |= (uint64_t)b[i + k] << (8 * k);
        num((int64_t)w);
    }
};

void put_spec(Digest& f, const HuffSpec& t)
{
    f.num(t.set ? 1 : 0);
    if (!t.set) return;
    f.bytes(t.bits, 17);
    f.num(t.nvals);
    f.bytes(t.vals, (size_t)t.nvals);
}

uint64_t header_digest(const JpegHeader& h)
{
    Digest f;
    f.num(h.ncomp);
    for (int c = 0; c < 3; ++c) { f.num(h.id[c]); f.num(h.hs[c]); f.num(h.vs[c]); f.num(h.tq[c]); f.num(h.td[c]); f.num(h.ta[c]); }
    f.num(h.restart_interval);
    f.num((int64_t)h.scan_begin);
    f.num(h.saw_jfif); f.num(h.saw_adobe); f.num(h.saw_exif); f.num(h.adobe_transform); f.num(h.progressive); f.num(h.multiscan);
    for (int q = 0; q < 4; ++q) {
        f.num(h.qt_set[q] ? 1 : 0);
        if (h.qt_set[q]) for (int k = 0; k < 64; ++k) f.num(h.qt[q][k]);
    }
    for (int t = 0; t < 4; ++t) { put_spec(f, h.dc[t]); put_spec(f, h.ac[t]); }
    f.bytes(h.pscans.data(), h.pscans.size() * sizeof(h.pscans[0]));
    f.bytes(h.ptabs.data(), h.ptabs.size() * sizeof(h.ptabs[0]));
    f.bytes(h.prst.data(), h.prst.size() * sizeof(h.prst[0]));
    f.num((int64_t)h.ms.size());
    for (const JpegHeader::MScan& s : h.ms) {
        put_spec(f, s.dc); put_spec(f, s.ac);
        f.num(s.restart_interval); f.num((int64_t)s.off); f.num((int64_t)s.len);
    }
    return f.h;
}

const int BITS[5] = {1, 2, 4, 16, 32};
int mask_of(const int k)
{
    int m = 0;
    for (int b = 0; b < 5; ++b) if (k >> b & 1) m |= BITS[b];
    return m;
}

// d[0 .. n) copied to an allocation of exactly n bytes (one byte when n is 0: never read)
struct Exact {
    uint8_t* p;
    Exact(const uint8_t* d, const size_t n) : p((uint8_t*)malloc(n ? n : 1)) { if (n) memcpy(p, d, n); }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

// what one parse answers: printed in whole mode, folded into the running digests in the sweeps
struct Answer {
    int rc, H, W, orient, orient_tag, supported;
    const char* why;
    uint64_t digest;
};
Answer parse_answer(const uint8_t* d, const size_t n, const int take)
{
    JpegHeader h;
    const int rc = parse_headers(d, n, h, take);
    return {rc, h.H, h.W, h.orient, h.orient_tag, rc == 0 && !h.why ? 1 : 0, h.why ? h.why : "", header_digest(h)};
}

struct Orientation { int o, progressive, same_without_flag; };
Orientation orientation_answer(const uint8_t* d, const size_t n)
{
    int prog = -1;
    const int o = jpeg_file_orientation(d, n, &prog);
    return {o, prog, jpeg_file_orientation(d, n) == o ? 1 : 0};
}

// one variant of a file into the 33 running digests: the 32 masks' lines and the orientation's
void fold(Digest* acc, const uint8_t* d, const size_t n)
{
    const Exact e(d, n);
    for (int k = 0; k < 32; ++k) {
        const Answer a = parse_answer(e.p, n, mask_of(k));
        Digest& f = acc[k];
        f.num(a.rc); f.num(a.H); f.num(a.W); f.num(a.orient); f.num(a.orient_tag); f.num(a.supported);
        f.bytes(a.why, strlen(a.why));
        f.num((int64_t)a.digest);
    }
    const Orientation o = orientation_answer(e.p, n);
    acc[32].num(o.o); acc[32].num(o.progressive); acc[32].num(o.same_without_flag);
}

void print_folded(const Digest* acc, const size_t variants)
{
    for (int k = 0; k < 32; ++k) printf("%d %016llx\n", mask_of(k), (unsigned long long)acc[k].h);
    printf("orientation %016llx\nvariants %zu\n", (unsigned long long)acc[32].h, variants);
}

bool read_file(const std::string& path, std::vector<uint8_t>& out)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    out.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    return true;
}

// one past the header of the first SOS (the first FF DA pair), or the file's size: what lies in front of the first scan's bytes
size_t first_scan(const std::vector<uint8_t>& d)
{
    for (size_t i = 0; i + 3 < d.size(); ++i)
        if (d[i] == 0xFF && d[i + 1] == 0xDA) {
            const size_t e = i + 2 + ((size_t)d[i + 2] << 8 | d[i + 3]);
            return e < d.size() ? e : d.size();
        }
    return d.size();
}

int run_job(const std::string& mode, size_t limit, const std::vector<uint8_t>& d)
{
    if (mode == "whole") {
        const Exact e(d.data(), d.size());
        for (int k = 0; k < 32; ++k) {
            const Answer a = parse_answer(e.p, d.size(), mask_of(k));
            printf("%d %d %d %d %d %d %d %s|%016llx\n", mask_of(k), a.rc, a.H, a.W, a.orient, a.orient_tag, a.supported, a.why, (unsigned long long)a.digest);
        }
        const Orientation o = orientation_answer(e.p, d.size());
        printf("orientation %d progressive %d same-without-flag %d\n", o.o, o.progressive, o.same_without_flag);
        return 0;
    }
    Digest acc[33];
    size_t variants = 0;
    if (mode == "cuts") {
        if (limit == 0 || limit > d.size()) limit = d.size();
        for (size_t n = 0; n <= limit; ++n, ++variants) fold(acc, d.data(), n);
    } else if (mode == "mutations") {
        std::vector<uint8_t> m(d);
        const size_t end = first_scan(d);
        for (size_t i = 0; i < end; ++i) {
            const uint8_t was = d[i], with[3] = {0x00, 0xFF, (uint8_t)(was ^ 0x01)};
            for (const uint8_t v : with) {
                m[i] = v;
                fold(acc, m.data(), m.size());
                ++variants;
            }
            m[i] = was;
        }
    } else {
        return 2;
    }
    print_folded(acc, variants);
    return 0;
}

int time_files(const int reps, char** paths, const int npaths)
{
    std::vector<std::vector<uint8_t>> files((size_t)npaths);
    for (int i = 0; i < npaths; ++i)
        if (!read_file(paths[i], files[(size_t)i])) { fprintf(stderr, "cannot read %s\n", paths[i]); return 2; }
    const int masks[2] = {0, 1 | 2 | 4 | 16 | 32};
    long sink = 0;
    for (int r = 0; r < reps; ++r)
        for (const int take : masks) {
            const auto t0 = std::chrono::steady_clock::now();
            for (const std::vector<uint8_t>& f : files) {
                JpegHeader h;
                sink += parse_headers(f.data(), f.size(), h, take) + h.H;
            }
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            printf("rep %d mask %d files %d us %.1f\n", r, take, npaths, us);
        }
    printf("sink %ld\n", sink);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 4 && !strcmp(argv[1], "--time")) return time_files(atoi(argv[2]), argv + 3, argc - 3);
    if (argc != 2) { fprintf(stderr, "usage: %s LIST | --time REPS FILES\n", argv[0]); return 2; }
    std::ifstream list(argv[1]);
    if (!list) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int jobs = 0;
    while (std::getline(list, line)) {
        std::istringstream in(line);
        std::string mode, path;
        size_t limit = 0;
        if (!(in >> mode >> limit >> path)) { fprintf(stderr, "bad job line: %s\n", line.c_str()); return 2; }
        std::vector<uint8_t> d;
        if (!read_file(path, d)) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
        printf("job %d %s\n", jobs, mode.c_str());
        if (int rc = run_job(mode, limit, d)) { fprintf(stderr, "bad mode: %s\n", mode.c_str()); return rc; }
        ++jobs;
    }
    printf("done %d\n", jobs);
    return 0;
}
