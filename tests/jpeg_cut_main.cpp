// The walk that finishes the cut MCU of a JPEG file that ends early (meterelf_amd/csrc/melf_jpeg_cut.h), as an ordinary host program:
// tests/test_jpeg_truncated.py builds it plain and under the host sanitizers and holds its blocks against the rule restated in
// Python (tests/jpeg_cut_cases.py: program_input writes what is read here).
//
//   jpeg_cut_main CASES
//
// CASES: "bpm comp_bits dc_bits ac_bits"; four lines of 16 limits, 16 value offsets and 256 symbols (DC 0, DC 1, AC 0, AC 1); "n hex"
// the whole clean stream; then per case "bits p blk k nb pred0 pred1 pred2 limit".  Every case walks on a heap copy of exactly the
// stream's first ceil(bits / 8) bytes, so that a read behind them is an error the address sanitizer reports.
// Output per case: "case i result nb_after", then "block nb c0 .. c63" (natural order) for every block from the state's to the last
// one passed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "melf_jpeg_cut.h"

using namespace melf;

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    jpeg_cut::Layout L;
    in >> L.bpm >> L.comp_bits >> L.dc_bits >> L.ac_bits;
    std::vector<jpeg_cut::Huff> tabs(4);
    for (jpeg_cut::Huff& t : tabs) {
        for (int i = 0; i < 16; ++i) in >> t.limit[i];
        for (int i = 0; i < 16; ++i) in >> t.valoff[i];
        for (int i = 0; i < 256; ++i) { int v; in >> v; t.huffval[i] = (uint8_t)v; }
    }
    size_t n;
    std::string hex;
    in >> n >> hex;
    if (!in || L.bpm < 1 || L.bpm > 6 || (n > 0 && hex.size() != 2 * n)) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<uint8_t> stream(n);
    for (size_t i = 0; i < n; ++i) stream[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    uint8_t nat[64];   // zig-zag position -> natural index, generated (T.81 figure A.6)
    {
        int k = 0;
        for (int s = 0; s < 15; ++s)
            for (int t = 0; t <= s; ++t) {
                const int y = (s & 1) ? t : s - t, x = s - y;
                if (y < 8 && x < 8) nat[k++] = (uint8_t)(y * 8 + x);
            }
        if (k != 64) return 3;
    }
    uint32_t bits;
    jpeg_cut::State st;
    int32_t limit;
    int idx = 0;
    while (in >> bits >> st.p >> st.blk >> st.k >> st.nb >> st.pred0 >> st.pred1 >> st.pred2 >> limit) {
        const size_t nbytes = (bits + 7u) / 8u;
        if (nbytes > n || st.p > bits) { fprintf(stderr, "bad case %d\n", idx); return 2; }
        uint8_t* s = (uint8_t*)malloc(nbytes ? nbytes : 1);   // exactly the stream's bytes: nothing readable behind them
        if (nbytes) memcpy(s, stream.data(), nbytes);
        std::map<int32_t, std::vector<int>> blocks;
        const int32_t first = st.nb;
        const int res = jpeg_cut::finish(s, bits, tabs.data(), nat, L, st, limit, [&](const int32_t nb, const int at, const int v) {
            std::vector<int>& b = blocks[nb];
            if (b.empty()) b.assign(64, 0);
            b[(size_t)at] = v;
        });
        free(s);
        printf("case %d %d %d\n", idx, res, (int)st.nb);
        for (int32_t nb = first; nb < st.nb + (st.k || st.blk ? 1 : 0); ++nb) {
            printf("block %d", (int)nb);
            const auto it = blocks.find(nb);
            for (int i = 0; i < 64; ++i) printf(" %d", it == blocks.end() ? 0 : it->second[(size_t)i]);
            printf("\n");
        }
        ++idx;
    }
    printf("done %d\n", idx);
    return 0;
}
