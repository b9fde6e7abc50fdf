// Stand-alone program (its own main; compiled alone against melf_jpeg_std_tables.h, plain and under the host sanitizers): prints the four
// default Huffman tables the parser installs, one per line as "<dc|ac> <id> <16 counts> : <symbols>", and checks what a DHT
// segment would have to satisfy: the counts sum to the number of symbols, the code set is neither over-subscribed nor uses the all-ones
// code (libjpeg's rule), no symbol twice, a DC table holds categories 0..15 only.  tests/test_jpeg_default_tables.py compares the
// printed tables with the ones an encoder writes.
#include "melf_jpeg_std_tables.h"

#include <cstdio>

int main()
{
    using namespace melf::jpeg_std;
    for (int cls = 0; cls < 2; ++cls)
        for (int id = 0; id < 2; ++id) {
            const Table& t = TABLES[cls][id];
            int total = 0;
            long code = 0;
            for (int l = 1; l <= 16; ++l) {
                total += t.counts[l - 1];
                code += t.counts[l - 1];
                if (code >= (1L << l)) { fprintf(stderr, "table %d %d: over-subscribed at length %d\n", cls, id, l); return 1; }
                code <<= 1;
            }
            if (total != t.nvals) { fprintf(stderr, "table %d %d: %d codes, %d symbols\n", cls, id, total, t.nvals); return 1; }
            bool seen[256] = {false};
            for (int i = 0; i < t.nvals; ++i) {
                if (seen[t.vals[i]] || (cls == 0 && t.vals[i] > 15)) { fprintf(stderr, "table %d %d: symbol %d\n", cls, id, t.vals[i]); return 1; }
                seen[t.vals[i]] = true;
            }
            printf("%s %d", cls ? "ac" : "dc", id);
            for (int l = 0; l < 16; ++l) printf(" %d", t.counts[l]);
            printf(" :");
            for (int i = 0; i < t.nvals; ++i) printf(" %d", t.vals[i]);
            printf("\n");
        }
    return 0;
}
