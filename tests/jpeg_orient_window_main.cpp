// Host sweep of meterelf_amd/csrc/melf_jpeg_orient_addr.h (tests/test_jpeg_orient.py builds and runs it, plain and under the host
// sanitizers): the window of the STORED frame that is decoded for an upright rectangle, for every orientation code, every stored size
// from 1 x 1 to 40 x 40 and every rectangle on a coarse grid of the upright frame.  The orientation table is restated here from
// include/meterelf_hip.h ("O[y][x] ="), and so is the upright window rule the decoder has always had; the header is the thing under test.
#include <algorithm>
#include <cstdio>

#include "../meterelf_amd/csrc/melf_jpeg_orient_addr.h"

using namespace melf::jpeg_orient;

// include/meterelf_hip.h: the stored pixel O[y][x] is taken from
static void stored_of(int code, int Hs, int Ws, int x, int y, int* sx, int* sy)
{
    switch (code) {
    case 1: *sy = y; *sx = x; break;
    case 2: *sy = y; *sx = Ws - 1 - x; break;
    case 3: *sy = Hs - 1 - y; *sx = Ws - 1 - x; break;
    case 4: *sy = Hs - 1 - y; *sx = x; break;
    case 5: *sy = x; *sx = y; break;
    case 6: *sy = Hs - 1 - x; *sx = y; break;
    case 7: *sy = Hs - 1 - x; *sx = Ws - 1 - y; break;
    default: *sy = x; *sx = Ws - 1 - y; break;
    }
}

static long failures = 0, cases = 0, whole = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main()
{
    for (int code = 1; code <= 8; ++code)
        for (int Hs = 1; Hs <= 40; ++Hs)
            for (int Ws = 1; Ws <= 40; ++Ws) {
                const int Hu = code >= 5 ? Ws : Hs, Wu = code >= 5 ? Hs : Ws;   // the upright frame
                // the place of every stored pixel, against the table
                for (int y = 0; y < Hu; y += 3)
                    for (int x = 0; x < Wu; x += 3) {
                        int sx, sy, ux, uy;
                        stored_of(code, Hs, Ws, x, y, &sx, &sy);
                        upright_of(code, Hs, Ws, sx, sy, &ux, &uy);
                        CHECK(ux == x && uy == y && sx >= 0 && sx < Ws && sy >= 0 && sy < Hs, "code %d %dx%d (%d,%d)", code, Hs, Ws, x, y);
                    }
                CHECK(swapped_h(code, Hu, Wu) == Hs && swapped_w(code, Hu, Wu) == Ws, "code %d sizes", code);
                const Window none = window(nullptr, code, Hs, Ws);
                CHECK(none.x0 == 0 && none.y0 == 0 && none.x1 == Ws && none.y1 == Hs, "code %d no rectangle", code);
                const int step = 5;
                for (int y0 = 0; y0 < Hu; y0 += step)
                    for (int y1 = y0 + 1; y1 <= Hu; y1 += (y1 == y0 + 1 ? step - 1 : step))
                        for (int x0 = 0; x0 < Wu; x0 += step)
                            for (int x1 = x0 + 1; x1 <= Wu; x1 += (x1 == x0 + 1 ? step - 1 : step)) {
                                const int rect[4] = {x0, y0, x1, y1};
                                const Window w = window(rect, code, Hs, Ws);
                                ++cases;
                                // 1. inside the stored frame, not empty   2. origin on a multiple of 16
                                CHECK(0 <= w.x0 && w.x0 < w.x1 && w.x1 <= Ws && 0 <= w.y0 && w.y0 < w.y1 && w.y1 <= Hs, "code %d %dx%d rect %d %d %d %d", code, Hs, Ws, x0, y0, x1, y1);
                                CHECK(w.x0 % 16 == 0 && w.y0 % 16 == 0, "code %d origin %d %d", code, w.x0, w.y0);
                                // the rectangle's stored pixels, by the table
                                int mx0 = Ws, my0 = Hs, mx1 = -1, my1 = -1;
                                for (int cy = 0; cy < 2; ++cy)
                                    for (int cx = 0; cx < 2; ++cx) {
                                        int sx, sy;
                                        stored_of(code, Hs, Ws, cx ? x1 - 1 : x0, cy ? y1 - 1 : y0, &sx, &sy);
                                        mx0 = std::min(mx0, sx); mx1 = std::max(mx1, sx); my0 = std::min(my0, sy); my1 = std::max(my1, sy);
                                    }
                                // 3. its image under the code holds the rectangle   4. ... and 16 stored pixels more on every side that is no frame edge
                                CHECK(w.x0 <= mx0 && mx1 < w.x1 && w.y0 <= my0 && my1 < w.y1, "code %d %dx%d rect %d %d %d %d not held", code, Hs, Ws, x0, y0, x1, y1);
                                CHECK(w.x0 <= std::max(0, mx0 - 16) && w.x1 >= std::min(Ws, mx1 + 1 + 16) && w.y0 <= std::max(0, my0 - 16) && w.y1 >= std::min(Hs, my1 + 1 + 16),
                                      "code %d %dx%d rect %d %d %d %d margin", code, Hs, Ws, x0, y0, x1, y1);
                                // ... and no more than the alignment asks for (a window that is the whole frame would pass all of the above)
                                CHECK(w.x0 >= mx0 - 31 && w.x1 <= mx1 + 1 + 31 && w.y0 >= my0 - 31 && w.y1 <= my1 + 1 + 31, "code %d %dx%d rect %d %d %d %d too large", code, Hs, Ws, x0, y0, x1, y1);
                                whole += (w.x0 == 0 && w.y0 == 0 && w.x1 == Ws && w.y1 == Hs) ? 1 : 0;
                                if (code == 1) {   // the upright rule, as the decoder has always had it
                                    int e[4] = {std::max(0, (rect[0] - 16) & ~15), std::max(0, (rect[1] - 16) & ~15), std::min(Ws, (rect[2] + 16 + 15) & ~15),
                                                std::min(Hs, (rect[3] + 16 + 15) & ~15)};
                                    if (e[2] <= e[0] || e[3] <= e[1]) { e[0] = e[1] = 0; e[2] = Ws; e[3] = Hs; }
                                    CHECK(w.x0 == e[0] && w.y0 == e[1] && w.x1 == e[2] && w.y1 == e[3], "code 1 %dx%d rect %d %d %d %d", Hs, Ws, x0, y0, x1, y1);
                                }
                            }
            }
    // rectangles that leave the frame or are empty: clamped, or the whole frame
    for (int code = 1; code <= 8; ++code) {
        const int Hs = 33, Ws = 21;
        const int rects[][4] = {{-50, -50, 100, 100}, {5, 5, 5, 9}, {100, 100, 120, 120}, {-40, 3, -20, 9}};
        for (const auto& r : rects) {
            const Window w = window(r, code, Hs, Ws);
            ++cases;
            CHECK(0 <= w.x0 && w.x0 < w.x1 && w.x1 <= Ws && 0 <= w.y0 && w.y0 < w.y1 && w.y1 <= Hs && w.x0 % 16 == 0 && w.y0 % 16 == 0, "code %d odd rectangle", code);
        }
    }
    printf("cases %ld, whole-frame windows %ld\n", cases, whole);
    printf("failures %ld\n", failures);
    return failures ? 1 : 0;
}
