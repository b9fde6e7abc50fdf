// Stand-alone program (its own main; compiled alone against melf_jpeg_scans.h and melf_jpeg_orient_addr.h, plain and under the host
// sanitizers): sweeps the scan plan of multi-scan sequential JPEG files over every frame size 1..70 x 1..70, every sampling the decoder
// takes (luma 1x1, 2x1, 2x2, 1x2, 4x1) and every window melf_jpeg_orient_addr.h can produce at those sizes (the whole frame; else edges
// at multiples of 16 or at the frame's edge).  It asserts, per size, sampling and window:
//   * a scan's window is never empty, lies inside the component, and holds exactly the real blocks of the MCUs k_jpeg_idct transforms
//     for the file's window (floor / ceiling in the file's own MCU): no block the IDCT reads is left undecoded, none outside is decoded;
//   * every sample a pixel the reader can use reads lies inside its component's scan window, the chroma filter's one-sample reach
//     included.  Such a pixel is one of the window that is not within the 16 pixels of margin jpeg_orient::window adds at an edge that
//     is not the frame's (the rectangle the caller reads is what the window was grown from);
//   * planar block addresses stay inside their areas: block_index < real blocks <= the area's MCU-padded size, written into a
//     buffer of exactly the file's coefficient blocks (the sanitizer build checks the stores);
//   * the three areas do not overlap and fill the file's blocks in order.
// Prints "ok <cases>" and returns 0, or the first violation and 1.
#include "melf_jpeg_orient_addr.h"
#include "melf_jpeg_scans.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace melf;

static long g_cases = 0;

static int fail(const char* what, int W, int H, int hs, int vs, int c, const jpeg_scans::Window& w)
{
    fprintf(stderr, "%s: frame %d x %d, luma %dx%d, component %d, window [%d, %d) x [%d, %d)\n", what, W, H, hs, vs, c, w.x0, w.x1, w.y0, w.y1);
    return 1;
}

// the candidates for one axis of a window: [a, b) with a a multiple of 16 below n, b a multiple of 16 or n, a < b <= n
static std::vector<std::pair<int, int>> axis_windows(const int n)
{
    std::vector<std::pair<int, int>> out;
    for (int a = 0; a < n; a += 16) {
        for (int b = a + 16; b < n; b += 16) out.push_back({a, b});
        out.push_back({a, n});
    }
    return out;
}

int main()
{
    static const int SAMP[5][2] = {{1, 1}, {2, 1}, {2, 2}, {1, 2}, {4, 1}};
    for (int H = 1; H <= 70; ++H)
        for (int W = 1; W <= 70; ++W)
            for (const auto& s : SAMP) {
                const int hs = s[0], vs = s[1];
                jpeg_scans::Comp k[3];
                uint32_t first[3], total = 0;
                for (int c = 0; c < 3; ++c) {
                    k[c] = jpeg_scans::component(W, H, hs, vs, c);
                    first[c] = jpeg_scans::area_first(W, H, hs, vs, c);
                    if (first[c] != total) return fail("areas overlap or leave a gap", W, H, hs, vs, c, {0, 0, W, H});
                    if (k[c].rbx > k[c].pbx || k[c].rby > k[c].pby || k[c].rbx < 1 || k[c].rby < 1) return fail("real grid outside the padded one", W, H, hs, vs, c, {0, 0, W, H});
                    total += (uint32_t)k[c].pbx * (uint32_t)k[c].pby;
                }
                // every planar block address, stored into a buffer of exactly the file's blocks: each block once, inside its area
                std::vector<unsigned char> area(total, 0);
                for (int c = 0; c < 3; ++c)
                    for (int by = 0; by < k[c].rby; ++by)
                        for (int bx = 0; bx < k[c].rbx; ++bx) {
                            const uint32_t i = jpeg_scans::block_index(k[c], bx, by);
                            if (i >= (uint32_t)k[c].pbx * (uint32_t)k[c].pby) return fail("block address outside its area", W, H, hs, vs, c, {bx, by, bx, by});
                            if (area[first[c] + i]++) return fail("two blocks at one address", W, H, hs, vs, c, {bx, by, bx, by});
                        }
                const int mw = 8 * hs, mh = 8 * vs;
                const int mcus_x = (W + mw - 1) / mw, mcus_y = (H + mh - 1) / mh;
                for (const auto& ax : axis_windows(W))
                    for (const auto& ay : axis_windows(H)) {
                        const jpeg_scans::Window win = {ax.first, ay.first, ax.second, ay.second};
                        // the MCUs k_jpeg_idct transforms
                        const int mx0 = win.x0 / mw, my0 = win.y0 / mh;
                        int mx1 = (win.x1 + mw - 1) / mw, my1 = (win.y1 + mh - 1) / mh;
                        if (mx1 > mcus_x) mx1 = mcus_x;
                        if (my1 > mcus_y) my1 = mcus_y;
                        // the pixels the reader can use
                        const int ux0 = win.x0 + (win.x0 > 0 ? jpeg_orient::MCU : 0), ux1 = win.x1 - (win.x1 < W ? jpeg_orient::MCU : 0);
                        const int uy0 = win.y0 + (win.y0 > 0 ? jpeg_orient::MCU : 0), uy1 = win.y1 - (win.y1 < H ? jpeg_orient::MCU : 0);
                        for (int c = 0; c < 3; ++c) {
                            ++g_cases;
                            const jpeg_scans::Window sw = jpeg_scans::scan_window(win, W, H, hs, vs, c);
                            if (sw.x0 < 0 || sw.y0 < 0 || sw.x0 >= sw.x1 || sw.y0 >= sw.y1 || sw.x0 >= k[c].w || sw.y0 >= k[c].h || sw.x1 > k[c].rbx * 8 ||
                                sw.y1 > k[c].rby * 8 || sw.x0 % 8 || sw.y0 % 8 || sw.x1 % 8 || sw.y1 % 8)
                                return fail("scan window empty, unaligned or outside the component", W, H, hs, vs, c, sw);
                            const int fx = c == 0 ? hs : 1, fy = c == 0 ? vs : 1;
                            const int bx0 = mx0 * fx, by0 = my0 * fy;
                            const int bx1 = mx1 * fx < k[c].rbx ? mx1 * fx : k[c].rbx, by1 = my1 * fy < k[c].rby ? my1 * fy : k[c].rby;
                            if (sw.x0 != bx0 * 8 || sw.x1 != bx1 * 8 || sw.y0 != by0 * 8 || sw.y1 != by1 * 8)
                                return fail("scan window is not the real blocks of the window's MCUs", W, H, hs, vs, c, sw);
                            // the samples the usable pixels read: their own, and one further each way (clamped to the component)
                            const int dx = c == 0 ? 1 : hs, dy = c == 0 ? 1 : vs;
                            if (ux0 < ux1 && uy0 < uy1) {
                                const int reach = c == 0 ? 0 : 1;
                                int sx0 = ux0 / dx - reach, sx1 = (ux1 - 1) / dx + reach, sy0 = uy0 / dy - reach, sy1 = (uy1 - 1) / dy + reach;
                                if (sx0 < 0) sx0 = 0;
                                if (sy0 < 0) sy0 = 0;
                                if (sx1 > k[c].w - 1) sx1 = k[c].w - 1;
                                if (sy1 > k[c].h - 1) sy1 = k[c].h - 1;
                                if (sx0 < sw.x0 || sx1 >= sw.x1 || sy0 < sw.y0 || sy1 >= sw.y1)
                                    return fail("a sample the reader's pixels read lies outside the scan window", W, H, hs, vs, c, sw);
                            }
                        }
                    }
            }
    // the whole frame, as jpeg_orient::window gives it without a rectangle, and a rectangle at the bottom right of a larger frame
    {
        const int rect[4] = {700, 1000, 940, 1270};
        const jpeg_orient::Window ow = jpeg_orient::window(rect, 1, 1280, 960);
        const jpeg_scans::Window cw = jpeg_scans::scan_window({ow.x0, ow.y0, ow.x1, ow.y1}, 960, 1280, 2, 2, 1);
        if (!(ow.x0 > 480 && cw.x0 < ow.x0 && cw.x0 == ow.x0 / 16 * 8 && cw.x1 <= 480 && cw.y0 == ow.y0 / 16 * 8))
            return fail("a chroma window left of the luma window's left edge", 960, 1280, 2, 2, 1, cw);
        const jpeg_orient::Window whole = jpeg_orient::window(nullptr, 1, 1280, 960);
        if (whole.x0 != 0 || whole.x1 != 960 || whole.y1 != 1280) return fail("whole-frame window", 960, 1280, 2, 2, 0, {whole.x0, whole.y0, whole.x1, whole.y1});
    }
    printf("ok %ld\n", g_cases);
    return 0;
}
