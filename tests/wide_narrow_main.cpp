// Stand-alone host program over meterelf_amd/csrc/melf_narrow.h (the narrowing rule of melf_process_wide*) and melf_narrow_addr.h (the
// addresses of k_narrow_rows and the host packer).  Two modes; tests/test_wide_narrow.py builds it under the host sanitizers and
// runs both.
//
//   wide_narrow_main patterns <in> <out>
//       The program knows no expected value: it writes bytes, and the test compares every one of them with numpy.  <in> is a
//       sequence of sets, each a record {int32 type, int32 arg, float scale, float offset, int32 floor, int32 count}: type 0 .. 2
//       (u16, f16, bf16) means ALL 65 536 patterns of the 16-bit type (arg: the shift for u16); type 3 (f32) is followed by `count`
//       float32 values.  Every set goes through narrow::narrow_samples -- the host packer's function -- as one run of samples that
//       ends where its malloc block ends, and its bytes are appended to <out>.
//
//   wide_narrow_main bounds
//       Frames that end exactly at the end of their malloc block (and start one sample into it: a base with the sample's own
//       alignment only), narrowed through the host packer's code path, narrow::pack_item, item by item: an over-read is an
//       AddressSanitizer report.  Every staged byte is compared with the sample the public header's addressing names.  And the
//       address header swept as the kernel walks it -- waves, rows, pieces --: the samples every piece loads lie in [0, extent) and
//       are, all pieces together, exactly the crop's, each once.  Prints `failures 0`.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../meterelf_amd/csrc/melf_frame_checks.h"
#include "../meterelf_amd/csrc/melf_narrow_addr.h"

using namespace melf;

static int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                   \
    } while (0)

// ------------------------------------------------------------------------------------------------------------ patterns ---
struct Record {
    int32_t type, arg;
    float scale, offset;
    int32_t floor_, count;
};

static int patterns(const char* in_path, const char* out_path)
{
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) { printf("cannot open %s / %s\n", in_path, out_path); return 2; }
    Record rec;
    size_t sets = 0, total = 0;
    while (fread(&rec, sizeof rec, 1, in) == 1) {
        narrow::Rule rule = {};
        rule.type = rec.type; rule.shift = rec.type == MELF_WIDE_U16 ? rec.arg : 0; rule.floor_ = rec.floor_; rule.channels = 1;
        rule.scale[0] = rec.scale; rule.offset[0] = rec.offset;
        const int ss = narrow::sample_bytes(rec.type);
        const size_t count = rec.type == MELF_WIDE_F32 ? (size_t)rec.count : 65536;
        // an exact block, one sample into it: the run ends where the block ends
        uint8_t* block = (uint8_t*)malloc((count + 1) * ss);
        uint8_t* src = block + ss;
        if (rec.type == MELF_WIDE_F32) {
            if (fread(src, 4, count, in) != count) { printf("short input\n"); return 2; }
        } else {
            for (uint32_t v = 0; v < 65536; ++v) { const uint16_t s = (uint16_t)v; memcpy(src + 2 * v, &s, 2); }
        }
        std::vector<uint8_t> dst(count);
        narrow::narrow_samples(dst.data(), src, (uint32_t)count, 0, 0, rule);
        fwrite(dst.data(), 1, count, out);
        free(block);
        ++sets; total += count;
    }
    fclose(in);
    fclose(out);
    printf("patterns: %zu sets, %zu samples\nfailures 0\n", sets, total);
    return 0;
}

// -------------------------------------------------------------------------------------------------------------- bounds ---
static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// the bits of the small integer v (0 .. 63) as a sample of `type`; u16: any 10-bit value
static uint32_t sample_bits(int type, uint32_t r)
{
    if (type == MELF_WIDE_U16) return r & 1023u;
    const uint32_t v = r & 63u;
    float f = (float)v;
    uint32_t b;
    memcpy(&b, &f, 4);
    if (type == MELF_WIDE_F32) return b;
    if (type == MELF_WIDE_BF16) return b >> 16;   // exact: 6 significant bits
    if (v == 0) return 0;
    const uint32_t p = 31u - (uint32_t)__builtin_clz(v);
    return ((p + 15u) << 10) | ((v - (1u << p)) << (10u - p));
}

static uint32_t expect_byte(int type, uint32_t bits, int shift, float s, float o, bool fl)
{
    switch (type) {
    case MELF_WIDE_U16: return narrow::narrow_sample<MELF_WIDE_U16>(bits, shift, s, o, fl);
    case MELF_WIDE_F16: return narrow::narrow_sample<MELF_WIDE_F16>(bits, shift, s, o, fl);
    case MELF_WIDE_BF16: return narrow::narrow_sample<MELF_WIDE_BF16>(bits, shift, s, o, fl);
    default: return narrow::narrow_sample<MELF_WIDE_F32>(bits, shift, s, o, fl);
    }
}

static size_t n_geometries = 0, n_pieces = 0, n_samples = 0, n_tail_pieces = 0;

// one frame: layout planar / packed with pixel format pix; pad: samples a row is longer than its samples; lead: samples the frame
// starts into its block
static void one_frame(int type, bool planar, int pix, int H, int W, int pad, int lead, const int rect[4])
{
    const int ss = narrow::sample_bytes(type);
    const int ch = planar ? 1 : pix_bytes(pix);
    melf_wide_frames d = {};
    d.sample_type = type; d.layout = planar ? MELF_WIDE_PLANAR : MELF_WIDE_PACKED; d.pixel_format = planar ? 0 : pix;
    d.shift = 2; d.rounding = (W & 1) ? MELF_ROUND_FLOOR : MELF_ROUND_NEAREST;
    const float sc[3] = {1.0f, 2.0f, 3.5f}, of[3] = {0.25f, 7.0f, 20.5f};
    for (int k = 0; k < 3; ++k) { d.scale[k] = sc[k]; d.offset[k] = of[k]; }
    d.n = 1; d.H = H; d.W = W;
    d.row_pitch = (int64_t)(W * ch + pad) * ss;
    const int64_t span = (int64_t)(H - 1) * d.row_pitch + (int64_t)W * ch * ss;
    // planes in the order G, R, B, a gap of 3 samples between the first two
    if (planar) { d.g_offset = 0; d.r_offset = span + 3 * ss; d.b_offset = d.r_offset + span; }
    const int64_t extent = planar ? d.b_offset + span : span;
    d.frame_stride = extent;
    uint8_t* block = (uint8_t*)malloc((size_t)extent + (size_t)lead * ss);
    uint8_t* frame = block + (size_t)lead * ss;   // ends where the block ends
    for (int64_t i = 0; i < extent / ss; ++i) {
        const uint32_t b = sample_bits(type, rnd());
        memcpy(frame + i * ss, &b, ss);
    }
    WideBatch wb;
    const char* msg = check_wide(frame, &d, &wb);
    EXPECT(msg == nullptr, "check_wide rejects the frame: %s", msg ? msg : "");
    if (msg) { free(block); return; }
    EXPECT((int64_t)wb.b.lay.extent * ss == extent, "extent %zu samples of %d bytes, want %lld bytes", wb.b.lay.extent, ss, (long long)extent);
    Crop cr;
    EXPECT(clamp_crop(rect, H, W, &cr), "empty crop");
    const StagePlan sp = narrow::wide_plan(wb, cr);
    ++n_geometries;

    // the host packer, item by item, into a staged frame of exactly its stride
    uint8_t* staged = (uint8_t*)malloc(sp.staged.frame_stride);
    memset(staged, 0xa5, sp.staged.frame_stride);
    for (int item = 0; item < sp.items; ++item) narrow::pack_item(frame, staged, item, sp, wb.rule, ss);
    const bool rgb = !planar && (pix == MELF_PIX_RGB || pix == MELF_PIX_RGBA);
    const int64_t plane_off[3] = {d.b_offset, d.g_offset, d.r_offset};
    const bool fl = d.rounding == MELF_ROUND_FLOOR;
    for (int y = 0; y < cr.rows; ++y)
        for (int x = 0; x < cr.cols; ++x)
            for (int c = 0; c < (planar ? 3 : ch); ++c) {
                // the public header's addressing: sample c of pixel (x0 + x, y0 + y) / that pixel's sample of plane c (B, G, R)
                const int64_t at = planar ? plane_off[c] + (int64_t)(cr.y0 + y) * d.row_pitch + (int64_t)(cr.x0 + x) * ss
                                          : (int64_t)(cr.y0 + y) * d.row_pitch + ((int64_t)(cr.x0 + x) * ch + c) * ss;
                uint32_t bits = 0;
                memcpy(&bits, frame + at, ss);
                const int chan = planar ? c : (rgb ? 2 - c : c);   // 0 / 1 / 2 = B / G / R
                const uint32_t want = c == 3 ? 0u : expect_byte(type, bits, d.shift, sc[chan % 3], of[chan % 3], fl);
                // the staged frame as the 8-bit kernels read it: sp.staged's layout
                const size_t got_at = planar ? (size_t)sp.runs.run[c].dst_off + (size_t)y * sp.runs.run[c].dst_pitch + x
                                             : (size_t)y * (size_t)sp.staged.row_stride + (size_t)(sp.rect[0] + x) * ch + c;
                EXPECT(staged[got_at] == want, "type %d planar %d pix %d H %d W %d pad %d: pixel (%d, %d) sample %d: %u, want %u", type, planar, pix,
                       H, W, pad, x, y, c, staged[got_at], want);
            }
    free(staged);

    // the address header, as k_narrow_rows walks it
    const uint64_t ext = wb.b.lay.extent;
    std::vector<uint8_t> loaded(ext, 0);
    const uint32_t waves = gather::frame_waves(sp.runs);
    for (uint32_t w = 0; w < waves; ++w) {
        const gather::WaveRows wr = gather::wave_rows(sp.runs, w);
        const uint32_t ppr = gather::row_pieces(wr.run.row_bytes);
        for (uint32_t i = 0; i < ppr * wr.nrows; ++i) {
            const uint32_t r = i / ppr, piece = i - r * ppr;
            const narrow::Samples s = narrow::samples_of(wr.run, wr.row0 + r, piece);
            ++n_pieces;
            n_tail_pieces += s.count < 16;
            EXPECT(s.count >= 1 && s.count <= 16 && narrow::samples_readable(s, ext), "piece outside the frame: sample %llu + %u of %llu",
                   (unsigned long long)s.sample, s.count, (unsigned long long)ext);
            EXPECT(s.dst_off % 16 == 0 && s.dst_off + 16 <= sp.staged.frame_stride, "store outside the staged frame");
            if (!planar) EXPECT(narrow::piece_phase(piece, ch) == s.j0 % ch, "phase");
            for (uint32_t j = 0; j < s.count && s.sample + j < ext; ++j) { ++loaded[s.sample + j]; ++n_samples; }
        }
    }
    std::vector<uint8_t> want(ext, 0);
    for (int y = 0; y < cr.rows; ++y)
        for (int p = 0; p < (planar ? 3 : 1); ++p) {
            const int64_t row = (planar ? plane_off[p] / ss : 0) + (int64_t)(cr.y0 + y) * (d.row_pitch / ss) + (int64_t)cr.x0 * ch;
            for (int j = 0; j < cr.cols * ch; ++j) want[row + j] = 1;
        }
    EXPECT(loaded == want, "type %d planar %d pix %d H %d W %d pad %d: the pieces' samples are not exactly the crop's, each once", type, planar, pix, H, W, pad);
    free(block);
}

static int bounds()
{
    const int widths[5] = {1, 5, 16, 17, 250};
    const int heights[2] = {3, 35};   // 35: two work items of the packer, five waves of the kernel
    const int forms[5][2] = {{0, MELF_PIX_BGR}, {0, MELF_PIX_RGB}, {0, MELF_PIX_BGRA}, {0, MELF_PIX_RGBA}, {1, 0}};
    for (int type = MELF_WIDE_U16; type <= MELF_WIDE_F32; ++type)
        for (const auto& form : forms)
            for (const int W : widths)
                for (const int H : heights)
                    for (int pad = 0; pad <= 5; pad += 5)
                        for (int lead = 0; lead <= 1; ++lead) {
                            const int whole[4] = {0, 0, W, H};
                            const int edge[4] = {W / 3, H / 3, W + 7, H + 7};   // clamped: touches the right and the bottom edge
                            one_frame(type, form[0] != 0, form[1], H, W, pad, lead, whole);
                            one_frame(type, form[0] != 0, form[1], H, W, pad, lead, edge);
                        }
    printf("bounds: %zu frames, %zu pieces (%zu of them tails), %zu samples loaded\n", n_geometries, n_pieces, n_tail_pieces, n_samples);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "patterns")) return patterns(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "bounds")) return bounds();
    printf("usage: wide_narrow_main patterns <in> <out> | bounds\n");
    return 2;
}
