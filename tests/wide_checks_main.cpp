// Stand-alone host program over check_wide (meterelf_amd/csrc/melf_frame_checks.h): the descriptor check of melf_process_wide*,
// swept on the CPU.  A set of accepted descriptors -- every sample type, packed in the four pixel formats and planar in several plane
// orders, padded pitches and strides, a base with the sample's own alignment and no more --, for each of which the batch the check
// leaves is compared with the public header's addressing; and from every accepted one, one mutation per rejection the header lists,
// each of which must give exactly its message (so every rejected descriptor has an accepted neighbour that differs in what the
// message names).  Counts, through the message table, that every message was produced.  Prints `failures 0`.
#include <limits>
#include <stdio.h>
#include <stdlib.h>

#include "../meterelf_amd/csrc/melf_frame_checks.h"

using namespace melf;

static int failures = 0;
static long produced[WIDE_MSGS];
static long accepted = 0, accepted_min_aligned = 0;

static void fail_line(int line, const char* what, const char* got)
{
    if (++failures <= 20) printf("FAIL line %d: %s (%s)\n", line, what, got ? got : "accepted");
}

static void expect_reject(int line, const void* frames, const melf_wide_frames* d, int want)
{
    WideBatch wb;
    const char* msg = check_wide(frames, d, &wb);
    if (msg != WIDE_MESSAGES[want]) { fail_line(line, WIDE_MESSAGES[want], msg); return; }
    ++produced[want];
}
#define REJECT(frames, desc, want) expect_reject(__LINE__, frames, desc, want)

static melf_wide_frames make(int type, bool planar, int pix, int H, int W, int pad, int gap, int order)
{
    const int ss = narrow::sample_bytes(type), ch = planar ? 1 : pix_bytes(pix);
    melf_wide_frames d = {};
    d.sample_type = type; d.layout = planar ? MELF_WIDE_PLANAR : MELF_WIDE_PACKED; d.pixel_format = planar ? 0 : pix;
    d.shift = type == MELF_WIDE_U16 ? 2 * (order % 5) : 0; d.rounding = order & 1;
    for (int k = 0; k < 3; ++k) { d.scale[k] = 255.0f - k; d.offset[k] = 0.5f * k; }
    d.n = 3; d.H = H; d.W = W;
    d.row_pitch = (int64_t)(W * ch + pad) * ss;
    const int64_t span = (int64_t)(H - 1) * d.row_pitch + (int64_t)W * ch * ss;
    int64_t extent = span;
    if (planar) {
        static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        int64_t* off[3] = {&d.b_offset, &d.g_offset, &d.r_offset};
        for (int k = 0; k < 3; ++k) *off[k] = perm[order % 6][k] * (span + (int64_t)gap * ss);
        extent = 2 * (span + (int64_t)gap * ss) + span;
    }
    d.frame_stride = extent + (int64_t)gap * ss;
    return d;
}

static void sweep_one(const melf_wide_frames& base, const void* frames)
{
    WideBatch wb;
    const char* msg = check_wide(frames, &base, &wb);
    if (msg) { fail_line(__LINE__, "an accepted descriptor", msg); return; }
    ++accepted;
    const bool planar = base.layout == MELF_WIDE_PLANAR;
    const int ss = narrow::sample_bytes(base.sample_type), ch = planar ? 1 : pix_bytes(base.pixel_format);
    accepted_min_aligned += ((uintptr_t)frames % (2 * ss)) != 0;
    // the batch against the header's addressing, in samples
    int64_t hi = 0;
    if (planar) hi = base.b_offset > base.g_offset ? base.b_offset : base.g_offset, hi = hi > base.r_offset ? hi : base.r_offset;
    const int64_t extent = hi + (int64_t)(base.H - 1) * base.row_pitch + (int64_t)base.W * ch * ss;
    if ((int64_t)wb.b.lay.extent * ss != extent || (int64_t)wb.b.frame_stride * ss != base.frame_stride || (int64_t)wb.b.row_stride * ss != base.row_pitch ||
        wb.ss != ss || wb.b.n != base.n || wb.b.H != base.H || wb.b.W != base.W || wb.rule.channels != ch || wb.rule.type != base.sample_type ||
        wb.rule.shift != base.shift || (wb.rule.floor_ != 0) != (base.rounding == MELF_ROUND_FLOOR) ||
        wb.b.lay.pix != (planar ? PIX_PLANAR : base.pixel_format))
        fail_line(__LINE__, "the batch of an accepted descriptor", "differs from the descriptor");
    if (planar && (wb.b.lay.planes.b_off * ss != base.b_offset || wb.b.lay.planes.g_off * ss != base.g_offset || wb.b.lay.planes.r_off * ss != base.r_offset))
        fail_line(__LINE__, "the planes of an accepted descriptor", "differ from the descriptor");
    const bool rgb = !planar && (base.pixel_format == MELF_PIX_RGB || base.pixel_format == MELF_PIX_RGBA);
    for (int p = 0; p < 3; ++p)
        if (wb.rule.scale[p] != base.scale[rgb ? 2 - p : p] || wb.rule.offset[p] != base.offset[rgb ? 2 - p : p])
            fail_line(__LINE__, "scale / offset by position", "differ from the descriptor's B, G, R");

    melf_wide_frames d;
    REJECT(frames, nullptr, WIDE_DESC_NULL);
    d = base; d.sample_type = -1; REJECT(frames, &d, WIDE_TYPE);
    d = base; d.sample_type = 4; REJECT(frames, &d, WIDE_TYPE);
    d = base; d.layout = 2; REJECT(frames, &d, WIDE_LAYOUT);
    d = base; d.layout = -1; REJECT(frames, &d, WIDE_LAYOUT);
    if (!planar) {
        d = base; d.pixel_format = 4; REJECT(frames, &d, WIDE_FORMAT);
        d = base; d.pixel_format = -1; REJECT(frames, &d, WIDE_FORMAT);
    }
    d = base; d.rounding = 2; REJECT(frames, &d, WIDE_ROUNDING);
    d = base; d.shift = 9; REJECT(frames, &d, WIDE_SHIFT);
    d = base; d.shift = -1; REJECT(frames, &d, WIDE_SHIFT);
    d = base; d.reserved = 1; REJECT(frames, &d, WIDE_RESERVED);
    d = base; d.reserved2 = 1; REJECT(frames, &d, WIDE_RESERVED);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int k = 0; k < 3; ++k) {
        d = base; d.scale[k] = 16777218.0f; REJECT(frames, &d, WIDE_COEF);   // the float32 behind 2^24
        d = base; d.scale[k] = -inf; REJECT(frames, &d, WIDE_COEF);
        d = base; d.scale[k] = nan; REJECT(frames, &d, WIDE_COEF);
        d = base; d.offset[k] = inf; REJECT(frames, &d, WIDE_COEF);
        d = base; d.offset[k] = nan; REJECT(frames, &d, WIDE_COEF);
        d = base; d.scale[k] = -16777216.0f; d.offset[k] = -3.0e38f;         // the bound itself, and any finite offset, pass
        if (check_wide(frames, &d, &wb)) fail_line(__LINE__, "|scale| == 2^24 with a large finite offset", check_wide(frames, &d, &wb));
    }
    d = base; d.n = -1; REJECT(frames, &d, WIDE_SHAPE);
    d = base; d.H = 0; REJECT(frames, &d, WIDE_SHAPE);
    d = base; d.W = -3; REJECT(frames, &d, WIDE_SHAPE);
    d = base; d.n = 0;
    if (check_wide(nullptr, &d, &wb) || wb.b.n != 0) fail_line(__LINE__, "n == 0 with NULL frames", "rejected");
    if (planar) {
        d = base; d.b_offset = -(int64_t)ss; REJECT(frames, &d, WIDE_NEG_OFFSET);
        d = base; d.r_offset = INT64_MIN; REJECT(frames, &d, WIDE_NEG_OFFSET);
        d = base; d.g_offset += 1; REJECT(frames, &d, WIDE_ALIGN);
        d = base; (d.b_offset > d.g_offset && d.b_offset > d.r_offset ? d.b_offset : (d.g_offset > d.r_offset ? d.g_offset : d.r_offset)) = INT64_MAX - (ss - 1);
        REJECT(frames, &d, WIDE_OFFSET_LARGE);
        d = base; d.g_offset = d.b_offset; REJECT(frames, &d, WIDE_OVERLAP);
        d = base; d.r_offset = d.g_offset + (d.r_offset > d.g_offset ? 1 : -1) * (((int64_t)(base.H - 1) * base.row_pitch + (int64_t)base.W * ss) - ss);
        if (d.r_offset >= 0) REJECT(frames, &d, WIDE_OVERLAP);
    }
    d = base; d.row_pitch += 1; REJECT(frames, &d, WIDE_ALIGN);
    d = base; d.frame_stride += ss - 1; REJECT(frames, &d, WIDE_ALIGN);
    d = base; d.row_pitch = (int64_t)base.W * ch * ss - ss; REJECT(frames, &d, WIDE_PITCH_SMALL);
    d = base; d.row_pitch = 0; REJECT(frames, &d, WIDE_PITCH_SMALL);
    d = base; d.row_pitch = (int64_t)1 << 31; d.frame_stride = INT64_MAX & ~(int64_t)15; d.b_offset = d.g_offset = d.r_offset = 0;
    REJECT(frames, &d, WIDE_PITCH_LARGE);
    d = base; d.frame_stride = extent - ss; REJECT(frames, &d, WIDE_STRIDE_SMALL);
    d = base; d.frame_stride = 0; REJECT(frames, &d, WIDE_STRIDE_SMALL);
    REJECT(nullptr, &base, WIDE_FRAMES_NULL);
    REJECT((const uint8_t*)frames + 1, &base, WIDE_BASE);
    if (ss == 4) REJECT((const uint8_t*)frames + 2, &base, WIDE_BASE);
}

int main()
{
    alignas(64) static uint8_t memory[256];   // never read: the check looks at the pointer's value only
    const int pixes[4] = {MELF_PIX_BGR, MELF_PIX_RGB, MELF_PIX_BGRA, MELF_PIX_RGBA};
    int forms = 0;
    for (int type = MELF_WIDE_U16; type <= MELF_WIDE_F32; ++type) {
        const int ss = narrow::sample_bytes(type);
        for (int lead = 0; lead <= 1; ++lead) {            // 1: a base one sample behind a 64-byte boundary
            const void* frames = memory + 64 + lead * ss;
            for (int order = 0; order < 6; ++order)
                for (int pad = 0; pad <= 3; pad += 3)
                    for (int gap = 0; gap <= 1; ++gap) {
                        sweep_one(make(type, true, 0, 5, 7, pad, gap, order), frames);
                        sweep_one(make(type, true, 0, 1, 1, pad, gap, order), frames);
                        sweep_one(make(type, false, pixes[order % 4], 4, 9, pad, gap, order), frames);
                        forms += 3;
                    }
        }
    }
    // the ends of 32 and 64 bits
    {
        melf_wide_frames d = make(MELF_WIDE_F32, false, MELF_PIX_RGBA, 2, INT32_MAX / 16, 0, 0, 0);
        sweep_one(d, memory + 64);
        d = make(MELF_WIDE_U16, true, 0, 1 << 30, 1, 0, 0, 0);
        d.row_pitch = INT32_MAX - 1; d.b_offset = 0; d.g_offset = (int64_t)1 << 61; d.r_offset = (int64_t)1 << 62;
        d.frame_stride = INT64_MAX - 1;
        sweep_one(d, memory + 66);
    }
    printf("check_wide accepted %ld (%ld of them at a base with the sample's own alignment only), messages:\n", accepted, accepted_min_aligned);
    int seen = 0;
    for (int k = 0; k < WIDE_MSGS; ++k) {
        printf("%8ld  %s\n", produced[k], WIDE_MESSAGES[k]);
        seen += produced[k] > 0;
    }
    printf("messages %d of %d, forms %d\n", seen, (int)WIDE_MSGS, forms);
    if (seen != WIDE_MSGS || accepted == 0 || accepted_min_aligned == 0) ++failures;
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
