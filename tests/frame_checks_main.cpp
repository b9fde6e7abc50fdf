// Stand-alone sweep of the six descriptor checks (meterelf_amd/csrc/melf_frame_checks.h: check_frames, check_yuv, check_yuv422,
// check_yuv_planar, check_yuv16, check_planes), on the CPU.  The checks decide which layouts the entry points take and compute the
// extent the kernels' bounds tests rely on; this program calls them as the library does and holds against them the addressing the
// public header documents, written out here (planes_of) and not taken from the header under test.
//
// For every ACCEPTED descriptor with n > 0 every sample of every frame is enumerated:
//   the highest byte + 1 equals (n - 1) * frame_stride + extent of the FrameBatch the check left;
//   no sample lies at a negative offset;
//   no byte of a frame belongs to two samples.  (check_yuv is excepted for I420's U against V: it tests both against the Y plane
//   and not against each other, and does not promise more.)
// For every REJECTED descriptor the one thing the message names is loosened (loosen: frame_stride raised to a frame, the chroma
// offsets moved out of the Y span, the pitch raised to a row ..) and the check is asked again, until the descriptor is taken: each
// step must clear its message and the walk must end accepted, so a rule that rejects too much shows up.
//
// Swept per family: H, W of 1, 2, 3, 4, 6; n of 0 .. 3; row, chroma, gap and stride padding of 0, 1, 2, 6 units (the family's
// alignment: 4 bytes for 4-byte pixels and packed 4:2:2, 2 for 16-bit samples, else 1); the plane orders; every format code, sub_x,
// sub_y, c_step, shift 0 / 2 / 8; base phases 0 .. 3 (crossed where the family has an alignment rule, in rotation elsewhere); the
// four matrices in rotation.  Hand-written beside the sweep (directed, edges): every message of every check from a descriptor with
// that one fault, and offsets, pitches and strides of INT32_MAX, INT32_MAX + 1, INT64_MAX - k and below zero -- no check may
// overflow on any of them under -fsanitize=undefined.  The program's own arithmetic is 128 bits wide.
// Printed per family: the accepted descriptors, the forms accepted, the count per message.  Every message must have been produced,
// every form accepted; the last line is `failures 0`.  Built and run by tests/test_frame_checks.py, plain and under
// -fsanitize=address,undefined.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "../meterelf_amd/csrc/melf_frame_checks.h"

using namespace melf;
typedef __int128 wide;

enum Fam { PACKED, YUV420, P422, YUVP, YUV16, PLANES, NFAM };
// the fields of the six public descriptors in one struct; off: U, V / B, G, R
struct Desc {
    Fam fam;
    int fmt, matrix, n, H, W, sub_x, sub_y, c_step, shift, reserved;
    int64_t pitch, c_pitch, off[3], stride;
    int phase;   // byte phase of the frames pointer; -1: NULL
    bool null_desc;
};

static const char* run_check(const Desc& d, FrameBatch* b)
{
    const void* frames = d.phase < 0 ? nullptr : (const void*)(uintptr_t)(0x1000 + d.phase);
    switch (d.fam) {
    case PACKED: {
        const melf_frames f = {d.fmt, d.n, d.H, d.W, d.pitch, d.stride};
        return check_frames(frames, d.null_desc ? nullptr : &f, b);
    }
    case YUV420: {
        const melf_yuv_frames f = {d.fmt, d.matrix, d.n, d.H, d.W, 0, d.pitch, d.c_pitch, d.off[0], d.off[1], d.stride};
        return check_yuv(frames, d.null_desc ? nullptr : &f, b);
    }
    case P422: {
        const melf_yuv422_frames f = {d.fmt, d.matrix, d.n, d.H, d.W, 0, d.pitch, d.stride};
        return check_yuv422(frames, d.null_desc ? nullptr : &f, b);
    }
    case YUVP: {
        const melf_yuv_planar_frames f = {d.matrix, d.n, d.H, d.W, d.sub_x, d.sub_y, d.c_step, d.reserved, d.pitch, d.c_pitch, d.off[0], d.off[1], d.stride};
        return check_yuv_planar(frames, d.null_desc ? nullptr : &f, b);
    }
    case YUV16: {
        const melf_yuv16_frames f = {d.matrix, d.n, d.H, d.W, d.sub_y, d.c_step, d.shift, d.reserved, d.pitch, d.c_pitch, d.off[0], d.off[1], d.stride};
        return check_yuv16(frames, d.null_desc ? nullptr : &f, b);
    }
    default: {
        const melf_planar_frames f = {d.n, d.H, d.W, d.reserved, d.off[0], d.off[1], d.off[2], d.pitch, d.stride};
        return check_planes(frames, d.null_desc ? nullptr : &f, b);
    }
    }
}

// ---- the addressing of include/meterelf_hip.h, written out: sample s of row r of a plane at frame + off + r * pitch + s * step, len bytes
struct Plane { wide off, pitch; int rows, samples, step, len; };
static int bpp_of(const Desc& d) { return d.fmt == MELF_PIX_BGRA || d.fmt == MELF_PIX_RGBA ? 4 : 3; }
static int planes_of(const Desc& d, Plane* p)
{
    switch (d.fam) {
    case PACKED: p[0] = {0, d.pitch, d.H, d.W, bpp_of(d), bpp_of(d)}; return 1;   // W pixels of 3 or 4 bytes
    case P422: p[0] = {0, d.pitch, d.H, d.W / 2, 4, 4}; return 1;                 // W / 2 macropixels of 4 bytes
    case YUV420: {   // NV12: W bytes U V U V .. per chroma row; I420: W / 2 bytes per plane
        const int cs = d.fmt == MELF_YUV_NV12 ? 2 : 1;
        p[0] = {0, d.pitch, d.H, d.W, 1, 1};
        p[1] = {d.off[0], d.c_pitch, d.H / 2, d.W / 2, cs, 1};
        p[2] = {d.off[1], d.c_pitch, d.H / 2, d.W / 2, cs, 1};
        return 3;
    }
    case YUVP:
        p[0] = {0, d.pitch, d.H, d.W, 1, 1};
        p[1] = {d.off[0], d.c_pitch, d.H >> (d.sub_y & 1), d.W >> (d.sub_x & 1), d.c_step, 1};
        p[2] = {d.off[1], d.c_pitch, d.H >> (d.sub_y & 1), d.W >> (d.sub_x & 1), d.c_step, 1};
        return 3;
    case YUV16:   // samples of 2 bytes, c_step in samples
        p[0] = {0, d.pitch, d.H, d.W, 2, 2};
        p[1] = {d.off[0], d.c_pitch, d.H >> (d.sub_y & 1), d.W >> 1, d.c_step * 2, 2};
        p[2] = {d.off[1], d.c_pitch, d.H >> (d.sub_y & 1), d.W >> 1, d.c_step * 2, 2};
        return 3;
    default:
        for (int k = 0; k < 3; ++k) p[k] = {d.off[k], d.pitch, d.H, d.W, 1, 1};
        return 3;
    }
}
// bytes from a plane's offset to the end of its last sample
static wide span_of(const Plane& p) { return (wide)(p.rows - 1) * p.pitch + (wide)(p.samples - 1) * p.step + p.len; }
static wide frame_end(const Desc& d)
{
    Plane p[3];
    const int np = planes_of(d, p);
    wide end = 0;
    for (int k = 0; k < np; ++k) end = std::max(end, p[k].off + span_of(p[k]));
    return end;
}
static int64_t align_of(const Desc& d) { return d.fam == P422 || (d.fam == PACKED && bpp_of(d) == 4) ? 4 : (d.fam == YUV16 ? 2 : 1); }
static int64_t up(int64_t v, int64_t a) { return v % a == 0 ? v : (v > INT64_MAX - a ? v - (v % a + a) % a : v + a - (v % a + a) % a); }
static int64_t down(int64_t v, int64_t a) { return v - (v % a + a) % a; }

// ---- what is counted -----------------------------------------------------------------------------------------------------------------
enum Action {
    A_DESC, A_FMT, A_MATRIX, A_SHAPE, A_PITCH, A_PITCH_LARGE, A_C_PITCH, A_STRIDE, A_FRAMES, A_ALIGN, A_BASE, A_EVEN_HW, A_EVEN_W, A_EVEN_H,
    A_HIGH, A_IN_Y, A_NV12, A_C_LARGE, A_RESERVED, A_SUB, A_C_STEP, A_SHIFT, A_NEGATIVE, A_ADJACENT, A_C_OVERLAP, A_P_LARGE, A_P_OVERLAP
};
struct Msg { const char* text; Action act; long long count; };
#define MATRIX_MSG "unknown YUV matrix (accepted: 0 BT.601 limited, 2 BT.601 full, 3 BT.709 limited, 4 BT.709 full)"
#define IN_Y_MSG "a chroma offset lies inside the Y plane's span (first to last sample): spans may not overlap"
#define C_OVERLAP_MSG "the spans (first to last sample) of the two chroma planes overlap: U and V rows sharing one pitch are not taken"
static Msg M_PACKED[] = {{"frame descriptor is NULL", A_DESC, 0}, {"unknown pixel_format", A_FMT, 0}, {"bad batch shape", A_SHAPE, 0},
                         {"row_pitch smaller than a row", A_PITCH, 0}, {"row_pitch too large", A_PITCH_LARGE, 0},
                         {"frame_stride smaller than a frame", A_STRIDE, 0}, {"frames pointer is NULL", A_FRAMES, 0},
                         {"4-byte pixel formats need a 4-byte aligned base, row_pitch and frame_stride", A_ALIGN, 0}, {nullptr, A_DESC, 0}};
static Msg M_YUV420[] = {{"YUV frame descriptor is NULL", A_DESC, 0}, {"unknown YUV format", A_FMT, 0}, {MATRIX_MSG, A_MATRIX, 0},
                         {"bad batch shape", A_SHAPE, 0}, {"YUV 4:2:0 frames need an even height and width", A_EVEN_HW, 0},
                         {"frame too high", A_HIGH, 0}, {"y_pitch smaller than a row (or too large)", A_PITCH, 0},
                         {"c_pitch smaller than a chroma row (or too large)", A_C_PITCH, 0}, {"a chroma plane overlaps the Y plane", A_IN_Y, 0},
                         {"NV12 needs v_offset == u_offset + 1 and an even u_offset", A_NV12, 0}, {"chroma offset too large", A_C_LARGE, 0},
                         {"frame_stride smaller than a frame", A_STRIDE, 0}, {"frames pointer is NULL", A_FRAMES, 0}, {nullptr, A_DESC, 0}};
static Msg M_P422[] = {{"YUV 4:2:2 frame descriptor is NULL", A_DESC, 0}, {"unknown YUV 4:2:2 format", A_FMT, 0}, {MATRIX_MSG, A_MATRIX, 0},
                       {"bad batch shape", A_SHAPE, 0}, {"YUV 4:2:2 frames need an even width", A_EVEN_W, 0},
                       {"row_pitch smaller than a row", A_PITCH, 0}, {"row_pitch too large", A_PITCH_LARGE, 0},
                       {"frame_stride smaller than a frame", A_STRIDE, 0},
                       {"YUV 4:2:2 frames need a 4-byte aligned row_pitch and frame_stride", A_ALIGN, 0}, {"frames pointer is NULL", A_FRAMES, 0},
                       {"YUV 4:2:2 frames need a 4-byte aligned base", A_BASE, 0}, {nullptr, A_DESC, 0}};
static Msg M_YUVP[] = {{"planar YUV frame descriptor is NULL", A_DESC, 0}, {"reserved field of the planar YUV frame descriptor is not 0", A_RESERVED, 0},
                       {"sub_x and sub_y must be 0 or 1 (log2 of the chroma subsampling)", A_SUB, 0},
                       {"c_step must be 1 (planar) or 2 (semi-planar)", A_C_STEP, 0}, {MATRIX_MSG, A_MATRIX, 0}, {"bad batch shape", A_SHAPE, 0},
                       {"horizontally subsampled chroma (sub_x) needs an even width", A_EVEN_W, 0},
                       {"vertically subsampled chroma (sub_y) needs an even height", A_EVEN_H, 0}, {"negative chroma offset", A_NEGATIVE, 0},
                       {"c_step 2 (semi-planar) needs adjacent u_offset and v_offset", A_ADJACENT, 0},
                       {"y_pitch smaller than a row (or too large)", A_PITCH, 0}, {"c_pitch smaller than a chroma row (or too large)", A_C_PITCH, 0},
                       {"chroma offset too large", A_C_LARGE, 0}, {IN_Y_MSG, A_IN_Y, 0}, {C_OVERLAP_MSG, A_C_OVERLAP, 0},
                       {"frame_stride smaller than a frame", A_STRIDE, 0}, {"frames pointer is NULL", A_FRAMES, 0}, {nullptr, A_DESC, 0}};
static Msg M_YUV16[] = {{"16-bit YUV frame descriptor is NULL", A_DESC, 0}, {"reserved field of the 16-bit YUV frame descriptor is not 0", A_RESERVED, 0},
                        {"sub_y must be 0 or 1 (log2 of the vertical chroma subsampling)", A_SUB, 0},
                        {"c_step must be 1 (planar) or 2 (semi-planar) samples", A_C_STEP, 0},
                        {"shift must be 0 .. 8 (low bits dropped from a 16-bit sample)", A_SHIFT, 0}, {MATRIX_MSG, A_MATRIX, 0},
                        {"bad batch shape", A_SHAPE, 0}, {"horizontally subsampled chroma needs an even width", A_EVEN_W, 0},
                        {"vertically subsampled chroma (sub_y) needs an even height", A_EVEN_H, 0}, {"negative chroma offset", A_NEGATIVE, 0},
                        {"16-bit samples need an even y_pitch, c_pitch, u_offset, v_offset and frame_stride (bytes)", A_ALIGN, 0},
                        {"c_step 2 (semi-planar) needs u_offset and v_offset 2 bytes apart", A_ADJACENT, 0},
                        {"y_pitch smaller than a row of 2-byte samples (or too large)", A_PITCH, 0},
                        {"c_pitch smaller than a chroma row of 2-byte samples (or too large)", A_C_PITCH, 0}, {"chroma offset too large", A_C_LARGE, 0},
                        {IN_Y_MSG, A_IN_Y, 0}, {C_OVERLAP_MSG, A_C_OVERLAP, 0}, {"frame_stride smaller than a frame", A_STRIDE, 0},
                        {"frames pointer is NULL", A_FRAMES, 0}, {"16-bit samples need a 2-byte aligned base", A_BASE, 0}, {nullptr, A_DESC, 0}};
static Msg M_PLANES[] = {{"planar frame descriptor is NULL", A_DESC, 0}, {"bad batch shape", A_SHAPE, 0},
                         {"reserved field of the planar frame descriptor is not 0", A_RESERVED, 0}, {"negative plane offset", A_NEGATIVE, 0},
                         {"row_pitch smaller than a row", A_PITCH, 0}, {"row_pitch too large", A_PITCH_LARGE, 0},
                         {"plane offset too large", A_P_LARGE, 0}, {"two planes overlap", A_P_OVERLAP, 0},
                         {"frame_stride smaller than a frame", A_STRIDE, 0}, {"frames pointer is NULL", A_FRAMES, 0}, {nullptr, A_DESC, 0}};
struct Family {
    const char* name;
    Msg* msgs;
    int nforms;   // format codes / (sub_x, sub_y, c_step) / (sub_y, c_step, shift 0, 2, 8) forms the sweep must see accepted
    long long accepted, no_neighbour;
    std::set<int> forms;
};
static Family g_fam[NFAM] = {{"check_frames", M_PACKED, 4, 0, 0, {}},  {"check_yuv", M_YUV420, 3, 0, 0, {}},       {"check_yuv422", M_P422, 3, 0, 0, {}},
                             {"check_yuv_planar", M_YUVP, 16, 0, 0, {}}, {"check_yuv16", M_YUV16, 24, 0, 0, {}}, {"check_planes", M_PLANES, 6, 0, 0, {}}};
static long long g_fail = 0, g_checked = 0, g_wraps = 0;

static void say(const Desc& d, const char* what, const char* msg)
{
    if (g_fail++ < 20)
        fprintf(stderr, "%s: %s%s%s (fmt %d n %d H %d W %d sub %d %d c_step %d pitch %lld c_pitch %lld off %lld %lld %lld stride %lld phase %d)\n",
                g_fam[d.fam].name, what, msg ? ": " : "", msg ? msg : "", d.fmt, d.n, d.H, d.W, d.sub_x, d.sub_y, d.c_step, (long long)d.pitch,
                (long long)d.c_pitch, (long long)d.off[0], (long long)d.off[1], (long long)d.off[2], (long long)d.stride, d.phase);
}
static int form_of(const Desc& d)
{
    const bool vfirst = d.off[1] < d.off[0];
    switch (d.fam) {
    case YUV420: return d.fmt == MELF_YUV_NV12 ? 0 : (vfirst ? 2 : 1);   // NV12, I420, YV12
    case YUVP: return ((d.sub_x * 2 + d.sub_y) * 2 + d.c_step - 1) * 2 + vfirst;
    case YUV16: return d.shift != 0 && d.shift != 2 && d.shift != 8 ? -1 : ((d.sub_y * 2 + d.c_step - 1) * 2 + vfirst) * 3 + (d.shift == 0 ? 0 : (d.shift == 2 ? 1 : 2));
    case PLANES: return (d.off[0] < d.off[1]) * 4 + (d.off[1] < d.off[2]) * 2 + (d.off[0] < d.off[2]);   // the six orders
    default: return d.fmt;
    }
}

// ---- an accepted descriptor: every sample of every frame -------------------------------------------------------------------------------
static std::vector<std::pair<wide, int>> g_bytes;
static void verify(const Desc& d, const FrameBatch& b)
{
    if (b.n != d.n || b.H != d.H || b.W != d.W || (wide)b.frame_stride != d.stride || b.row_stride != d.pitch) say(d, "the batch is not the descriptor's", nullptr);
    if (d.n == 0) return;
    Plane p[3];
    const int np = planes_of(d, p);
    wide lo = 0, hi = 0;
    g_bytes.clear();
    for (int f = 0; f < d.n; ++f)
        for (int k = 0; k < np; ++k)
            for (int r = 0; r < p[k].rows; ++r)
                for (int s = 0; s < p[k].samples; ++s) {
                    const wide at = (wide)f * d.stride + p[k].off + (wide)r * p[k].pitch + (wide)s * p[k].step;
                    lo = std::min(lo, at);
                    hi = std::max(hi, at + p[k].len);
                    if (f == 0)
                        for (int j = 0; j < p[k].len; ++j) g_bytes.push_back({at + j, k});
                }
    ++g_checked;
    const wide readable = (wide)(d.n - 1) * (wide)b.frame_stride + (wide)b.lay.extent;
    if (hi != readable) say(d, "the highest byte + 1 is not (n - 1) * frame_stride + extent", nullptr);
    if (lo < 0) say(d, "a sample lies before the base", nullptr);
    if (readable >> 64) ++g_wraps;   // (not a failure: the entry points compute it as size_t)
    std::sort(g_bytes.begin(), g_bytes.end());
    for (size_t i = 1; i < g_bytes.size(); ++i)
        if (g_bytes[i].first == g_bytes[i - 1].first) {
            // check_yuv does not test I420's U span against its V span: not promised, not asserted
            if (d.fam == YUV420 && d.fmt == MELF_YUV_I420 && g_bytes[i].second + g_bytes[i - 1].second == 3) continue;
            say(d, "two samples share a byte", nullptr);
            break;
        }
}

// ---- a rejected descriptor: the one thing the message names, loosened; false: there is no such neighbour --------------------------------
static bool loosen(Desc& d, Action act)
{
    const int64_t a = align_of(d);
    Plane p[3] = {};
    planes_of(d, p);
    const wide y_end = span_of(p[0]), c_len = span_of(p[1]);
    const int lo = d.off[0] < d.off[1] ? 0 : 1, hi = 1 - lo;
    const bool semi = (d.fam == YUV420 && d.fmt == MELF_YUV_NV12) || ((d.fam == YUVP || d.fam == YUV16) && d.c_step == 2);
    const int64_t bps = d.fam == YUV16 ? 2 : 1;
    switch (act) {
    case A_DESC: d.null_desc = false; return true;
    case A_FMT: d.fmt = 0; return true;
    case A_MATRIX: d.matrix = 0; return true;
    case A_RESERVED: d.reserved = 0; return true;
    case A_SHIFT: d.shift = 8; return true;
    case A_C_STEP: d.c_step = 1; return true;
    case A_SUB:
        if (d.sub_x != 0 && d.sub_x != 1) d.sub_x = 0;
        if (d.sub_y != 0 && d.sub_y != 1) d.sub_y = 0;
        return true;
    case A_SHAPE:
        if (d.n < 0) d.n = 0;
        if (d.H <= 0) d.H = 2;
        if (d.W <= 0) d.W = 2;
        return true;
    case A_FRAMES: case A_BASE: d.phase = 0; return true;
    case A_EVEN_HW: case A_EVEN_W: case A_EVEN_H:   // a pixel less: the planes shrink inside their pitches (of one pixel: one more)
        if (act != A_EVEN_H && d.W & 1) d.W += d.W == 1 ? 1 : -1;
        if (act != A_EVEN_W && d.H & 1) d.H += d.H == 1 ? 1 : -1;
        return true;
    case A_HIGH: d.H = 131070; return true;
    case A_PITCH: case A_PITCH_LARGE: {   // raised to a row, or lowered to the largest pitch
        const int64_t row = (int64_t)(p[0].samples - 1) * p[0].step + p[0].len;
        d.pitch = d.pitch > INT32_MAX ? down(INT32_MAX, a) : up(row, a);
        return true;
    }
    case A_C_PITCH: {   // a chroma row: of both planes' samples where they are interleaved
        const int64_t row = (int64_t)p[1].samples * p[1].step;
        d.c_pitch = d.c_pitch > INT32_MAX ? down(INT32_MAX, a) : up(row, a);
        return true;
    }
    case A_STRIDE: {   // raised to a frame
        const wide end = frame_end(d);
        if (end > INT64_MAX) return false;
        d.stride = up((int64_t)end, a);
        return true;
    }
    case A_ALIGN:
        if (d.fam != YUV16) {
            if (d.fam == PACKED) d.phase = 0;
        } else {
            d.c_pitch = up(d.c_pitch, a); d.off[0] = up(d.off[0], a); d.off[1] = up(d.off[1], a);
        }
        d.pitch = up(d.pitch, a); d.stride = up(d.stride, a);
        return true;
    case A_NEGATIVE:
        for (int k = 0; k < 3; ++k)
            if (d.off[k] < 0) d.off[k] = 0;
        return true;
    case A_IN_Y: {   // both chroma offsets moved up by what the lower one lacks
        wide delta = y_end - d.off[lo];
        if (d.fam == YUV420 && semi) delta += delta & 1;
        if (d.off[hi] + delta > INT64_MAX) return false;
        d.off[0] = (int64_t)(d.off[0] + delta); d.off[1] = (int64_t)(d.off[1] + delta);
        return true;
    }
    case A_NV12: d.off[0] = up(d.off[0], 2); d.off[1] = d.off[0] + 1; return true;
    case A_ADJACENT:
        if (d.off[lo] > INT64_MAX - bps) d.off[lo] = d.off[hi] - bps; else d.off[hi] = d.off[lo] + bps;
        return true;
    case A_C_OVERLAP:
        if (d.off[lo] + c_len > INT64_MAX) return false;
        d.off[hi] = (int64_t)(d.off[lo] + c_len);
        return true;
    case A_C_LARGE: {   // the higher offset (a pair: both) moved down to the last place where the plane's end is a number
        int64_t to = down((int64_t)(INT64_MAX - c_len), a);
        if (d.fam == YUV420 && semi) to -= !(to & 1);   // NV12: the higher is V, one behind an even U
        const int64_t delta = d.off[hi] - to;
        d.off[hi] = to;
        if (semi) d.off[lo] -= delta;
        return true;
    }
    case A_P_LARGE:
        for (int k = 0; k < 3; ++k)
            if (d.off[k] > INT64_MAX - y_end) d.off[k] = (int64_t)(INT64_MAX - y_end);
        return true;
    case A_P_OVERLAP: {   // the planes in their order, a span apart where they were closer
        int idx[3] = {0, 1, 2};
        std::sort(idx, idx + 3, [&](int x, int y) { return d.off[x] < d.off[y]; });
        for (int k = 1; k < 3; ++k)
            if (d.off[idx[k]] - d.off[idx[k - 1]] < y_end) {
                if (d.off[idx[k - 1]] + y_end > INT64_MAX) return false;
                d.off[idx[k]] = (int64_t)(d.off[idx[k - 1]] + y_end);
            }
        return true;
    }
    }
    return false;
}

static Msg* find(Family& F, const char* text)
{
    for (Msg* m = F.msgs; m->text; ++m)
        if (!strcmp(m->text, text)) return m;
    return nullptr;
}
// One descriptor: counted, verified if accepted, walked to an accepted neighbour if not.  want: the message it must give ("" accepted),
// NULL: whatever the check says.
static void visit(Desc d, const char* want = nullptr)
{
    Family& F = g_fam[d.fam];
    FrameBatch b;
    const char* msg = run_check(d, &b);
    if (want && strcmp(want, msg ? msg : "")) say(d, "expected another answer", msg ? msg : "accepted");
    if (!msg) {
        ++F.accepted;
        if (form_of(d) >= 0) F.forms.insert(form_of(d));
        verify(d, b);
        return;
    }
    Msg* m = find(F, msg);
    if (!m) { say(d, "a message this program does not know", msg); return; }
    ++m->count;
    for (int step = 0; step < 12; ++step) {
        if (!loosen(d, m->act)) { ++F.no_neighbour; return; }
        const char* next = run_check(d, &b);
        if (!next) { verify(d, b); return; }
        if (!strcmp(next, msg)) { say(d, "loosening what the message names does not clear it", msg); return; }
        msg = next;
        m = find(F, msg);
        if (!m) { say(d, "a message this program does not know", msg); return; }
    }
    say(d, "no accepted neighbour after twelve steps", msg);
}

// ---- the frames of the sweep: the planes in their order, `gap` between their spans, the pitches and the stride padded -------------------------
static const int MATRICES[4] = {MELF_YUV_BT601_LIMITED, MELF_YUV_BT601_FULL, MELF_YUV_BT709_LIMITED, MELF_YUV_BT709_FULL};
static unsigned g_turn = 0;
static Desc blank(Fam fam, int n, int H, int W)
{
    Desc d;
    memset(&d, 0, sizeof d);
    d.fam = fam; d.n = n; d.H = H; d.W = W;
    d.matrix = MATRICES[++g_turn & 3];
    d.c_step = 1; d.shift = 8;
    d.phase = (int)(g_turn >> 2 & 3) * (int)align_of(d);   // (a rule on the phase: the caller sets it)
    return d;
}
static Desc one_plane(Fam fam, int fmt, int n, int H, int W, int pad, int spad, int phase)
{
    Desc d = blank(fam, n, H, W);
    d.fmt = fmt; d.phase = phase;
    const int64_t a = align_of(d);
    d.pitch = (fam == P422 ? 2 : bpp_of(d)) * (int64_t)W + pad * a;
    Plane p[1];
    planes_of(d, p);
    d.stride = (int64_t)span_of(p[0]) + spad * a;
    return d;
}
static Desc yuv_frames(Fam fam, int fmt, int sub_x, int sub_y, int c_step, int shift, bool vfirst, int n, int H, int W, int pad, int cpad, int gap, int spad)
{
    Desc d = blank(fam, n, H, W);
    d.fmt = fmt; d.sub_x = sub_x; d.sub_y = sub_y; d.c_step = c_step; d.shift = shift;
    const int64_t a = align_of(d);
    if (fam == YUV16) d.phase = (int)(g_turn >> 2 & 3);   // odd phases: the base rule
    Plane p[3];
    planes_of(d, p);
    d.pitch = (int64_t)W * p[0].len + pad * a;
    const bool semi = p[1].step != p[1].len;
    d.c_pitch = (int64_t)p[1].samples * p[1].step + cpad * a;   // a chroma row: of both planes' samples where they are interleaved
    planes_of(d, p);
    const int64_t lo = (int64_t)span_of(p[0]) + gap * a, hi = semi ? lo + p[1].len : lo + (int64_t)span_of(p[1]) + gap * a;
    d.off[0] = vfirst ? hi : lo; d.off[1] = vfirst ? lo : hi;
    d.stride = hi + (int64_t)span_of(p[1]) + spad * a;
    return d;
}
static Desc rgb_planes(int order, int n, int H, int W, int pad, int gap, int spad)
{
    static const int orders[6][3] = {{0, 1, 2}, {2, 1, 0}, {1, 2, 0}, {0, 2, 1}, {1, 0, 2}, {2, 0, 1}};
    Desc d = blank(PLANES, n, H, W);
    d.pitch = W + pad;
    Plane p[3];
    planes_of(d, p);
    const int64_t span = (int64_t)span_of(p[0]);
    for (int k = 0; k < 3; ++k) d.off[k] = orders[order][k] * (span + gap);
    d.stride = 3 * span + 2 * gap + spad;
    return d;
}

static void sweep()
{
    const int sizes[5] = {1, 2, 3, 4, 6}, pads[4] = {0, 1, 2, 6}, shifts[3] = {0, 2, 8};
    for (int hi = 0; hi < 5; ++hi)
        for (int wi = 0; wi < 5; ++wi)
            for (int n = 0; n < 4; ++n)
                for (int pi = 0; pi < 4; ++pi)
                    for (int si = 0; si < 4; ++si) {
                        const int H = sizes[hi], W = sizes[wi], pad = pads[pi], spad = pads[si];
                        for (int ph = 0; ph < 4; ++ph) {
                            for (int fmt = 0; fmt < 4; ++fmt) visit(one_plane(PACKED, fmt, n, H, W, pad, spad, ph));
                            for (int fmt = 0; fmt < 3; ++fmt) visit(one_plane(P422, fmt, n, H, W, pad, spad, ph));
                        }
                        for (int gi = 0; gi < 4; ++gi) {
                            for (int order = 0; order < 6; ++order) visit(rgb_planes(order, n, H, W, pad, pads[gi], spad));
                            for (int ci = 0; ci < 4; ++ci)
                                for (int vfirst = 0; vfirst < 2; ++vfirst) {
                                    const int cpad = pads[ci], gap = pads[gi];
                                    visit(yuv_frames(YUV420, MELF_YUV_NV12, 1, 1, 2, 0, vfirst, n, H, W, pad, cpad, gap, spad));
                                    visit(yuv_frames(YUV420, MELF_YUV_I420, 1, 1, 1, 0, vfirst, n, H, W, pad, cpad, gap, spad));
                                    for (int form = 0; form < 8; ++form)
                                        visit(yuv_frames(YUVP, 0, form >> 2, form >> 1 & 1, 1 + (form & 1), 0, vfirst, n, H, W, pad, cpad, gap, spad));
                                    if (pad == 1 || cpad == 1 || gap == 1 || spad == 1) continue;   // 16-bit: paddings of 0, 2, 6 samples' bytes
                                    for (int form = 0; form < 4; ++form)
                                        visit(yuv_frames(YUV16, 0, 1, form >> 1, 1 + (form & 1), shifts[(n + ci + gi + form) % 3], vfirst, n, H, W, pad / 2 + (pad == 6),
                                                         cpad / 2 + (cpad == 6), gap / 2 + (gap == 6), spad / 2 + (spad == 6)));
                                }
                        }
                    }
}

// ---- by hand: every message from a descriptor with that one fault --------------------------------------------------------------------------
static Desc base_of(Fam fam, int variant = 0)
{
    switch (fam) {
    case PACKED: return one_plane(PACKED, variant ? MELF_PIX_BGRA : MELF_PIX_BGR, 2, 4, 4, 1, 1, 0);
    case P422: return one_plane(P422, MELF_YUV422_UYVY, 2, 4, 4, 1, 1, 0);
    case YUV420: return yuv_frames(YUV420, variant ? MELF_YUV_I420 : MELF_YUV_NV12, 1, 1, variant ? 1 : 2, 0, false, 2, 4, 4, 2, 2, 2, 2);
    case YUVP: return yuv_frames(YUVP, 0, 1, 1, variant ? 1 : 2, 0, false, 2, 4, 4, 2, 2, 2, 2);
    case YUV16: { Desc d = yuv_frames(YUV16, 0, 1, 1, variant ? 1 : 2, 2, false, 2, 4, 4, 1, 1, 1, 1); d.phase = 0; return d; }
    default: return rgb_planes(0, 2, 4, 4, 2, 2, 2);
    }
}
template <class Edit>
static void directed(Fam fam, int variant, const char* want, const Edit& edit)
{
    Desc d = base_of(fam, variant);
    edit(d);
    visit(d, want);
}
static void by_hand()
{
    for (int fam = 0; fam < NFAM; ++fam)
        for (int variant = 0; variant < 2; ++variant) {
            const Fam f = (Fam)fam;
            directed(f, variant, "", [](Desc&) {});
            directed(f, variant, "", [](Desc& d) { d.n = 0; d.phase = -1; });   // n == 0 passes whatever the frames pointer
            directed(f, variant, g_fam[fam].msgs[0].text, [](Desc& d) { d.null_desc = true; });
            directed(f, variant, "frames pointer is NULL", [](Desc& d) { d.phase = -1; });
            directed(f, variant, "bad batch shape", [](Desc& d) { d.n = -1; });
            directed(f, variant, "bad batch shape", [](Desc& d) { d.H = 0; });
            directed(f, variant, "bad batch shape", [](Desc& d) { d.W = -2; });
            directed(f, variant, "frame_stride smaller than a frame", [](Desc& d) { d.stride = (int64_t)frame_end(d) - align_of(d); });
            directed(f, variant, "", [](Desc& d) { d.stride = (int64_t)frame_end(d); });
            if (f != PACKED && f != PLANES)
                for (int code = -1; code <= 5; ++code)
                    directed(f, variant, code == 0 || (code >= 2 && code <= 4) ? "" : MATRIX_MSG, [&](Desc& d) { d.matrix = code; });
            if (f == YUVP || f == YUV16 || f == PLANES) directed(f, variant, g_fam[fam].msgs[f == PLANES ? 2 : 1].text, [](Desc& d) { d.reserved = 1; });
        }
    // packed pixels
    directed(PACKED, 0, "unknown pixel_format", [](Desc& d) { d.fmt = 4; });
    directed(PACKED, 0, "unknown pixel_format", [](Desc& d) { d.fmt = -1; });
    directed(PACKED, 0, "row_pitch smaller than a row", [](Desc& d) { d.pitch = d.W * 3 - 1; });
    directed(PACKED, 0, "", [](Desc& d) { d.pitch = d.W * 3; });
    directed(PACKED, 1, "row_pitch smaller than a row", [](Desc& d) { d.pitch = d.W * 4 - 4; });
    directed(PACKED, 0, "row_pitch too large", [](Desc& d) { d.pitch = (int64_t)INT32_MAX + 1; d.stride = INT64_MAX; });
    const char* const al4 = "4-byte pixel formats need a 4-byte aligned base, row_pitch and frame_stride";
    for (int k = 1; k < 4; ++k) {
        directed(PACKED, 1, al4, [&](Desc& d) { d.phase = k; });
        directed(PACKED, 1, al4, [&](Desc& d) { d.pitch += k; d.stride += 4 * d.H; });
        directed(PACKED, 1, al4, [&](Desc& d) { d.stride += k; });
        directed(PACKED, 0, "", [&](Desc& d) { d.phase = k; d.stride += k; });
    }
    // packed 4:2:2
    directed(P422, 0, "unknown YUV 4:2:2 format", [](Desc& d) { d.fmt = 3; });
    directed(P422, 0, "YUV 4:2:2 frames need an even width", [](Desc& d) { d.W = 3; });
    directed(P422, 0, "row_pitch smaller than a row", [](Desc& d) { d.pitch = d.W * 2 - 4; });
    directed(P422, 0, "row_pitch too large", [](Desc& d) { d.pitch = (int64_t)INT32_MAX + 1; d.stride = INT64_MAX - 3; });
    for (int k = 1; k < 4; ++k) {
        directed(P422, 0, "YUV 4:2:2 frames need a 4-byte aligned base", [&](Desc& d) { d.phase = k; });
        directed(P422, 0, "YUV 4:2:2 frames need a 4-byte aligned row_pitch and frame_stride", [&](Desc& d) { d.pitch += k; d.stride += 4 * d.H; });
        directed(P422, 0, "YUV 4:2:2 frames need a 4-byte aligned row_pitch and frame_stride", [&](Desc& d) { d.stride += k; });
    }
    // 4:2:0: its own rules
    directed(YUV420, 0, "unknown YUV format", [](Desc& d) { d.fmt = 2; });
    directed(YUV420, 0, "YUV 4:2:0 frames need an even height and width", [](Desc& d) { d.H = 3; });
    directed(YUV420, 1, "YUV 4:2:0 frames need an even height and width", [](Desc& d) { d.W = 3; });
    directed(YUV420, 0, "frame too high", [](Desc& d) { d = yuv_frames(YUV420, MELF_YUV_NV12, 1, 1, 2, 0, false, 1, 131072, 2, 0, 0, 0, 0); });
    directed(YUV420, 0, "", [](Desc& d) { d = yuv_frames(YUV420, MELF_YUV_NV12, 1, 1, 2, 0, false, 1, 131070, 2, 0, 0, 0, 0); });
    for (int variant = 0; variant < 2; ++variant) {
        directed(YUV420, variant, "y_pitch smaller than a row (or too large)", [](Desc& d) { d.pitch = d.W - 1; });
        directed(YUV420, variant, "y_pitch smaller than a row (or too large)", [](Desc& d) { d.pitch = (int64_t)INT32_MAX + 1; });
        directed(YUV420, variant, "c_pitch smaller than a chroma row (or too large)", [&](Desc& d) { d.c_pitch = (variant ? d.W / 2 : d.W) - 1; });
        directed(YUV420, variant, "", [&](Desc& d) { d.c_pitch = variant ? d.W / 2 : d.W; });
        directed(YUV420, variant, "c_pitch smaller than a chroma row (or too large)", [](Desc& d) { d.c_pitch = (int64_t)INT32_MAX + 1; });
        directed(YUV420, variant, "a chroma plane overlaps the Y plane", [](Desc& d) { d.off[0] -= 4; d.off[1] -= 4; });
        directed(YUV420, variant, "a chroma plane overlaps the Y plane", [](Desc& d) { d.off[0] = -2; d.off[1] = -1; });
    }
    directed(YUV420, 1, "a chroma plane overlaps the Y plane", [](Desc& d) { d.off[1] = d.off[0]; d.off[0] = 3 * d.pitch + d.W - 1; });
    directed(YUV420, 0, "NV12 needs v_offset == u_offset + 1 and an even u_offset", [](Desc& d) { d.off[0] += 1; d.off[1] += 1; d.stride += 1; });
    directed(YUV420, 0, "NV12 needs v_offset == u_offset + 1 and an even u_offset", [](Desc& d) { std::swap(d.off[0], d.off[1]); });
    directed(YUV420, 0, "NV12 needs v_offset == u_offset + 1 and an even u_offset", [](Desc& d) { d.off[1] += 1; });
    directed(YUV420, 0, "NV12 needs v_offset == u_offset + 1 and an even u_offset", [](Desc& d) { d.off[0] = INT64_MAX - 1; d.off[1] = 40; });
    directed(YUV420, 1, "", [](Desc& d) { d.off[1] = d.off[0]; });   // I420's U and V are not held against each other: taken
    // the descriptor of the issue: I420 2 frames of 4 x 4, u_offset INT64_MAX - 3
    directed(YUV420, 1, "chroma offset too large", [](Desc& d) { d.pitch = 4; d.c_pitch = 2; d.off[0] = INT64_MAX - 3; d.off[1] = 16; d.stride = 24; d.matrix = 0; });
    directed(YUV420, 1, "chroma offset too large", [](Desc& d) { d.off[1] = INT64_MAX; d.stride = INT64_MAX; });
    directed(YUV420, 0, "chroma offset too large", [](Desc& d) { d.off[0] = INT64_MAX - 1; d.off[1] = INT64_MAX; d.stride = INT64_MAX; });
    // planar YUV, 8 and 16 bits: the shared span rules, and each one's own
    for (int fam = YUVP; fam <= YUV16; ++fam) {
        const Fam f = (Fam)fam;
        const int64_t bps = f == YUV16 ? 2 : 1;
        const char* const ypm = f == YUV16 ? "y_pitch smaller than a row of 2-byte samples (or too large)" : "y_pitch smaller than a row (or too large)";
        const char* const cpm = f == YUV16 ? "c_pitch smaller than a chroma row of 2-byte samples (or too large)" : "c_pitch smaller than a chroma row (or too large)";
        for (int variant = 0; variant < 2; ++variant) {
            directed(f, variant, f == YUV16 ? "c_step must be 1 (planar) or 2 (semi-planar) samples" : "c_step must be 1 (planar) or 2 (semi-planar)", [](Desc& d) { d.c_step = 3; });
            directed(f, variant, f == YUV16 ? "c_step must be 1 (planar) or 2 (semi-planar) samples" : "c_step must be 1 (planar) or 2 (semi-planar)", [](Desc& d) { d.c_step = 0; });
            directed(f, variant, f == YUV16 ? "sub_y must be 0 or 1 (log2 of the vertical chroma subsampling)" : "sub_x and sub_y must be 0 or 1 (log2 of the chroma subsampling)", [](Desc& d) { d.sub_y = 2; });
            directed(f, variant, f == YUV16 ? "horizontally subsampled chroma needs an even width" : "horizontally subsampled chroma (sub_x) needs an even width", [](Desc& d) { d.W = 3; });
            directed(f, variant, "vertically subsampled chroma (sub_y) needs an even height", [](Desc& d) { d.H = 3; });
            directed(f, variant, "negative chroma offset", [&](Desc& d) { d.off[0] = -2 * bps; d.off[1] = -bps; });
            directed(f, variant, "negative chroma offset", [](Desc& d) { d.off[1] = INT64_MIN; });
            directed(f, variant, ypm, [&](Desc& d) { d.pitch = d.W * bps - bps; });
            directed(f, variant, ypm, [](Desc& d) { d.pitch = (int64_t)INT32_MAX + 1; });
            directed(f, variant, cpm, [&](Desc& d) { d.c_pitch = (d.W / 2) * d.c_step * bps - bps; });
            directed(f, variant, "", [&](Desc& d) { d.c_pitch = (d.W / 2) * d.c_step * bps; });
            directed(f, variant, cpm, [](Desc& d) { d.c_pitch = (int64_t)INT32_MAX + 1; });
            directed(f, variant, IN_Y_MSG, [&](Desc& d) { d.off[0] -= 2 * bps + 2; d.off[1] -= 2 * bps + 2; });
            directed(f, variant, IN_Y_MSG, [](Desc& d) { d.off[0] = 0; d.off[1] = d.c_step == 2 ? (d.fam == YUV16 ? 2 : 1) : d.off[1]; });
            directed(f, variant, "chroma offset too large", [&](Desc& d) { d.off[1] = INT64_MAX - 1; if (d.c_step == 2) d.off[0] = d.off[1] - bps; d.stride = INT64_MAX - 1; });
            directed(f, variant, "chroma offset too large", [&](Desc& d) { d.off[0] = INT64_MAX - 1 - 2 * bps; if (d.c_step == 2) d.off[1] = d.off[0] - bps; });
        }
        directed(f, 0, f == YUV16 ? "c_step 2 (semi-planar) needs u_offset and v_offset 2 bytes apart" : "c_step 2 (semi-planar) needs adjacent u_offset and v_offset", [&](Desc& d) { d.off[1] += bps; d.stride += bps; });
        directed(f, 0, f == YUV16 ? "c_step 2 (semi-planar) needs u_offset and v_offset 2 bytes apart" : "c_step 2 (semi-planar) needs adjacent u_offset and v_offset", [](Desc& d) { d.off[1] = d.off[0]; });
        directed(f, 0, "", [](Desc& d) { std::swap(d.off[0], d.off[1]); });
        directed(f, 1, C_OVERLAP_MSG, [&](Desc& d) { d.off[1] = d.off[0] + d.c_pitch + (d.W / 2) * bps - bps; });
        directed(f, 1, C_OVERLAP_MSG, [](Desc& d) { d.off[1] = d.off[0]; });
        directed(f, 1, C_OVERLAP_MSG, [&](Desc& d) { d.c_pitch += 4 * bps; d.off[1] = d.off[0] + 2 * bps; d.stride += 8 * bps; });   // U and V rows side by side in one pitch
        directed(f, 1, "", [&](Desc& d) { d.off[1] = d.off[0] + d.c_pitch + (d.W / 2) * bps; });
    }
    directed(YUVP, 0, "sub_x and sub_y must be 0 or 1 (log2 of the chroma subsampling)", [](Desc& d) { d.sub_x = -1; });
    directed(YUV16, 0, "shift must be 0 .. 8 (low bits dropped from a 16-bit sample)", [](Desc& d) { d.shift = 9; });
    directed(YUV16, 1, "shift must be 0 .. 8 (low bits dropped from a 16-bit sample)", [](Desc& d) { d.shift = -1; });
    directed(YUV16, 0, "16-bit samples need a 2-byte aligned base", [](Desc& d) { d.phase = 1; });
    directed(YUV16, 1, "16-bit samples need a 2-byte aligned base", [](Desc& d) { d.phase = 3; });
    directed(YUV16, 1, "", [](Desc& d) { d.phase = 2; });
    const char* const even16 = "16-bit samples need an even y_pitch, c_pitch, u_offset, v_offset and frame_stride (bytes)";
    directed(YUV16, 1, even16, [](Desc& d) { d.pitch += 1; });
    directed(YUV16, 1, even16, [](Desc& d) { d.c_pitch += 1; });
    directed(YUV16, 1, even16, [](Desc& d) { d.off[0] += 1; });
    directed(YUV16, 1, even16, [](Desc& d) { d.off[1] += 1; });
    directed(YUV16, 0, even16, [](Desc& d) { d.off[0] += 1; d.off[1] += 1; });
    directed(YUV16, 1, even16, [](Desc& d) { d.stride += 1; });
    // planar RGB
    directed(PLANES, 0, "negative plane offset", [](Desc& d) { d.off[0] = -1; });
    directed(PLANES, 0, "negative plane offset", [](Desc& d) { d.off[2] = INT64_MIN; });
    directed(PLANES, 0, "row_pitch smaller than a row", [](Desc& d) { d.pitch = d.W - 1; });
    directed(PLANES, 0, "row_pitch too large", [](Desc& d) { d.pitch = (int64_t)INT32_MAX + 1; });
    directed(PLANES, 0, "two planes overlap", [](Desc& d) { d.off[1] -= 3; });
    directed(PLANES, 0, "two planes overlap", [](Desc& d) { d.off[2] = d.off[0]; });
    directed(PLANES, 0, "", [](Desc& d) { d.off[1] -= 2; d.off[0] = 0; });
    for (int k = 0; k < 3; ++k) {
        directed(PLANES, 0, "plane offset too large", [&](Desc& d) { d.off[k] = INT64_MAX; });
        directed(PLANES, 0, "plane offset too large", [&](Desc& d) { d.off[k] = INT64_MAX - 3 * d.pitch - d.W + 1; d.stride = INT64_MAX; });
        directed(PLANES, 0, "", [&](Desc& d) { d.off[k] = INT64_MAX - 3 * d.pitch - d.W; d.stride = INT64_MAX; d.n = 1; });
    }
}

// ---- edges: every 64-bit field of every family at the ends of 32 and 64 bits; whatever the check says, it says without overflow ------------
static void edges()
{
    const int64_t values[] = {INT32_MAX, (int64_t)INT32_MAX + 1, (int64_t)INT32_MAX - 1, (int64_t)INT32_MAX + 2, (int64_t)1 << 32, INT64_MAX, INT64_MAX - 1,
                              INT64_MAX - 2,  INT64_MAX - 3, INT64_MAX - 4, INT64_MAX - 16, INT64_MAX - 24, -1, -2, -4, INT32_MIN, INT64_MIN, INT64_MIN + 2};
    for (int fam = 0; fam < NFAM; ++fam)
        for (int variant = 0; variant < 2; ++variant)
            for (int field = 0; field < 6; ++field)
                for (int64_t v : values)
                    for (int with_stride = 0; with_stride < 2; ++with_stride)   // the stride as it was, and one no frame outgrows
                        for (int n = 1; n <= 4; n += 3) {
                            Desc d = base_of((Fam)fam, variant);
                            d.n = n;
                            if (with_stride) d.stride = down(INT64_MAX, 4);
                            int64_t* const fields[6] = {&d.pitch, &d.c_pitch, &d.off[0], &d.off[1], &d.off[2], &d.stride};
                            *fields[field] = v;
                            visit(d);
                            if (field == 2 && d.c_step == 2) {   // a pair, moved together
                                d.off[1] = v > INT64_MAX - 2 ? v - 2 : v + (fam == YUV16 ? 2 : 1);
                                visit(d);
                            }
                        }
}

int main()
{
    sweep();
    by_hand();
    edges();
    for (int fam = 0; fam < NFAM; ++fam) {
        Family& F = g_fam[fam];
        int nmsg = 0, seen = 0;
        for (const Msg* m = F.msgs; m->text; ++m) { ++nmsg; seen += m->count > 0; }
        printf("%-16s accepted %lld, forms %d of %d, messages %d of %d, rejected without a neighbour %lld\n", F.name, F.accepted, (int)F.forms.size(), F.nforms,
               seen, nmsg, F.no_neighbour);
        for (const Msg* m = F.msgs; m->text; ++m) {
            printf("    %9lld  %s\n", m->count, m->text);
            if (m->count == 0) { ++g_fail; fprintf(stderr, "%s: never produced: %s\n", F.name, m->text); }
        }
        if (F.accepted == 0 || (int)F.forms.size() != F.nforms) { ++g_fail; fprintf(stderr, "%s: a form was never accepted\n", F.name); }
    }
    printf("descriptors enumerated sample by sample %lld; of them with (n - 1) * frame_stride + extent beyond 64 bits %lld\n", g_checked, g_wraps);
    printf("failures %lld\n", g_fail);
    return g_fail ? 1 : 0;
}
