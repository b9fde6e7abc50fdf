// The descriptor checks of the C ABI's melf_*_frames: every entry point that takes a descriptor starts with its check, which decides
// what layouts are taken and leaves the batch -- with FrameLayout::extent, which becomes MatchSrc::readable / DialsSrc::readable -- in
// *b.  Pure functions of the frames pointer (its NULL and alignment rules only) and the descriptor: no context, no HIP, nothing
// global.  They return the error message, or nullptr when the descriptor is taken; n == 0 passes whatever the frames pointer.
// melf_api.hip reports the message through fail(MELF_ERR_INVALID, ..); tests/frame_checks_main.cpp sweeps the checks on the CPU, and
// the bounds programs beside it allocate what the checks accept.
#pragma once
#include "melf_frame_layout.h"
#include "melf_narrow.h"

namespace melf {

// A batch of frames as an entry point's checks leave it: n frames of H x W pixels, frame_stride bytes apart, their rows (of the
// packed pixels, of the Y plane, of every plane) row_stride bytes apart, everything else in the layout
struct FrameBatch {
    int n, H, W;
    size_t frame_stride;
    int row_stride;
    FrameLayout lay;
};
// packed BGR frames with packed rows: melf_process_batch*, melf_process_stream_dev, the decoded JPEG frames
inline FrameBatch bgr_batch(int n, int H, int W, size_t frame_stride)
{
    return FrameBatch{n, H, W, frame_stride, W * 3, FrameLayout::packed(MELF_PIX_BGR, (size_t)H * W * 3)};
}

// Bytes from a plane's first sample to the end of its last: `rows` rows pitch bytes apart (0 <= pitch <= INT32_MAX), each of
// `samples` samples of bps bytes, `step` samples from one to the next (2: the other plane's samples lie between them).
inline int64_t plane_span(int64_t rows, int64_t pitch, int64_t samples, int step, int bps)
{
    return (rows - 1) * pitch + ((samples - 1) * step + 1) * bps;
}
// The spans of a Y plane at offset 0 and two chroma planes behind it, in bytes of one frame.
struct YuvSpans {
    int64_t y_end;       // the Y plane, first to last sample
    int64_t c_lo, c_hi;  // the lower and the higher of the two chroma offsets
    int64_t c_len;       // from a chroma plane's offset to the end of its last sample
    bool fits;           // c_hi + c_len is an int64_t
    int64_t c_end;       // fits: c_hi + c_len, the extent of a frame
};
// (pitches already known to be 0 .. INT32_MAX: no product here leaves 63 bits)
inline YuvSpans yuv_spans(int H, int W, int64_t y_pitch, int c_rows, int c_samples, int64_t c_pitch, int c_step, int bps, int64_t u_offset,
                          int64_t v_offset)
{
    YuvSpans s;
    s.y_end = plane_span(H, y_pitch, W, 1, bps);
    s.c_lo = u_offset < v_offset ? u_offset : v_offset;
    s.c_hi = u_offset < v_offset ? v_offset : u_offset;
    s.c_len = plane_span(c_rows, c_pitch, c_samples, c_step, bps);
    s.fits = s.c_hi <= INT64_MAX - s.c_len;
    s.c_end = s.fits ? s.c_hi + s.c_len : 0;
    return s;
}
// The span rules of melf_yuv_planar_frames and melf_yuv16_frames (offsets already known to be >= 0).  By spans, first to last
// sample: chroma kept inside the Y rows' padding, or U and V rows side by side in one pitch, do not overlap sample by sample but are
// not taken -- the header states the span rule.
inline const char* yuv_spans_error(const YuvSpans& s, bool semi, int64_t frame_stride)
{
    if (!s.fits) return "chroma offset too large";
    if (s.c_lo < s.y_end) return "a chroma offset lies inside the Y plane's span (first to last sample): spans may not overlap";
    if (!semi && s.c_hi - s.c_lo < s.c_len)
        return "the spans (first to last sample) of the two chroma planes overlap: U and V rows sharing one pitch are not taken";
    if (frame_stride < s.c_end) return "frame_stride smaller than a frame";
    return nullptr;
}

constexpr const char* UNKNOWN_YUV_MATRIX = "unknown YUV matrix (accepted: 0 BT.601 limited, 2 BT.601 full, 3 BT.709 limited, 4 BT.709 full)";

// melf_frames (melf_process_frames*)
inline const char* check_frames(const void* frames, const melf_frames* f, FrameBatch* b)
{
    if (!f) return "frame descriptor is NULL";
    if (f->pixel_format < MELF_PIX_BGR || f->pixel_format > MELF_PIX_RGBA) return "unknown pixel_format";
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return "bad batch shape";
    const int64_t bpp = pix_bytes(f->pixel_format);
    if (f->row_pitch < (int64_t)f->W * bpp) return "row_pitch smaller than a row";
    if (f->row_pitch > INT32_MAX) return "row_pitch too large";
    const int64_t extent = plane_span(f->H, f->row_pitch, f->W, 1, (int)bpp);   // the last row of a pitched buffer needs no padding
    if (f->frame_stride < extent) return "frame_stride smaller than a frame";
    *b = FrameBatch{f->n, f->H, f->W, (size_t)f->frame_stride, (int)f->row_pitch, FrameLayout::packed(f->pixel_format, (size_t)extent)};
    if (f->n == 0) return nullptr;
    if (!frames) return "frames pointer is NULL";
    if (bpp == 4 && (((uintptr_t)frames | (uint64_t)f->row_pitch | (uint64_t)f->frame_stride) & 3))
        return "4-byte pixel formats need a 4-byte aligned base, row_pitch and frame_stride";
    return nullptr;
}

// melf_yuv_frames (melf_process_yuv*, melf_yuv_to_bgr): base, frame_stride and row_stride describe the Y plane; the extent reaches
// to the last sample of the frame's last plane.  The spans are yuv_spans'; the rules are this descriptor's own: NV12's offsets, the
// height limit, and no test of I420's U span against its V span.
inline const char* check_yuv(const void* frames, const melf_yuv_frames* f, FrameBatch* b)
{
    if (!f) return "YUV frame descriptor is NULL";
    if (f->format != MELF_YUV_NV12 && f->format != MELF_YUV_I420) return "unknown YUV format";
    const YuvMatrix* mx = yuv_matrix(f->matrix);
    if (!mx) return UNKNOWN_YUV_MATRIX;
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return "bad batch shape";
    if ((f->H | f->W) & 1) return "YUV 4:2:0 frames need an even height and width";
    if (f->H > 131070) return "frame too high";
    const bool nv12 = f->format == MELF_YUV_NV12;
    const int64_t cw = nv12 ? f->W : f->W / 2;   // bytes of a chroma row
    if (f->y_pitch < f->W || f->y_pitch > INT32_MAX) return "y_pitch smaller than a row (or too large)";
    if (f->c_pitch < cw || f->c_pitch > INT32_MAX) return "c_pitch smaller than a chroma row (or too large)";
    const YuvSpans s = yuv_spans(f->H, f->W, f->y_pitch, f->H / 2, f->W / 2, f->c_pitch, nv12 ? 2 : 1, 1, f->u_offset, f->v_offset);
    if (s.c_lo < s.y_end) return "a chroma plane overlaps the Y plane";
    if (nv12 && (f->v_offset - f->u_offset != 1 || (f->u_offset & 1)))   // (both offsets >= y_end > 0 here: the difference cannot overflow)
        return "NV12 needs v_offset == u_offset + 1 and an even u_offset";
    if (!s.fits) return "chroma offset too large";
    if (f->frame_stride < s.c_end) return "frame_stride smaller than a frame";
    const YuvPlanes yp = {f->u_offset, f->v_offset, (int)f->c_pitch, 0};
    *b = FrameBatch{f->n, f->H, f->W, (size_t)f->frame_stride, (int)f->y_pitch,
                    FrameLayout::yuv420(nv12 ? PIX_NV12 : PIX_I420, yp, *mx, (size_t)s.c_end)};
    if (f->n == 0) return nullptr;
    if (!frames) return "frames pointer is NULL";
    return nullptr;
}

// melf_yuv422_frames (melf_process_yuv422*, melf_yuv422_to_bgr)
inline const char* check_yuv422(const void* frames, const melf_yuv422_frames* f, FrameBatch* b)
{
    if (!f) return "YUV 4:2:2 frame descriptor is NULL";
    if (f->format != MELF_YUV422_YUYV && f->format != MELF_YUV422_UYVY && f->format != MELF_YUV422_YVYU) return "unknown YUV 4:2:2 format";
    const YuvMatrix* mx = yuv_matrix(f->matrix);
    if (!mx) return UNKNOWN_YUV_MATRIX;
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return "bad batch shape";
    if (f->W & 1) return "YUV 4:2:2 frames need an even width";
    if (f->row_pitch < (int64_t)f->W * 2) return "row_pitch smaller than a row";
    if (f->row_pitch > INT32_MAX) return "row_pitch too large";
    const int64_t extent = plane_span(f->H, f->row_pitch, f->W, 1, 2);
    if (f->frame_stride < extent) return "frame_stride smaller than a frame";
    if (((uint64_t)f->row_pitch | (uint64_t)f->frame_stride) & 3) return "YUV 4:2:2 frames need a 4-byte aligned row_pitch and frame_stride";
    const int pix = f->format == MELF_YUV422_UYVY ? PIX_UYVY : (f->format == MELF_YUV422_YVYU ? PIX_YVYU : PIX_YUYV);
    *b = FrameBatch{f->n, f->H, f->W, (size_t)f->frame_stride, (int)f->row_pitch, FrameLayout::yuv422(pix, *mx, (size_t)extent)};
    if (f->n == 0) return nullptr;
    if (!frames) return "frames pointer is NULL";
    if ((uintptr_t)frames & 3) return "YUV 4:2:2 frames need a 4-byte aligned base";
    return nullptr;
}

// melf_yuv_planar_frames (melf_process_yuv_planar*, melf_yuv_planar_to_bgr): base, frame_stride and row_stride describe the Y plane;
// the extent reaches to the last sample of the frame's last plane
inline const char* check_yuv_planar(const void* frames, const melf_yuv_planar_frames* f, FrameBatch* b)
{
    if (!f) return "planar YUV frame descriptor is NULL";
    if (f->reserved != 0) return "reserved field of the planar YUV frame descriptor is not 0";
    if ((f->sub_x != 0 && f->sub_x != 1) || (f->sub_y != 0 && f->sub_y != 1))
        return "sub_x and sub_y must be 0 or 1 (log2 of the chroma subsampling)";
    if (f->c_step != 1 && f->c_step != 2) return "c_step must be 1 (planar) or 2 (semi-planar)";
    const YuvMatrix* mx = yuv_matrix(f->matrix);
    if (!mx) return UNKNOWN_YUV_MATRIX;
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return "bad batch shape";
    if (f->sub_x && (f->W & 1)) return "horizontally subsampled chroma (sub_x) needs an even width";
    if (f->sub_y && (f->H & 1)) return "vertically subsampled chroma (sub_y) needs an even height";
    if (f->u_offset < 0 || f->v_offset < 0) return "negative chroma offset";
    const bool semi = f->c_step == 2;
    if (semi && f->u_offset - f->v_offset != 1 && f->v_offset - f->u_offset != 1)
        return "c_step 2 (semi-planar) needs adjacent u_offset and v_offset";
    if (f->y_pitch < f->W || f->y_pitch > INT32_MAX) return "y_pitch smaller than a row (or too large)";
    const int cs = f->W >> f->sub_x, ch = f->H >> f->sub_y;   // samples of a chroma plane's row, rows
    if (f->c_pitch < (int64_t)cs * f->c_step || f->c_pitch > INT32_MAX) return "c_pitch smaller than a chroma row (or too large)";
    const YuvSpans s = yuv_spans(f->H, f->W, f->y_pitch, ch, cs, f->c_pitch, f->c_step, 1, f->u_offset, f->v_offset);
    if (const char* msg = yuv_spans_error(s, semi, f->frame_stride)) return msg;
    const YuvPlanarPlanes yp = {f->u_offset, f->v_offset, (int)f->c_pitch, f->sub_x, f->sub_y, f->c_step};
    *b = FrameBatch{f->n, f->H, f->W, (size_t)f->frame_stride, (int)f->y_pitch, FrameLayout::yuv_planar(yp, *mx, (size_t)s.c_end)};
    if (f->n == 0) return nullptr;
    if (!frames) return "frames pointer is NULL";
    return nullptr;
}

// melf_yuv16_frames (melf_process_yuv16*, melf_yuv16_to_bgr): samples of 2 bytes, sub_x 1; base, frame_stride and row_stride (bytes)
// describe the Y plane; the extent reaches to the end of the last sample of the frame's last plane
inline const char* check_yuv16(const void* frames, const melf_yuv16_frames* f, FrameBatch* b)
{
    if (!f) return "16-bit YUV frame descriptor is NULL";
    if (f->reserved != 0) return "reserved field of the 16-bit YUV frame descriptor is not 0";
    if (f->sub_y != 0 && f->sub_y != 1) return "sub_y must be 0 or 1 (log2 of the vertical chroma subsampling)";
    if (f->c_step != 1 && f->c_step != 2) return "c_step must be 1 (planar) or 2 (semi-planar) samples";
    if (f->shift < 0 || f->shift > 8) return "shift must be 0 .. 8 (low bits dropped from a 16-bit sample)";
    const YuvMatrix* mx = yuv_matrix(f->matrix);
    if (!mx) return UNKNOWN_YUV_MATRIX;
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return "bad batch shape";
    if (f->W & 1) return "horizontally subsampled chroma needs an even width";
    if (f->sub_y && (f->H & 1)) return "vertically subsampled chroma (sub_y) needs an even height";
    if (f->u_offset < 0 || f->v_offset < 0) return "negative chroma offset";
    if ((f->y_pitch | f->c_pitch | f->u_offset | f->v_offset | f->frame_stride) & 1)
        return "16-bit samples need an even y_pitch, c_pitch, u_offset, v_offset and frame_stride (bytes)";
    const bool semi = f->c_step == 2;
    if (semi && f->u_offset - f->v_offset != 2 && f->v_offset - f->u_offset != 2)
        return "c_step 2 (semi-planar) needs u_offset and v_offset 2 bytes apart";
    if (f->y_pitch < (int64_t)f->W * 2 || f->y_pitch > INT32_MAX) return "y_pitch smaller than a row of 2-byte samples (or too large)";
    const int cs = f->W >> 1, ch = f->H >> f->sub_y;   // samples of a chroma plane's row, rows
    if (f->c_pitch < (int64_t)cs * f->c_step * 2 || f->c_pitch > INT32_MAX) return "c_pitch smaller than a chroma row of 2-byte samples (or too large)";
    const YuvSpans s = yuv_spans(f->H, f->W, f->y_pitch, ch, cs, f->c_pitch, f->c_step, 2, f->u_offset, f->v_offset);
    if (const char* msg = yuv_spans_error(s, semi, f->frame_stride)) return msg;
    const Yuv16Planes yp = {f->u_offset, f->v_offset, (int)f->c_pitch, f->sub_y, f->c_step, f->shift};
    *b = FrameBatch{f->n, f->H, f->W, (size_t)f->frame_stride, (int)f->y_pitch, FrameLayout::yuv16(yp, *mx, (size_t)s.c_end)};
    if (f->n == 0) return nullptr;
    if (!frames) return "frames pointer is NULL";
    if ((uintptr_t)frames & 1) return "16-bit samples need a 2-byte aligned base";
    return nullptr;
}

// melf_yuv422_10_frames (melf_process_yuv422_10*, melf_yuv422_10_to_bgr): v210 rows are whole 16-byte groups of six pixels, Y21x rows
// macropixels of 8 bytes; the extent reaches to the end of the last row's last group / macropixel.  Its messages have names, in one
// table: tests/p10_bounds_main.cpp sweeps this check and counts, through the table, that every one of them was produced
// (tests/frame_checks_main.cpp does that for the six checks above, from their text).
enum Yuv422_10Msg { P10_DESC_NULL, P10_FORMAT, P10_RESERVED, P10_SHAPE, P10_ODD_W, P10_PITCH_SMALL, P10_PITCH_LARGE, P10_STRIDE_SMALL,
                    P10_V210_STRIDES, P10_Y210_STRIDES, P10_FRAMES_NULL, P10_V210_BASE, P10_Y210_BASE, P10_MESSAGES };
constexpr const char* YUV422_10_MESSAGES[P10_MESSAGES] = {
    "packed 10-bit YUV 4:2:2 frame descriptor is NULL",
    "unknown packed 10-bit YUV 4:2:2 format",
    "reserved field of the packed 10-bit YUV 4:2:2 frame descriptor is not 0",
    "bad batch shape",
    "YUV 4:2:2 frames need an even width",
    "row_pitch smaller than a row",
    "row_pitch too large",
    "frame_stride smaller than a frame",
    "v210 frames need a 16-byte aligned row_pitch and frame_stride",
    "Y210 frames need an 8-byte aligned row_pitch and frame_stride",
    "frames pointer is NULL",
    "v210 frames need a 16-byte aligned base",
    "Y210 frames need an 8-byte aligned base",
};
inline const char* check_yuv422_10(const void* frames, const melf_yuv422_10_frames* f, FrameBatch* b)
{
    const char* const* const msg = YUV422_10_MESSAGES;
    if (!f) return msg[P10_DESC_NULL];
    if (f->format != MELF_YUV422_10_V210 && f->format != MELF_YUV422_10_Y210) return msg[P10_FORMAT];
    const YuvMatrix* mx = yuv_matrix(f->matrix);
    if (!mx) return UNKNOWN_YUV_MATRIX;
    if (f->reserved != 0) return msg[P10_RESERVED];
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return msg[P10_SHAPE];
    if (f->W & 1) return msg[P10_ODD_W];
    const bool v210 = f->format == MELF_YUV422_10_V210;
    const int64_t row = v210 ? ((int64_t)f->W + 5) / 6 * 16 : (int64_t)f->W * 4;   // bytes of a row: whole groups / macropixels
    if (f->row_pitch < row) return msg[P10_PITCH_SMALL];
    if (f->row_pitch > INT32_MAX) return msg[P10_PITCH_LARGE];
    const int64_t extent = (int64_t)(f->H - 1) * f->row_pitch + row;
    if (f->frame_stride < extent) return msg[P10_STRIDE_SMALL];
    const uint64_t amask = v210 ? 15 : 7;
    if (((uint64_t)f->row_pitch | (uint64_t)f->frame_stride) & amask) return msg[v210 ? P10_V210_STRIDES : P10_Y210_STRIDES];
    *b = FrameBatch{f->n, f->H, f->W, (size_t)f->frame_stride, (int)f->row_pitch,
                    FrameLayout::yuv422_10(v210 ? PIX_V210 : PIX_Y210, *mx, (size_t)extent)};
    if (f->n == 0) return nullptr;
    if (!frames) return msg[P10_FRAMES_NULL];
    if ((uintptr_t)frames & amask) return msg[v210 ? P10_V210_BASE : P10_Y210_BASE];
    return nullptr;
}

// melf_packed32_frames (melf_process_packed32*, melf_packed32_to_bgr): one 32-bit word per pixel, three 8-bit reads at pos[0..2]; the
// extent reaches to the end of the last row's last word.  Its messages have names, in one table, as YUV422_10_MESSAGES:
// tests/p32_bounds_main.cpp sweeps this check and counts, through the table, that every one of them was produced.
enum Packed32Msg { P32_DESC_NULL, P32_COLOUR, P32_MATRIX_YUV, P32_MATRIX_RGB, P32_RESERVED, P32_POS_RANGE, P32_POS_OVERLAP, P32_SHAPE,
                   P32_PITCH_SMALL, P32_PITCH_LARGE, P32_STRIDE_SMALL, P32_STRIDES, P32_FRAMES_NULL, P32_BASE, P32_MESSAGES };
constexpr const char* PACKED32_MESSAGES[P32_MESSAGES] = {
    "32-bit packed frame descriptor is NULL",
    "unknown colour of 32-bit packed frames (accepted: 0 YUV, 1 RGB)",
    "unknown YUV matrix of 32-bit packed frames (accepted: 0 BT.601 limited, 2 BT.601 full, 3 BT.709 limited, 4 BT.709 full)",
    "matrix of 32-bit packed RGB frames is not 0",
    "reserved field of the 32-bit packed frame descriptor is not 0",
    "a read position of 32-bit packed frames is outside 0 .. 24",
    "two reads of 32-bit packed frames overlap (positions less than 8 bits apart)",
    "bad batch shape of 32-bit packed frames",
    "row_pitch of 32-bit packed frames smaller than a row",
    "row_pitch of 32-bit packed frames too large",
    "frame_stride of 32-bit packed frames smaller than a frame",
    "32-bit packed frames need a 4-byte aligned row_pitch and frame_stride",
    "frames pointer of 32-bit packed frames is NULL",
    "32-bit packed frames need a 4-byte aligned base",
};
inline const char* check_packed32(const void* frames, const melf_packed32_frames* f, FrameBatch* b)
{
    const char* const* const msg = PACKED32_MESSAGES;
    if (!f) return msg[P32_DESC_NULL];
    if (f->colour != MELF_P32_YUV && f->colour != MELF_P32_RGB) return msg[P32_COLOUR];
    const bool yuv = f->colour == MELF_P32_YUV;
    const YuvMatrix* mx = yuv ? yuv_matrix(f->matrix) : nullptr;
    if (yuv && !mx) return msg[P32_MATRIX_YUV];
    if (!yuv && f->matrix != 0) return msg[P32_MATRIX_RGB];
    if (f->reserved != 0 || f->reserved2 != 0) return msg[P32_RESERVED];
    for (int k = 0; k < 3; ++k)
        if (f->pos[k] < 0 || f->pos[k] > 24) return msg[P32_POS_RANGE];
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) {
            const int d = f->pos[i] - f->pos[j];
            if (d > -8 && d < 8) return msg[P32_POS_OVERLAP];
        }
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return msg[P32_SHAPE];
    const int64_t row = (int64_t)f->W * 4;
    if (f->row_pitch < row) return msg[P32_PITCH_SMALL];
    if (f->row_pitch > INT32_MAX) return msg[P32_PITCH_LARGE];
    const int64_t extent = (int64_t)(f->H - 1) * f->row_pitch + row;
    if (f->frame_stride < extent) return msg[P32_STRIDE_SMALL];
    if (((uint64_t)f->row_pitch | (uint64_t)f->frame_stride) & 3) return msg[P32_STRIDES];
    const Packed32Fields fields = {{(uint32_t)f->pos[0], (uint32_t)f->pos[1], (uint32_t)f->pos[2]}};
    *b = FrameBatch{f->n, f->H, f->W, (size_t)f->frame_stride, (int)f->row_pitch,
                    FrameLayout::packed32(yuv ? PIX_P32_YUV : PIX_P32_RGB, fields, mx, (size_t)extent)};
    if (f->n == 0) return nullptr;
    if (!frames) return msg[P32_FRAMES_NULL];
    if ((uintptr_t)frames & 3) return msg[P32_BASE];
    return nullptr;
}

// melf_planar_frames (melf_process_planes*): the extent reaches to the last sample of the frame's last plane
inline const char* check_planes(const void* frames, const melf_planar_frames* f, FrameBatch* b)
{
    if (!f) return "planar frame descriptor is NULL";
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return "bad batch shape";
    if (f->reserved != 0) return "reserved field of the planar frame descriptor is not 0";
    if (f->b_offset < 0 || f->g_offset < 0 || f->r_offset < 0) return "negative plane offset";
    if (f->row_pitch < f->W) return "row_pitch smaller than a row";
    if (f->row_pitch > INT32_MAX) return "row_pitch too large";
    const int64_t span = plane_span(f->H, f->row_pitch, f->W, 1, 1);   // bytes of one plane, first to last sample
    const int64_t off[3] = {f->b_offset, f->g_offset, f->r_offset};
    int64_t hi = 0;
    for (int a = 0; a < 3; ++a) {
        if (off[a] > INT64_MAX - span) return "plane offset too large";
        if (off[a] > hi) hi = off[a];
        for (int k = a + 1; k < 3; ++k) {
            const int64_t lo2 = off[a] < off[k] ? off[a] : off[k], hi2 = off[a] < off[k] ? off[k] : off[a];
            if (hi2 - lo2 < span) return "two planes overlap";
        }
    }
    if (f->frame_stride < hi + span) return "frame_stride smaller than a frame";
    const PlanarPlanes pl = {f->b_offset, f->g_offset, f->r_offset};
    *b = FrameBatch{f->n, f->H, f->W, (size_t)f->frame_stride, (int)f->row_pitch, FrameLayout::planar(pl, (size_t)(hi + span))};
    if (f->n == 0) return nullptr;
    if (!frames) return "frames pointer is NULL";
    return nullptr;
}

// melf_wide_frames (melf_process_wide*, melf_wide_to_bgr): RGB frames of 16-bit or floating-point samples.  The check leaves the
// 8-bit batch OF THE SAME GEOMETRY -- every offset, pitch, stride and the extent counted in SAMPLES, which the alignment rule makes
// whole numbers --, a packed batch of the descriptor's pixel format or a planar one: its staging plan (melf_stage_plan.h) is the
// staged frame the narrowing writes, and its runs times the sample size are the source's (melf_narrow_addr.h).  And the rule
// (melf_narrow.h), scale and offset laid out by position.  Its messages have names, in one table, as PACKED32_MESSAGES:
// tests/wide_checks_main.cpp sweeps this check and counts, through the table, that every one of them was produced.
struct WideBatch {
    FrameBatch b;         // in samples; b.lay: packed(pixel_format) or planar
    narrow::Rule rule;
    int ss;               // bytes of a sample: frame f starts at frames + f * b.frame_stride * ss
};
enum WideMsg { WIDE_DESC_NULL, WIDE_TYPE, WIDE_LAYOUT, WIDE_FORMAT, WIDE_ROUNDING, WIDE_SHIFT, WIDE_RESERVED, WIDE_COEF, WIDE_SHAPE,
               WIDE_NEG_OFFSET, WIDE_ALIGN, WIDE_PITCH_SMALL, WIDE_PITCH_LARGE, WIDE_OFFSET_LARGE, WIDE_OVERLAP, WIDE_STRIDE_SMALL,
               WIDE_FRAMES_NULL, WIDE_BASE, WIDE_MSGS };
constexpr const char* WIDE_MESSAGES[WIDE_MSGS] = {
    "wide frame descriptor is NULL",
    "unknown sample_type of wide frames (accepted: 0 u16, 1 f16, 2 bf16, 3 f32)",
    "unknown layout of wide frames (accepted: 0 packed, 1 planar)",
    "unknown pixel_format of packed wide frames",
    "unknown rounding of wide frames (accepted: 0 nearest, 1 floor)",
    "shift of wide frames must be 0 .. 8 (low bits dropped from a 16-bit sample)",
    "reserved field of the wide frame descriptor is not 0",
    "scale and offset of wide frames must be finite, |scale| <= 2^24",
    "bad batch shape of wide frames",
    "negative plane offset of wide frames",
    "wide frames need offsets, a row_pitch and a frame_stride that are multiples of the sample size",
    "row_pitch of wide frames smaller than a row",
    "row_pitch of wide frames too large",
    "plane offset of wide frames too large",
    "two planes of wide frames overlap",
    "frame_stride of wide frames smaller than a frame",
    "frames pointer of wide frames is NULL",
    "wide frames need a base that is a multiple of the sample size",
};
inline const char* check_wide(const void* frames, const melf_wide_frames* f, WideBatch* wb)
{
    const char* const* const msg = WIDE_MESSAGES;
    if (!f) return msg[WIDE_DESC_NULL];
    if (f->sample_type < MELF_WIDE_U16 || f->sample_type > MELF_WIDE_F32) return msg[WIDE_TYPE];
    if (f->layout != MELF_WIDE_PACKED && f->layout != MELF_WIDE_PLANAR) return msg[WIDE_LAYOUT];
    const bool planar = f->layout == MELF_WIDE_PLANAR;
    if (!planar && (f->pixel_format < MELF_PIX_BGR || f->pixel_format > MELF_PIX_RGBA)) return msg[WIDE_FORMAT];
    if (f->rounding != MELF_ROUND_NEAREST && f->rounding != MELF_ROUND_FLOOR) return msg[WIDE_ROUNDING];
    if (f->shift < 0 || f->shift > 8) return msg[WIDE_SHIFT];
    if (f->reserved != 0 || f->reserved2 != 0) return msg[WIDE_RESERVED];
    for (int k = 0; k < 3; ++k)
        if (!(fabsf(f->scale[k]) <= 16777216.0f) || !(fabsf(f->offset[k]) <= 3.402823466e38f)) return msg[WIDE_COEF];   // (NaN fails both)
    if (f->n < 0 || f->H <= 0 || f->W <= 0) return msg[WIDE_SHAPE];
    if (planar && (f->b_offset < 0 || f->g_offset < 0 || f->r_offset < 0)) return msg[WIDE_NEG_OFFSET];
    const int ss = narrow::sample_bytes(f->sample_type);
    const int ch = planar ? 1 : pix_bytes(f->pixel_format);   // samples of a pixel in one row
    const uint64_t amask = (uint64_t)ss - 1;
    if (((uint64_t)f->row_pitch | (uint64_t)f->frame_stride) & amask) return msg[WIDE_ALIGN];
    if (planar && (((uint64_t)f->b_offset | (uint64_t)f->g_offset | (uint64_t)f->r_offset) & amask)) return msg[WIDE_ALIGN];
    if (f->row_pitch < (int64_t)f->W * ch * ss) return msg[WIDE_PITCH_SMALL];
    if (f->row_pitch > INT32_MAX) return msg[WIDE_PITCH_LARGE];
    const int64_t span = plane_span(f->H, f->row_pitch, f->W, 1, ch * ss);   // bytes of the packed plane / of one plane
    int64_t hi = 0;
    if (planar) {
        const int64_t off[3] = {f->b_offset, f->g_offset, f->r_offset};
        for (int a = 0; a < 3; ++a) {
            if (off[a] > INT64_MAX - span) return msg[WIDE_OFFSET_LARGE];
            if (off[a] > hi) hi = off[a];
            for (int k = a + 1; k < 3; ++k) {
                const int64_t lo2 = off[a] < off[k] ? off[a] : off[k], hi2 = off[a] < off[k] ? off[k] : off[a];
                if (hi2 - lo2 < span) return msg[WIDE_OVERLAP];
            }
        }
    }
    if (f->frame_stride < hi + span) return msg[WIDE_STRIDE_SMALL];
    const size_t extent = (size_t)((hi + span) / ss);
    const PlanarPlanes pl = {f->b_offset / ss, f->g_offset / ss, f->r_offset / ss};
    wb->b = FrameBatch{f->n, f->H, f->W, (size_t)(f->frame_stride / ss), (int)(f->row_pitch / ss),
                       planar ? FrameLayout::planar(pl, extent) : FrameLayout::packed(f->pixel_format, extent)};
    wb->ss = ss;
    narrow::Rule& r = wb->rule;
    r = narrow::Rule{};
    r.type = f->sample_type; r.shift = f->shift; r.floor_ = f->rounding == MELF_ROUND_FLOOR; r.channels = ch;
    const bool rgb = !planar && (f->pixel_format == MELF_PIX_RGB || f->pixel_format == MELF_PIX_RGBA);
    for (int p = 0; p < 3; ++p) {   // position p holds channel p (B G R ..; the planes of the staged frame) or 2 - p (R G B ..)
        r.scale[p] = f->scale[rgb ? 2 - p : p];
        r.offset[p] = f->offset[rgb ? 2 - p : p];
    }
    if (f->n == 0) return nullptr;
    if (!frames) return msg[WIDE_FRAMES_NULL];
    if ((uintptr_t)frames & amask) return msg[WIDE_BASE];
    return nullptr;
}

// melf_wide_frames beside a list of frame pointers (melf_process_wide_list*, melf_wide_list_to_bgr): the descriptor through check_wide
// as a one-frame batch -- with a frame_stride that it takes, a multiple of 16 no extent reaches, against a pointer that breaks no
// rule --, its messages WIDE_MESSAGES' own; then the array and every pointer of the list, whose messages have a table of their own.
// *wb: the one-frame batch with n the list's length (frame_stride means nothing).  *bad: -1, or the index of the frame the message
// is about, which the caller puts in front of it ("frame i of the list: ").  tests/wide_list_main.cpp sweeps this check and counts,
// through the table, that every message was produced.
enum WideListMsg { WLIST_TABLE_NULL, WLIST_PTR_NULL, WLIST_PTR_ALIGN, WLIST_MSGS };
constexpr const char* WIDE_LIST_MESSAGES[WLIST_MSGS] = {
    "the wide list's array of frame pointers is NULL",
    "frame pointer of wide frames is NULL",
    "wide frames need frame pointers that are multiples of the sample size",
};
// the descriptor as a one-frame batch: what the two list checks share (n: the caller's, put back by them)
inline melf_wide_frames wide_one_frame(const melf_wide_frames& f)
{
    melf_wide_frames one = f;
    one.n = f.n > 0 ? 1 : f.n;
    one.frame_stride = INT64_MAX & ~(int64_t)15;
    return one;
}
inline const char* check_wide_list(const melf_wide_frames* f, const void* const* frames, WideBatch* wb, int* bad)
{
    *bad = -1;
    if (!f) return check_wide(nullptr, nullptr, wb);
    const melf_wide_frames one = wide_one_frame(*f);
    if (const char* msg = check_wide((const void*)(uintptr_t)64, &one, wb)) return msg;
    wb->b.n = f->n;
    if (f->n == 0) return nullptr;
    if (!frames) return WIDE_LIST_MESSAGES[WLIST_TABLE_NULL];
    for (int i = 0; i < f->n; ++i) {
        *bad = i;
        if (!frames[i]) return WIDE_LIST_MESSAGES[WLIST_PTR_NULL];
        if ((uintptr_t)frames[i] & ((uintptr_t)wb->ss - 1)) return WIDE_LIST_MESSAGES[WLIST_PTR_ALIGN];
    }
    *bad = -1;
    return nullptr;
}

}  // namespace melf
