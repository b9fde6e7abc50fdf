/*
 * meterelf_hip.h -- C ABI of libmeterelf_hip.so, the MI355X (gfx950) drop-in
 * for meterelf's per-image hot path.
 *
 * The reference (suutari/meterelf) has no FFI/plugin boundary: its hot path is
 * Python calling cv2.  The boundary is therefore its Python API, which
 * meterelf_amd/ keeps (get_meter_values, MeterImageData, ImageFile,
 * get_meter_value), and this header is what that host layer binds through
 * ctypes.  Each entry point cites the reference code it replaces (paths relative
 * to the reference checkout).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every function
 * returns 0 on success or a negative melf_status; the message is available from
 * melf_last_error() (thread-local).  A context belongs to one GPU and is driven
 * by one host thread at a time.  The caller owns every buffer it passes in; the
 * context owns its device memory.  "_dev" entry points take device pointers
 * (e.g. torch tensors' data_ptr()) and enqueue on `stream` (a hipStream_t passed
 * as void*; NULL = the null / legacy default stream, exactly as in a HIP launch,
 * which is also what torch's default stream handle 0 means) without synchronising
 * it unless stated: work the caller enqueued on `stream` before the call is seen
 * by the kernels, and whatever the caller enqueues on it afterwards sees the
 * records.  A context owns two sets of work buffers ("lanes") and hands a lane
 * to each caller stream: *_dev calls that arrive on two different streams run
 * concurrently on the GPU, a third stream (or a call that needs the lane
 * another stream used last) is ordered behind that stream's work by an event.
 * Two batches' kernels never run against the same buffers at once.
 *
 * Stream order of the _dev entry points (tests/test_stream_order.py holds the library to it):
 * - Without melf_ctx_set_frames_resident every command of a call -- a list's pointer-table upload, the gather / narrowing /
 *   orienting kernel, prep, match and the kernel that writes the records -- is enqueued on `stream`; melf_process_stream_dev
 *   enqueues on the two lanes' own streams, which first wait for everything `stream` held at the call, and `stream` then waits
 *   for both.  The call waits for everything the caller's stream held at the call; what the caller enqueues on `stream` afterwards
 *   is ordered behind the whole call: it sees the records and may overwrite the frames and the records.
 * - With it, a contiguous batch (melf_process_batch_dev and the descriptor families' _dev calls): the caller's one promise is that
 *   the frames are complete at the call.  Prep and match run on a lane's own stream and wait for nothing of `stream`; the kernel
 *   that writes the records waits for everything `stream` held at the call; `stream` then waits for the end of the call.
 * - With it, the list flow (frame lists, plane lists, wide frames, wide lists, oriented frames): no promise.  Only the pointer
 *   table goes up at once; the gather / narrowing / orienting kernel and all behind it wait for everything `stream` held at the
 *   call; `stream` then waits for the end of the call.  melf_process_stream_dev and melf_hls_inrange_close_dev do not look at the
 *   mode (the mask is one kernel on `stream`).
 * - A call that gets a lane another stream used last -- a third caller stream, a call after a switch of the mode -- waits for
 *   everything that stream held.
 * The host waits in three cases only: out_host is given (the call synchronises `stream`); a work buffer of the lane has to grow
 * (the first call of a larger shape on that lane: the device is drained); a list call with a pointer table waits until the
 * previous upload of that lane's table has finished.
 */
#ifndef METERELF_HIP_H
#define METERELF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define MELF_MAX_DIALS 8
#define MELF_ABI_VERSION 3

/* API status codes (negative) */
enum {
    MELF_SUCCESS = 0,
    MELF_ERR_INVALID = -1,  /* bad argument / shape mismatch          */
    MELF_ERR_HIP = -2,      /* HIP runtime error, see melf_last_error  */
    MELF_ERR_NO_DEVICE = -3,
    MELF_ERR_TOO_LARGE = -4 /* template/dial does not fit the kernels' LDS tiles */
};

/* Per-frame status: mirrors the reference's exception classes
 * (meterelf/exceptions.py:35-52). */
enum {
    MELF_FRAME_OK = 0,
    MELF_FRAME_DIALS_NOT_FOUND = 1,           /* DialsNotFoundError, meterelf/_image.py:62-64      */
    MELF_FRAME_NEEDLE_CONTOURS_NOT_FOUND = 2, /* NeedleContoursNotFoundError, _reading.py:137-138  */
    MELF_FRAME_ANGLE_UNDETERMINED = 3         /* DialAngleDeterminingError, _reading.py:98-106     */
};

/* One entry of params.yml `needle_data` (meterelf/_params.py:71-81). */
typedef struct {
    double cx, cy;            /* center                                   */
    double angle_of_zero;     /* degrees                                  */
    int32_t range_h, range_l, range_s; /* color_range                     */
    int32_t negative_momentum;
    int32_t diameter;
    int32_t dist_from_center;
    int32_t circle_thickness;
    int32_t reserved;
} melf_dial;

/* Scalars of params.yml (meterelf/_params.py:30-64). */
typedef struct {
    int32_t abi_version;      /* MELF_ABI_VERSION                          */
    int32_t rect_x0, rect_y0, rect_x1, rect_y1; /* meter_rect              */
    int32_t th, tw;           /* template rows, cols (dials_template_size as (h, w)) */
    int32_t hue_shift;
    int32_t ndials;
    int32_t needle_lo[3];     /* fixed H,L,S bounds of the fused full-frame */
    int32_t needle_hi[3];     /*   stage: needle_color -/+ needle_color_range, clamped */
    int32_t name_order[MELF_MAX_DIALS]; /* dial indices sorted by name string (_reading.py:171) */
    int32_t reserved;
    double match_threshold;   /* dials_template_match_threshold            */
    melf_dial dial[MELF_MAX_DIALS];
} melf_params;

/* Per-frame record.  The Python host rebuilds the reference's return dict /
 * exception objects from it (meterelf/_reading.py:19-115). */
typedef struct {
    int32_t status;           /* MELF_FRAME_*                              */
    int32_t match_x, match_y; /* minMaxLoc max_loc, meterelf/_utils.py:94-95 */
    int32_t failed_dial;      /* NEEDLE_CONTOURS_NOT_FOUND: dial index, else -1 */
    uint32_t unreadable_mask; /* ANGLE_UNDETERMINED: bit d = dial d unreadable */
    float match_val;          /* minMaxLoc max_val (float32)               */
    double pos[MELF_MAX_DIALS];   /* dial positions in [0, 10)             */
    double angle[MELF_MAX_DIALS]; /* needle angle in turns, before angle_of_zero */
    double value;             /* determine_value_by_dial_positions, valid iff OK and ndials == 4 */
} melf_result;

typedef struct melf_ctx melf_ctx;

const char* melf_last_error(void);
int melf_abi_version(void);
int melf_device_count(int* count);

/* Host precompute of the per-dial masks, replaces _dial_data._get_dial_data
 * (meterelf/_dial_data.py:22-55): masks[ndials][2][th*tw], plane 0 = `mask`
 * (disk), plane 1 = `circle_mask` (annulus). */
int melf_build_dial_masks(const melf_params* p, uint8_t* masks);

/* The calibration blob = params + template + dial masks, the only shared
 * read-only state of the path (meterelf/_image.py:69-81, _dial_data.py:11-19).
 * Rank 0 packs it, the host layer broadcasts it (RCCL) and every rank creates
 * its context from the same bytes. */
size_t melf_blob_size(const melf_params* p);
int melf_blob_pack(const melf_params* p, const uint8_t* templ /* th*tw */, void* blob, size_t blob_bytes);
int melf_blob_params(const void* blob, size_t blob_bytes, melf_params* out);

/* One context per GPU.  `blob` is a host pointer unless blob_on_device != 0. */
int melf_ctx_create(int device, const void* blob, size_t blob_bytes, int blob_on_device, melf_ctx** out);
/* One process, n GPUs (SURVEY 8b's `melf_ctx_bcast`, 8e; the reference has one process and no GPU: meterelf/_api.py:16-33):
 * the host blob goes to devices[0] and from there to every other listed GPU by ONE ncclBroadcast (ncclUint8, root 0; RCCL
 * over xGMI, bound with dlopen at the first call), and out[i] is created on devices[i] from that GPU's copy.  A device may
 * not be listed twice.  All or nothing: on failure every out[i] is NULL.  (One process PER GPU broadcasts the same bytes
 * through its own communicator -- torch.distributed in meterelf_amd/_dist.py -- and calls melf_ctx_create with
 * blob_on_device = 1.) */
int melf_ctx_create_bcast(const int* devices, int n, const void* blob, size_t blob_bytes, melf_ctx** out);
void melf_ctx_destroy(melf_ctx* ctx);
int melf_ctx_params(const melf_ctx* ctx, melf_params* out);
/* Waits for all work the context has enqueued on caller streams and forgets those streams.  Call it before
 * destroying a stream that *_dev calls of this context were issued on. */
int melf_ctx_sync(melf_ctx* ctx);
/* copy the context's dial masks back (tests) */
int melf_ctx_get_masks(const melf_ctx* ctx, uint8_t* masks);

/* ---- the whole path: replaces get_meter_value(imgf) per frame
 * (meterelf/_reading.py:19-115 with meterelf/_image.py:23-66) ---------------
 * frames: n full camera frames, H x W x 3 u8 BGR (cv2.imread layout), frame f at
 * frames + f*frame_stride bytes.  The meter_rect crop is taken inside, with
 * numpy-slice clamping (meterelf/_image.py:54-55).  Host frames: only that crop
 * crosses PCIe (packed by host threads into pinned staging buffers, copied by
 * DMA in chunks that overlap the previous chunk's kernels). */
int melf_process_batch(melf_ctx* ctx, const uint8_t* frames_host, int n, int H, int W,
                       size_t frame_stride, melf_result* out_host);
/* frames already in HBM; results go to d_results (device, may be NULL) and/or
 * out_host (host, may be NULL; when given the call synchronises the stream). */
int melf_process_batch_dev(melf_ctx* ctx, const void* d_frames, int n, int H, int W,
                           size_t frame_stride, void* d_results, melf_result* out_host, void* stream);

/* ---- the same path for the frames callers have: RGB, BGRA / BGRx, RGBA / RGBx, padded rows ---------------
 * What get_bgr_image + _crop_meter would have read (meterelf/_image.py:46-55) from the packed BGR frame made of each
 * frame: the records are byte-identical to melf_process_batch(_dev) on that frame, without the conversion pass.  The
 * kernels read the layout in place; only the meter_rect crop is ever read.
 * Frame f's row y starts at frames + f * frame_stride + y * row_pitch.  The last row of the last frame needs no padding:
 * the buffer must hold (n - 1) * frame_stride + (H - 1) * row_pitch + W * bytes per pixel bytes.  The 4-byte formats need
 * a 4-byte aligned base, row_pitch and frame_stride; the 3-byte formats take any alignment.  An unknown format, a pitch
 * or stride too small, a misaligned 4-byte layout or a NULL descriptor return MELF_ERR_INVALID before anything runs.
 * melf_process_stream_dev, the fused full-frame mask (melf_hls_inrange_close*), melf_aligned_average and the JPEG entry
 * points take packed BGR only; YUV 4:2:0 frames and packed YUV 4:2:2 frames have their own descriptors and entry points
 * (melf_process_yuv*, melf_process_yuv422*, below), planar and semi-planar YUV of the other subsamplings too
 * (melf_process_yuv_planar*), and so have planar RGB frames (melf_process_planes*, below). */
enum { MELF_PIX_BGR = 0, MELF_PIX_RGB = 1, MELF_PIX_BGRA = 2, MELF_PIX_RGBA = 3 };
typedef struct melf_frames {
    int32_t pixel_format;  /* MELF_PIX_*; the 4th byte of BGRA / RGBA is ignored                          */
    int32_t n, H, W;
    int64_t row_pitch;     /* bytes between rows, >= W * bytes per pixel                                 */
    int64_t frame_stride;  /* bytes between frames, >= (H - 1) * row_pitch + W * bytes per pixel          */
} melf_frames;
/* Host frames, as melf_process_batch: only the crop rows (ccols * bytes per pixel, read at the caller's pitch) are
 * packed into the pinned staging buffers and cross PCIe. */
int melf_process_frames(melf_ctx* ctx, const void* frames_host, const melf_frames* f, melf_result* out_host);
/* Frames in HBM, exactly as melf_process_batch_dev: the same lanes, melf_ctx_set_frames_resident, caller streams,
 * and NULL d_results / out_host semantics. */
int melf_process_frames_dev(melf_ctx* ctx, const void* d_frames, const melf_frames* f, void* d_results,
                            melf_result* out_host, void* stream);

/* ---- the same path for YUV 4:2:0 video frames: NV12 (hardware decoders, capture stacks), I420 / YV12 (software decoders) ----
 * The records are byte-identical to melf_process_batch(_dev) on the packed BGR frame that the conversion below makes of each
 * frame, without a conversion pass: the kernels read the planes in place, and only the meter_rect crop of them.  In integers,
 * >> arithmetic, with the offset and the five coefficients of the descriptor's matrix:
 *     chroma: the nearest sample, no interpolation: pixel (x, y) uses U[y >> 1][x >> 1], V[y >> 1][x >> 1]
 *     yy = max(Y - YOFF, 0) * CY             u = U - 128          v = V - 128
 *     R = clamp((yy + (1 << 19) + CRV * v)           >> 20, 0, 255)
 *     G = clamp((yy + (1 << 19) + CGV * v + CGU * u) >> 20, 0, 255)
 *     B = clamp((yy + (1 << 19) + CBU * u)           >> 20, 0, 255)
 *
 *     code  matrix                    YOFF       CY      CRV      CGV      CGU      CBU
 *       0   MELF_YUV_BT601_LIMITED      16  1220542  1673527  -852492  -409993  2116026
 *       2   MELF_YUV_BT601_FULL          0  1048576  1470104  -748826  -360853  1858077
 *       3   MELF_YUV_BT709_LIMITED      16  1220945  1879825  -558796  -223607  2215014
 *       4   MELF_YUV_BT709_FULL          0  1048576  1651297  -490864  -196424  1945738
 * Frames as they come from: 0 cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420 / _YUY2 ..), SD video; 2 MJPEG webcams and phone cameras
 * (JFIF; ffmpeg's yuvj420p / yuvj422p, raw UVC); 3 H.264 / HEVC of HD cameras out of a hardware decoder; 4 screen and capture
 * pipelines.
 *
 * Code 1 is never assigned and stays MELF_ERR_INVALID (it was the one rejected code callers tested against while code 0 was the
 * only matrix).  Row 0 keeps the three-decimal constants of cv2 bit for bit.  Rows 2 - 4 are round(2^20 c) of the standards'
 * exact coefficients: with Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709) and Kg = 1 - Kr - Kb, c is 2 (1 - Kr) for
 * CRV, 2 (1 - Kb) for CBU, -Kb 2 (1 - Kb) / Kg for CGU, -Kr 2 (1 - Kr) / Kg for CGV and 1 for CY; limited range scales the
 * chroma coefficients by 255 / 224 and CY by 255 / 219.  Over all 2^24 (Y, U, V) every product fits a 24-bit multiply, every sum
 * stays below 2^30 in magnitude, and every channel is within 1 of the float64 conversion rounded half up and clipped (8 924
 * triples differ from it at all under code 2, 1 315 under code 3, none under code 4).  Code 2 is the JFIF matrix but not
 * libjpeg's tables bit for bit: libjpeg rounds the chroma terms separately at 16 bits, and 8 332 triples differ by 1 (the JPEG
 * entry points below decode with libjpeg's own arithmetic and are not affected by any of this).
 * Out of scope: BT.2020, interpolated chroma, chroma siting.  (Frames in separate allocations: melf_process_frame_list*, a
 * frame's planes in separate allocations: melf_process_plane_list*, both below.  4:2:2, 4:4:4 and 4:4:0 planes and
 * NV21: melf_process_yuv_planar*; 10-, 12- and 16-bit samples: melf_process_yuv16*, both below.)
 * Frame f starts at frames + f * frame_stride; its Y row y at + y * y_pitch (W bytes), its chroma row y >> 1 at
 * + u_offset / v_offset + (y >> 1) * c_pitch: NV12 W bytes U V U V .. (v_offset == u_offset + 1), I420 W / 2 bytes per plane.
 * YV12 is I420 with the two offsets exchanged.  The buffer must hold every plane of every frame up to the last sample of its
 * last row, and nothing behind that: no load of the kernels reaches past it.  Odd H or W, a pitch or stride too small, a chroma
 * plane that overlaps the Y plane or whose last sample lies beyond INT64_MAX, an unknown format or matrix or a NULL descriptor
 * return MELF_ERR_INVALID before anything is launched or copied. */
enum { MELF_YUV_NV12 = 0, MELF_YUV_I420 = 1 };
enum { MELF_YUV_BT601_LIMITED = 0, MELF_YUV_BT601_FULL = 2, MELF_YUV_BT709_LIMITED = 3, MELF_YUV_BT709_FULL = 4 };
                                                /* matrix; anything else, 1 included: MELF_ERR_INVALID    */
typedef struct melf_yuv_frames {
    int32_t format, matrix;
    int32_t n, H, W;                            /* H and W even                                           */
    int32_t reserved;
    int64_t y_pitch;                            /* bytes between Y rows, >= W                             */
    int64_t c_pitch;                            /* bytes between chroma rows: >= W (NV12), >= W / 2 (I420) */
    int64_t u_offset, v_offset;                 /* from a frame's first byte to its U / V samples;
                                                   NV12: v_offset == u_offset + 1, u_offset even          */
    int64_t frame_stride;                       /* bytes between frames                                   */
} melf_yuv_frames;
/* Host frames, as melf_process_batch: only the Y rows of the crop and the chroma rows under it cross PCIe (packed into the
 * pinned staging buffers as small frames of the same format); no byte is converted on the CPU. */
int melf_process_yuv(melf_ctx* ctx, const void* frames_host, const melf_yuv_frames* f, melf_result* out_host);
/* Frames in HBM, exactly as melf_process_frames_dev: the same lanes, melf_ctx_set_frames_resident, caller streams, and NULL
 * d_results / out_host semantics. */
int melf_process_yuv_dev(melf_ctx* ctx, const void* d_frames, const melf_yuv_frames* f, void* d_results, melf_result* out_host,
                         void* stream);
/* Stage entry point (parity tests, and a debug view for callers): the conversion alone, n packed H x W x 3 BGR frames out. */
int melf_yuv_to_bgr(melf_ctx* ctx, const void* frames_host, const melf_yuv_frames* f, uint8_t* bgr_out_host);

/* ---- the same path for packed YUV 4:2:2 frames: YUYV / YUY2 (UVC webcams, V4L2), UYVY (SDI / HDMI capture cards), YVYU ----
 * The records are byte-identical to melf_process_batch(_dev) on the packed BGR frame that the conversion makes of each frame
 * (the integer formulas above under the descriptor's matrix, any of the four; MELF_YUV_BT601_LIMITED is
 * cv2.cvtColor(COLOR_YUV2BGR_YUY2 / _UYVY / _YVYU)), which replaces the BGR copy of every frame such a caller had to write: that
 * frame is never formed, the kernels read the
 * macropixels in place, and only the meter_rect crop of them.
 *     chroma: the two pixels of a macropixel share its U and V; no interpolation, no vertical subsampling
 * Frame f starts at frames + f * frame_stride, its row y at + y * row_pitch: W / 2 macropixels of 4 bytes, two pixels each, in
 * the byte order of the format.  Pixel (x, y) has its Y in the macropixel at + 4 * (x >> 1) and uses that macropixel's U and V.
 * The base pointer, row_pitch and frame_stride must be 4-byte aligned (as for the 4-byte RGB formats): a macropixel is then one
 * aligned dword.  The buffer must hold (n - 1) * frame_stride + (H - 1) * row_pitch + 2 * W bytes, and nothing behind that: no
 * load of the kernels reaches past it.  An odd W, a pitch or stride too small, a misaligned base, pitch or stride, an unknown
 * format or matrix, H or W <= 0, n < 0, a NULL descriptor or NULL frames return MELF_ERR_INVALID (melf_last_error says which)
 * before anything is launched or copied; n == 0 passes. */
enum { MELF_YUV422_YUYV = 0, MELF_YUV422_UYVY = 1, MELF_YUV422_YVYU = 2 };   /* bytes of a macropixel: Y0 U Y1 V / U Y0 V Y1 / Y0 V Y1 U */
typedef struct melf_yuv422_frames {
    int32_t format, matrix;                     /* MELF_YUV422_*; matrix: MELF_YUV_BT* as above           */
    int32_t n, H, W;                            /* W even, H any                                          */
    int32_t reserved;
    int64_t row_pitch;                          /* bytes between rows, >= 2 * W                           */
    int64_t frame_stride;                       /* bytes between frames                                   */
} melf_yuv422_frames;
/* Host frames, as melf_process_yuv: only the crop crosses PCIe, packed into the pinned staging buffers as a small frame of the
 * same format (its x origin rounded down and its far corner up to a whole macropixel, every row of the crop: no vertical
 * rounding); no byte is converted or reordered on the CPU. */
int melf_process_yuv422(melf_ctx* ctx, const void* frames_host, const melf_yuv422_frames* f, melf_result* out_host);
/* Frames in HBM, exactly as melf_process_yuv_dev: the same lanes, melf_ctx_set_frames_resident, caller streams, and NULL
 * d_results / out_host semantics. */
int melf_process_yuv422_dev(melf_ctx* ctx, const void* d_frames, const melf_yuv422_frames* f, void* d_results, melf_result* out_host,
                            void* stream);
/* Stage entry point (parity tests, and a debug view for callers): the conversion alone, n packed H x W x 3 BGR frames out. */
int melf_yuv422_to_bgr(melf_ctx* ctx, const void* frames_host, const melf_yuv422_frames* f, uint8_t* bgr_out_host);

/* ---- the same path for planar and semi-planar YUV frames of any 8-bit chroma subsampling: what software JPEG / MJPEG decoders
 * leave of a webcam's 4:2:2 (I422, ffmpeg's yuv422p / yuvj422p), screen capture and high-quality JPEG of 4:4:4 (I444, NV24), Rockchip
 * and V4L2 decoders (NV16), Android's camera API (NV21) ----
 * The contract of melf_process_yuv*: the records are byte-identical to melf_process_batch(_dev) on the packed BGR frame that the
 * integer conversion above makes of each frame under the descriptor's matrix (any of the four; code 1 stays invalid).  That frame
 * is never formed: the kernels read the planes in place, and only the meter_rect crop of them.
 *     chroma: the nearest sample, no interpolation: pixel (x, y) uses U[y >> sub_y][x >> sub_x], V[y >> sub_y][x >> sub_x]
 * One general descriptor instead of a format code.  Frame f starts at frames + f * frame_stride; its Y row y at + y * y_pitch (W
 * bytes); U of pixel (x, y) is the byte at + u_offset + (y >> sub_y) * c_pitch + (x >> sub_x) * c_step, V the same from v_offset.
 *     sub_x, sub_y  log2 of the chroma subsampling: 4:4:4 (0, 0)   4:2:2 (1, 0)   4:2:0 (1, 1)   4:4:0 (0, 1)
 *     c_step        1: planar, U and V in planes of their own; 2: semi-planar, U and V interleaved in one plane: the two offsets are
 *                   adjacent, and which is the lower says which byte of a pair comes first
 *     4:2:2  I422 / yuv422p / yuvj422p (c_step 1, U first), YV16 (V first), NV16 (c_step 2, U first), NV61 (V first)
 *     4:4:4  I444 / yuv444p / yuvj444p, YV24, NV24, NV42            4:4:0  I440 / yuvj440p
 *     4:2:0  NV21 (c_step 2, V first); NV12, I420 and YV12 can be described as well and give the records of melf_process_yuv*
 * Planes are bytes: any alignment of the base, the offsets, the pitches and frame_stride is taken.  The buffer must hold every
 * plane of every frame up to the last sample of its last row, and need hold nothing behind that nor before the base: no load of
 * the kernels reaches outside it.  MELF_ERR_INVALID (melf_last_error says which) before anything is launched or copied for: a NULL
 * descriptor or NULL frames; reserved != 0; sub_x or sub_y outside {0, 1}; c_step outside {1, 2}; c_step 2 with offsets that are not
 * adjacent; an odd W with sub_x, an odd H with sub_y; H or W <= 0, n < 0 (n == 0 passes); a negative offset; an unknown matrix;
 * y_pitch < W; c_pitch smaller than a chroma row ((W >> sub_x) * c_step bytes); a pitch > 2^31 - 1; a chroma plane closer to the
 * other than its span (overlapping) or starting inside the Y plane's span; a frame_stride smaller than the span of one frame. */
typedef struct melf_yuv_planar_frames {
    int32_t matrix;                             /* MELF_YUV_BT* as above                                  */
    int32_t n, H, W;                            /* W even if sub_x, H even if sub_y                       */
    int32_t sub_x, sub_y;                       /* log2 chroma subsampling, 0 or 1 each                   */
    int32_t c_step;                             /* bytes from one sample of a chroma plane to the next in
                                                   its row: 1 planar, 2 semi-planar                       */
    int32_t reserved;                           /* 0                                                      */
    int64_t y_pitch;                            /* bytes between Y rows, >= W                             */
    int64_t c_pitch;                            /* bytes between chroma rows, >= (W >> sub_x) * c_step    */
    int64_t u_offset, v_offset;                 /* from a frame's first byte to its first U / V sample;
                                                   c_step 2: |u_offset - v_offset| == 1                   */
    int64_t frame_stride;                       /* bytes between frames                                   */
} melf_yuv_planar_frames;
/* Host frames, as melf_process_yuv: only the crop crosses PCIe, packed into the pinned staging buffers as a small frame of the same
 * layout (its origin rounded down and its far corner up to whole chroma blocks of 1 << sub_x by 1 << sub_y pixels: the Y rows of
 * that rectangle and the chroma rows under them); no byte is converted or reordered on the CPU. */
int melf_process_yuv_planar(melf_ctx* ctx, const void* frames_host, const melf_yuv_planar_frames* f, melf_result* out_host);
/* Frames in HBM, exactly as melf_process_yuv_dev: the same lanes, melf_ctx_set_frames_resident, caller streams, and NULL
 * d_results / out_host semantics. */
int melf_process_yuv_planar_dev(melf_ctx* ctx, const void* d_frames, const melf_yuv_planar_frames* f, void* d_results,
                                melf_result* out_host, void* stream);
/* Stage entry point (parity tests, and a debug view for callers): the conversion alone, n packed H x W x 3 BGR frames out. */
int melf_yuv_planar_to_bgr(melf_ctx* ctx, const void* frames_host, const melf_yuv_planar_frames* f, uint8_t* bgr_out_host);

/* ---- the same path for planar and semi-planar YUV frames of 10, 12 or 16 bits per sample: what a hardware HEVC / AV1 Main10
 * decoder leaves (P010: semi-planar 4:2:0, the value in the high bits of a 16-bit word), ffmpeg's software decoders (yuv420p10le /
 * I010: planar, the value in the low bits), capture cards (P210, P216) ----
 * Samples are little-endian uint16.  A sample s is read as the 8-bit sample
 *     s8 = min(s >> shift, 255)
 * truncation, a pure selection of bits: for P010 (shift 8) it is the sample's high byte.  The clamp matters only for LSB-aligned
 * data with out-of-spec high bits.  The records are byte-identical to melf_process_yuv_planar(_dev) on the 8-bit frame of the same
 * geometry (sub_x 1, the same sub_y and planar / semi-planar form and order of U and V) whose samples are s8 -- and so, by that
 * entry point's contract, to melf_process_batch(_dev) on the BGR frame the integer conversion above makes of it under the
 * descriptor's matrix (the existing table, any of the four codes; 1 stays invalid).
 *     chroma: the nearest sample, no interpolation: pixel (x, y) uses U[y >> sub_y][x >> 1], V[y >> sub_y][x >> 1]
 * Neither that 8-bit frame nor a BGR frame is ever formed: the kernels read the 16-bit planes in place, and only the meter_rect
 * crop of them.
 * Frame f starts at frames + f * frame_stride (bytes); its Y row y at + y * y_pitch: W samples of 2 bytes; U of pixel (x, y) is
 * the sample at byte + u_offset + (y >> sub_y) * c_pitch + (x >> 1) * c_step * 2, V the same from v_offset.
 *     c_step   SAMPLES from one sample of a chroma plane to the next in its row: 1 planar, 2 semi-planar (U and V interleaved in
 *              one plane: the two offsets are 2 bytes apart, and which is the lower says which sample of a pair comes first)
 *     shift    low bits dropped, 0 .. 8:  8 for MSB-aligned and full 16-bit samples (P010, P012, P016, P210, P216, yuv420p16le,
 *              yuv422p16le), 4 for 12 bits in the low bits (yuv420p12le, yuv422p12le), 2 for 10 bits in the low bits (I010 /
 *              yuv420p10le, I210 / yuv422p10le)
 * Alignment: the base, the offsets, the pitches and frame_stride are 2-byte aligned (whole samples), and need be no more than that.
 * The buffer must hold every plane of every frame up to the last sample of its last row, and need hold nothing behind that nor
 * before the base: no load of the kernels reaches outside (n - 1) * frame_stride + the last sample of the last frame, nor before
 * the base.  MELF_ERR_INVALID (melf_last_error says which) before anything is launched or copied for: a NULL descriptor or NULL
 * frames; reserved != 0; sub_y outside {0, 1}; c_step outside {1, 2}; shift outside 0 .. 8; c_step 2 with offsets that are not
 * 2 bytes apart; an odd W, an odd H with sub_y; H or W <= 0, n < 0 (n == 0 passes); a negative offset; an unknown matrix; an odd
 * base, y_pitch, c_pitch, u_offset, v_offset or frame_stride; y_pitch < 2 * W bytes; c_pitch smaller than a chroma row ((W >> 1) *
 * c_step samples of 2 bytes); a pitch > 2^31 - 1; a chroma plane closer to the other than its span (overlapping) or starting
 * inside the Y plane's span; a frame_stride smaller than the span of one frame.
 * Out of scope: sub_x = 0 (planar and semi-planar 4:4:4 / 4:4:0 at 16 bits: yuv444p10le, P410); big-endian samples; BT.2020 (and any
 * transfer function: the samples are taken as they are); rounding or dithering of the dropped bits.  (The packed 10-bit formats,
 * v210 and Y210 / Y212 / Y216: melf_process_yuv422_10*, below.  4:4:4 at 10 bits as one 32-bit word per pixel, Y410 / XV30:
 * melf_process_packed32*, below.) */
typedef struct melf_yuv16_frames {
    int32_t matrix;                             /* MELF_YUV_BT* as above (the four codes; 1 stays invalid) */
    int32_t n, H, W;                            /* W even; H even if sub_y                                */
    int32_t sub_y;                              /* 0: 4:2:2, 1: 4:2:0 (sub_x is 1: see scope)             */
    int32_t c_step;                             /* SAMPLES from one sample of a chroma plane to the next
                                                   in its row: 1 planar, 2 semi-planar                    */
    int32_t shift;                              /* 0 .. 8: low bits dropped (8, 12-bit LSB: 4, 10-bit LSB: 2) */
    int32_t reserved;                           /* 0                                                      */
    int64_t y_pitch;                            /* BYTES between Y rows, even, >= 2 * W                   */
    int64_t c_pitch;                            /* BYTES between chroma rows, even, >= W * c_step         */
    int64_t u_offset, v_offset;                 /* BYTES, even, from a frame's first byte to its first
                                                   U / V sample; c_step 2: |u_offset - v_offset| == 2     */
    int64_t frame_stride;                       /* BYTES between frames, even                             */
} melf_yuv16_frames;
/* Host frames, as melf_process_yuv_planar: only the crop crosses PCIe, packed into the pinned staging buffers as a small frame of
 * the same layout (16-bit samples as they are: the Y rows of the crop rounded out to whole chroma blocks and the chroma rows under
 * them); no sample is reduced, converted or reordered on the CPU. */
int melf_process_yuv16(melf_ctx* ctx, const void* frames_host, const melf_yuv16_frames* f, melf_result* out_host);
/* Frames in HBM, exactly as melf_process_yuv_planar_dev: the same lanes, melf_ctx_set_frames_resident, caller streams, and NULL
 * d_results / out_host semantics. */
int melf_process_yuv16_dev(melf_ctx* ctx, const void* d_frames, const melf_yuv16_frames* f, void* d_results, melf_result* out_host,
                           void* stream);
/* Stage entry point (parity tests, and a debug view for callers): reduction and conversion alone, n packed H x W x 3 BGR frames out. */
int melf_yuv16_to_bgr(melf_ctx* ctx, const void* frames_host, const melf_yuv16_frames* f, uint8_t* bgr_out_host);

/* ---- the same path for packed 10-bit YUV 4:2:2 frames: v210, the native 10-bit format of SDI / HDMI capture cards (DeckLink
 * bmdFormat10BitYUV, AJA, ffmpeg's v210), and Y210 / Y212 / Y216, what hardware 4:2:2 10-bit decoders leave (D3D11, VAAPI, oneVPL) ----
 * Every sample is read as an 8-bit sample s8 by truncation, a pure selection of bits, and the records are byte-identical to
 * melf_process_yuv422(_dev) on the 8-bit YUYV frame with the same n, H, W and matrix whose samples are the s8 -- and so, by that
 * entry point's contract, to melf_process_batch(_dev) on the BGR frame the integer conversion above makes of it under the
 * descriptor's matrix (any of the four codes; 1 stays invalid).  Neither that 8-bit frame nor a BGR frame is ever formed: the
 * kernels read the packed frames in place, and only the meter_rect crop of them.
 *     chroma: the two pixels of a pair share its U and V; no interpolation, no vertical subsampling
 * MELF_YUV422_10_V210: row y of frame f starts at frames + f * frame_stride + y * row_pitch and is ceil(W / 6) whole groups of 16
 * bytes.  A group is four little-endian 32-bit words, each with three 10-bit fields at bits 0-9, 10-19 and 20-29; bits 30-31 are
 * ignored, whatever they hold.  A group holds pixels 6 g .. 6 g + 5 as three pairs, pair q = pixels 6 g + 2 q and 6 g + 2 q + 1
 * sharing U and V; its fields, as (word, bit offset):
 *     pair   first Y   second Y   U        V
 *     0      w0, 10    w1, 0      w0, 0    w0, 20
 *     1      w1, 20    w2, 10     w1, 10   w2, 0
 *     2      w3, 0     w3, 20     w2, 20   w3, 10
 * (the twelve fields in order are U Y V Y U Y V Y U Y V Y).  s8 = (field >> 2) & 255.  Fields of pixels >= W in a row's last
 * group are never looked at.  W is even, H any; row_pitch >= ceil(W / 6) * 16 (the conventional pitch is ((W + 47) / 48) * 128);
 * the base, row_pitch and frame_stride are multiples of 16, so that a group is one aligned 16-byte load.  A frame extends over
 * (H - 1) * row_pitch + ceil(W / 6) * 16 bytes.
 * MELF_YUV422_10_Y210 (also Y212 and Y216): a row is W / 2 macropixels of four MSB-aligned little-endian 16-bit words Y0 U Y1 V,
 * 8 bytes for two pixels.  s8 = s >> 8, the word's high byte: under truncation the three formats are one.  W is even;
 * row_pitch >= 4 * W; the base, row_pitch and frame_stride are multiples of 8.  A frame extends over (H - 1) * row_pitch + 4 * W
 * bytes.
 * The buffer must hold (n - 1) * frame_stride + one frame's extent, and need hold nothing behind that nor before the base: no
 * load of the kernels reaches outside.  MELF_ERR_INVALID (melf_last_error says which) before anything is launched or copied for:
 * a NULL descriptor or NULL frames; an unknown format or matrix; reserved != 0; H or W <= 0, n < 0 (n == 0 passes); an odd W; a
 * row_pitch smaller than a row or > 2^31 - 1; a frame_stride smaller than a frame; a misaligned base, row_pitch or frame_stride.
 * Out of scope: big-endian and LSB-aligned Y21x; the big-endian r210 RGB format; rounding or dithering of the dropped bits; BT.2020
 * and transfer functions; interpolated chroma.  (Y410 and the other 4:4:4 formats of one 32-bit word per pixel, X2RGB10 among
 * them: melf_process_packed32*, below.) */
enum { MELF_YUV422_10_V210 = 0, MELF_YUV422_10_Y210 = 1 };   /* Y210: also Y212, Y216 */
typedef struct melf_yuv422_10_frames {
    int32_t format, matrix;                     /* MELF_YUV422_10_*; matrix: MELF_YUV_BT* as above        */
    int32_t n, H, W;                            /* W even, H any                                          */
    int32_t reserved;                           /* 0                                                      */
    int64_t row_pitch;                          /* bytes between rows: v210 >= ceil(W / 6) * 16 and a
                                                   multiple of 16; Y210 >= 4 * W and a multiple of 8      */
    int64_t frame_stride;                       /* bytes between frames, aligned like row_pitch           */
} melf_yuv422_10_frames;
/* Host frames, as melf_process_yuv422: only the crop crosses PCIe, packed into the pinned staging buffers as a small frame of the
 * same format (its x origin rounded down and its far corner up to whole groups of 6 pixels (v210) or whole macropixels (Y210),
 * the rows copied as they are); no sample is unpacked on the CPU. */
int melf_process_yuv422_10(melf_ctx* ctx, const void* frames_host, const melf_yuv422_10_frames* f, melf_result* out_host);
/* Frames in HBM, exactly as melf_process_yuv422_dev: the same lanes, melf_ctx_set_frames_resident, caller streams, and NULL
 * d_results / out_host semantics. */
int melf_process_yuv422_10_dev(melf_ctx* ctx, const void* d_frames, const melf_yuv422_10_frames* f, void* d_results,
                               melf_result* out_host, void* stream);
/* Stage entry point (parity tests, and a debug view for callers): unpacking and conversion alone, n packed H x W x 3 BGR frames out. */
int melf_yuv422_10_to_bgr(melf_ctx* ctx, const void* frames_host, const melf_yuv422_10_frames* f, uint8_t* bgr_out_host);

/* ---- the same path for 4:4:4 frames of ONE 32-BIT WORD PER PIXEL: AYUV / VUYA (8-bit) and Y410 / XV30 (10-bit) as D3D11, VA-API and
 * oneVPL deliver HEVC RExt, AV1 and VP9 4:4:4; XRGB2101010 / XBGR2101010 (R10G10B10A2) as DRM scan-out, DXGI desktop duplication and
 * 10-bit camera ISPs deliver RGB ----
 * A pixel is one little-endian 32-bit word.  It holds three 8-bit reads at bit positions pos[0..2], each a pure selection of bits:
 *     s8_k = (word >> pos[k]) & 255
 * For a 10-bit field at bit o, pos = o + 2: the field's top 8 bits, by truncation, as for v210 and P010.  For byte b, pos = 8 b.
 * Every other bit of the word is ignored, whatever it holds: alpha / X bits and the low bits of 10-bit fields.
 * MELF_P32_YUV: the reads are Y, U, V, and the records are byte-identical to melf_process_yuv_planar(_dev) on the 8-bit 4:4:4 planar
 * frame (i444: sub_x = sub_y = 0) with the same n, H, W and matrix whose samples are the s8 -- and so, by that entry point's
 * contract, to melf_process_batch(_dev) on the BGR frame the integer conversion above makes of it (any of the four matrix codes; 1
 * stays invalid).  MELF_P32_RGB: the reads are R, G, B, and the records are byte-identical to melf_process_batch(_dev) on the packed
 * BGR frame of the s8; nothing is converted and matrix must be 0.  Neither the 8-bit frame nor a BGR frame is ever formed: the
 * kernels read the words in place, and only the meter_rect crop of them.
 * The layouts by name, as drm_fourcc.h and ffmpeg's pixfmt.h state them (pos: Y, U, V / R, G, B):
 *     name                                   colour  pos         the word
 *     VUYA / VUYX                            YUV     16,  8,  0  bytes V U Y A in memory (what Microsoft and DRM call AYUV)
 *     AYUV                                   YUV      8, 16, 24  bytes A Y U V in memory (ffmpeg's and GStreamer's byte order)
 *     UYVA                                   YUV      8,  0, 16  bytes U Y V A in memory
 *     Y410 / XV30                            YUV     12,  2, 22  U bits 0-9, Y 10-19, V 20-29, A 30-31
 *     V30X                                   YUV     14,  4, 24  X bits 0-1, U 2-11, Y 12-21, V 22-31
 *     X2RGB10 (XRGB2101010)                  RGB     22, 12,  2  B bits 0-9, G 10-19, R 20-29, X 30-31
 *     X2BGR10 (XBGR2101010, R10G10B10A2)     RGB      2, 12, 22  R bits 0-9, G 10-19, B 20-29, X 30-31
 * and any other layout three non-overlapping positions express.  Row y of frame f starts at frames + f * frame_stride + y *
 * row_pitch and is W words; any W, any H.  The base, row_pitch and frame_stride are multiples of 4.  A frame extends over
 * (H - 1) * row_pitch + 4 * W bytes; the buffer must hold (n - 1) * frame_stride + that extent, and need hold nothing behind that
 * nor before the base: no load of the kernels reaches outside.  MELF_ERR_INVALID (melf_last_error says which) before anything is
 * launched or copied for: a NULL descriptor or NULL frames; a colour outside the two codes; an unknown matrix for YUV, a non-zero
 * matrix for RGB; a non-zero reserved field; a pos[k] outside 0 .. 24; two reads that overlap (|pos[i] - pos[j]| < 8); H or W <= 0,
 * n < 0 (n == 0 passes); a row_pitch smaller than a row or > 2^31 - 1; a frame_stride smaller than a frame; a base, row_pitch or
 * frame_stride that is not 4-byte aligned.
 * Measured on one MI355X (1024-frame config-3 steps, profiles/packed32/packed32_rate.txt): Y410 in place 0.2614 ms a step, VUYA
 * 0.2619, X2RGB10 0.2500 -- 1.05, 1.05 and 1.01 times BGRA through melf_process_frames (0.2484 ms), which moves the same bytes per
 * pixel -- where unpacking every whole Y410 frame to three planes first and reading those takes 4.2432 ms, 16.2 times as long.
 * Out of scope: 64-bit pixels (Y416, XV36 / XV48, RGBA64); planar and semi-planar 4:4:4 at 16 bits (yuv444p10le, P410: their quads
 * are 24 - 32 bytes per lane and need a different window hand-over); big-endian r210; alpha; RGB565; rounding or dithering of the
 * dropped bits; BT.2020 and transfer functions. */
enum { MELF_P32_YUV = 0, MELF_P32_RGB = 1 };
typedef struct melf_packed32_frames {
    int32_t colour, matrix;                     /* MELF_P32_*; MELF_YUV_BT* for YUV, 0 for RGB            */
    int32_t n, H, W;                            /* any W, any H                                           */
    int32_t pos[3];                             /* 0 .. 24: low bit of the 8 bits read of Y,U,V / R,G,B   */
    int64_t row_pitch;                          /* bytes, multiple of 4, >= 4 * W, <= 2^31 - 1            */
    int64_t frame_stride;                       /* bytes, multiple of 4, >= (H - 1) * row_pitch + 4 * W   */
    int32_t reserved, reserved2;                /* 0                                                      */
} melf_packed32_frames;
/* Host frames, as melf_process_yuv422_10: only the crop crosses PCIe, its rows copied as they are into the pinned staging buffers;
 * no word is unpacked on the CPU. */
int melf_process_packed32(melf_ctx* ctx, const void* frames_host, const melf_packed32_frames* f, melf_result* out_host);
/* Frames in HBM, exactly as melf_process_yuv422_10_dev: the same lanes, melf_ctx_set_frames_resident, caller streams, and NULL
 * d_results / out_host semantics. */
int melf_process_packed32_dev(melf_ctx* ctx, const void* d_frames, const melf_packed32_frames* f, void* d_results,
                              melf_result* out_host, void* stream);
/* Stage entry point (parity tests, and a debug view for callers): unpacking and conversion alone, n packed H x W x 3 BGR frames out. */
int melf_packed32_to_bgr(melf_ctx* ctx, const void* frames_host, const melf_packed32_frames* f, uint8_t* bgr_out_host);

/* ---- the same path for planar, channels-first frames: (N, 3, H, W) uint8 as torch's decoders and pre-processing pipelines
 * hold them, ffmpeg's gbrp, rgb24 split into planes ----
 * The records are byte-identical to melf_process_batch(_dev) on the packed BGR frame whose pixel (x, y) is
 * (B[y][x], G[y][x], R[y][x]); that frame is never formed: the kernels read the three planes in place, and only the meter_rect
 * crop of them.  No colour conversion is involved.
 * Frame f starts at frames + f * frame_stride; row y of its B / G / R plane at + b_offset / g_offset / r_offset + y * row_pitch,
 * W bytes.  The three offsets give the channel order and there is no format code: RGB planes of P bytes each are r_offset = 0,
 * g_offset = P, b_offset = 2 P, BGR planes the reverse, ffmpeg's gbrp G, B, R; a 4-plane RGBA / RGBx tensor names three of its
 * four planes and the fourth is never looked at.  Planes are bytes: any alignment of the base, the offsets, row_pitch and
 * frame_stride is taken.  The buffer must hold every named plane of every frame up to the last sample of its last row,
 * (n - 1) * frame_stride + max(offset) + (H - 1) * row_pitch + W bytes, and need hold nothing behind that nor before the base:
 * no load of the kernels reaches outside it.  H or W <= 0, n < 0, a NULL descriptor or NULL frames, reserved != 0, a negative
 * offset, row_pitch < W or > 2^31 - 1, two planes closer together than (H - 1) * row_pitch + W (overlapping) or a frame_stride
 * smaller than the span of one frame's planes return MELF_ERR_INVALID (melf_last_error says which) before anything is launched
 * or copied; n == 0 passes.
 * melf_process_stream_dev, the fused full-frame mask, melf_aligned_average and the JPEG entry points stay packed BGR only. */
typedef struct melf_planar_frames {
    int32_t n, H, W;
    int32_t reserved;                           /* 0                                                      */
    int64_t b_offset, g_offset, r_offset;       /* bytes from a frame's first byte to the first sample of
                                                   its B / G / R plane, >= 0                              */
    int64_t row_pitch;                          /* bytes between rows of a plane (the same for the three), >= W */
    int64_t frame_stride;                       /* bytes between frames                                   */
} melf_planar_frames;
/* Host frames, as melf_process_frames: only the crop crosses PCIe -- the crop's rows of the three planes, packed into the pinned
 * staging buffers as a small planar frame, which the kernels read; no byte is interleaved on the CPU. */
int melf_process_planes(melf_ctx* ctx, const void* frames_host, const melf_planar_frames* f, melf_result* out_host);
/* Frames in HBM, exactly as melf_process_frames_dev: the same lanes, melf_ctx_set_frames_resident, caller streams, and NULL
 * d_results / out_host semantics. */
int melf_process_planes_dev(melf_ctx* ctx, const void* d_frames, const melf_planar_frames* f, void* d_results, melf_result* out_host,
                            void* stream);

/* ---- the same path for RGB frames of WIDE samples: 16-bit words (RGB16 / BGR12 of machine-vision SDKs, ffmpeg's rgb48le, bgra64le,
 * gbrp10le / gbrp12le / gbrp16le, decoded 16-bit PNG and TIFF) and floating point (float16, bfloat16, float32 images of a torch
 * program, (N, 3, H, W) or (N, H, W, 3), often still under a Normalize(mean, std)) ----
 * A sample of channel c becomes one byte, and from there on the frame is an 8-bit frame of the same geometry:
 *     MELF_WIDE_U16   little-endian 16-bit word s:   min(s >> shift, 255), shift 0 .. 8: the rule of melf_process_yuv16
 *     MELF_WIDE_F16, MELF_WIDE_BF16, MELF_WIDE_F32:
 *         x = the sample widened to float32 (exact; bfloat16 is its bits << 16)
 *         t = x * scale[c]      rounded to float32
 *         q = t + offset[c]     rounded to float32 -- two roundings, never a fused multiply-add
 *         r = rintf(q) (ties to even: what torch.round and np.rint do) under MELF_ROUND_NEAREST, floorf(q) under MELF_ROUND_FLOOR
 *         the byte is 0 if r is NaN or r < 0, 255 if r > 255, otherwise r: -inf gives 0, +inf 255
 * numpy reproduces it exactly in float32 (x * s, then + o; np.rint / np.floor; NaN to 0; clip).  scale and offset are three float32
 * each, in B, G, R order whatever the order of the frames' channels; they must be finite, |scale| <= 2^24 (under that bound the
 * byte does not depend on whether denormals are flushed).  They are not looked at for MELF_WIDE_U16, nor is shift for the others.
 *     scale = 255, offset = 0, nearest           x.mul(255).round().clamp(0, 255) of a [0, 1] image
 *     scale = std * 255, offset = mean * 255     the same of an image under Normalize(mean, std)
 *     scale = 255.999, floor                     torchvision's convert_image_dtype
 *     scale = 255, floor                         .mul(255).byte() for in-range values
 * The wrong choice raises no error: it moves samples by one, and with them what the dials are read from -- as the wrong matrix does
 * for YUV frames.
 * The records are byte-identical to melf_process_frames(_dev) (packed) / melf_process_planes(_dev) (planar) on the 8-bit frames of
 * those bytes.  A narrowing kernel (k_narrow_rows, timed as MELF_K_GATHER: one launch per chunk of 1024 frames) reads the meter_rect
 * crop of every frame in place -- 2 or 4 bytes a sample, no other byte of a frame -- and writes the crop's bytes into the lane's
 * staged batch, the staged frames of melf_process_frame_list_dev; the unchanged kernels read those.
 *     layout MELF_WIDE_PACKED   pixel_format MELF_PIX_*: 3 or 4 samples a pixel in that order; the 4th sample is never converted.
 *                               Row y of frame f at frames + f * frame_stride + y * row_pitch.  The offsets are not looked at.
 *     layout MELF_WIDE_PLANAR   b_offset / g_offset / r_offset, row_pitch, frame_stride exactly as in melf_planar_frames (a 4th
 *                               plane is never touched); pixel_format is not looked at.
 * Everything is in BYTES and a multiple of the sample size (2, float32: 4), the base included; no larger alignment is needed: a
 * torch view x[:, :, y0:, x0:] passes.  The buffer must hold every sample of every named plane / pixel of every frame and nothing
 * more: no load reaches behind the last sample of a row, outside a frame's extent or before the base.  MELF_ERR_INVALID
 * (melf_last_error says which) before anything is launched or copied for: a NULL descriptor or NULL frames; an unknown sample_type,
 * layout, pixel_format (packed) or rounding; shift outside 0 .. 8; reserved or reserved2 != 0; a scale or offset that is not
 * finite, |scale| > 2^24; H or W <= 0, n < 0 (n == 0 passes); a negative plane offset; a base, offset, row_pitch or frame_stride
 * that is no multiple of the sample size; row_pitch smaller than a row or > 2^31 - 1; planes closer together than the span of one
 * (overlapping); a frame_stride smaller than the span of a frame.
 * Measured at 1024-frame steps of 640 x 480 frames, buffers in rotation beyond the cache (profiles/wide_frames/wide_rate.txt): the
 * wide batch takes 1.54 - 2.00 times the 8-bit batch of the same samples in place (16-bit words 1.75 packed / 1.54 planar, float16
 * 1.85 / 1.62, float32 2.00 / 1.77), where torch's conversion of every whole frame to uint8 followed by that 8-bit read takes 5.1 -
 * 13.1 times the wide batch; k_narrow_rows alone takes 0.16 - 0.28 ms a launch.
 * Wide frames in separate allocations, and wide planes in separate allocations: melf_process_wide_list* and
 * melf_process_wide_plane_list*, below.
 * Out of scope: big-endian samples; wide frames in the oriented calls; wide YUV beyond melf_process_yuv16*. */
enum { MELF_WIDE_U16 = 0, MELF_WIDE_F16 = 1, MELF_WIDE_BF16 = 2, MELF_WIDE_F32 = 3 };
enum { MELF_WIDE_PACKED = 0, MELF_WIDE_PLANAR = 1 };
enum { MELF_ROUND_NEAREST = 0, MELF_ROUND_FLOOR = 1 };
typedef struct melf_wide_frames {
    int32_t sample_type;                        /* MELF_WIDE_*                                            */
    int32_t layout;                             /* MELF_WIDE_PACKED / MELF_WIDE_PLANAR                    */
    int32_t pixel_format;                       /* packed: MELF_PIX_*                                     */
    int32_t shift;                              /* MELF_WIDE_U16: 0 .. 8, low bits dropped                */
    int32_t rounding;                           /* MELF_ROUND_*                                           */
    int32_t reserved;                           /* 0                                                      */
    float scale[3], offset[3];                  /* B, G, R; the float types                               */
    int32_t n, H, W;
    int32_t reserved2;                          /* 0                                                      */
    int64_t b_offset, g_offset, r_offset;       /* planar: BYTES from a frame's first byte to the first
                                                   sample of its B / G / R plane, >= 0                    */
    int64_t row_pitch;                          /* BYTES between rows (planar: of a plane)                */
    int64_t frame_stride;                       /* BYTES between frames                                   */
} melf_wide_frames;
/* Host frames: only the crop crosses PCIe, and as bytes -- the host threads narrow the crop's rows (the same rule, from the same
 * header, meterelf_amd/csrc/melf_narrow.h) while they pack them into the pinned staging buffers. */
int melf_process_wide(melf_ctx* ctx, const void* frames_host, const melf_wide_frames* f, melf_result* out_host);
/* Frames in HBM, with the lanes, caller streams and NULL d_results / out_host semantics of melf_process_frames_dev; under
 * melf_ctx_set_frames_resident the narrowing waits for what the caller's stream held at the call, as the gather of
 * melf_process_frame_list_dev does. */
int melf_process_wide_dev(melf_ctx* ctx, const void* d_frames, const melf_wide_frames* f, void* d_results, melf_result* out_host,
                          void* stream);
/* Stage entry point (parity tests, and a debug view for callers): the narrowing alone, through the GPU kernel, n packed H x W x 3 BGR
 * frames out. */
int melf_wide_to_bgr(melf_ctx* ctx, const void* frames_host, const melf_wide_frames* f, uint8_t* bgr_out_host);

/* ---- wide frames in SEPARATE ALLOCATIONS: one (H, W, 3) uint16 array per decoded 16-bit PNG or TIFF, one RGB16 buffer per frame of
 * a machine-vision SDK, a list of float16 / float32 (3, H, W) tensors from a torch Dataset or a video reader; and wide planar frames
 * whose PLANES lie in separate allocations: libav's gbrp10le / gbrp12le / gbrp16le AVFrame with its three plane pointers ----
 * melf_wide_frames beside a HOST array of pointers (device pointers for _dev, host pointers otherwise), as melf_process_frame_list*
 * and melf_process_plane_list* take the 8-bit descriptors; the library copies the array before it returns.  These entry points take
 * the wide descriptor directly: there is no MELF_LIST_* code for it.
 *   Frame list (melf_process_wide_list*): either layout.  n is the list's length; frame_stride is not looked at; everything else is
 *     checked as for a batch of one frame, with melf_process_wide's messages.  Every pointer is checked for NULL and for alignment to
 *     the sample size, the message led by "frame i of the list:".  From each pointer one frame's extent is readable -- up to the last
 *     sample of the frame's last row (packed) or of its last plane (planar) -- and nothing behind it nor before the pointer is read.
 *     Frames may alias or repeat.
 *   Plane list (melf_process_wide_plane_list*): MELF_WIDE_PLANAR only, nplanes == 3, planes[i * 3 + k] plane slot k of frame i, slots
 *     0 / 1 / 2 = B / G / R as for melf_planar_frames plane lists.  b_offset, g_offset and r_offset count from each plane's own
 *     pointer and must be 0; there is one row_pitch for the three planes.  A packed descriptor is MELF_ERR_INVALID (the message names
 *     melf_process_wide_list), as is any other nplanes.  From each plane pointer (H - 1) * row_pitch + W * sample size bytes are
 *     readable, and nothing more.  Every pointer is checked for NULL and alignment to the sample size, the message led by "frame i,
 *     plane k of the list:".  Planes may alias or repeat.
 * The records are byte-identical to melf_process_wide(_dev) on one contiguous batch holding the same samples in list order.
 * Everything else is melf_process_frame_list_dev's: the lanes and caller streams; under melf_ctx_set_frames_resident the narrowing
 * waits for what the caller's stream held at the call; lists longer than 1024 frames go through the lane's staging buffer in chunks
 * of 1024; the NULL d_results / out_host semantics; n == 0 passes; nothing is launched or copied for a rejected call.  Two siblings
 * of k_narrow_rows with its launch shape and its conversion code take the source pointer of a wave from the table in HBM
 * (k_narrow_list_rows: frames[f]; k_narrow_plane_rows: planes[f * 3 + k], the piece tested against that plane's own extent), timed
 * as MELF_K_GATHER, one launch per chunk.  The host calls narrow while they pack, from the i-th pointer(s) as frame i: one byte per
 * sample crosses PCIe.
 * Measured at 1024-frame config-3 steps of 640 x 480 frames, buffers in rotation beyond the cache
 * (profiles/wide_list/wide_list_rate.txt), 16-bit words / float16 / float32: the frame list (b) takes 0.990 / 0.982 / 0.972 (packed) and
 * 0.990 / 0.990 / 0.990 (planar) times the step of the wide batch in place (a) -- it moves the same bytes; 0.40 - 0.50 ms --, the
 * plane list (c) 1.019 / 1.017 / 1.018 times the frame list, and torch.stack of the listed frames followed by the batch read (d)
 * 4.02 / 3.93 / 4.15 (packed) and 4.19 / 4.04 / 4.26 (planar) times the frame list; torch.stack of the listed planes and the batch
 * read takes 4.12 / 3.97 / 4.25 times the plane list.  The batch path itself runs as before: melf_process_wide_dev under the parent
 * commit's library and under this one, in the same session, differ by -0.9 .. +0.1 %, inside the spread of the parent's own turns.
 * Out of scope: big-endian samples (rgb48be, raw PNG / PPM words: melf_wide_frames has no free field left -- sample_type 4 and non-zero
 * reserved fields are rejected --, so they need a descriptor revision and an ABI bump); wide frames in melf_process_oriented* (its
 * kernel would have to narrow elements of 6 - 16 bytes through LDS: another kernel); a 4th plane; planes with differing pitches. */
int melf_process_wide_list_dev(melf_ctx* ctx, const melf_wide_frames* f, const void* const* d_frames, void* d_results,
                               melf_result* out_host, void* stream);
int melf_process_wide_list(melf_ctx* ctx, const melf_wide_frames* f, const void* const* frames_host, melf_result* out_host);
int melf_process_wide_plane_list_dev(melf_ctx* ctx, const melf_wide_frames* f, const void* const* d_planes, int nplanes, void* d_results,
                                     melf_result* out_host, void* stream);
int melf_process_wide_plane_list(melf_ctx* ctx, const melf_wide_frames* f, const void* const* planes_host, int nplanes,
                                 melf_result* out_host);
/* Stage entry point (parity tests, and a debug view for callers): the narrowing alone through the list kernels.  ptrs_host: n host
 * pointers, one per frame (nplanes == 0), or n * 3, one per plane (nplanes == 3), checked as above.  The library uploads every listed
 * frame or plane into a device allocation OF ITS OWN, of exactly its readable extent, runs the list kernel with the rectangle set to
 * the whole frame and returns n packed H x W x 3 BGR frames, as melf_wide_to_bgr does for a batch.  The allocations are temporary
 * and are freed before it returns.  n <= 1024. */
int melf_wide_list_to_bgr(melf_ctx* ctx, const melf_wide_frames* f, const void* const* ptrs_host, int nplanes, uint8_t* bgr_out_host);

/* ---- the same path for frames in SEPARATE ALLOCATIONS: the surfaces of a hardware decoder's pool (rocDecode, VA-API), a list of
 * tensors from a video reader or torchvision.io.decode_jpeg(device=...), one V4L2 / DRM capture buffer per frame ----
 * Every entry point above takes one base pointer and a frame_stride.  These two take, beside the descriptor of one of the eight
 * families above, a HOST array of n frame pointers (device pointers for _dev, host pointers otherwise); the library copies the
 * array before it returns, so the caller may free it at once.  Frames may alias or repeat: they are only read.
 *     family   MELF_LIST_*: which descriptor `desc` points to
 *     desc     the family's descriptor.  Its n is the length of the list; its frame_stride is not looked at.  Everything else is
 *              checked as for a batch of one frame, and every pointer of the list against the family's NULL and alignment rules:
 *              MELF_ERR_INVALID before anything is launched or copied, the message naming the offending frame's index.  n == 0
 *              passes; an unknown family is MELF_ERR_INVALID.
 *     frames   from each pointer one frame's extent must be readable -- (H - 1) * row_pitch + a row, or up to the last sample of
 *              the frame's last plane, as the family states it for the last frame of a batch -- and nothing behind it nor before
 *              the pointer is read: each frame may be the last thing in its mapping.
 * The records are byte-identical to the family's melf_process_* / melf_process_*_dev call on one contiguous batch that holds the
 * same frames in list order.
 * How: no reading kernel takes a pointer table.  One kernel (k_gather_rows) first copies the rows of the meter_rect crop of every
 * listed frame -- the rows as they are, the origin rounded to whole chroma blocks, macropixels or v210 groups where the format
 * needs it, exactly the small staged frames the host-fed path packs on the CPU -- into a staged batch in HBM, which the unchanged
 * kernels then read.  The price is one extra read and one extra write of the crop's bytes only (187 500 of a 640 x 480 BGR frame's
 * 921 600), against the read and write of every whole frame that torch.stack or n hipMemcpy calls cost a caller before.  Measured
 * on one MI355X, 1024-frame config-3 steps (profiles/frame_list/frame_list_rate.txt): see README.md, "Frames in separate
 * allocations".
 * The device call takes a lane as melf_process_frames_dev does.  The staged batch and the pointer table belong to the lane, so
 * calls on two caller streams do not share them; lists longer than 1024 frames go through the lane's staging buffer in chunks of
 * 1024.  The gather kernel is ordered after everything the caller's stream held at the call, also under
 * melf_ctx_set_frames_resident (the promise there covers batches, not lists: a decoder may still be writing the frames; the call
 * then runs on the lane's own stream and the caller's stream continues when it is done).  d_results / out_host / stream: as for
 * melf_process_frames_dev.  The host call is melf_process_frames and its siblings with the i-th pointer as frame i.
 * frames in separate allocations: melf_process_frame_list*; a frame's planes in separate allocations are still not there.
 * (Not in these two, that is, which take one pointer per frame: one pointer per PLANE is melf_process_plane_list*, below.) */
enum { MELF_LIST_FRAMES = 0,      /* desc: const melf_frames*            */
       MELF_LIST_YUV = 1,         /* const melf_yuv_frames*              */
       MELF_LIST_YUV422 = 2,      /* const melf_yuv422_frames*           */
       MELF_LIST_YUV_PLANAR = 3,  /* const melf_yuv_planar_frames*       */
       MELF_LIST_YUV16 = 4,       /* const melf_yuv16_frames*            */
       MELF_LIST_YUV422_10 = 5,   /* const melf_yuv422_10_frames*        */
       MELF_LIST_PACKED32 = 6,    /* const melf_packed32_frames*         */
       MELF_LIST_PLANES = 7 };    /* const melf_planar_frames*           */
int melf_process_frame_list_dev(melf_ctx* ctx, int family, const void* desc, const void* const* d_frames, void* d_results,
                                melf_result* out_host, void* stream);
int melf_process_frame_list(melf_ctx* ctx, int family, const void* desc, const void* const* frames_host, melf_result* out_host);

/* ---- the same path for frames whose PLANES lie in separate allocations: libav's AVFrame (data[0..2] + linesize[0..2]), V4L2
 * multi-planar capture (NV12M, YUV420M, NV16M: one buffer per plane), VA-API / DRM exports with one object per plane, a torch
 * pipeline that holds (y, uv) or (r, g, b) as separate tensors ----
 * The four families with more than one plane: MELF_LIST_YUV, MELF_LIST_YUV_PLANAR, MELF_LIST_YUV16, MELF_LIST_PLANES (the codes
 * above).  The four one-plane families return MELF_ERR_INVALID (their frames go through melf_process_frame_list*), as does an
 * unknown family.
 *     planes   a HOST array of n * nplanes pointers, frame-major: planes[i * nplanes + k] is plane slot k of frame i (device pointers
 *              for _dev, host pointers otherwise).  The library copies the array before it returns.  Slots of the YUV families:
 *              0 = Y, 1 = the U plane or the one interleaved chroma plane, 2 = the V plane; of melf_planar_frames: 0 / 1 / 2 = B / G / R.
 *     nplanes  what the descriptor implies, else MELF_ERR_INVALID: 2 for MELF_YUV_NV12 and for c_step == 2, 3 otherwise.
 *     desc     the family's descriptor.  Its n is the length of the list; frame_stride is not looked at.  W, H, the pitches (one
 *              y_pitch for all Y planes, one c_pitch for all chroma planes, one row_pitch for B, G and R), subsampling, shift,
 *              matrix and reserved fields follow the family's rules exactly.  The plane offsets (u_offset / v_offset, b_ / g_ /
 *              r_offset) count from the plane's OWN pointer: 0 for every plane of a planar layout; for a semi-planar layout {0,
 *              bytes per sample} in the order that says which of U and V comes first ({u, v} = {0, 1}: NV12, NV16, NV24; {1, 0}:
 *              NV21, NV61, NV42; {0, 2}: P010 ..; melf_yuv_frames' NV12 takes {0, 1} only); anything else is MELF_ERR_INVALID.
 *     pointers every one is checked for NULL and for the family's alignment (2 bytes for melf_yuv16_frames, none otherwise), the
 *              message naming the frame's and the plane's index; MELF_ERR_INVALID before anything is launched or copied.  n == 0
 *              passes.
 * Readable extent: from each plane pointer the bytes up to and including the last sample of that plane's last row -- Y: (H - 1) *
 * y_pitch + W * bytes per sample; a chroma plane: (chroma rows - 1) * c_pitch + the bytes of a chroma row (of both samples for an
 * interleaved plane); B / G / R: (H - 1) * row_pitch + W.  Nothing before a pointer or behind its extent is read: every plane may
 * be the last thing in its mapping.  Planes and frames may alias or repeat: they are only read.
 * The records are byte-identical to the family's melf_process_* / melf_process_*_dev call on one contiguous batch whose frames
 * hold the same samples in list order.
 * How: as the frame lists.  The library forms the canonical one-allocation descriptor of the same geometry (the planes back to
 * back), runs the family's unchanged check and staging plan on it -- one row run per plane --, and one kernel (k_plane_rows, the
 * sibling of k_gather_rows: one launch for all planes of a chunk, timed as MELF_K_GATHER) copies run k of every frame from the
 * frame's k-th pointer into the lane's staged batch, which the unchanged kernels read.  Lanes, melf_ctx_set_frames_resident, caller
 * streams, ordering (the copy waits for what the caller's stream held at the call), chunks of 1024 frames and the NULL d_results /
 * out_host semantics are exactly melf_process_frame_list_dev's; the lane's pointer tables grow to 1024 * nplanes entries.  The host
 * call packs each run's rows from that run's own plane on the host pool, as melf_process_frame_list does from the one frame.
 * Measured on one MI355X, 1024-frame config-3 steps (profiles/plane_list/plane_list_rate.txt), NV12 / I420 / P010 / planar RGB:
 * the plane list (c) takes 1.021 / 1.019 / 0.990 / 0.991 times the step of the frame list (b) of one-allocation frames holding the
 * same samples (0.29 - 0.33 ms); concatenating each frame's planes into one allocation first (torch.cat per frame) and then the
 * frame list (d) takes 18.4 / 21.7 / 16.7 / 18.7 times the plane list's step.
 * Out of scope: planes of one frame with differing chroma pitches (U and V share c_pitch, B, G and R share row_pitch); a 4th
 * plane; plane lists for melf_process_stream_dev, the fused full-frame mask, melf_aligned_average and the JPEG entry points. */
int melf_process_plane_list_dev(melf_ctx* ctx, int family, const void* desc, const void* const* d_planes, int nplanes,
                                void* d_results, melf_result* out_host, void* stream);
int melf_process_plane_list(melf_ctx* ctx, int family, const void* desc, const void* const* planes_host, int nplanes,
                            melf_result* out_host);

/* ---- the same path for frames that are stored ROTATED or MIRRORED: the raw frames of a camera mounted on its side (V4L2 buffers,
 * decoder surfaces, tensors), phone and IP-camera video whose rotation sits in the container's display matrix while the hardware
 * decoder leaves NV12 unrotated ----
 * The reference reads every frame through cv2.imread, which applies the EXIF orientation tag: what it reads is upright.  These
 * entry points take the stored batch and the orientation and read the frame a viewer shows, without forming it.
 * Orientation codes are the EXIF / TIFF tag 0x0112 values.  With S the stored frame of H rows x W columns and O the oriented frame
 * of H' x W' -- the frame a viewer shows and cv2.imread returns --:
 *     code  name                     H' x W'   O[y][x] =
 *     1     MELF_ORIENT_NORMAL       H x W     S[y][x]
 *     2     MELF_ORIENT_MIRROR       H x W     S[y][W-1-x]
 *     3     MELF_ORIENT_ROT180       H x W     S[H-1-y][W-1-x]
 *     4     MELF_ORIENT_FLIP         H x W     S[H-1-y][x]
 *     5     MELF_ORIENT_TRANSPOSE    W x H     S[x][y]
 *     6     MELF_ORIENT_ROT90CW      W x H     S[H-1-x][y]
 *     7     MELF_ORIENT_TRANSVERSE   W x H     S[H-1-x][W-1-y]
 *     8     MELF_ORIENT_ROT90CCW     W x H     S[x][W-1-y]
 * A video stream's "rotate by 90 / 180 / 270 degrees clockwise to display" is 6 / 3 / 8.
 * For a layout with chroma planes every plane is oriented by the same formula on its own sample grid: for a chroma plane of
 * (H >> sub_y) x (W >> sub_x) samples the formula applies with those dimensions, and an interleaved U/V pair moves as one element.
 * Because H and W are whole chroma blocks this is the same as orienting the converted BGR frame -- for codes 2-4 under any
 * subsampling, for codes 5-8 where sub_x == sub_y.
 *     family       MELF_LIST_*: which descriptor `desc` points to
 *     desc         that family's descriptor of the STORED batch: one base pointer, its own frame_stride, every rule of the family's
 *                  check unchanged
 *     orientation  1 .. 8
 * meter_rect is taken on the ORIENTED frame, with the same clamping; H' x W' must hold the crop and the template exactly as the
 * family's call requires of an upright frame, with the same error otherwise.
 * The records are byte-identical to the family's own melf_process_* / melf_process_*_dev call on a contiguous batch holding the
 * oriented frames O in the same layout.  Neither O nor any other whole frame is formed: only the source samples of the crop are
 * read -- the crop rounded out to chroma blocks exactly as the family's staging plan rounds it --, and no load reaches outside
 * [base, base + (n - 1) * frame_stride + one frame's extent).
 * Families: MELF_LIST_FRAMES, MELF_LIST_PACKED32, MELF_LIST_PLANES and MELF_LIST_YUV take all eight codes; MELF_LIST_YUV_PLANAR all
 * eight when sub_x == sub_y and 1-4 otherwise; MELF_LIST_YUV16 all eight when sub_y == 1 and 1-4 otherwise.  MELF_LIST_YUV422 and
 * MELF_LIST_YUV422_10 return MELF_ERR_INVALID: a mirrored macropixel is not a permutation of equal-sized elements.  Also
 * MELF_ERR_INVALID before anything is launched or copied, melf_last_error saying which: an orientation outside 1 .. 8, a NULL
 * pointer, an unknown family.  n == 0 passes.
 * How: code 1 calls the family's in-place entry point and nothing else.  For codes 2-8 one kernel (k_orient_tiles, timed as
 * MELF_K_GATHER) writes the oriented crop of every frame into the lane's staged batch -- the same staged frame, rectangle and layout
 * the family's staging plan gives for an upright frame of the oriented geometry --, which the unchanged kernels then read exactly as
 * they read a frame list's.  A workgroup takes a tile of 64 x 64 elements (a Y, chroma, B / G / R sample; an interleaved pair; a
 * 3- or 4-byte pixel; a 16-bit sample or pair), loads its source rectangle along the stored rows into LDS and writes the
 * destination rows from there in aligned 16-byte pieces.  The price is one read and one write of the crop's bytes only (187 500 of a
 * 640 x 480 BGR frame's 921 600), against the read and write of every whole frame that torch.rot90(frames, ..).contiguous() or
 * flip costs a caller before.  Lanes, caller streams, melf_ctx_set_frames_resident, ordering, chunks of 1024 frames and the NULL
 * d_results / out_host semantics are exactly melf_process_frame_list_dev's.  The host call packs the same staged frames on the host
 * pool from the same address functions: only the crop crosses PCIe.
 * Measured on one MI355X, 1024-frame config-3 steps (profiles/oriented/oriented_rate.txt), BGR under 3, BGR / BGRA / NV12 / P010
 * under 6: the stored batch (b) takes 0.3353 / 0.3316 / 0.3551 / 0.2866 / 0.3269 ms a step, 1.43 / 1.41 / 1.44 / 1.21 / 1.28 times the
 * upright batch in place (a); torch.rot90 / flip of the whole stored frames and then the batch read (c) takes 6.8 / 11.3 / 11.9 / 8.5 /
 * 8.5 times the step of (b); k_orient_tiles takes 0.109 / 0.106 / 0.101 / 0.056 / 0.084 ms a launch, 1.30 / 1.26 / 0.95 / 1.28 / 1.17
 * times the plain-copy kernel of a frame list (k_gather_rows) moving the same bytes in the same run.
 * Out of scope: oriented frame lists and plane lists; the two packed 4:2:2 families; re-describing 4:2:2 as 4:4:0 (and back) under
 * transposition; melf_process_stream_dev and the fused full-frame mask.  (JPEG FILES that carry an EXIF orientation are decoded
 * upright by the JPEG entry points themselves once melf_ctx_set_jpeg_orientation is on: see "JPEG decode", below.) */
enum { MELF_ORIENT_NORMAL = 1, MELF_ORIENT_MIRROR = 2, MELF_ORIENT_ROT180 = 3, MELF_ORIENT_FLIP = 4, MELF_ORIENT_TRANSPOSE = 5,
       MELF_ORIENT_ROT90CW = 6, MELF_ORIENT_TRANSVERSE = 7, MELF_ORIENT_ROT90CCW = 8 };
int melf_process_oriented_dev(melf_ctx* ctx, int family, const void* desc, int orientation, const void* d_frames, void* d_results,
                              melf_result* out_host, void* stream);
int melf_process_oriented(melf_ctx* ctx, int family, const void* desc, int orientation, const void* frames_host, melf_result* out_host);
/* Stage entry point (parity tests, debug view): the orientation alone.  The same kernel with the rectangle set to the whole oriented
 * frame, for all eight codes; out receives n oriented frames of H' x W' in the family's layout at TIGHT pitches, one after the
 * other, out_bytes >= n * one such frame.  The tight frame per family -- MELF_LIST_FRAMES: H' rows of W' pixels of 3 or 4 bytes;
 * MELF_LIST_PACKED32: H' rows of W' words; MELF_LIST_PLANES: the B, the G and the R plane, H' x W' bytes each, in that order whatever
 * the stored order; the YUV families: the Y plane, H' rows of W' samples, then for an interleaved layout the one chroma plane of
 * (H' >> sub_y) rows of (W' >> sub_x) pairs in the stored order of a pair, for a planar layout the U plane and then the V plane,
 * (H' >> sub_y) x (W' >> sub_x) samples each, whatever the stored order; samples of 2 bytes for MELF_LIST_YUV16. */
int melf_orient_frames(melf_ctx* ctx, int family, const void* desc, int orientation, const void* frames_host, void* out_host,
                       size_t out_bytes);

/* ---- stage entry points (parity tests and roofline runs) ----------------- */

/* convert_to_hls (meterelf/_utils.py:100-102): cvtColor(BGR2HLS_FULL) + uint8
 * hue shift.  src rows x cols x 3 u8 with row stride in bytes; dst packed. */
int melf_bgr2hls(melf_ctx* ctx, const uint8_t* src_host, int rows, int cols, size_t row_stride,
                 uint8_t* dst_host);

/* Fused full-frame stage (BASELINE config 2): HLS(+shift) -> inRange with the
 * context's fixed needle bounds (get_mask_by_color, meterelf/_utils.py:113-119,
 * bounds as meterelf/_calibration.py:82-84) -> dilate 3x3 -> erode 3x3
 * (meterelf/_reading.py:128-130).  n frames H x W x 3 -> n masks H x W u8 {0,255}. */
int melf_hls_inrange_close(melf_ctx* ctx, const uint8_t* frames_host, int n, int H, int W,
                           uint8_t* masks_host);
int melf_hls_inrange_close_dev(melf_ctx* ctx, const void* d_frames, int n, int H, int W,
                               void* d_masks, void* stream);

#ifdef MELF_DIAG
/* DIAGNOSTIC BUILD ONLY (make -C meterelf_amd/csrc diag -> libmeterelf_hip_diag.so; the product library does not export it).
 * Measurement aid for the fused stage's roofline (bench.py: fused_mask.stream_ceiling), nothing the reference has: one launch
 * of a BARE persistent stream with the fused kernel's traffic mix and launch shape -- 48 bytes read and 16 bytes written per
 * thread and step, no pixel arithmetic -- over the caller's device buffers: floor(in_bytes / 48 KiB) chunks of d_in are read,
 * a third as many bytes of d_out are overwritten with garbage (XOR of the input: point it at a mask buffer that is rewritten
 * afterwards).  chunks_per_block = 0: static grid-stride split; -1: the same with the kernel's register prefetch (the next
 * chunk requested before this one is stored); -2 .. -5: every workgroup walks its own contiguous run of chunks like the kernel's
 * segments (-3: + the kernel's 48-byte lane stride, -4: + two barriers and an LDS hand-over per step, -5: + 64 KiB of LDS
 * tables filled first); > 0: blocks of that many chunks from a work queue.  The launch
 * is timed like the fused kernel's (melf_ctx_set_profiling(1), entry MELF_K_STREAM_PROBE of melf_ctx_timings). */
int melf_stream_probe_dev(melf_ctx* ctx, const void* d_in, size_t in_bytes, void* d_out, int chunks_per_block, void* stream);
/* DIAGNOSTIC BUILD ONLY, measurement aid of tools/frame_list_rate.py: melf_process_frame_list_dev up to and including its gather
 * kernel -- the checks, the lane, the pointer table, k_gather_rows into the lane's staged batch -- and nothing of the reading path.
 * *bytes_moved (may be NULL): the bytes the gather read plus the bytes it wrote.  Timed as entry MELF_K_GATHER of melf_ctx_timings. */
int melf_gather_frame_list_dev(melf_ctx* ctx, int family, const void* desc, const void* const* d_frames, void* stream, size_t* bytes_moved);
#endif

/* Number of entries of the fused stage's hue lookup table whose in-range answer
 * depends on the float32 rounding of the individual BGR triple (exact rounding
 * ties at a bound).  > 0 selects the kernel variant that re-evaluates those
 * pixels with the exact float path; results are identical either way. */
int melf_ctx_fused_table_ties(const melf_ctx* ctx, int* count);

/* Which kernel body the fused stage (melf_hls_inrange_close*) runs for this context's needle bounds, and the three
 * numbers the choice was made from.  Builds the tables on first use, like melf_ctx_fused_table_ties.  Every output
 * pointer may be NULL.
 *   variant         0 / 1 / 2: one hue sector (maximum r / g / b), bit tables; 3: any sectors; 4: any sectors, rounding ties
 *                   re-evaluated with the float path; 6 / 7 / 8: one hue sector r / g / b, interval tables.  It is what the
 *                   table kernel k_fused_mask_lut is instantiated with AFTER MELF_FUSED_VARIANT has been applied.
 *   active_sectors  bit c set: hue sector c (0 = r, 1 = g, 2 = b) has an in-range table entry
 *   noniv[c]        rows of sector c's tables whose set bits are not one contiguous run (0: interval tables possible)
 *   last_launch     what this context's most recent fused-mask launch ran: [0] the variant, or -1 for the float-path
 *                   kernel k_fused_mask (W % 16 != 0, a buffer that is not 16-byte aligned, MELF_FORCE_GENERIC_MASK=1),
 *                   or -2 if nothing has been launched yet; [1] the work-queue slot of that launch, -1 when its segments
 *                   were split statically over the workgroups.  A call of more frames than one launch takes reports its last
 *                   piece.  The two values are plain fields written by every launch, without synchronisation: they mean
 *                   something only right after the caller's own launch, with no other thread launching on the context. */
int melf_ctx_fused_variant(const melf_ctx* ctx, int* variant, int* active_sectors, int noniv[3], int last_launch[2]);

/* match_template (meterelf/_utils.py:91-97): TM_CCOEFF of n single-channel u8
 * images (rows x cols, packed) against the context's template + minMaxLoc.
 * result_map (optional) receives n*(rows-th+1)*(cols-tw+1) float32. */
int melf_match_ccoeff(melf_ctx* ctx, const uint8_t* images_host, int n, int rows, int cols,
                      float* max_val, int32_t* max_x, int32_t* max_y, float* result_map);

/* Per-dial reading on n already-located dials crops (th x tw x 3 HLS u8, packed):
 * get_needle_points + angle estimate + digit combine
 * (meterelf/_reading.py:28-111, :118-182). */
int melf_read_dials(melf_ctx* ctx, const uint8_t* dials_hls_host, int n, melf_result* out_host);

/* ---- calibration stages (reference: meterelf/_calibration.py, offline) ------ */

/* get_average_meter_image (meterelf/_calibration.py:60-63 with _image.py:34-44 and
 * _utils.py:64-88): the meter_rect crop of every frame is translated so that its dial match
 * (match_x[i], match_y[i]) lands at (align_x, align_y), the float64 running mean is taken in the
 * reference's operation order and denormalised to u8.  out_crop: crop_rows x crop_cols x 3. */
int melf_aligned_average(melf_ctx* ctx, const uint8_t* frames_host, int n, int H, int W, size_t frame_stride,
                         const int32_t* match_x, const int32_t* match_y, int align_x, int align_y,
                         uint8_t* out_crop_host);

/* cv2.inRange on a packed 3-channel u8 image (get_mask_by_color, meterelf/_utils.py:113-119). */
int melf_inrange(melf_ctx* ctx, const uint8_t* img_host, int rows, int cols, const int32_t lo[3],
                 const int32_t hi[3], uint8_t* mask_host);

/* nbatches batches of n frames each, already in HBM (batch b at d_frames + b * batch_stride bytes, its records at
 * d_results + b * results_stride records; a stride of 0 re-reads / overwrites the same batch), enqueued from
 * `stream`: consecutive batches run on the context's two pipeline lanes, so that their kernels overlap; `stream`
 * continues when all of them are done.  Results as melf_process_batch_dev. */
int melf_process_stream_dev(melf_ctx* ctx, const void* d_frames, int nbatches, size_t batch_stride, int n, int H, int W,
                            size_t frame_stride, void* d_results, size_t results_stride, void* stream);

/* ---- JPEG decode (reference: cv2.imread in ImageFile.get_bgr_image, meterelf/_image.py:46-51) ----
 * Baseline sequential 8-bit Huffman JPEGs (one interleaved scan; YCbCr 4:2:0 / 4:2:2 / 4:4:4 or
 * greyscale; restart intervals allowed) are decoded on the GPU to the bytes libjpeg produces with its
 * defaults (ISLOW IDCT, fancy upsampling), i.e. what cv2.imread returns: H x W x 3 BGR u8.
 * Per-file status: 0 decoded, 1 valid JPEG outside that subset (decode it on the host instead) -- also a file
 * WITHOUT restart markers whose entropy-coded data exceed 4 MB (the segment-parallel Huffman kernel addresses
 * 1024 segments of at most 32 000 bits; melf_jpeg_probe cannot tell, the decode calls report it), unless
 * melf_ctx_set_jpeg_long_scans is on (below): such a file is then decoded on the GPU as well --,
 * 2 unreadable / corrupt, 3 its size is not H x W.  Frames with a non-zero status are zero-filled. */
enum { MELF_JPEG_OK = 0, MELF_JPEG_UNSUPPORTED = 1, MELF_JPEG_CORRUPT = 2, MELF_JPEG_SIZE_MISMATCH = 3,
       MELF_JPEG_UNREADABLE = 4 /* melf_jpeg_process_files: the file could not be opened or read */ };

/* Header check only (no GPU, no context): image size and whether the GPU decoder handles the file. */
int melf_jpeg_probe(const uint8_t* data, size_t size, int32_t* H, int32_t* W, int32_t* supported);

/* The same check for n files at once (one call instead of n from a scripting host). */
int melf_jpeg_probe_batch(const uint8_t* const* data, const size_t* sizes, int n, int32_t* H, int32_t* W,
                          int32_t* supported);

/* ---- JPEG files with an EXIF orientation (tag 0x0112 in IFD0 of the first Exif APP1 segment): a camera mounted on its side, a phone ----
 * cv2.imread applies the tag, so the reference reads such a file upright.  melf_jpeg_probe and melf_jpeg_probe_batch report a file
 * whose tag is 2..8 unsupported (reason "EXIF orientation ..."), and by default every decode call below gives it status 1 for the
 * caller's host decoder to decode and rotate; none of that changes.  melf_ctx_set_jpeg_orientation(ctx, 1) makes melf_jpeg_decode_batch,
 * melf_jpeg_process_batch, melf_jpeg_process_files and melf_jpeg_process_files_begin / _end of that context take such a file, if the
 * decoder takes it otherwise.  Off at context creation; with it off every JPEG entry point behaves exactly as before, status codes
 * included.  Not while a _begin call is in flight.
 * Semantics, bit for bit: with S the frame libjpeg(-turbo) decodes from the file -- ISLOW IDCT, fancy upsampling in STORED geometry
 * (the chroma filter runs along the stored axes whatever the code), libjpeg's colour tables, exactly as for an upright file -- the
 * frame produced is O[y][x] of the orientation table above ("stored ROTATED or MIRRORED"): decode first, permute afterwards, which is
 * what cv2.imread and Pillow's exif_transpose do.  The caller's H and W, and H_used / W_used, are UPRIGHT sizes throughout: a file of
 * stored size h x w counts as w x h under codes 5-8, and a file whose upright size is not H x W gets MELF_JPEG_SIZE_MISMATCH.  Upright
 * and oriented files, and files of different codes, may share one call; frames and records come back in the caller's order.
 * How: the entropy decoder, the IDCT and the chroma filter never see the orientation.  The files of a call are decoded code by code
 * (scheduling only), each code on its own window of the stored frame -- the meter_rect taken back through the code, grown by one MCU
 * on every side, aligned to 16 and clamped (melf_jpeg_orient_addr.h; for code 1 the window it always was) -- and one kernel
 * (k_jpeg_color_exif, timed as MELF_K_JPEG_COLOR) converts a 64 x 64 tile of that window along the stored rows, parks it in LDS and
 * writes the tile's rows of the upright frame.  O is never formed outside the window.  A call without an oriented file launches
 * exactly what it launches with the switch off.
 * Measured on one MI355X, 1024-file config-3 calls of melf_jpeg_process_batch (profiles/jpeg_orient/jpeg_orient_rate.txt): the
 * fixture's content stored under orientation 6 / 3 takes 3.21 / 3.36 ms a call, 0.975 / 1.018 times the same content in upright files
 * (3.30 ms; quality 95, 68 KB a file), where the host branch such files took before (Pillow decode + exif_transpose on 8 threads,
 * then the batch read) takes 714 / 685 ms: 222 / 204 times as long.  The colour stage takes 0.815 / 0.803 ms a call against 0.193 ms
 * for upright 4:2:0 files.  Upright files, this library against the one before the switch existed, same lease: 1.962 / 1.981 against
 * 1.981 / 1.976 ms a call.
 * Out of scope: a tag anywhere but IFD0 of the first Exif APP1 (a second Exif block that asks for a rotation sends the file to the
 * host); progressive files unless melf_ctx_set_jpeg_progressive is on too (below), and multi-scan sequential files, which (unless melf_ctx_set_jpeg_multiscan is on, below) stay
 * unsupported with or without a tag; a 4:2:0 fast path for oriented files. */
/* The header check that takes the tag: H and W are the STORED size, *orientation is 1..8 (1 when the tag is absent, unreadable or
 * outside 1..8, which Pillow and cv2 leave alone too), *supported is what melf_jpeg_probe would answer if the file had no tag.  The
 * upright size is W x H for codes 5-8. */
int melf_jpeg_probe_oriented(const uint8_t* data, size_t size, int32_t* H, int32_t* W, int32_t* orientation, int32_t* supported);
/* The same for n files at once (MeterReader.read_jpeg_files groups a list by upright size with it). */
int melf_jpeg_probe_oriented_batch(const uint8_t* const* data, const size_t* sizes, int n, int32_t* H, int32_t* W, int32_t* orientation,
                                   int32_t* supported);
int melf_ctx_set_jpeg_orientation(melf_ctx* ctx, int on);
int melf_ctx_get_jpeg_orientation(melf_ctx* ctx, int* on);

/* ---- Progressive JPEG files (SOF2): phones, web exporters, jpegtran -progressive, cameras' "optimised" mode ----
 * melf_jpeg_probe and the probes above report such a file unsupported (reason "... progressive ..."), and by default every decode call
 * gives it status 1 for the caller's host decoder; none of that changes.  melf_ctx_set_jpeg_progressive(ctx, 1) makes
 * melf_jpeg_decode_batch, melf_jpeg_process_batch, melf_jpeg_process_files and melf_jpeg_process_files_begin / _end of that context take
 * progressive files of the subset below.  Off at context creation; with it off every JPEG entry point behaves exactly as before,
 * status codes and melf_last_error texts included.  Not while a _begin call is in flight.  Independent of the orientation switch: a
 * progressive file with an EXIF orientation 2..8 is taken when both are on.
 * Taken: SOF2 with 8-bit samples; components, sampling, JFIF / Adobe / component-id and empty-image rules exactly as for baseline
 * files; at most MELF_JPEG_PROG_SCANS_MAX scans, each well formed (Ss = 0 implies Se = 0, a DC scan of 1..ncomp components in frame
 * order; Ss > 0 implies one component and Ss <= Se <= 63; Ah = 0 or Al = Ah - 1; Al <= 13) and consistent (a first scan covers only
 * coefficients not sent before, a refinement only coefficients whose precision is Ah, a component's AC scans follow its first DC
 * scan: libjpeg only warns about an inconsistent script, here it is unsupported); after the last scan EVERY coefficient of every
 * component at full precision -- libjpeg smooths blocks whose AC precision is incomplete, and then the pixels are no longer those of
 * the coefficient blocks, so a file that ends early in its script or never sends some band is unsupported; Huffman table ids 0..3,
 * redefined between scans at will (a scan uses the tables in force at its SOS; a table it needs must exist and pass libjpeg's checks;
 * a DC refinement needs none); quantisation tables as in force at the first SOS (a DQT behind it: unsupported); DRI, also between
 * scans (the interval counts the MCUs of the scan it applies to -- single blocks in a non-interleaved scan); bytes behind EOI are
 * ignored.  Entropy-coded data that run out before a scan's blocks are done, an RSTn out of sequence or a Huffman code that does not
 * exist give MELF_JPEG_CORRUPT and a zero-filled frame, and so does a file whose bytes end inside a scan.  The 4 MB limit of
 * restart-less baseline scans (lifted for those by melf_ctx_set_jpeg_long_scans, below) never applied to progressive files.
 * Semantics, bit for bit: the frame libjpeg(-turbo) decodes from the file with its defaults.  Every scan is accumulated into the
 * coefficient blocks (k_jpeg_prog_scan, melf_jpeg_prog.h; timed as MELF_K_JPEG_HUFF): one wave per (file, scan, restart interval),
 * one launch per LEVEL of scans -- a scan's level is one more than the highest level of the earlier scans that send a coefficient it
 * sends too, so the scans of a level touch no common coefficient and run side by side (libjpeg's default colour script of ten
 * scans has three levels) --, then the baseline decoder's IDCT, upsampling, colour and orientation stages run unchanged, on the
 * window they always ran on; the coefficient area of a progressive file is zeroed and decoded whole.  The host walks a progressive
 * file's entropy-coded bytes once, to find its scans and restart intervals; a call without a progressive file launches what it
 * launched before.
 * Measured on one MI355X, melf_jpeg_process_batch on the 640 x 480 fixture frames re-saved progressive at quality 95 (50 KB a file):
 * 256 / 1024 files a call take 150 / 305 ms (1.7 K / 3.4 K files/s) without restart markers, where a scan is ONE sequential chain on
 * one lane, and 31 / 111 ms (8.3 K / 9.3 K files/s) with a restart interval of one MCU row; the host branch such files took reads
 * 1.4 - 1.5 K files/s.  A call of 512 baseline + 512 progressive files takes 161 ms.  The baseline files' own rate is unchanged.
 * What a call pays is the LATENCY of one file's chain, not a rate: a 256-file call with 1 / 8 / 32 / 128 / 256 restart-less
 * progressive files among baseline ones takes 116 / 121 / 125 / 129 / 137 ms, where Pillow on 8 threads for those files plus the GPU
 * call for the rest takes 4 / 15 / 43 / 140 / 282 ms (profiles/jpeg_prog/jpeg_prog_rate.txt): the switch pays from about half a chunk
 * of progressive files on, or for files with restart markers.  That is why it is opt-in everywhere, get_meter_values included
 * (METERELF_JPEG_PROGRESSIVE=gpu). */
#define MELF_JPEG_PROG_SCANS_MAX 32
/* (8 is no switch: a probe with that bit is a bad argument, as it has been since the flags word had three bits) */
enum { MELF_JPEG_TAKE_ORIENTED = 1, MELF_JPEG_TAKE_PROGRESSIVE = 2, MELF_JPEG_TAKE_SAMPLINGS = 4, MELF_JPEG_TAKE_DEFAULT_TABLES = 16,
       MELF_JPEG_TAKE_MULTISCAN = 32 };
int melf_ctx_set_jpeg_progressive(melf_ctx* ctx, int on);
int melf_ctx_get_jpeg_progressive(melf_ctx* ctx, int* on);

/* ---- YCbCr 4:4:0 and 4:1:1 JPEG files ----
 * 4:4:0 (luma 1x2, chroma 1x1) is what a lossless 90-degree rotation (jpegtran -rotate, exiftran, gallery apps) makes of a 4:2:2 file,
 * the layout of ESP32-CAM-class and many MJPEG / UVC cameras; 4:1:1 (luma 4x1, chroma 1x1) is written by DV-derived and older
 * IP-camera / capture-card encoders.  Every probe reports such a file unsupported (reason "luma sampling other than 1x1, 2x1, 2x2"),
 * and by default every decode call gives it status 1 for the caller's host decoder; none of that changes.
 * melf_ctx_set_jpeg_samplings(ctx, 1) makes melf_jpeg_decode_batch, melf_jpeg_process_batch, melf_jpeg_process_files and
 * melf_jpeg_process_files_begin / _end of that context take them.  Off at context creation; with it off every JPEG entry point
 * behaves exactly as before, status codes, probe answers and melf_last_error texts included.  Not while a _begin call is in flight.
 * Independent of the other two switches: a progressive 4:4:0 file with an EXIF orientation is taken when all three are on.
 * Taken: three-component YCbCr files whose luma sampling is 1x2 or 4x1 and whose chroma sampling is 1x1, baseline or (with that
 * switch) progressive, under every other rule of the decoder as it stands.  An MCU is then 8 x 16 pixels and 4 blocks, or 32 x 8
 * pixels and 6 blocks.
 * Semantics, bit for bit: the frame libjpeg(-turbo) decodes from the file with its defaults.  With P a chroma plane of
 * ch = ceil(H / 2) real rows (4:4:0) or cw = ceil(W / 4) real columns (4:1:1):
 *     4:4:0 ("h1v2 fancy"), output row y, cy = y >> 1:
 *         even y   (3 * P[cy][x] + P[max(cy - 1, 0)][x] + 1) >> 2
 *         odd y    (3 * P[cy][x] + P[min(cy + 1, ch - 1)][x] + 2) >> 2
 *       the neighbour clamped to the REAL rows, not the MCU-padded ones; no narrow-image fallback (libjpeg has one for h2v1 / h2v2 only)
 *     4:1:1: plain replication, P[y][x >> 2], no filter
 * and everything else is the existing pipeline: the ISLOW IDCT and libjpeg's colour tables.
 * How: the entropy decoders, the IDCT and the progressive decoder were general in the luma factors already; the general colour kernels
 * (k_jpeg_color, k_jpeg_color_exif) get the two upsamplers.  The decode window stays the one it was (16 pixels of margin, 16-aligned):
 * every stage rounds it outwards to the file's own MCUs, so a 32-wide MCU the window cuts is decoded whole.  Files of the four older
 * samplings launch exactly what they launched, k_jpeg_color420 included.
 * Measured on one MI355X, 1024-file config-3 calls of melf_jpeg_process_batch on fixture frames re-encoded with the same tables
 * (profiles/jpeg_sampling/jpeg_sampling_rate.txt): 4:4:0 / 4:1:1 files take 2.34 / 2.58 ms
 * a call (439 K / 396 K files/s), 0.929 / 1.028 times the same frames as 4:2:2 files (2.51 ms; the nearest sibling: the same colour
 * kernel), where the host branch such files took before (Pillow on 8 threads, then the batch read) takes 655 / 630 ms: 281 / 244
 * times as long.  Per call, summed over its chunks: Huffman 1.75 / 2.64 ms (4:2:2: 1.84), IDCT 0.20 / 0.19 (0.20), colour 0.70 / 0.68
 * (0.94; the 4:2:0 fast path: 0.16).  The fixture's own 4:2:0 files, this library against the one before the switch existed, same
 * lease, taking turns: 1.987 / 2.055 against 2.039 / 2.048 ms a call, 0.992 on the medians, inside either's spread.
 * Out of scope: 4:1:0 (luma 4x2, 10 blocks an MCU) and anything with more than 6 blocks an MCU; chroma factors other than 1x1,
 * including the "2x2 / 1x2 / 1x2" spelling of 4:2:2; RGB / CMYK / Adobe-transform-0 files; multi-scan sequential files (melf_ctx_set_jpeg_multiscan, below); a packed
 * fast path like k_jpeg_color420 for the new layouts. */
int melf_ctx_set_jpeg_samplings(melf_ctx* ctx, int on);
int melf_ctx_get_jpeg_samplings(melf_ctx* ctx, int* on);

/* ---- Multi-scan sequential JPEG files ----
 * A sequential file (SOF0 / SOF1) may send its three components in three scans of one component each instead of one interleaved
 * scan (jpegtran -scans, some camera firmwares and hardware encoders).  Every probe reports such a file unsupported (reason "more than
 * one scan (non-interleaved components)"), and by default every decode call gives it status 1 for the caller's host decoder; none of
 * that changes.  melf_ctx_set_jpeg_multiscan(ctx, 1) makes melf_jpeg_decode_batch, melf_jpeg_process_batch, melf_jpeg_process_files and
 * melf_jpeg_process_files_begin / _end of that context take them.  Off at context creation; with it off every JPEG entry point
 * behaves exactly as before, status codes, probe answers and melf_last_error texts included.  Not while a _begin call is in flight.
 * Independent of the other switches: a 4:4:0 multi-scan file with an EXIF orientation is taken when the three are on.
 * Taken: SOF0 or SOF1, 8 bit, three components, YCbCr of any sampling the context takes otherwise; exactly three scans of one
 * component each, every component once, in any order, each with Ss = 0, Se = 63, Ah = Al = 0.  Between the scans: DHT with ids 0-3
 * (a scan uses the tables in force at its own SOS; a redefinition between scans is legal; every table a scan uses must exist and pass
 * libjpeg's checks), DRI (the interval counts the blocks of the scan it applies to), COM and APPn.
 * Unsupported, each with a reason of its own: a scan of two components, a component sent twice, a file that ends (EOI) before every
 * component has had its scan, a DQT or a frame header behind the first SOS, anything behind the third scan other than EOI (bytes behind
 * EOI are ignored, as ever).  A file whose bytes end inside a scan is MELF_JPEG_CORRUPT, as a truncated file ever was.
 * Semantics, bit for bit: the frame libjpeg(-turbo) decodes with its defaults.  libjpeg smooths only progressive files, so that is the
 * frame of the interleaved file that holds the same coefficient blocks.  Corruption in any scan (the data run out, restart markers
 * missing or surplus, a code that does not exist) gives the file MELF_JPEG_CORRUPT and a zero-filled frame; its neighbours are unaffected.
 * How: a non-interleaved scan of a component is, bit for bit, the entropy-coded segment of a greyscale file of the component's size
 * (ceil(W hs_c / hs_max) x ceil(H vs_c / vs_max)): one block an MCU, the REAL blocks in raster order, its own DC predictor, restart
 * interval and tables.  Each scan therefore goes through k_jpeg_clean, k_jpeg_huff and k_jpeg_huff_rst unchanged as a one-component
 * record of its own, with a snapshot of its two tables, and writes the component's blocks into an area of its own; k_jpeg_idct reads a
 * marked file's blocks from those areas and leaves the MCU-padding blocks, which no scan sends and no pixel reads, flat.  Unlike
 * progressive files these keep the segment-parallel decoder and pay no chain latency.  The scans' records are launched in groups of one
 * window: a chroma scan's window is the file's window divided by the sampling factors and rounded outwards to MCUs, not a subset of
 * the luma window (meterelf_amd/csrc/melf_jpeg_scans.h).  Each scan has the 1024-segment / 4 MB allowance of a file's one scan.  The
 * host walks these files' entropy-coded bytes once, to find the second and third SOS; a call without such a file launches exactly what
 * it launched before.
 * Measured on one MI355X, 1024-file config-3 calls of melf_jpeg_process_batch on fixture frames written as interleaved files, as their
 * multi-scan twins and as their twins without DHT segments (profiles/jpeg_scans/jpeg_scans_rate.txt): multi-scan 4:2:0 / 4:2:2 files
 * take 2.56 / 2.92 ms a call (401 K / 350 K files/s), 1.148 / 1.192 times their interleaved twins (2.23 / 2.45 ms), where the host branch
 * such files took before (Pillow on 8 threads, then the batch read) takes 567 ms: 222 times as long.  Per call, summed over its chunks:
 * Huffman 1.18 / 1.61 ms (twins: 1.99 / 1.72), IDCT 0.13 / 0.18 (0.18 / 0.21), colour 0.16 / 0.75 (0.20 / 1.09); what a call pays above
 * its twin is launches (one more Huffman launch per group, four records a file through k_jpeg_clean) and the host's walk, not kernel
 * time.  A 256-file call with ONE multi-scan file among baseline files takes 1.22 ms, the same call with that file through the host
 * branch 2.85 ms: that is why get_meter_values turns the switch on (METERELF_JPEG_MULTISCAN=host restores the host branch).  The
 * fixture's own 4:2:0 files, this library against the one before the switch existed, same lease, taking turns: 2.133 / 2.047 against
 * 2.007 / 2.068 ms a call, 1.023 on the medians with 4 - 5 % between either library's own turns; eight more alternating turns gave
 * 2.19 / 2.06 / 2.06 / 2.09 against 2.03 / 2.10 / 2.12 / 2.10 ms, 0.987 on the medians: no difference beyond the turns' own spread.
 * Out of scope: partially interleaved scripts (Y, then CbCr together), 4:1:0 and chroma factors above 1, RGB / CMYK files, a DQT
 * between scans. */
int melf_ctx_set_jpeg_multiscan(melf_ctx* ctx, int on);
int melf_ctx_get_jpeg_multiscan(melf_ctx* ctx, int* on);

/* ---- JPEG files without their Huffman tables (Motion-JPEG frames) ----
 * Frames of UVC webcams, ESP32-class boards and AVI MJPG streams come without a DHT segment: Motion-JPEG leaves the tables to the
 * decoder, and libjpeg-turbo (so cv2.imread and Pillow) installs the ones ITU-T T.81 Annex K.3 prints.  Every probe reports such a
 * file unsupported (reason "missing Huffman table"), and by default every decode call gives it status 1 for the caller's host decoder;
 * none of that changes.  melf_ctx_set_jpeg_default_tables(ctx, 1) makes the decode calls of that context take them.  Off at context
 * creation; with it off every JPEG entry point behaves exactly as before.  Not while a _begin call is in flight.  Independent of the
 * other switches.
 * Semantics, exactly libjpeg-turbo's std_huff_tables: when the Huffman decoder starts -- behind the headers up to the first SOS -- each
 * of the slots DC 0, AC 0, DC 1 and AC 1 that no DHT has defined receives the Annex K table for it, luminance for id 0 and
 * chrominance for id 1.  Slots 2 and 3 receive nothing.  A file without any DHT and a file that defines only some of the four are
 * both covered; for a multi-scan file the fill happens once, before the first scan.  Progressive files are not covered and keep their
 * answer.  Host code only (meterelf_amd/csrc/melf_jpeg_std_tables.h): the files go through the pipeline as it stands, at their twins'
 * rate (profiles/jpeg_scans/jpeg_scans_rate.txt: 2.22 / 2.38 ms a 1024-file call of 4:2:0 / 4:2:2 files without DHT, 0.996 / 0.972 times
 * the same files with their tables, where the host branch takes 593 ms, 268 times as long).  get_meter_values turns the switch on;
 * METERELF_JPEG_TABLES=host restores the host branch. */
int melf_ctx_set_jpeg_default_tables(melf_ctx* ctx, int on);
int melf_ctx_get_jpeg_default_tables(melf_ctx* ctx, int* on);

/* ---- JPEG files that end early ----
 * A snapshot read while the camera software is still writing it, an upload that lost its connection, an MJPEG frame clipped by the
 * transport: a baseline file whose bytes stop inside the scan.  libjpeg(-turbo), so cv2.imread and Pillow, reads such a file: its data
 * source answers the end of the bytes with a fake EOI, the decoder goes on over zero bits, and warns.  By default every decode call
 * gives such a file MELF_JPEG_CORRUPT and a zero frame; none of that changes.  melf_ctx_set_jpeg_truncated(ctx, 1) makes
 * melf_jpeg_decode_batch, melf_jpeg_process_batch, melf_jpeg_process_files and melf_jpeg_process_files_begin / _end of that context give
 * status 0 and libjpeg's frame to a sequential single-scan file (SOF0 / SOF1) the decoder takes otherwise whose scan ends, before its
 * last block, at the end of the bytes or at an EOI.  Off at context creation; with it off every entry point behaves exactly as
 * before, status codes, melf_last_error texts and launches included.  Not while a _begin call is in flight.  Independent of the other
 * five switches.  No probe knows the switch: truncation does not show in the headers.
 * The rule, bit for bit libjpeg's.  Let the stream be the entropy-coded bytes without stuffing and markers, followed by an endless run
 * of zero bits, decoded MCU by MCU as ever.  The cut MCU is the MCU during whose decode a bit behind the real bytes is first required,
 * by a Huffman code or by the value bits behind it; it is decoded completely, from the zero bits, and is the last one decoded.  Every
 * block of every later MCU is all zero, DC included (no predictor is applied): mid grey.  IDCT, upsampling and colour conversion run
 * unchanged; the chroma filter blends across the boundary as anywhere.  A stream that ends exactly on an MCU boundary with MCUs still
 * owing makes the next MCU the cut MCU, decoded entirely from zeros.  With restart intervals: every interval before the last one found
 * must be complete; the last one found may be short, or empty; if it is complete and intervals are owing, the first MCU of the next
 * interval, predictors reset, is the cut MCU; intervals never reached stay zero.
 * Exactness holds where libjpeg's range limit is a plain clamp.  The zero-decoded MCU is garbage (with the Annex K tables a luma block of
 * 63 AC coefficients of -1) and can leave that range with coarse quantisation tables; the pixels of the cut MCU, and those whose chroma
 * filter reads it, are then unspecified -- no fault, no access out of bounds -- and every other pixel is still exact.
 * Still MELF_JPEG_CORRUPT, with or without the switch: a scan that ends at a marker other than EOI, a Huffman code that does not exist,
 * a restart interval that runs out of data but is not the last one found, surplus RSTn, a progressive file that ends inside a scan
 * (libjpeg smooths it), a multi-scan file that ends inside a scan or before its third scan, a file cut inside its headers.
 * A file cut behind the meter_rect window plus its margin was always read by melf_jpeg_process_batch (the window-limited decode never
 * looks behind the window); that path is untouched and such a file is not counted below.
 * How: k_jpeg_clean records what ended the scan.  With the switch on, k_jpeg_huff and k_jpeg_huff_rst report a file that holds no
 * impossible code but runs out of data with a status value of their own (the IDCT and colour stages treat it as 0; the host maps it to
 * 0 and counts it), k_jpeg_huff leaving the exact entry states of its last two segments.  k_jpeg_cut_tail, one wave per file, which a
 * file that is not cut leaves at once, walks on from there over the masked stream (meterelf_amd/csrc/melf_jpeg_cut.h: the zeros are
 * produced, not read), writes the cut MCU's blocks inside the window, zeroes the blocks behind it that the segment decoders' 32 bits
 * of over-run may have completed, and settles the status.
 * melf_ctx_jpeg_truncated_files: the files this context's calls completed under the rule since the last reset (what libjpeg's
 * warning would have told the caller); reset != 0 zeroes the count. */
int melf_ctx_set_jpeg_truncated(melf_ctx* ctx, int on);
int melf_ctx_get_jpeg_truncated(melf_ctx* ctx, int* on);
int melf_ctx_jpeg_truncated_files(const melf_ctx* ctx, int64_t* files, int reset);

/* ---- Baseline JPEG files with scans beyond 4 MB: 12 MP and larger snapshots at high quality ----
 * k_jpeg_huff gives each of its 1024 lanes one segment of at most 32 000 bits of the stream, so by default a file WITHOUT restart
 * markers whose entropy-coded data exceed 4 MB gets status 1 from every decode call; none of that changes.
 * melf_ctx_set_jpeg_long_scans(ctx, 1, 0) makes melf_jpeg_decode_batch, melf_jpeg_process_batch, melf_jpeg_process_files and
 * melf_jpeg_process_files_begin / _end of that context decode such a file on the GPU, byte for byte like libjpeg, up to 532 774 904
 * bytes of entropy-coded data (where 32-bit bit positions end: meterelf_amd/csrc/melf_jpeg_long.h has the derivation); longer scans
 * keep status 1.  Off at context creation; with it off every JPEG entry point behaves exactly as before, status codes, melf_last_error
 * texts and launches included.  Not while a _begin call is in flight.  Independent of the other switches; no probe knows it (whether
 * a scan is long does not show in what the probes report).
 * How: such a file's record is of a kind of its own, which k_jpeg_huff and k_jpeg_huff_rst pass by, and k_jpeg_chapters (timed as
 * MELF_K_JPEG_HUFF; launched only for runs of files that hold one) cuts its scan into consecutive chapters of 1024 segments and takes
 * them in order, each through k_jpeg_huff's three phases.  The first segment of a chapter starts from the settled exit state of the
 * chapter before, which is exact; the block count and the DC predictors carry over.  The loop ends after the chapter that holds the end
 * of the meter_rect window (melf_jpeg_process_batch and the file-name calls), or after the last chapter.
 * chapter_bytes = 0 is production: scans up to 4 MB take the ordinary kernels as ever, longer ones chapters of 4 091 904 bytes (999
 * dwords a segment, the most the kernel addresses).  chapter_bytes > 0 is for tests and tuning: every restart-less baseline scan
 * longer than one chapter takes k_jpeg_chapters, with chapters of that length rounded up to 4096 x an odd number of bytes, at least
 * 36 864 and at most the production length; melf_ctx_get_jpeg_long_scans returns the chapter length in force (4 091 904 in production).  (What the
 * host compares is the scan's length in the file, stuffing and EOI included; the chapters count the clean bytes.)
 * chapter_bytes < 0, or a NULL context: MELF_ERR_INVALID.
 * Measured on one MI355X (profiles/jpeg_long/jpeg_long_rate.txt; noise at quality 100, 4:4:4): melf_jpeg_process_batch on 64 / 256 files
 * of 4.9 MB (two chapters) takes 18.4 / 111 ms a call, on 64 / 256 files of 10.5 MB (three chapters) 29.9 / 277 ms -- 10.8 / 16.6 and
 * 12.6 / 18.4 ms of that in k_jpeg_chapters, the rest the staging copy and upload of 0.3 - 2.7 GB -- where the host branch such files
 * took (Pillow on 8 threads, then the batch read) takes 257 / 955 and 628 / 2141 ms.  A 256-name list of 640 x 480 camera files with
 * 1 / 8 / 32 files of 4.9 MB among them takes 9.3 / 11.8 / 19.4 ms against 22.5 / 32.3 / 121 ms with those files through the host
 * branch.  Files the ordinary kernels take run at the rate they had (2.03 against 2.10 ms a 1024-file call, inside the spread).
 * Out of scope: files with restart intervals and progressive files, which have no such limit; a component scan beyond 4 MB of a
 * multi-scan file, which stays status 1; a long file that runs out of data is MELF_JPEG_CORRUPT whether or not
 * melf_ctx_set_jpeg_truncated is on. */
int melf_ctx_set_jpeg_long_scans(melf_ctx* ctx, int on, int chapter_bytes);
int melf_ctx_get_jpeg_long_scans(melf_ctx* ctx, int* on, int* chapter_bytes);
/* The header check with switches: *supported is what the decode calls of a context with the switches `flags` (MELF_JPEG_TAKE_*) on
 * would answer from the headers; H and W are the STORED size, *orientation the EXIF code 1..8 whether or not oriented files are
 * taken.  With flags 0 this is melf_jpeg_probe plus the orientation code.  melf_last_error holds the reason of a refusal. */
int melf_jpeg_probe_flags(const uint8_t* data, size_t size, int flags, int32_t* H, int32_t* W, int32_t* orientation, int32_t* supported);
int melf_jpeg_probe_flags_batch(const uint8_t* const* data, const size_t* sizes, int n, int flags, int32_t* H, int32_t* W,
                                int32_t* orientation, int32_t* supported);

/* Decodes n files of H x W pixels.  out: n*H*W*3 bytes, on the host (out_on_device = 0) or in HBM.
 * Synchronises the context's stream. */
int melf_jpeg_decode_batch(melf_ctx* ctx, const uint8_t* const* data, const size_t* sizes, int n, int H, int W,
                           void* out, int out_on_device, int32_t* status);

/* Stage entry point (parity tests): the first decode stage alone -- byte stuffing (FF 00), fill bytes and RSTn markers taken out
 * of ONE entropy-coded segment on the GPU, as libjpeg's bit reader does while it reads (cv2.imread, meterelf/_image.py:49).
 * raw[n]: any bytes; restart_expected > 0: the segment of a file with restart intervals, rst receives the bit offsets of its
 * restart_expected + 1 intervals (as the kernel leaves them) and rst_cnt the number found.  out must hold n + 192 bytes (clean
 * bytes, then zero fill); out_len receives the cleaned length.  Returns 0, or -1 on a bad argument / HIP error. */
int melf_jpeg_clean_segment(const uint8_t* raw, int n, int restart_expected, uint8_t* out, int32_t* out_len, uint32_t* rst,
                            int32_t* rst_cnt);

/* get_meter_value for n JPEG files (meterelf/_api.py:22-33 with _image.py:46-51): decode on the GPU
 * straight into HBM, then the same path as melf_process_batch.  Records of files whose status is
 * non-zero are meaningless. */
int melf_jpeg_process_batch(melf_ctx* ctx, const uint8_t* const* data, const size_t* sizes, int n, int H, int W,
                            melf_result* out_host, int32_t* status);

/* The same for n file names (the loop of get_meter_values, meterelf/_api.py:22-33): the library reads the files
 * (on threads) and processes them frame size by frame size (a list may mix sizes; H_used / W_used return the size of
 * the first file its decoder accepts); files it does not decode come back with status 1 / 2 / 4 for the caller to
 * route (host decode for another format).  Status 3 is not used by this call.  The files are read straight into a
 * pinned buffer of the context, from which they are uploaded as they are (byte stuffing and restart markers are taken
 * out on the GPU): the host touches no byte of a file after read() has written it. */
int melf_jpeg_process_files(melf_ctx* ctx, const char* const* paths, int n, int32_t* H_used, int32_t* W_used,
                            melf_result* out_host, int32_t* status);

/* The same call in two halves, for a host that wants to work on the previous chunk's records meanwhile
 * (get_meter_values does: meterelf_amd/_api.py): _begin returns at once and the call runs on a thread of the library,
 * _end waits for the OLDEST call begun and returns its status code (message via melf_last_error as usual).  Up to
 * MELF_FILES_IN_FLIGHT_MAX calls may be in flight per context -- one reading its files, one preparing and enqueueing
 * its GPU work, one waiting for its kernels (one more _begin fails with MELF_ERR_INVALID); every pointer must stay
 * valid until the call's own _end; no other call on the context while any is in flight. */
#define MELF_FILES_IN_FLIGHT_MAX 3
int melf_jpeg_files_in_flight_max(void); /* the value the library was built with */
int melf_jpeg_process_files_begin(melf_ctx* ctx, const char* const* paths, int n, int32_t* H_used, int32_t* W_used,
                                  melf_result* out_host, int32_t* status);
int melf_jpeg_process_files_end(melf_ctx* ctx);
/* Where the _begin calls of this context spent their host time since the last reset (sums, milliseconds): out[0] calls,
 * [1] files, [2] read stage (open / fstat / read / close / header parse on the I/O pool), [3] waiting for the call's turn at the
 * context, [4] enqueueing (chunk layout, uploads, launches) until the context is handed to the next call, [5] waiting for the
 * call's kernels and records; [6] threads of the read stage, [7] of the other host loops (the caller included), [8] cores the
 * process may use (affinity mask cut down to the cgroup CPU quota), [9] devices the process has contexts on (what the pools divide the cores by).
 * Not while a _begin call is in flight. */
/* Measurement aid: open() + close() of every path on the I/O pool of `device` (no context needed, nothing is read):
 * milliseconds for the n files and the threads that took part -- what the file system allows the read stage. */
int melf_files_open_probe(const char* const* paths, int n, int device, double* ms, int* threads);
#define MELF_FILES_STATS_COUNT 10
int melf_ctx_files_stats(melf_ctx* ctx, double out[MELF_FILES_STATS_COUNT], int reset);

/* Promise that the frames handed to melf_process_batch_dev are complete in device memory at the time of each call (they
 * do not depend on work still pending on the call's stream -- e.g. frames that were uploaded or decoded earlier and
 * synchronised).  Consecutive calls, also on ONE caller stream, then alternate between the context's two lanes: a call's
 * prep and match kernels start at once on the lane's own stream, beside the previous call's kernels; only the kernel
 * that writes the records waits for the work the caller's stream held at the time of the call, and the caller's stream
 * continues when the call is done (what is enqueued on it afterwards sees the records, as without the promise).
 * Same results; steps 10-30 % shorter.  Off by default: without the promise every kernel of a call is ordered behind
 * the stream's earlier work. */
int melf_ctx_set_frames_resident(melf_ctx* ctx, int on);

/* ---- measurement ---------------------------------------------------------
 * With profiling on, every kernel launched by a *_dev entry point is bracketed
 * by hipEvents on its stream; melf_ctx_timings drains them (synchronising) and
 * returns per-kernel accumulated milliseconds and launch counts. */
enum { MELF_K_LPLANE = 0, MELF_K_MATCH = 1, MELF_K_DIALS = 2, MELF_K_FUSED_MASK = 3, MELF_K_HLS = 4,
       MELF_K_JPEG_HUFF = 5, MELF_K_JPEG_IDCT = 6, MELF_K_JPEG_COLOR = 7, MELF_K_STREAM_PROBE = 8,
       MELF_K_GATHER = 9 /* k_gather_rows: melf_process_frame_list_dev; k_plane_rows: melf_process_plane_list_dev; k_orient_tiles:
                            melf_process_oriented_dev; k_narrow_rows: melf_process_wide_dev; k_narrow_list_rows / k_narrow_plane_rows:
                            melf_process_wide_list_dev / melf_process_wide_plane_list_dev */, MELF_K_COUNT = 10 };
/* Which kernel, in which layout, computed the template match (meterelf/_utils.py:91-97: ONE cv2.matchTemplate code
 * path in the reference; here the batch size and the crop shape select among three kernels and, for the tuned one,
 * among wave layouts) of the context's most recent call.  Tests assert it, so that a change of a dispatch threshold
 * cannot silently move a parity test onto another kernel. */
enum { MELF_MATCH_KERNEL_DOT4 = 0, MELF_MATCH_KERNEL_MFMA = 1, MELF_MATCH_KERNEL_GEN = 2 };
typedef struct {
    int32_t kernel;          /* MELF_MATCH_KERNEL_*                                                      */
    int32_t n, rows, cols;   /* images of the launch, searched image size                                */
    int32_t groups;          /* 32-frame groups                                                          */
    int32_t waves;           /* waves of the launch (matrix-core kernels)                                */
    int32_t rows_per_wave;   /* tuned kernel: map rows of a full-row wave (RB); general kernel: tile rows */
    int32_t full_waves;      /* tuned kernel, per group: waves of RB full rows                           */
    int32_t pair_waves;      /* tuned kernel, per group: waves of RB + 1 rows that share a middle row    */
    int32_t tiles;           /* general / dot4 kernel: tiles (partials) per frame                        */
    int32_t reserved[6];
} melf_match_info;
int melf_ctx_last_match(const melf_ctx* ctx, melf_match_info* out);
/* Which dial-reader kernel the context's most recent launch ran: the kernel family that reads the frames' layout and NR, the
 * window rows a lane requests up front -- one of 32, 40, 48, 52, 56, 64, the smallest that holds ws_max, the context's largest
 * dial window (2 R + 5 rows).  Twelve families (and the two each of the 16-bit, the packed 10-bit and the 32-bit packed frames, below) times six NR: tests assert the pair, so
 * that every instantiation production can pick is known to have been the one a parity test launched.  family is -1 and nr 0
 * before the first launch; a call of more frames than one launch takes reports its last piece.  Plain fields written by every
 * launch, as for melf_ctx_fused_variant's last_launch.  Every output pointer may be NULL. */
enum { MELF_DIALS_HLS = 0,            /* k_dials<true>: packed HLS dials crops (melf_read_dials)            */
       MELF_DIALS_BGR = 1,            /* k_dials<false>: packed B G R                                       */
       MELF_DIALS_PACKED3 = 2,        /* k_needles<3>: packed R G B                                         */
       MELF_DIALS_PACKED4 = 3,        /* k_needles<4>: B G R A / R G B A                                    */
       MELF_DIALS_NV12 = 4,           /* k_yneedle<false>: melf_process_yuv*, NV12                          */
       MELF_DIALS_I420 = 5,           /* k_yneedle<true>: melf_process_yuv*, I420 / YV12                    */
       MELF_DIALS_P422 = 6,           /* k_p422_needle: packed 4:2:2                                        */
       MELF_DIALS_YP_SUB0_STEP1 = 7,  /* k_yp_needle<0, 1>: melf_process_yuv_planar*, sub_x 0, planar       */
       MELF_DIALS_YP_SUB0_STEP2 = 8,  /* k_yp_needle<0, 2>: ... sub_x 0, interleaved pairs                  */
       MELF_DIALS_YP_SUB1_STEP1 = 9,  /* k_yp_needle<1, 1>: ... sub_x 1, planar                             */
       MELF_DIALS_YP_SUB1_STEP2 = 10, /* k_yp_needle<1, 2>: ... sub_x 1, interleaved pairs                  */
       MELF_DIALS_PLANAR = 11,        /* k_planar_needle: melf_process_planes*                              */
       MELF_DIALS_FAMILIES = 12 };
/* The families of the 16-bit frames (melf_process_yuv16*), also values of `family`.  An enum and a prefix of their own: the twelve
 * MELF_DIALS_* names and MELF_DIALS_FAMILIES == 12 are what the instantiation tests of the 8-bit layouts enumerate and pin, and
 * these kernels are enumerated by tests of their own; the values go on from 12 so that `family` stays one number space. */
enum { MELF_DIALS16_STEP1 = 12,       /* k_y16_needle<1>: melf_process_yuv16*, planar                        */
       MELF_DIALS16_STEP2 = 13 };     /* k_y16_needle<2>: ... interleaved pairs                              */
/* The families of the packed 10-bit 4:2:2 frames (melf_process_yuv422_10*), in the same way: an enum of their own that goes on. */
enum { MELF_DIALS10_V210 = 14,        /* k_v210_needle: melf_process_yuv422_10*, MELF_YUV422_10_V210         */
       MELF_DIALS10_Y210 = 15 };      /* k_y210_needle: ... MELF_YUV422_10_Y210                              */
/* The families of the 32-bit packed 4:4:4 frames (melf_process_packed32*), in the same way. */
enum { MELF_DIALS32_YUV = 16,         /* k_p32_needle<true>: melf_process_packed32*, MELF_P32_YUV            */
       MELF_DIALS32_RGB = 17 };       /* k_p32_needle<false>: ... MELF_P32_RGB                               */
int melf_ctx_last_dials(const melf_ctx* ctx, int* nr, int* family, int* ws_max);
/* The tuned kernel's wave layout for a template / searched-image shape and a batch of n images, without a GPU or a
 * context (host logic; kernel = MELF_MATCH_KERNEL_MFMA when the shape belongs to the tuned kernel's class, else the
 * kernel that takes it).  reserved[0] = padded template rows, reserved[1] = L-plane rows per frame group. */
int melf_match_layout_query(int th, int tw, int rows, int cols, int n, melf_match_info* out);
/* The GENERAL matrix-core kernel's plan for a shape and batch size, without a GPU (host logic; tests pin its invariants for
 * every batch size).  out->kernel = the kernel DEFAULT dispatch launches for this shape and n (the plan returned is the
 * general kernel's either way: MELF_MATCH=gen forces it).  For the general kernel -- here, in melf_match_layout_query and
 * in melf_ctx_last_match -- rows_per_wave = rows a tile computes, tiles = tiles (= workgroups, = partials) per frame group,
 * waves = waves of the launch, reserved[0] = Toeplitz blocks per template row, [1] = L-plane rows per frame group,
 * [2] = column blocks per tile, [3] = K slices per tile = waves per workgroup, [4] = remainder ("V form") map columns,
 * [5] = image blocks per V-form row.
 * tasks (optional, cap entries): one entry per wave of a frame group's workgroups, *ntasks = how many there are.
 * A wave computes map rows y0 .. y0 + rows - 1 (rows_computed >= rows are accumulated) of column blocks xb0 .. xb0 + nxb - 1
 * (32 map columns each) over the slice [k_lo, k_hi) of the tile's K range (Toeplitz block x template row); rows == 0: a
 * V-form tile = ONE map column (remainder column index xb0) x the 32 map rows from y0, K range = (image row - y0, image
 * block).  The nslices waves of a tile are one workgroup and add their accumulators up in its LDS (lds_bytes). */
typedef struct {
    int32_t y0, rows, rows_computed, xb0, nxb, tile, slice, nslices, k_lo, k_hi, lds_bytes, reserved;
} melf_gen_task;
int melf_match_gen_plan_query(int th, int tw, int rows, int cols, int n, melf_match_info* out, melf_gen_task* tasks, int cap,
                              int32_t* ntasks);

int melf_ctx_set_profiling(melf_ctx* ctx, int on);  /* 0 off, 1 every kernel, 2 only the match kernel (two event records per batch instead of eight) */
int melf_ctx_timings(melf_ctx* ctx, double ms[MELF_K_COUNT], int64_t launches[MELF_K_COUNT]);
const char* melf_kernel_name(int k);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* METERELF_HIP_H */
