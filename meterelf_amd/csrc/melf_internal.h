// Internal declarations shared by the translation units of libmeterelf_hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <stdint.h>

#include "../../include/meterelf_hip.h"

namespace melf {

// Environment switches.  The PRODUCT library reads only the documented ones (README.md, "Environment switches": MELF_MATCH,
// MELF_MATCH_LAYOUT, MELF_GEN_SHAPE, MELF_FUSED_VARIANT, MELF_FORCE_GENERIC_MASK, MELF_JPEG_CHUNK, MELF_IO_THREADS,
// MELF_HOST_THREADS).  diag_env reads only the trace switches (MELF_*_TRACE), which exist only in the diagnostic build
// (`make -C meterelf_amd/csrc diag`, -DMELF_DIAG, loaded through MELF_LIB_PATH): there diag_env is getenv, here it is nothing.
#ifdef MELF_DIAG
inline const char* diag_env(const char* name) { return getenv(name); }
#else
inline const char* diag_env(const char*) { return nullptr; }
#endif

}  // namespace melf

#include "melf_frame_layout.h"

namespace melf {

// ---- K2: template match -----------------------------------------------------
// One partial (max, first-argmax) per workgroup tile of the correlation map.
struct MatchPartial {
    float val;
    int32_t idx;  // y * rw + x in the frame's correlation map; INT32_MAX = empty
};

constexpr int MATCH_R = 11;           // output rows per lane
constexpr int MATCH_WAVES = 4;        // waves per workgroup
constexpr int MATCH_RBLK = MATCH_R * MATCH_WAVES;  // output rows per workgroup
constexpr int MATCH_CBLK = 64;        // output cols per workgroup (one per lane)

struct MatchGeom {
    int th, tw;        // template rows, cols
    int tw4;           // template row length in dwords (tw padded to 4)
    int trows;         // padded template rows: th + 2*(MATCH_R-1)
    uint32_t last_ones;  // byte mask (0x01 per valid byte) of the last template dword
    int ldsw;          // LDS tile row width in dwords
    int lds_rows;      // LDS tile rows: MATCH_RBLK + th - 1
    double tmean;      // cv::mean(template) = sum * (1.0 / N)
};

// source description for K2: either packed single-channel u8 images or camera frames (BGR, RGB, BGRA, RGBA: the launch's pix)
struct MatchSrc {
    const uint8_t* base;
    size_t frame_stride;  // bytes between consecutive images/frames
    int row_stride;       // bytes between rows
    int x0, y0;           // origin of the searched image inside the frame (pixels)
    int rows, cols;       // searched image size
    size_t readable;      // bytes from `base` the caller guarantees readable: (images - 1) * frame_stride + the last image's rows
};

void launch_match(const MatchSrc& src, const FrameLayout& lay, int n, const MatchGeom& g, const uint32_t* d_tplT,
                  float* d_result_map, MatchPartial* d_partials, int* nparts_out, hipStream_t stream);
int match_parts(const MatchGeom& g, int rows, int cols);

// ---- K2 on the matrix cores (k_match_mfma.hip) --------------------------------
struct MfmaPlan {
    int rh, rw, nxb, nkb, th_pad, nparts, rows_pad, groups;
    int rb, na, np;   // layout: na waves of rb full map rows + np pairs of (rb + 1)-row waves sharing their middle row
    int ks, ntiles;   // K slices per tile (waves of a tile's workgroup; nparts = ntiles x ks), tiles per frame group = na + 2 np
    size_t lg_bytes, r_bytes;
};
bool mfma_match_ok(int th, int tw, int rows, int cols);
MfmaPlan mfma_plan(int th, int tw, int rows, int cols, int nframes);
size_t mfma_atab_bytes(int th);
void mfma_build_atab(const uint8_t* templ, int th, int tw, int8_t* atab);
void launch_mfma_prep(const MatchSrc& src, const FrameLayout& lay, int n, const MfmaPlan& p, int th, int tw, int8_t* d_lg,
                      uint16_t* d_r, hipStream_t stream);
// launch_mfma_match: d_ws = the row-window sums R in epilogue order (k_prep_lplane); the waves add them up
void launch_mfma_match(int n, const MfmaPlan& p, int th, int tw, long tsum, double tmean, const int8_t* d_atab,
                       const int8_t* d_lg, const uint32_t* d_ws, float* d_result_map, MatchPartial* d_partials,
                       hipStream_t stream, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// ---- K2, general form (k_match_gen.hip): any template up to 256 columns, any map size ----
struct GenTile {           // one workgroup's tile of the correlation map (per frame group)
    int16_t y0;            // first map row of the tile (V form: first of its 32 map rows)
    int8_t R, Rc;          // map rows of the tile, rows computed (R rounded up to 2/4/6/8); R == 0: V-form tile
    int8_t nxb;            // column blocks (1 or 2)
    int8_t pad0;
    int16_t xb0;           // first column block (V form: index of the remainder column)
    int32_t klen;          // length of the tile's linearised K range; wave w of ns takes [w klen / ns, (w + 1) klen / ns)
};
struct GenPlan {
    int rh, rw, rwp, nd, nkb, rows_pad, groups, ntiles, ntasks, rc;
    int nxb_tile, nslices;   // column blocks per H-form tile, K slices = waves per workgroup (the planner's choice)
    int nxb_h;               // column blocks the H form covers
    int vcols, vx0, vkb0, ndv, ndelta;
    size_t lg_bytes, r_bytes, atab_bytes, atabv_bytes, lds_bytes;
    std::vector<GenTile> tiles;
};
struct GenDev {            // device copies that belong to one plan
    int8_t* atab = nullptr;
    int8_t* atabv = nullptr;
    GenTile* tiles = nullptr;
};
bool gen_match_ok(int th, int tw, int rows, int cols);
GenPlan gen_plan(int th, int tw, int rows, int cols, int nframes);
void gen_build_atab(const uint8_t* templ, int th, int tw, const GenPlan& p, int8_t* atab);
void gen_build_atabv(const uint8_t* templ, int th, int tw, const GenPlan& p, int8_t* atabv);
void launch_gen_match(int n, const GenPlan& p, int rows, int th, int tw, long tsum, double tmean, const GenDev& dev, const int8_t* d_lg,
                      const uint16_t* d_r, float* d_result_map, MatchPartial* d_partials, hipStream_t stream,
                      hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// prep for either matrix-core kernel: Lg (fragment order) and the row-window sums R in the match waves' epilogue order
// (pairs > 0: the tuned kernel's paired-operand row layout, see k_prep_lplane)
void launch_match_prep(const MatchSrc& src, const FrameLayout& lay, int n, int groups, int rows_pad, int nkb, int rwp, int tw,
                       int8_t* d_lg, uint16_t* d_r, hipStream_t stream, int pairs = 0);

// ---- K3: per-dial reading ---------------------------------------------------
struct DialGeom {
    int32_t wx0, wy0;    // window origin in dials-crop coordinates
    int32_t ws;          // window size (2R+5 <= 64)
    int32_t core_x, core_y;  // int(cx), int(cy): centre of the 5x5 colour core
};

// (MatchSrc under other field names: one struct would rename every kernel's mangled symbol and touch both .inc bodies -- not done)
struct DialsSrc {
    const uint8_t* base;   // camera frames (the launch's pix) or packed HLS dials crops
    size_t frame_stride;
    int row_stride;        // bytes
    int x0, y0;            // origin of the meter crop inside the frame (BGR mode)
    int crop_rows, crop_cols;  // meter crop size (BGR mode): cvtColor image width for the tail rule
    size_t readable;       // bytes from `base` the caller guarantees readable: (frames - 1) * frame_stride + the last frame's rows
};

// which instantiation a launch_dials call picked: its NR (window rows requested up front) and its kernel family (MELF_DIALS_*)
struct DialsLaunch {
    int nr, family;
};
DialsLaunch launch_dials(const DialsSrc& src, const FrameLayout& lay, int n, const melf_params& P, const DialGeom* d_geom,
                         const uint64_t* d_rowmasks /* [ndials][3][64] */, const MatchPartial* d_partials,
                         int nparts, int rw, melf_result* d_results, hipStream_t stream, int ws_max /* largest DialGeom::ws */);

// ---- K1b / HLS --------------------------------------------------------------
void launch_bgr2hls(const uint8_t* d_src, int rows, int cols, size_t row_stride, int hue_shift,
                    uint8_t* d_dst, hipStream_t stream);
void launch_fused_mask(const uint8_t* d_frames, int n, int H, int W, int hue_shift, const int lo[3],
                       const int hi[3], uint8_t* d_masks, hipStream_t stream);
// table-driven fast path of K1b (W % 16 == 0, 16-byte aligned buffers)
constexpr int FUSED_TABLE_DWORDS = 3 * 65536 * 2 / 32 + 65536 / 32 + 3 * 65536 / 32 + 3 * (512 * 512 / 32) + 3 * (256 + 512) + 16;
// behind the tables: the work queues of the launches in flight (round 5: a launch's persistent workgroups take their segments
// from a counter), FUSED_QUEUE_SLOTS of them in rotation, one 64-byte line each: {next segment, workgroups done}; a launch's
// last workgroup leaves its slot zeroed
constexpr int FUSED_QUEUE_SLOTS = 64, FUSED_QUEUE_DWORDS = FUSED_QUEUE_SLOTS * 16;
constexpr int FUSED_BUF_DWORDS = FUSED_TABLE_DWORDS + FUSED_QUEUE_DWORDS;
int fused_tables_count_offset();
int fused_tables_active_offset();
int fused_tables_noniv_offset();
void launch_build_fused_tables(int hue_shift, const int lo[3], const int hi[3], uint32_t* d_tables, hipStream_t stream);
bool fused_mask_lut_ok(const void* d_frames, const void* d_masks, int H, int W);
// the next launch_fused_mask_lut of this thread carries these events as its dispatch's own start / stop stamps
void fused_mask_timing_events(hipEvent_t start, hipEvent_t stop);
// returns the work-queue slot the launch took, -1 for the static split
int launch_fused_mask_lut(const uint8_t* d_frames, int n, int H, int W, int hue_shift, const int lo[3],
                           const int hi[3], uint32_t* d_tables /* FUSED_BUF_DWORDS: tables + work queues */, int variant, uint8_t* d_masks,
                           hipStream_t stream);

// measurement aid: bare 3:1 stream over the caller's buffers (bench.py's stream_ceiling); returns the bytes moved
size_t launch_stream_probe(const void* d_in, size_t in_bytes, void* d_out, int chunks_per_block, uint32_t* d_tables, hipStream_t stream,
                           hipEvent_t ev_start, hipEvent_t ev_stop);

// ---- k_yuv.hip: the YUV 4:2:0 -> BGR conversion alone (melf_yuv_to_bgr) ----
// n frames: Y plane at d_src (y_pitch, frame_stride), chroma planes per YuvPlanes, converted under mx; d_dst: n packed H x W x 3
// BGR frames
void launch_yuv2bgr(const uint8_t* d_src, int pix, int n, int H, int W, int y_pitch, size_t frame_stride, const YuvPlanes& yuv,
                    const YuvMatrix& mx, uint8_t* d_dst, hipStream_t stream);

// the same for planar / semi-planar YUV of any subsampling (melf_yuv_planar_to_bgr): the Y plane at d_src (y_pitch, frame_stride)
void launch_yuvp_to_bgr(const uint8_t* d_src, int n, int H, int W, int y_pitch, size_t frame_stride, const YuvPlanarPlanes& yp,
                        const YuvMatrix& mx, uint8_t* d_dst, hipStream_t stream);

// the same for 16-bit planar / semi-planar YUV (melf_yuv16_to_bgr): y_pitch and frame_stride in bytes
void launch_y16_to_bgr(const uint8_t* d_src, int n, int H, int W, int y_pitch, size_t frame_stride, const Yuv16Planes& yp,
                       const YuvMatrix& mx, uint8_t* d_dst, hipStream_t stream);

// the same for packed 10-bit YUV 4:2:2 (melf_yuv422_10_to_bgr): pix PIX_V210 / PIX_Y210
void launch_p10_to_bgr(const uint8_t* d_src, int pix, int n, int H, int W, int row_pitch, size_t frame_stride, const YuvMatrix& mx,
                       uint8_t* d_dst, hipStream_t stream);

// the same for 32-bit packed 4:4:4 (melf_packed32_to_bgr): pix PIX_P32_YUV (mx: the conversion) / PIX_P32_RGB (mx NULL)
void launch_p32_to_bgr(const uint8_t* d_src, int pix, int n, int H, int W, int row_pitch, size_t frame_stride, const Packed32Fields& fields,
                       const YuvMatrix* mx, uint8_t* d_dst, hipStream_t stream);

// the same for packed YUV 4:2:2 (melf_yuv422_to_bgr): n frames at d_src (row_pitch, frame_stride), pix PIX_YUYV / _UYVY / _YVYU
void launch_p422_to_bgr(const uint8_t* d_src, int pix, int n, int H, int W, int row_pitch, size_t frame_stride, const YuvMatrix& mx,
                        uint8_t* d_dst, hipStream_t stream);

// ---- k_gather.hip: frames in separate allocations (melf_process_frame_list_dev) ----
// Copies the row runs of a staging plan (melf_stage_plan.h: RowRuns) from each of the n frames d_frames[i] -- a DEVICE array of n
// device pointers, `extent` bytes readable from each -- into the staged frame d_staged + i * staged_stride.  n <= 65535.
struct RowRuns;
void launch_gather_rows(const void* const* d_frames, int n, const RowRuns& runs, uint8_t* d_staged, size_t staged_stride, size_t extent,
                        hipStream_t stream);
// The same for frames whose planes lie in separate allocations (melf_process_plane_list_dev): d_planes is a DEVICE array of
// n * nplanes device pointers, frame-major; run k of the plan reads plane slot k at the offset and within the extent `split` gives
// (melf_stage_plan.h: plane_split).  nplanes == runs.count.
struct PlaneSplit;
void launch_plane_rows(const void* const* d_planes, int nplanes, int n, const RowRuns& runs, const PlaneSplit& split, uint8_t* d_staged,
                       size_t staged_stride, hipStream_t stream);

// ---- k_orient.hip: frames stored rotated or mirrored (melf_process_oriented_dev, melf_orient_frames) ----
// Writes the runs of an oriented plan (melf_orient_addr.h: orient::Runs) of each of the n stored frames d_frames + i * frame_stride
// upright into the staged frame d_staged + i * staged_stride.  n <= 65535.
namespace orient { struct Runs; }
void launch_orient_tiles(const void* d_frames, size_t frame_stride, int n, const orient::Runs& runs, uint8_t* d_staged, size_t staged_stride,
                         hipStream_t stream);

// ---- k_narrow.hip: frames of wide samples (melf_process_wide_dev, melf_wide_to_bgr) ----
// Narrows the runs of a wide batch's plan (melf_narrow_addr.h: the runs count SAMPLES of the source) of each of the n frames d_frames
// + i * frame_stride (bytes) into the staged frame d_staged + i * staged_stride, under `rule` (melf_narrow.h); `extent` samples of
// a frame are readable.  n <= 65535.
namespace narrow { struct Rule; }
void launch_narrow_rows(const void* d_frames, size_t frame_stride, int n, const RowRuns& runs, const narrow::Rule& rule, uint8_t* d_staged,
                        size_t staged_stride, size_t extent, hipStream_t stream);
// The same from a DEVICE array of n frame pointers (melf_process_wide_list_dev; `extent` samples are readable from each), and from a
// device array of n * 3 plane pointers, frame-major (melf_process_wide_plane_list_dev; split in samples: narrow::wide_plane_split).
void launch_narrow_list_rows(const void* const* d_frames, int n, const RowRuns& runs, const narrow::Rule& rule, uint8_t* d_staged,
                             size_t staged_stride, size_t extent, hipStream_t stream);
void launch_narrow_plane_rows(const void* const* d_planes, int n, const RowRuns& runs, const PlaneSplit& split, const narrow::Rule& rule,
                              uint8_t* d_staged, size_t staged_stride, hipStream_t stream);

// ---- calibration stage kernels ------------------------------------------------
void launch_aligned_average(const uint8_t* d_frames, int n, size_t frame_stride, int row_stride, int x0, int y0, int rows,
                            int cols, const int32_t* d_mx, const int32_t* d_my, int ax, int ay, uint8_t* d_out,
                            hipStream_t stream);
void launch_inrange3(const uint8_t* d_img, int npx, const int lo[3], const int hi[3], uint8_t* d_out, hipStream_t stream);

// ---- k_jpeg.hip: baseline JPEG decode ----
struct JpegWorkspace;
// (the header parser, the probes and jpeg_file_orientation: melf_jpeg_parse.h, host-only and inline)
// Headers (and, when asked for, the Huffman decode data built from them) of n files, parsed file by file, from any thread (one
// thread per index): the file-name entry points parse a file right after reading it, on the thread that read it, and build its
// decode tables there too
struct JpegParsed;
JpegParsed* jpeg_parsed_new(int n, bool with_tables);
void jpeg_parsed_resize(JpegParsed* p, int n);   // room for n files; nothing is cleared (jpeg_parse_one resets its entry)
// take_orient: a file with an orientation tag 2..8 is supported, and H, W are its UPRIGHT size
// (take: MELF_JPEG_TAKE_* flags; with MELF_JPEG_TAKE_PROGRESSIVE progressive files of the header's subset are supported too, with
// MELF_JPEG_TAKE_SAMPLINGS 4:4:0 and 4:1:1 files, with MELF_JPEG_TAKE_MULTISCAN sequential files of three one-component scans, with
// MELF_JPEG_TAKE_DEFAULT_TABLES sequential files that leave Huffman tables 0 / 1 out)
void jpeg_parse_one(JpegParsed* p, int i, const uint8_t* data, size_t size, int* H, int* W, int* supported, int take = 0);
void jpeg_parsed_free(JpegParsed* p);
int jpeg_parsed_orientation(const JpegParsed* p, int i);
int jpeg_parsed_progressive(const JpegParsed* p, int i);
// parsed: headers made earlier -- of file pidx[first + j] for the batch's file j (pidx NULL: of file first + j); host_status is
// then the caller's.  pin_base / pin_len: a pinned host buffer the files' bytes may already lie in (the file-name entry points
// read into one): a batch whose files all do is uploaded from there, no byte of it is copied on the host.
// take_orient: files with an orientation tag 2..8 are decoded too (H, W: the upright size); headers in `parsed` must have been
// parsed with the same setting.
int jpeg_prepare_batch(JpegWorkspace** ws, const uint8_t* const* data, const size_t* sizes, int n, int H, int W,
                       int32_t* host_status, std::string* err, const JpegParsed* parsed = nullptr, int first = 0,
                       const int* pidx = nullptr, const uint8_t* pin_base = nullptr, size_t pin_len = 0, int take = 0);
int jpeg_launch_batch(JpegWorkspace* ws, int n, int H, int W, uint8_t* d_frames, int32_t* status_out_host,
                      hipStream_t stream, std::string* err, void (*timer)(void*, int, int), void* timer_arg,
                      const int* rect /* x0, y0, x1, y1: only this part of each frame is needed; NULL = all */);
int jpeg_upload_batch(JpegWorkspace* ws, int n, hipStream_t copy_stream, std::string* err);
int jpeg_decode_batch_kernels(JpegWorkspace* ws, int n, int H, int W, uint8_t* d_frames, hipStream_t stream, std::string* err,
                              void (*timer)(void*, int, int), void* timer_arg, const int* rect);
const int32_t* jpeg_device_status(const JpegWorkspace* ws);
// Files that end early (melf_ctx_set_jpeg_truncated).  The switch travels with the MELF_JPEG_TAKE_* flags of a batch as a bit of its own
// (JPEG_TAKE_TRUNCATED_INTERNAL, melf_jpeg_parse.h); the Huffman stage reports a file it completed under the rule of
// melf_jpeg_cut.h with JPEG_ST_CUT in the device status array, which the later stages treat as 0 and the host maps to 0 and counts.
constexpr int32_t JPEG_ST_CUT = 3;
void jpeg_workspace_free(JpegWorkspace* ws);

}  // namespace melf
