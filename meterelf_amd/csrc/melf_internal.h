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

// Pixel layout of the images the reading kernels take: MELF_PIX_* (include/meterelf_hip.h) for camera frames, PIX_PLANE for
// the stage entry points' packed single-channel images (melf_match_ccoeff) and HLS dials crops (melf_read_dials).
constexpr int PIX_PLANE = -1;
inline int pix_bytes(int pix) { return pix == MELF_PIX_BGRA || pix == MELF_PIX_RGBA ? 4 : 3; }
// YUV 4:2:0 frames (melf_process_yuv*): the launch's pix, beside the MELF_PIX_* codes.  The Y plane is described like a
// single-channel image (base, frame_stride, row_stride of MatchSrc / DialsSrc), the chroma planes by YuvPlanes.
constexpr int PIX_NV12 = 16, PIX_I420 = 17;
inline bool pix_yuv(int pix) { return pix == PIX_NV12 || pix == PIX_I420; }
struct YuvPlanes {
    int64_t u_off, v_off;  // bytes from a frame's first byte to its U / V samples (NV12: v_off == u_off + 1)
    int c_pitch;           // bytes between chroma rows
    int pad;
};
// The colour conversion of YUV frames, 4:2:0 and 4:2:2 alike: the offset and the five coefficients of melf_device.h's yuv_chroma /
// yuv_luma (include/meterelf_hip.h states the formula).  A by-value kernel argument of every kernel that converts, the same for
// every lane: the compiler keeps it in SGPRs.  The four constants below are the single statement of the numbers: row 0 the
// three-decimal constants of cv2, the others round(2^20 c) of the standards' exact coefficients (derivation: include/meterelf_hip.h).
struct YuvMatrix {
    int yoff;                 // 16 (limited range) or 0 (full range)
    int cy;                   // luma gain
    int crv, cgv, cgu, cbu;   // R from v; G from v and from u; B from u
};
// Every coefficient fits a signed 24-bit operand (|c| < 2^23): the kernels multiply with v_mul_i32_i24 / v_mad_i32_i24, which read
// the low 24 bits of an operand as a signed number, and yuv_chroma's two forms of the G term (melf_device.h) stay equal only then.
constexpr bool yuv_matrix_fits24(const YuvMatrix& m)
{
    constexpr int lim = 1 << 23;
    return (m.yoff == 0 || m.yoff == 16) && m.cy > -lim && m.cy < lim && m.crv > -lim && m.crv < lim && m.cgv > -lim && m.cgv < lim &&
           m.cgu > -lim && m.cgu < lim && m.cbu > -lim && m.cbu < lim;
}
constexpr YuvMatrix YUV_BT601_LIMITED_MATRIX = {16, 1220542, 1673527, -852492, -409993, 2116026};
constexpr YuvMatrix YUV_BT601_FULL_MATRIX = {0, 1048576, 1470104, -748826, -360853, 1858077};
constexpr YuvMatrix YUV_BT709_LIMITED_MATRIX = {16, 1220945, 1879825, -558796, -223607, 2215014};
constexpr YuvMatrix YUV_BT709_FULL_MATRIX = {0, 1048576, 1651297, -490864, -196424, 1945738};
static_assert(yuv_matrix_fits24(YUV_BT601_LIMITED_MATRIX) && yuv_matrix_fits24(YUV_BT601_FULL_MATRIX) &&
                  yuv_matrix_fits24(YUV_BT709_LIMITED_MATRIX) && yuv_matrix_fits24(YUV_BT709_FULL_MATRIX),
              "a YUV coefficient does not fit the 24-bit multiply");
// the matrix of a descriptor's code (MELF_YUV_BT*); NULL: not a code (1 is never assigned)
inline const YuvMatrix* yuv_matrix(int code)
{
    static const YuvMatrix table[4] = {YUV_BT601_LIMITED_MATRIX, YUV_BT601_FULL_MATRIX, YUV_BT709_LIMITED_MATRIX,
                                       YUV_BT709_FULL_MATRIX};
    switch (code) {
    case MELF_YUV_BT601_LIMITED: return &table[0];
    case MELF_YUV_BT601_FULL: return &table[1];
    case MELF_YUV_BT709_LIMITED: return &table[2];
    case MELF_YUV_BT709_FULL: return &table[3];
    default: return nullptr;
    }
}
// Packed YUV 4:2:2 frames (melf_process_yuv422*): the launch's pix.  Two pixels per 4-byte macropixel; base, frame_stride and
// row_stride (bytes, all 4-byte aligned) describe the frames as for any packed layout, x0 and cols count pixels.  The formats
// differ in a byte permute only, which the kernels take as a runtime value (v_perm_b32 selector): macropixel -> Y0 U Y1 V.
constexpr int PIX_YUYV = 24, PIX_UYVY = 25, PIX_YVYU = 26;
inline bool pix_p422(int pix) { return pix >= PIX_YUYV && pix <= PIX_YVYU; }
inline uint32_t p422_sel(int pix) { return pix == PIX_UYVY ? 0x02030001u : (pix == PIX_YVYU ? 0x01020300u : 0x03020100u); }
// Planar frames (melf_process_planes*): the launch's pix.  Three planes of one byte per sample; base, frame_stride and row_stride
// (bytes, any alignment) describe a frame and the rows of each of its planes, PlanarPlanes where the planes start inside a frame
// (which gives the channel order), x0 and cols count pixels.  `readable` counts from base to the last sample of the last frame's
// last plane: no load may start before base or end behind base + readable.
constexpr int PIX_PLANAR = 32;
struct PlanarPlanes {
    int64_t b_off, g_off, r_off;  // bytes from a frame's first byte to the first sample of its B / G / R plane
};
// Planar and semi-planar YUV frames of any of the four chroma subsamplings (melf_process_yuv_planar*): the launch's pix.  The Y
// plane is described like a single-channel image (base, frame_stride, row_stride of MatchSrc / DialsSrc, any byte alignment), the
// chroma by YuvPlanarPlanes: U of pixel (x, y) at frame + u_off + (y >> sub_y) * c_pitch + (x >> sub_x) * c_step, V the same from
// v_off.  c_step 2: the two are the bytes of one interleaved pair (|u_off - v_off| == 1; which comes first is a runtime, wave-uniform
// matter).  A by-value kernel argument of its own: YuvPlanes and the kernels that take it stay as they are.  The hot kernels are
// instantiated per (sub_x, c_step) -- the four forms of the chroma fetch -- and take sub_y as the runtime shift of the chroma row.
constexpr int PIX_YUVP = 40;
struct YuvPlanarPlanes {
    int64_t u_off, v_off;  // bytes from a frame's first byte to its first U / V sample
    int c_pitch;           // bytes between chroma rows
    int sub_x, sub_y;      // log2 of the chroma subsampling, 0 or 1 each
    int c_step;            // bytes from one sample of a chroma plane to the next in its row: 1 planar, 2 semi-planar
};
// Planar and semi-planar YUV frames of 16-bit little-endian samples, chroma subsampled horizontally (melf_process_yuv16*): the
// launch's pix.  The Y plane is described by base, frame_stride and row_stride of MatchSrc / DialsSrc in BYTES (all 2-byte aligned),
// x0 and cols count pixels (samples); the chroma by Yuv16Planes: U of pixel (x, y) is the sample at byte frame + u_off + (y >> sub_y)
// * c_pitch + (x >> 1) * c_step * 2, V the same from v_off.  A sample s is read as min(s >> shift, 255) (melf_y16_addr.h: reduce),
// and from there on the arithmetic is that of PIX_YUVP.  A by-value kernel argument of its own; the hot kernels are instantiated
// per c_step and take sub_y, shift and the order of a pair's samples as runtime, wave-uniform values.
constexpr int PIX_YUV16 = 48;
struct Yuv16Planes {
    int64_t u_off, v_off;  // bytes from a frame's first byte to its first U / V sample
    int c_pitch;           // bytes between chroma rows
    int sub_y;             // log2 of the vertical chroma subsampling, 0 or 1
    int c_step;            // samples from one sample of a chroma plane to the next in its row: 1 planar, 2 semi-planar
    int shift;             // low bits dropped from a sample, 0 .. 8
};

// How the frames of one launch lie in memory, beside the base, the strides and the rectangle of MatchSrc / DialsSrc: the pixel
// layout and what goes with it.  Host side only: the launchers hand the kernels the members by value.  Made by the makers below
// and by nothing else, so that which member means something for which pix is settled where the value is made, not at every use.
struct FrameLayout {
    int pix;
    YuvPlanes yuv;         // pix_yuv(pix): the chroma planes
    PlanarPlanes planes;   // PIX_PLANAR: where the three planes start
    const YuvMatrix* mx;   // pix_yuv(pix), pix_p422(pix), PIX_YUVP, PIX_YUV16: the frames' colour conversion, never NULL there
    size_t extent;         // bytes a kernel may read of the LAST frame, from its first byte (the others: frame_stride)
    YuvPlanarPlanes yuvp;  // PIX_YUVP: the chroma planes and their subsampling (mx: the conversion, as above)
    Yuv16Planes y16;       // PIX_YUV16: the chroma planes of 16-bit samples and the reduction (mx: the conversion, as above)

    static FrameLayout packed(int pix /* MELF_PIX_* */, size_t extent) { return FrameLayout{pix, {}, {}, nullptr, extent}; }
    static FrameLayout yuv420(int pix /* PIX_NV12, PIX_I420 */, const YuvPlanes& yp, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{pix, yp, {}, &mx, extent};
    }
    static FrameLayout yuv422(int pix /* PIX_YUYV, PIX_UYVY, PIX_YVYU */, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{pix, {}, {}, &mx, extent};
    }
    static FrameLayout yuv_planar(const YuvPlanarPlanes& yp, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{PIX_YUVP, {}, {}, &mx, extent, yp};
    }
    static FrameLayout yuv16(const Yuv16Planes& yp, const YuvMatrix& mx, size_t extent)
    {
        return FrameLayout{PIX_YUV16, {}, {}, &mx, extent, {}, yp};
    }
    static FrameLayout planar(const PlanarPlanes& pl, size_t extent) { return FrameLayout{PIX_PLANAR, {}, pl, nullptr, extent}; }
    static FrameLayout plane(size_t extent) { return FrameLayout{PIX_PLANE, {}, {}, nullptr, extent}; }
};

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

// the same for packed YUV 4:2:2 (melf_yuv422_to_bgr): n frames at d_src (row_pitch, frame_stride), pix PIX_YUYV / _UYVY / _YVYU
void launch_p422_to_bgr(const uint8_t* d_src, int pix, int n, int H, int W, int row_pitch, size_t frame_stride, const YuvMatrix& mx,
                        uint8_t* d_dst, hipStream_t stream);

// ---- calibration stage kernels ------------------------------------------------
void launch_aligned_average(const uint8_t* d_frames, int n, size_t frame_stride, int row_stride, int x0, int y0, int rows,
                            int cols, const int32_t* d_mx, const int32_t* d_my, int ax, int ay, uint8_t* d_out,
                            hipStream_t stream);
void launch_inrange3(const uint8_t* d_img, int npx, const int lo[3], const int hi[3], uint8_t* d_out, hipStream_t stream);

// ---- k_jpeg.hip: baseline JPEG decode ----
struct JpegWorkspace;
int jpeg_probe(const uint8_t* data, size_t size, int* H, int* W, int* supported, std::string* why);
// Headers (and, when asked for, the Huffman decode data built from them) of n files, parsed file by file, from any thread (one
// thread per index): the file-name entry points parse a file right after reading it, on the thread that read it, and build its
// decode tables there too
struct JpegParsed;
JpegParsed* jpeg_parsed_new(int n, bool with_tables);
void jpeg_parsed_resize(JpegParsed* p, int n);   // room for n files; nothing is cleared (jpeg_parse_one resets its entry)
void jpeg_parse_one(JpegParsed* p, int i, const uint8_t* data, size_t size, int* H, int* W, int* supported);
void jpeg_parsed_free(JpegParsed* p);
// parsed: headers made earlier -- of file pidx[first + j] for the batch's file j (pidx NULL: of file first + j); host_status is
// then the caller's.  pin_base / pin_len: a pinned host buffer the files' bytes may already lie in (the file-name entry points
// read into one): a batch whose files all do is uploaded from there, no byte of it is copied on the host.
int jpeg_prepare_batch(JpegWorkspace** ws, const uint8_t* const* data, const size_t* sizes, int n, int H, int W,
                       int32_t* host_status, std::string* err, const JpegParsed* parsed = nullptr, int first = 0,
                       const int* pidx = nullptr, const uint8_t* pin_base = nullptr, size_t pin_len = 0);
int jpeg_launch_batch(JpegWorkspace* ws, int n, int H, int W, uint8_t* d_frames, int32_t* status_out_host,
                      hipStream_t stream, std::string* err, void (*timer)(void*, int, int), void* timer_arg,
                      const int* rect /* x0, y0, x1, y1: only this part of each frame is needed; NULL = all */);
int jpeg_upload_batch(JpegWorkspace* ws, int n, hipStream_t copy_stream, std::string* err);
int jpeg_decode_batch_kernels(JpegWorkspace* ws, int n, int H, int W, uint8_t* d_frames, hipStream_t stream, std::string* err,
                              void (*timer)(void*, int, int), void* timer_arg, const int* rect);
const int32_t* jpeg_device_status(const JpegWorkspace* ws);
void jpeg_workspace_free(JpegWorkspace* ws);

}  // namespace melf
