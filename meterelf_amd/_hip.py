"""ctypes binding of libmeterelf_hip.so (C ABI: include/meterelf_hip.h).

There is deliberately no CPU fallback: if the HIP library is missing or no
MI355X is visible, everything here raises.
"""
import ctypes as C
import os
import sys
from typing import NamedTuple, Optional

import numpy as np

# Streams overlap on the GPU only if they sit on different hardware queues; the HIP runtime spreads all of a process's
# streams over GPU_MAX_HW_QUEUES = 4 by default.  Eight keeps the context's two lanes (two caller streams) apart from each
# other and from the copy stream in practice.  Read when HIP initialises: harmless if that has already happened.
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MELF_LIB_PATH') or os.path.join(_PKG, 'libmeterelf_hip.so')  # override: A/B builds

MAX_DIALS = 8
ABI_VERSION = 3

FRAME_OK = 0
FRAME_DIALS_NOT_FOUND = 1
FRAME_NEEDLE_CONTOURS_NOT_FOUND = 2
FRAME_ANGLE_UNDETERMINED = 3

K_LPLANE, K_MATCH, K_DIALS, K_FUSED_MASK, K_HLS, K_JPEG_HUFF, K_JPEG_IDCT, K_JPEG_COLOR, K_STREAM_PROBE, K_GATHER, K_COUNT = range(11)
# MELF_LIST_* of include/meterelf_hip.h: the family of a frame list's descriptor, by the name MeterReader.read_frame_list gives it
LIST_FAMILIES = {'views': 0, 'yuv': 1, 'yuv422': 2, 'yuv_planar': 3, 'yuv16': 4, 'yuv422_10': 5, 'packed32': 6, 'planar': 7}
# MELF_ORIENT_* of include/meterelf_hip.h (the EXIF / TIFF tag 0x0112 values), by the name MeterReader.read_oriented_frames takes
ORIENTATIONS = {'normal': 1, 'mirror': 2, 'rot180': 3, 'flip': 4, 'transpose': 5, 'rot90cw': 6, 'transverse': 7, 'rot90ccw': 8}
JPEG_OK, JPEG_UNSUPPORTED, JPEG_CORRUPT, JPEG_SIZE_MISMATCH, JPEG_UNREADABLE = 0, 1, 2, 3, 4
FILES_IN_FLIGHT_MAX = 3   # MELF_FILES_IN_FLIGHT_MAX (include/meterelf_hip.h); tests compare with melf_jpeg_files_in_flight_max()


class MelfDial(C.Structure):
    _fields_ = [('cx', C.c_double), ('cy', C.c_double), ('angle_of_zero', C.c_double),
                ('range_h', C.c_int32), ('range_l', C.c_int32), ('range_s', C.c_int32),
                ('negative_momentum', C.c_int32), ('diameter', C.c_int32),
                ('dist_from_center', C.c_int32), ('circle_thickness', C.c_int32),
                ('reserved', C.c_int32)]


class MelfParams(C.Structure):
    _fields_ = [('abi_version', C.c_int32),
                ('rect_x0', C.c_int32), ('rect_y0', C.c_int32), ('rect_x1', C.c_int32), ('rect_y1', C.c_int32),
                ('th', C.c_int32), ('tw', C.c_int32), ('hue_shift', C.c_int32), ('ndials', C.c_int32),
                ('needle_lo', C.c_int32 * 3), ('needle_hi', C.c_int32 * 3),
                ('name_order', C.c_int32 * MAX_DIALS), ('reserved', C.c_int32),
                ('match_threshold', C.c_double),
                ('dial', MelfDial * MAX_DIALS)]


class MelfResult(C.Structure):
    _fields_ = [('status', C.c_int32), ('match_x', C.c_int32), ('match_y', C.c_int32),
                ('failed_dial', C.c_int32), ('unreadable_mask', C.c_uint32), ('match_val', C.c_float),
                ('pos', C.c_double * MAX_DIALS), ('angle', C.c_double * MAX_DIALS), ('value', C.c_double)]


class MelfMatchInfo(C.Structure):
    _fields_ = [('kernel', C.c_int32), ('n', C.c_int32), ('rows', C.c_int32), ('cols', C.c_int32), ('groups', C.c_int32),
                ('waves', C.c_int32), ('rows_per_wave', C.c_int32), ('full_waves', C.c_int32), ('pair_waves', C.c_int32),
                ('tiles', C.c_int32), ('reserved', C.c_int32 * 6)]


class MelfFrames(C.Structure):
    _fields_ = [('pixel_format', C.c_int32), ('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('row_pitch', C.c_int64), ('frame_stride', C.c_int64)]


# pixel layouts of melf_process_frames* (MELF_PIX_*); the 4th byte of BGRA / RGBA (BGRx / RGBx) is ignored
PIX_BGR, PIX_RGB, PIX_BGRA, PIX_RGBA = 0, 1, 2, 3
PIX_CODES = {'bgr': PIX_BGR, 'rgb': PIX_RGB, 'bgra': PIX_BGRA, 'rgba': PIX_RGBA, 'bgrx': PIX_BGRA, 'rgbx': PIX_RGBA}
PIX_BYTES = {PIX_BGR: 3, PIX_RGB: 3, PIX_BGRA: 4, PIX_RGBA: 4}



class MelfYuvFrames(C.Structure):
    _fields_ = [('format', C.c_int32), ('matrix', C.c_int32), ('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('reserved', C.c_int32), ('y_pitch', C.c_int64), ('c_pitch', C.c_int64), ('u_offset', C.c_int64),
                ('v_offset', C.c_int64), ('frame_stride', C.c_int64)]


# YUV 4:2:0 layouts of melf_process_yuv* (MELF_YUV_*); 'yv12' is I420 with the two chroma planes exchanged
YUV_NV12, YUV_I420 = 0, 1
# colour conversion of YUV frames, 4:2:0 and 4:2:2 alike (MELF_YUV_BT*, include/meterelf_hip.h has the coefficients); 1 is never
# assigned.
# Which sources produce which: 'bt709' (limited range) H.264 / HEVC of an HD camera as a hardware decoder leaves it in NV12;
# 'bt601-full' MJPEG webcams and phone cameras (JFIF: ffmpeg's yuvj420p / yuvj422p, raw UVC); 'bt709-full' screen and capture
# pipelines; 'bt601' (limited range) what cv2.cvtColor(COLOR_YUV2BGR_*) assumes, SD video.
YUV_BT601_LIMITED, YUV_BT601_FULL, YUV_BT709_LIMITED, YUV_BT709_FULL = 0, 2, 3, 4
YUV_MATRIX_CODES = {'bt601': YUV_BT601_LIMITED, 'bt601-full': YUV_BT601_FULL, 'bt709': YUV_BT709_LIMITED, 'bt709-full': YUV_BT709_FULL}
YUV_CODES = {'nv12': YUV_NV12, 'i420': YUV_I420, 'yv12': YUV_I420}


class MelfYuv422Frames(C.Structure):
    _fields_ = [('format', C.c_int32), ('matrix', C.c_int32), ('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('reserved', C.c_int32), ('row_pitch', C.c_int64), ('frame_stride', C.c_int64)]


# packed YUV 4:2:2 layouts of melf_process_yuv422* (MELF_YUV422_*): the bytes of a macropixel; 'yuy2' is YUYV's other name
YUV422_YUYV, YUV422_UYVY, YUV422_YVYU = 0, 1, 2
YUV422_CODES = {'yuyv': YUV422_YUYV, 'yuy2': YUV422_YUYV, 'uyvy': YUV422_UYVY, 'yvyu': YUV422_YVYU}



class MelfYuvPlanarFrames(C.Structure):
    _fields_ = [('matrix', C.c_int32), ('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('sub_x', C.c_int32),
                ('sub_y', C.c_int32), ('c_step', C.c_int32), ('reserved', C.c_int32), ('y_pitch', C.c_int64),
                ('c_pitch', C.c_int64), ('u_offset', C.c_int64), ('v_offset', C.c_int64), ('frame_stride', C.c_int64)]


# planar and semi-planar YUV layouts of melf_process_yuv_planar* by name: (sub_x, sub_y, c_step, V before U).  sub_x, sub_y: log2 of
# the chroma subsampling; c_step 1: U and V in planes of their own, 2: interleaved pairs in one plane.
YUV_PLANAR_FORMATS = {
    'i422': (1, 0, 1, False), 'yv16': (1, 0, 1, True), 'nv16': (1, 0, 2, False), 'nv61': (1, 0, 2, True),
    'i444': (0, 0, 1, False), 'yv24': (0, 0, 1, True), 'nv24': (0, 0, 2, False), 'nv42': (0, 0, 2, True),
    'i440': (0, 1, 1, False),
    'nv21': (1, 1, 2, True), 'nv12': (1, 1, 2, False), 'i420': (1, 1, 1, False), 'yv12': (1, 1, 1, True),
}


class MelfYuv16Frames(C.Structure):
    _fields_ = [('matrix', C.c_int32), ('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('sub_y', C.c_int32),
                ('c_step', C.c_int32), ('shift', C.c_int32), ('reserved', C.c_int32), ('y_pitch', C.c_int64),
                ('c_pitch', C.c_int64), ('u_offset', C.c_int64), ('v_offset', C.c_int64), ('frame_stride', C.c_int64)]


# planar and semi-planar YUV layouts of 16-bit little-endian samples (melf_process_yuv16*) by name: (sub_y, c_step, V before U,
# shift).  sub_y: log2 of the vertical chroma subsampling (the horizontal one is 2); c_step 1: U and V in planes of their own, 2:
# interleaved pairs in one plane; shift: the low bits dropped from a sample -- 8 where the value sits in the high bits (the P0xx /
# P2xx formats of hardware decoders) or fills the word, 16 - 8 - (16 - depth) = depth - 8 where it sits in the low bits.
YUV16_FORMATS = {
    'p010': (1, 2, False, 8), 'p012': (1, 2, False, 8), 'p016': (1, 2, False, 8),
    'p210': (0, 2, False, 8), 'p216': (0, 2, False, 8),
    'i010': (1, 1, False, 2), 'yuv420p10le': (1, 1, False, 2), 'i210': (0, 1, False, 2), 'yuv422p10le': (0, 1, False, 2),
    'i012': (1, 1, False, 4), 'yuv420p12le': (1, 1, False, 4), 'i212': (0, 1, False, 4), 'yuv422p12le': (0, 1, False, 4),
    'yuv420p16le': (1, 1, False, 8), 'yuv422p16le': (0, 1, False, 8),
}


class MelfYuv422_10Frames(C.Structure):
    _fields_ = [('format', C.c_int32), ('matrix', C.c_int32), ('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('reserved', C.c_int32), ('row_pitch', C.c_int64), ('frame_stride', C.c_int64)]


# packed 10-bit YUV 4:2:2 layouts of melf_process_yuv422_10* (MELF_YUV422_10_*) by name: 'v210', six pixels in a 16-byte group of
# four 32-bit words; 'y210' / 'y212' / 'y216', MSB-aligned 16-bit words Y0 U Y1 V, one format once the low bits are dropped
(YUV422_10_V210, YUV422_10_Y210) = (0, 1)
YUV422_10_FORMATS = {'v210': 0, 'y210': 1, 'y212': 1, 'y216': 1}


class MelfPacked32Frames(C.Structure):
    _fields_ = [('colour', C.c_int32), ('matrix', C.c_int32), ('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('pos', C.c_int32 * 3), ('row_pitch', C.c_int64), ('frame_stride', C.c_int64), ('reserved', C.c_int32),
                ('reserved2', C.c_int32)]


# 4:4:4 layouts of one little-endian 32-bit word per pixel (melf_process_packed32*) by name -> (colour, pos): colour MELF_P32_*,
# pos the low bit of the 8 bits read of Y, U, V (P32_YUV) or of R, G, B (P32_RGB); a 10-bit field at bit o is read from o + 2, byte b
# from 8 b.  The layouts are those of drm_fourcc.h and ffmpeg's pixfmt.h (include/meterelf_hip.h has the table):
#   'vuya' / 'vuyx'  bytes V U Y A in memory (Microsoft's and DRM's AYUV)     'ayuv'  bytes A Y U V (ffmpeg, GStreamer)
#   'uyva'           bytes U Y V A                                             'y410' / 'xv30'  U bits 0-9, Y 10-19, V 20-29
#   'v30x'           U bits 2-11, Y 12-21, V 22-31
#   'x2rgb10' / 'xrgb2101010'  B bits 0-9, G 10-19, R 20-29                   'x2bgr10' / 'xbgr2101010' / 'r10g10b10a2'  R in the low bits
(P32_YUV, P32_RGB) = (0, 1)
PACKED32_FORMATS = {
    'vuya': (P32_YUV, (16, 8, 0)), 'vuyx': (P32_YUV, (16, 8, 0)),
    'ayuv': (P32_YUV, (8, 16, 24)),
    'uyva': (P32_YUV, (8, 0, 16)),
    'y410': (P32_YUV, (12, 2, 22)), 'xv30': (P32_YUV, (12, 2, 22)),
    'v30x': (P32_YUV, (14, 4, 24)),
    'x2rgb10': (P32_RGB, (22, 12, 2)), 'xrgb2101010': (P32_RGB, (22, 12, 2)),
    'x2bgr10': (P32_RGB, (2, 12, 22)), 'xbgr2101010': (P32_RGB, (2, 12, 22)), 'r10g10b10a2': (P32_RGB, (2, 12, 22)),
}


class MelfPlanarFrames(C.Structure):
    _fields_ = [('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('reserved', C.c_int32), ('b_offset', C.c_int64),
                ('g_offset', C.c_int64), ('r_offset', C.c_int64), ('row_pitch', C.c_int64), ('frame_stride', C.c_int64)]


# plane orders of planar_frames_view: the planes present in an (N, C, H, W) array, in the array's order; 'a' / 'x' is never read
PLANAR_ORDERS = ('rgb', 'bgr', 'gbr', 'rgba', 'rgbx', 'bgra', 'bgrx')


class MelfWideFrames(C.Structure):
    _fields_ = [('sample_type', C.c_int32), ('layout', C.c_int32), ('pixel_format', C.c_int32), ('shift', C.c_int32),
                ('rounding', C.c_int32), ('reserved', C.c_int32), ('scale', C.c_float * 3), ('offset', C.c_float * 3),
                ('n', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('reserved2', C.c_int32), ('b_offset', C.c_int64),
                ('g_offset', C.c_int64), ('r_offset', C.c_int64), ('row_pitch', C.c_int64), ('frame_stride', C.c_int64)]


# RGB frames of wide samples (melf_process_wide*): MELF_WIDE_* by dtype name, the layouts, the roundings; channel orders of
# wide_frames_view by layout -- 'hwc': the samples of a pixel, 'chw': the planes present, in the array's order ('a' / 'x' is never read)
(WIDE_U16, WIDE_F16, WIDE_BF16, WIDE_F32) = (0, 1, 2, 3)
(WIDE_PACKED, WIDE_PLANAR) = (0, 1)
(ROUND_NEAREST, ROUND_FLOOR) = (0, 1)
WIDE_TYPES = {'uint16': WIDE_U16, 'int16': WIDE_U16, 'float16': WIDE_F16, 'bfloat16': WIDE_BF16, 'float32': WIDE_F32}
WIDE_SAMPLE_BYTES = {WIDE_U16: 2, WIDE_F16: 2, WIDE_BF16: 2, WIDE_F32: 4}
WIDE_ROUNDINGS = {'nearest': ROUND_NEAREST, 'floor': ROUND_FLOOR}
WIDE_PACKED_ORDERS = ('rgb', 'bgr', 'rgba', 'rgbx', 'bgra', 'bgrx')

MATCH_KERNEL_NAMES = ('dot4', 'mfma', 'gen')

RESULT_DTYPE = np.dtype([('status', '<i4'), ('match_x', '<i4'), ('match_y', '<i4'), ('failed_dial', '<i4'),
                         ('unreadable_mask', '<u4'), ('match_val', '<f4'),
                         ('pos', '<f8', (MAX_DIALS,)), ('angle', '<f8', (MAX_DIALS,)), ('value', '<f8')])
assert RESULT_DTYPE.itemsize == C.sizeof(MelfResult)


class HipError(RuntimeError):
    pass


# MELF_DIALS_* of include/meterelf_hip.h, by value: the dial reader's kernel families (melf_ctx_last_dials)
DIALS_FAMILIES = ('hls', 'bgr', 'packed3', 'packed4', 'nv12', 'i420', 'p422', 'yp_sub0_step1', 'yp_sub0_step2', 'yp_sub1_step1',
                  'yp_sub1_step2', 'planar')

# MELF_DIALS16_* of include/meterelf_hip.h, the families of the 16-bit frames: values 12, 13 of melf_ctx_last_dials' family.  A tuple
# of their own, as the header keeps them in an enum of their own: DIALS_FAMILIES is the twelve the instantiation tests enumerate.
DIALS16_FAMILIES = ('yuv16_step1', 'yuv16_step2')

# MELF_DIALS10_* in the same way, the families of the packed 10-bit 4:2:2 frames: values 14, 15
DIALS10_FAMILIES = ('v210', 'y210')

# MELF_DIALS32_* in the same way, the families of the 32-bit packed 4:4:4 frames: values 16, 17
DIALS32_FAMILIES = ('p32yuv', 'p32rgb')

# every symbol include/meterelf_hip.h declares for the product library; DIAG_EXPORTS: what its `#ifdef MELF_DIAG` part adds (the
# diagnostic build, make -C meterelf_amd/csrc diag, loaded through MELF_LIB_PATH)
DIAG_EXPORTS = ['melf_stream_probe_dev', 'melf_gather_frame_list_dev']
EXPORTS = [
    'melf_last_error', 'melf_abi_version', 'melf_device_count', 'melf_build_dial_masks',
    'melf_blob_size', 'melf_blob_pack', 'melf_blob_params', 'melf_ctx_create', 'melf_ctx_create_bcast', 'melf_ctx_destroy',
    'melf_ctx_params', 'melf_ctx_sync', 'melf_ctx_get_masks', 'melf_process_batch', 'melf_process_batch_dev', 'melf_process_stream_dev',
    'melf_process_frames', 'melf_process_frames_dev', 'melf_process_yuv', 'melf_process_yuv_dev', 'melf_yuv_to_bgr',
    'melf_process_yuv422', 'melf_process_yuv422_dev', 'melf_yuv422_to_bgr', 'melf_process_planes', 'melf_process_planes_dev',
    'melf_process_yuv_planar', 'melf_process_yuv_planar_dev', 'melf_yuv_planar_to_bgr',
    'melf_process_yuv16', 'melf_process_yuv16_dev', 'melf_yuv16_to_bgr',
    'melf_process_yuv422_10', 'melf_process_yuv422_10_dev', 'melf_yuv422_10_to_bgr',
    'melf_process_packed32', 'melf_process_packed32_dev', 'melf_packed32_to_bgr',
    'melf_process_frame_list', 'melf_process_frame_list_dev', 'melf_process_plane_list', 'melf_process_plane_list_dev',
    'melf_process_oriented', 'melf_process_oriented_dev', 'melf_orient_frames',
    'melf_process_wide', 'melf_process_wide_dev', 'melf_wide_to_bgr',
    'melf_process_wide_list', 'melf_process_wide_list_dev', 'melf_process_wide_plane_list', 'melf_process_wide_plane_list_dev',
    'melf_wide_list_to_bgr',
    'melf_bgr2hls', 'melf_hls_inrange_close', 'melf_hls_inrange_close_dev', 'melf_match_ccoeff',
    'melf_read_dials', 'melf_aligned_average', 'melf_inrange', 'melf_ctx_fused_table_ties', 'melf_ctx_fused_variant', 'melf_ctx_set_frames_resident', 'melf_ctx_last_match', 'melf_ctx_last_dials', 'melf_match_layout_query', 'melf_match_gen_plan_query', 'melf_ctx_set_profiling', 'melf_ctx_timings', 'melf_kernel_name',
    'melf_jpeg_probe', 'melf_jpeg_probe_batch', 'melf_jpeg_decode_batch', 'melf_jpeg_clean_segment', 'melf_jpeg_process_batch',
    'melf_jpeg_process_files', 'melf_jpeg_process_files_begin', 'melf_jpeg_process_files_end', 'melf_jpeg_files_in_flight_max', 'melf_ctx_files_stats', 'melf_files_open_probe',
    'melf_jpeg_probe_oriented', 'melf_jpeg_probe_oriented_batch', 'melf_ctx_set_jpeg_orientation', 'melf_ctx_get_jpeg_orientation',
    'melf_jpeg_probe_flags', 'melf_jpeg_probe_flags_batch', 'melf_ctx_set_jpeg_progressive', 'melf_ctx_get_jpeg_progressive',
    'melf_ctx_set_jpeg_samplings', 'melf_ctx_get_jpeg_samplings',
    'melf_ctx_set_jpeg_multiscan', 'melf_ctx_get_jpeg_multiscan', 'melf_ctx_set_jpeg_default_tables', 'melf_ctx_get_jpeg_default_tables',
    'melf_ctx_set_jpeg_truncated', 'melf_ctx_get_jpeg_truncated', 'melf_ctx_jpeg_truncated_files',
    'melf_ctx_set_jpeg_long_scans', 'melf_ctx_get_jpeg_long_scans',
]

_lib = None


def lib():
    """Loads the shared library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipError(
            'libmeterelf_hip.so is not built (run `python -c "import __graft_entry__ as g; g.build()"` '
            'or `make -C meterelf_amd/csrc`); meterelf_amd has no CPU fallback')
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.melf_last_error.restype = C.c_char_p
    L.melf_kernel_name.restype = C.c_char_p
    L.melf_kernel_name.argtypes = [C.c_int]
    L.melf_device_count.argtypes = [C.POINTER(C.c_int)]
    L.melf_build_dial_masks.argtypes = [C.POINTER(MelfParams), vp]
    L.melf_blob_size.restype = C.c_size_t
    L.melf_blob_size.argtypes = [C.POINTER(MelfParams)]
    L.melf_blob_pack.argtypes = [C.POINTER(MelfParams), vp, vp, C.c_size_t]
    L.melf_blob_params.argtypes = [vp, C.c_size_t, C.POINTER(MelfParams)]
    L.melf_ctx_create.argtypes = [C.c_int, vp, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.melf_ctx_create_bcast.argtypes = [C.POINTER(C.c_int), C.c_int, vp, C.c_size_t, C.POINTER(vp)]
    L.melf_ctx_destroy.argtypes = [vp]
    L.melf_ctx_destroy.restype = None
    L.melf_ctx_params.argtypes = [vp, C.POINTER(MelfParams)]
    L.melf_ctx_get_masks.argtypes = [vp, vp]
    L.melf_ctx_sync.argtypes = [vp]
    L.melf_process_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, vp]
    L.melf_process_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, vp]
    L.melf_process_frames.argtypes = [vp, vp, C.POINTER(MelfFrames), vp]
    L.melf_process_frames_dev.argtypes = [vp, vp, C.POINTER(MelfFrames), vp, vp, vp]
    L.melf_process_yuv.argtypes = [vp, vp, C.POINTER(MelfYuvFrames), vp]
    L.melf_process_yuv_dev.argtypes = [vp, vp, C.POINTER(MelfYuvFrames), vp, vp, vp]
    L.melf_yuv_to_bgr.argtypes = [vp, vp, C.POINTER(MelfYuvFrames), vp]
    L.melf_process_yuv422.argtypes = [vp, vp, C.POINTER(MelfYuv422Frames), vp]
    L.melf_process_yuv422_dev.argtypes = [vp, vp, C.POINTER(MelfYuv422Frames), vp, vp, vp]
    L.melf_yuv422_to_bgr.argtypes = [vp, vp, C.POINTER(MelfYuv422Frames), vp]
    L.melf_process_yuv_planar.argtypes = [vp, vp, C.POINTER(MelfYuvPlanarFrames), vp]
    L.melf_process_yuv_planar_dev.argtypes = [vp, vp, C.POINTER(MelfYuvPlanarFrames), vp, vp, vp]
    L.melf_yuv_planar_to_bgr.argtypes = [vp, vp, C.POINTER(MelfYuvPlanarFrames), vp]
    L.melf_process_yuv16.argtypes = [vp, vp, C.POINTER(MelfYuv16Frames), vp]
    L.melf_process_yuv16_dev.argtypes = [vp, vp, C.POINTER(MelfYuv16Frames), vp, vp, vp]
    L.melf_yuv16_to_bgr.argtypes = [vp, vp, C.POINTER(MelfYuv16Frames), vp]
    L.melf_process_yuv422_10.argtypes = [vp, vp, C.POINTER(MelfYuv422_10Frames), vp]
    L.melf_process_yuv422_10_dev.argtypes = [vp, vp, C.POINTER(MelfYuv422_10Frames), vp, vp, vp]
    L.melf_yuv422_10_to_bgr.argtypes = [vp, vp, C.POINTER(MelfYuv422_10Frames), vp]
    L.melf_process_packed32.argtypes = [vp, vp, C.POINTER(MelfPacked32Frames), vp]
    L.melf_process_packed32_dev.argtypes = [vp, vp, C.POINTER(MelfPacked32Frames), vp, vp, vp]
    L.melf_packed32_to_bgr.argtypes = [vp, vp, C.POINTER(MelfPacked32Frames), vp]
    L.melf_process_planes.argtypes = [vp, vp, C.POINTER(MelfPlanarFrames), vp]
    L.melf_process_planes_dev.argtypes = [vp, vp, C.POINTER(MelfPlanarFrames), vp, vp, vp]
    L.melf_process_wide.argtypes = [vp, vp, C.POINTER(MelfWideFrames), vp]
    L.melf_process_wide_dev.argtypes = [vp, vp, C.POINTER(MelfWideFrames), vp, vp, vp]
    L.melf_wide_to_bgr.argtypes = [vp, vp, C.POINTER(MelfWideFrames), vp]
    if hasattr(L, 'melf_process_wide_list'):   # (tools/wide_rate.py loads the library from before the wide lists through MELF_LIB_PATH)
        L.melf_process_wide_list.argtypes = [vp, C.POINTER(MelfWideFrames), vp, vp]
        L.melf_process_wide_list_dev.argtypes = [vp, C.POINTER(MelfWideFrames), vp, vp, vp, vp]
        L.melf_process_wide_plane_list.argtypes = [vp, C.POINTER(MelfWideFrames), vp, C.c_int, vp]
        L.melf_process_wide_plane_list_dev.argtypes = [vp, C.POINTER(MelfWideFrames), vp, C.c_int, vp, vp, vp]
        L.melf_wide_list_to_bgr.argtypes = [vp, C.POINTER(MelfWideFrames), vp, C.c_int, vp]
    L.melf_process_frame_list.argtypes = [vp, C.c_int, vp, vp, vp]
    L.melf_process_frame_list_dev.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.melf_process_plane_list.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
    L.melf_process_plane_list_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    L.melf_process_oriented.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    L.melf_process_oriented_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.melf_orient_frames.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, C.c_size_t]
    if hasattr(L, 'melf_gather_frame_list_dev'):   # the diagnostic build only
        L.melf_gather_frame_list_dev.argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(C.c_size_t)]
    L.melf_process_stream_dev.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, vp]
    L.melf_bgr2hls.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp]
    L.melf_hls_inrange_close.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.melf_hls_inrange_close_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    if hasattr(L, 'melf_stream_probe_dev'):   # the diagnostic build only
        L.melf_stream_probe_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, vp]
    L.melf_match_ccoeff.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.melf_read_dials.argtypes = [vp, vp, C.c_int, vp]
    L.melf_aligned_average.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_int, C.c_int, vp]
    L.melf_inrange.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.melf_ctx_fused_table_ties.argtypes = [vp, C.POINTER(C.c_int)]
    L.melf_ctx_fused_variant.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.melf_ctx_set_profiling.argtypes = [vp, C.c_int]
    L.melf_ctx_last_match.argtypes = [vp, C.POINTER(MelfMatchInfo)]
    L.melf_ctx_last_dials.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.melf_match_layout_query.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MelfMatchInfo)]
    L.melf_match_gen_plan_query.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MelfMatchInfo), vp, C.c_int,
                                            C.POINTER(C.c_int32)]
    L.melf_ctx_set_frames_resident.argtypes = [vp, C.c_int]
    L.melf_ctx_timings.argtypes = [vp, vp, vp]
    i32p = C.POINTER(C.c_int32)
    L.melf_jpeg_probe.argtypes = [vp, C.c_size_t, i32p, i32p, i32p]
    L.melf_jpeg_probe_batch.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.melf_jpeg_probe_oriented.argtypes = [vp, C.c_size_t, i32p, i32p, i32p, i32p]
    L.melf_jpeg_probe_oriented_batch.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.melf_jpeg_probe_flags.argtypes = [vp, C.c_size_t, C.c_int, i32p, i32p, i32p, i32p]
    L.melf_jpeg_probe_flags_batch.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    for (name, _flag, _doc) in JPEG_SWITCHES:
        if name != 'jpeg_long_scans' and hasattr(L, 'melf_ctx_set_' + name):   # (tools/jpeg_cut_rate.py loads the library from before melf_ctx_set_jpeg_truncated through MELF_LIB_PATH)
            getattr(L, 'melf_ctx_set_' + name).argtypes = [vp, C.c_int]
            getattr(L, 'melf_ctx_get_' + name).argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, 'melf_ctx_set_jpeg_long_scans'):   # (the one switch with a second argument: the chapter length)
        L.melf_ctx_set_jpeg_long_scans.argtypes = [vp, C.c_int, C.c_int]
        L.melf_ctx_get_jpeg_long_scans.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, 'melf_ctx_set_jpeg_truncated'):
        L.melf_ctx_jpeg_truncated_files.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    L.melf_jpeg_decode_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]
    L.melf_jpeg_process_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.melf_jpeg_process_files.argtypes = [vp, vp, C.c_int, i32p, i32p, vp, vp]
    L.melf_jpeg_process_files_begin.argtypes = [vp, vp, C.c_int, i32p, i32p, vp, vp]
    L.melf_jpeg_process_files_end.argtypes = [vp]
    L.melf_jpeg_files_in_flight_max.argtypes = []
    L.melf_ctx_files_stats.argtypes = [vp, vp, C.c_int]
    L.melf_files_open_probe.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    if L.melf_abi_version() != ABI_VERSION:
        raise HipError('libmeterelf_hip.so ABI version mismatch')
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise HipError('libmeterelf_hip: %s (code %d)' % (lib().melf_last_error().decode(), rc))


def device_count():
    n = C.c_int(0)
    rc = lib().melf_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class FramesView(NamedTuple):
    """How the kernels read a batch of frames in place (frames_view)."""
    ptr: int            # address of frame 0, row 0, pixel 0
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]   # that GPU's index (None for host memory)
    pixel_format: int   # PIX_*
    n: int
    H: int
    W: int
    row_pitch: int      # bytes between rows
    frame_stride: int   # bytes between frames
    extent: int         # bytes read from ptr: (n - 1) * frame_stride + (H - 1) * row_pitch + W * bytes per pixel
    copied: bool        # the layout could not be described and the frames were copied once to a packed array
    array: object       # what ptr points into (the caller's array, or the copy): keep it alive while the call runs


def _is_torch(x):
    return type(x).__module__.split('.')[0] == 'torch'


def _owner_span(a, is_torch):
    """(start, end) of the memory that `a`'s storage owns: the bytes a view may read beyond its own elements."""
    if is_torch:
        st = a.untyped_storage()
        return st.data_ptr(), st.data_ptr() + st.nbytes()
    root = a
    while isinstance(root.base, np.ndarray):
        root = root.base
    lo = hi = root.ctypes.data
    for (k, st) in zip(root.shape, root.strides):
        if k == 0:
            return lo, lo
        if st < 0:
            lo += (k - 1) * st
        else:
            hi += (k - 1) * st
    return lo, hi + root.itemsize


def _unwrap(frames):
    """(frames, is_torch, shape, strides, ptr, on_device, device) of a uint8 torch tensor or of what np.asarray makes of anything
    else; strides in bytes, device: the GPU's index of a tensor on one.  Not uint8: ValueError."""
    if _is_torch(frames):
        if str(frames.dtype) != 'torch.uint8':
            raise ValueError('frames must be uint8, not %s' % frames.dtype)
        on_device = frames.device.type == 'cuda'
        return (frames, True, tuple(frames.shape), tuple(frames.stride()),          # elements = bytes for uint8
                frames.data_ptr(), on_device, frames.device.index if on_device else None)
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        raise ValueError('frames must be uint8, not %s' % frames.dtype)
    return (frames, False, frames.shape, frames.strides, frames.ctypes.data, False, None)


def _packed_copy(frames, is_torch):
    """(copy, its address): the frames copied once to a packed array -- a fresh allocation (aligned) even where they are contiguous
    already."""
    if is_torch:
        import torch
        frames = frames.clone(memory_format=torch.contiguous_format)
        return frames, frames.data_ptr()
    frames = np.array(frames, order='C', copy=True)
    return frames, frames.ctypes.data


def frames_view(frames, pixel_format='bgr'):
    """Describes an (N, H, W, C) uint8 numpy array or torch tensor as melf_process_frames* read it -- the one place that maps an
    array's layout to pointer, pixel format, row pitch and frame stride.  pixel_format: the order of the array's channels,
    'bgr' / 'rgb' for C = 3, 'bgra' / 'rgba' (or 'bgrx' / 'rgbx') for C = 4.  A 3-channel view whose pixels are 4 bytes apart
    (rgba[..., :3]) is read as the 4-byte format of the same order; padded rows and frames (frames[:, :, :w], frames[::2]) are
    read in place.  A layout the kernels cannot read -- a channel stride other than 1, negative or odd strides, a misaligned
    4-byte layout -- is copied once to a packed array (FramesView.copied).  Not uint8, or C not 3 / 4: ValueError."""
    (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap(frames)
    if len(shape) != 4 or shape[3] not in (3, 4):
        raise ValueError('frames must be (N, H, W, 3) or (N, H, W, 4), not %s' % (shape,))
    fmt = str(pixel_format).lower()
    if fmt not in PIX_CODES or (shape[3] == 3) != (PIX_BYTES[PIX_CODES[fmt]] == 3):
        raise ValueError('pixel_format %r does not name the %d channels of the frames' % (pixel_format, shape[3]))
    code = PIX_CODES[fmt]
    (n, H, W, ch) = shape
    (fs, rp, ps, cs) = strides
    if ch == 3 and ps == 4 and cs == 1:
        code = PIX_BGRA if code == PIX_BGR else PIX_RGBA   # a 3-channel view of 4-byte pixels: read the 4-byte format
    bpp = PIX_BYTES[code]
    # strides of dimensions of size 1 are never stepped over: make them what a packed array has
    if W == 1:
        ps = bpp
    if H == 1:
        rp = W * bpp
    if n == 1:
        fs = (H - 1) * rp + W * bpp
    extent = (n - 1) * fs + (H - 1) * rp + W * bpp if n else 0
    ok = (cs == 1 and ps == bpp and rp >= W * bpp and fs >= (H - 1) * rp + W * bpp and rp <= 2 ** 31 - 1)
    if ok and bpp == 4:
        ok = (ptr | rp | fs) % 4 == 0
    if ok and n and bpp == 4 and ch == 3:
        # the ignored 4th byte of the last pixel lies behind the view's own bytes: it must belong to the same memory
        (lo, hi) = _owner_span(frames, is_torch)
        ok = lo <= ptr and ptr + extent <= hi
    if not ok:
        (frames, ptr) = _packed_copy(frames, is_torch)   # also where the array is contiguous already (a misaligned 4-byte layout)
        code = PIX_CODES[fmt]
        bpp = PIX_BYTES[code]
        (rp, fs) = (W * bpp, H * W * bpp)
        extent = n * fs
    return FramesView(int(ptr), on_device, device, code, n, H, W, int(rp), int(fs), int(extent), not ok, frames)


def yuv_matrix_code(matrix):
    """The MELF_YUV_BT* code of a matrix given by name (YUV_MATRIX_CODES) or by code; anything else: ValueError."""
    if isinstance(matrix, str):
        code = YUV_MATRIX_CODES.get(matrix.lower())
    else:
        try:
            code = int(matrix) if int(matrix) == matrix and int(matrix) in YUV_MATRIX_CODES.values() else None
        except (TypeError, ValueError):
            code = None
    if code is None:
        raise ValueError('matrix %r is not a YUV matrix (%s, or a code out of %s)'
                         % (matrix, ', '.join(YUV_MATRIX_CODES), sorted(YUV_MATRIX_CODES.values())))
    return code


class YuvFramesView(NamedTuple):
    """How the kernels read a batch of YUV 4:2:0 frames in place (yuv_frames_view)."""
    ptr: int            # address of frame 0's first Y sample
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    format: int         # YUV_NV12 / YUV_I420
    n: int
    H: int
    W: int
    y_pitch: int        # bytes between Y rows
    c_pitch: int        # bytes between chroma rows
    u_offset: int       # bytes from a frame's first byte to its U / V samples
    v_offset: int
    frame_stride: int   # bytes between frames
    extent: int         # bytes read from ptr: every plane of every frame up to the last sample of its last row
    copied: bool        # the layout could not be described and the frames were copied once to a packed array
    array: object       # what ptr points into (the caller's array, or the copy): keep it alive while the call runs
    matrix: int = YUV_BT601_LIMITED   # YUV_BT* code of the colour conversion

    def descriptor(self):
        return MelfYuvFrames(self.format, self.matrix, self.n, self.H, self.W, 0, self.y_pitch, self.c_pitch, self.u_offset,
                             self.v_offset, self.frame_stride)


def yuv_frames_view(frames, pixel_format='nv12', matrix='bt601'):
    """Describes the conventional (N, H * 3 // 2, W) uint8 array of YUV 4:2:0 frames (numpy array or torch tensor) as
    melf_process_yuv* read it: rows 0 .. H - 1 are Y; 'nv12': rows H .. H * 3 // 2 - 1 are the interleaved U V rows; 'i420': the
    H * W // 4 bytes behind the Y rows are the U plane (rows of W // 2), the next H * W // 4 the V plane; 'yv12': V first.
    'nv12' honours the row stride and the frame stride in place (frames[:, :, :w], frames[::2], frames[a:b]); the planar formats
    are read in place when the rows are contiguous (row stride == W: their chroma rows are half rows of the array), otherwise the
    frames are copied once to a packed array (YuvFramesView.copied), as is any layout with an element stride other than 1 or
    negative strides.  matrix: the frames' colour conversion, a name of YUV_MATRIX_CODES or a YUV_BT* code: 'bt601' (limited range,
    cv2's convention), 'bt709' (H.264 / HEVC of an HD camera out of a hardware decoder), 'bt601-full' (MJPEG webcams and phone
    cameras: ffmpeg's yuvj420p, raw UVC), 'bt709-full' (screen and capture pipelines).  Not uint8, not three-dimensional, an odd H
    or W, an unknown format or an unknown matrix: ValueError."""
    mcode = yuv_matrix_code(matrix)
    (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap(frames)
    fmt = str(pixel_format).lower()
    if fmt not in YUV_CODES:
        raise ValueError('pixel_format %r is not a YUV 4:2:0 layout (nv12, i420, yv12)' % (pixel_format,))
    if len(shape) != 3 or shape[1] % 3 != 0 or (shape[1] // 3 * 2) % 2 != 0 or shape[1] == 0 or shape[2] == 0 or shape[2] % 2 != 0:
        raise ValueError('YUV 4:2:0 frames must be (N, H * 3 // 2, W) with even H and W, not %s' % (shape,))
    code = YUV_CODES[fmt]
    (n, rows, W) = shape
    H = rows // 3 * 2
    (fs, rp, es) = strides
    if n == 1:
        fs = rows * rp if rp > 0 else 0
    planar = code == YUV_I420
    ok = es == 1 and rp >= W and fs >= (rows - 1) * rp + W and rp <= 2 ** 31 - 1 and (not planar or rp == W)
    if not ok:
        (frames, ptr) = _packed_copy(frames, is_torch)
        (rp, fs) = (W, rows * W)
    if planar:
        (c_pitch, first, second) = (W // 2, H * W, H * W + (H // 2) * (W // 2))
        (u_off, v_off) = (second, first) if fmt == 'yv12' else (first, second)
        last = second + (H // 2) * (W // 2)
    else:
        (c_pitch, u_off, v_off) = (rp, H * rp, H * rp + 1)
        last = (rows - 1) * rp + W
    extent = (n - 1) * fs + last if n else 0
    return YuvFramesView(int(ptr), on_device, device, code, n, H, W, int(rp), int(c_pitch), int(u_off), int(v_off), int(fs), int(extent),
                         not ok, frames, mcode)


class Yuv422FramesView(NamedTuple):
    """How the kernels read a batch of packed YUV 4:2:2 frames in place (yuv422_frames_view)."""
    ptr: int            # address of frame 0's first macropixel
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    format: int         # YUV422_YUYV / YUV422_UYVY / YUV422_YVYU
    n: int
    H: int
    W: int
    row_pitch: int      # bytes between rows
    frame_stride: int   # bytes between frames
    extent: int         # bytes read from ptr: (n - 1) * frame_stride + (H - 1) * row_pitch + 2 * W
    copied: bool        # the layout could not be described and the frames were copied once to a packed array
    array: object       # what ptr points into (the caller's array, or the copy): keep it alive while the call runs
    matrix: int = YUV_BT601_LIMITED   # YUV_BT* code of the colour conversion

    def descriptor(self):
        return MelfYuv422Frames(self.format, self.matrix, self.n, self.H, self.W, 0, self.row_pitch, self.frame_stride)


def yuv422_frames_view(frames, pixel_format='yuyv', matrix='bt601'):
    """Describes the conventional (N, H, W, 2) uint8 array of packed YUV 4:2:2 frames (numpy array or torch tensor) as
    melf_process_yuv422* read it: the two bytes of pixel x are bytes 2 x, 2 x + 1 of its row, 'yuyv' (or 'yuy2'): Y0 U Y1 V per
    pair of pixels, 'uyvy': U Y0 V Y1, 'yvyu': Y0 V Y1 U.  The row stride and the frame stride are honoured in place
    (frames[:, :, :w], frames[::2], frames[a:b]).  A layout the descriptor cannot express -- an element or pixel stride other
    than 1 / 2, a base, row stride or frame stride that is not a multiple of 4, negative strides -- is copied once to a packed
    array (Yuv422FramesView.copied).  matrix: the frames' colour conversion as for yuv_frames_view, a name of YUV_MATRIX_CODES or a
    YUV_BT* code (raw UVC webcams deliver 'bt601-full', HD capture cards 'bt709').  Not uint8, not four-dimensional, a last dimension
    other than 2, an odd or zero W, a zero H, an unknown format name or an unknown matrix: ValueError."""
    mcode = yuv_matrix_code(matrix)
    (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap(frames)
    fmt = str(pixel_format).lower()
    if fmt not in YUV422_CODES:
        raise ValueError('pixel_format %r is not a packed YUV 4:2:2 layout (yuyv / yuy2, uyvy, yvyu)' % (pixel_format,))
    if len(shape) != 4 or shape[3] != 2 or shape[1] == 0 or shape[2] == 0 or shape[2] % 2 != 0:
        raise ValueError('packed YUV 4:2:2 frames must be (N, H, W, 2) with an even W, not %s' % (shape,))
    code = YUV422_CODES[fmt]
    (n, H, W, _two) = shape
    (fs, rp, ps, es) = strides
    # strides of dimensions of size 1 are never stepped over: make them what a packed array has
    if H == 1:
        rp = W * 2
    if n == 1:
        fs = (H - 1) * rp + W * 2 if rp > 0 else 0
        fs += -fs % 4
    ok = (es == 1 and ps == 2 and rp >= W * 2 and fs >= (H - 1) * rp + W * 2 and rp <= 2 ** 31 - 1 and (ptr | rp | fs) % 4 == 0)
    if not ok:
        (frames, ptr) = _packed_copy(frames, is_torch)   # also where the array is contiguous already (a misaligned base)
        (rp, fs) = (W * 2, H * W * 2)
    extent = (n - 1) * fs + (H - 1) * rp + W * 2 if n else 0
    return Yuv422FramesView(int(ptr), on_device, device, code, n, H, W, int(rp), int(fs), int(extent), not ok, frames, mcode)


class YuvPlanarFramesView(NamedTuple):
    """How the kernels read a batch of planar / semi-planar YUV frames in place (yuv_planar_frames_view)."""
    ptr: int            # address of frame 0's first Y sample
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    n: int
    H: int
    W: int
    sub_x: int          # log2 of the chroma subsampling
    sub_y: int
    c_step: int         # bytes between the samples of a chroma plane: 1 planar, 2 semi-planar
    y_pitch: int        # bytes between Y rows
    c_pitch: int        # bytes between chroma rows
    u_offset: int       # bytes from a frame's first byte to its first U / V sample
    v_offset: int
    frame_stride: int   # bytes between frames
    extent: int         # bytes read from ptr: every plane of every frame up to the last sample of its last row
    copied: bool        # the layout could not be described and the frames were copied once to a packed array
    array: object       # what ptr points into (the caller's array, or the copy): keep it alive while the call runs
    matrix: int = YUV_BT601_LIMITED   # YUV_BT* code of the colour conversion

    def descriptor(self):
        return MelfYuvPlanarFrames(self.matrix, self.n, self.H, self.W, self.sub_x, self.sub_y, self.c_step, 0, self.y_pitch,
                                   self.c_pitch, self.u_offset, self.v_offset, self.frame_stride)


def _yuv_rows_layout(frames, is_torch, shape, strides, ptr, bps, sx, sy, step, vfirst, fmt, even_words):
    """Rows of a raw-video (N, rows, W) array of bps-byte samples -> the planar YUV descriptor's numbers (yuv_planar_frames_view: bps 1;
    yuv16_frames_view: bps 2, sx 1).  strides in bytes; step in samples.  Returns (frames, ptr, n, H, W, y_pitch, c_pitch, u_offset,
    v_offset, frame_stride, extent, copied), frames and ptr those of the packed copy where the layout could not be described in place.
    A shape that is not the format's: ValueError."""
    blocks = (1 << sx) * (1 << sy)                    # pixels per chroma sample: rows = H * (blocks + 2) / blocks
    bad = len(shape) != 3 or shape[1] == 0 or shape[2] == 0 or (shape[1] * blocks) % (blocks + 2) != 0
    if not bad:
        (n, rows, W) = shape
        H = rows * blocks // (blocks + 2)
        bad = (sx and W % 2) or (sy and H % 2)
    if bad:
        raise ValueError('%s frames must be (N, H * %d // %d, W)%s, not %s' % (fmt, blocks + 2, blocks, even_words, shape))
    (fs, rp, es) = strides
    (row, cw, ch) = (W * bps, (W >> sx) * step * bps, H >> sy)   # bytes of a Y row, of a chroma row (semi-planar: of both), chroma rows
    if W == 1:
        es = bps
    if n == 1:
        fs = rows * rp if rp > 0 else 0
    whole_rows = cw == row                            # a chroma row is one row of the array: padded rows can be described
    whole_samples = rp % bps == 0 and fs % bps == 0 and ptr % bps == 0   # odd byte strides or an odd base cannot be described
    ok = es == bps and whole_samples and row <= rp <= 2 ** 31 - 1 and fs >= (rows - 1) * rp + row and (whole_rows or rp == row)
    if not ok:
        (frames, ptr) = _packed_copy(frames, is_torch)
        (rp, fs) = (row, rows * row)
    c_pitch = rp if whole_rows else cw
    first = H * rp
    if step == 2:
        (u_off, v_off) = (first + bps, first) if vfirst else (first, first + bps)
        last = first + (ch - 1) * c_pitch + cw
    else:
        second = first + ch * c_pitch
        (u_off, v_off) = (second, first) if vfirst else (first, second)
        last = second + (ch - 1) * c_pitch + cw
    extent = (n - 1) * fs + last if n else 0
    return (frames, int(ptr), n, H, W, int(rp), int(c_pitch), int(u_off), int(v_off), int(fs), int(extent), not ok)


def yuv_planar_frames_view(frames, pixel_format='i422', matrix='bt601'):
    """Describes the raw-video (N, rows, W) uint8 array of planar / semi-planar YUV frames (numpy array or torch tensor) as
    melf_process_yuv_planar* read it.  pixel_format, a name of YUV_PLANAR_FORMATS: 4:2:2 'i422' (yuv422p / yuvj422p), 'yv16', 'nv16',
    'nv61' (rows = 2 H); 4:4:4 'i444' (yuv444p / yuvj444p), 'yv24', 'nv24', 'nv42' (rows = 3 H); 4:4:0 'i440' (rows = 2 H); 4:2:0
    'nv21', 'nv12', 'i420', 'yv12' (rows = 3 H / 2).  Rows 0 .. H - 1 are Y; behind them the U plane and then the V plane ('yv..': V
    first), H >> sub_y rows of W >> sub_x bytes each, or one plane of interleaved U V pairs ('nv16', 'nv24', 'nv12'; V U: 'nv61',
    'nv42', 'nv21').  For 'i444' / 'yv24' an (N, 3, H, W) array is taken as well (planes Y U V / Y V U).  The frame stride is
    honoured in place (frames[::2], frames[a:b]); a row-padded view (frames[:, :, :w]) where a chroma row is one row of the array:
    the semi-planar 4:2:x formats, 'i440', and 'i444' / 'yv24' in either shape.  Anything else -- padded rows of a layout whose chroma
    rows are half or double rows of the array, an element stride other than 1, negative strides -- is copied once to a packed array
    (YuvPlanarFramesView.copied).  matrix as for yuv_frames_view.  Not uint8, a shape that is not that of the format, an odd W (H)
    where the chroma is subsampled horizontally (vertically), an unknown format or an unknown matrix: ValueError."""
    mcode = yuv_matrix_code(matrix)
    (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap(frames)
    fmt = str(pixel_format).lower()
    if fmt not in YUV_PLANAR_FORMATS:
        raise ValueError('pixel_format %r is not a planar / semi-planar YUV layout (%s)' % (pixel_format, ', '.join(YUV_PLANAR_FORMATS)))
    (sx, sy, step, vfirst) = YUV_PLANAR_FORMATS[fmt]
    if len(shape) == 4 and (sx, sy, step) == (0, 0, 1):
        # (N, 3, H, W): three whole planes, Y first
        if shape[1] != 3 or shape[2] == 0 or shape[3] == 0:
            raise ValueError('planar 4:4:4 frames must be (N, 3 * H, W) or (N, 3, H, W), not %s' % (shape,))
        (n, _c, H, W) = shape
        (fs, ps, rp, es) = strides
        if W == 1:
            es = 1
        if H == 1:
            rp = W
        span = (H - 1) * rp + W
        if n == 1:
            fs = 2 * ps + span if ps >= 0 else 0
        ok = es == 1 and W <= rp <= 2 ** 31 - 1 and ps >= span and fs >= 2 * ps + span
        if not ok:
            (frames, ptr) = _packed_copy(frames, is_torch)
            (rp, ps, fs) = (W, H * W, 3 * H * W)
            span = H * W
        (first, second) = (ps, 2 * ps)
        (u_off, v_off) = (second, first) if vfirst else (first, second)
        extent = (n - 1) * fs + 2 * ps + span if n else 0
        return YuvPlanarFramesView(int(ptr), on_device, device, n, H, W, 0, 0, 1, int(rp), int(rp), int(u_off), int(v_off), int(fs),
                                   int(extent), not ok, frames, mcode)
    (frames, ptr, n, H, W, rp, c_pitch, u_off, v_off, fs, extent, copied) = _yuv_rows_layout(
        frames, is_torch, shape, strides, ptr, 1, sx, sy, step, vfirst, fmt, ' with an even W' * sx + ' with an even H' * sy)
    return YuvPlanarFramesView(ptr, on_device, device, n, H, W, sx, sy, step, rp, c_pitch, u_off, v_off, fs, extent, copied, frames, mcode)


class Yuv16FramesView(NamedTuple):
    """How the kernels read a batch of 16-bit planar / semi-planar YUV frames in place (yuv16_frames_view)."""
    ptr: int            # address of frame 0's first Y sample
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    n: int
    H: int
    W: int
    sub_y: int          # log2 of the vertical chroma subsampling
    c_step: int         # SAMPLES between the samples of a chroma plane: 1 planar, 2 semi-planar
    shift: int          # low bits dropped from a sample
    y_pitch: int        # BYTES between Y rows
    c_pitch: int        # BYTES between chroma rows
    u_offset: int       # BYTES from a frame's first byte to its first U / V sample
    v_offset: int
    frame_stride: int   # BYTES between frames
    extent: int         # bytes read from ptr: every plane of every frame up to the last sample of its last row
    copied: bool        # the layout could not be described and the frames were copied once to a packed array
    array: object       # what ptr points into (the caller's array, or the copy): keep it alive while the call runs
    matrix: int         # YUV_BT* code of the colour conversion

    def descriptor(self):
        return MelfYuv16Frames(self.matrix, self.n, self.H, self.W, self.sub_y, self.c_step, self.shift, 0, self.y_pitch,
                               self.c_pitch, self.u_offset, self.v_offset, self.frame_stride)


def reduce16(samples, shift):
    """The 8-bit samples the kernels read 16-bit ones as: min(s >> shift, 255), uint8 (include/meterelf_hip.h)."""
    return np.minimum(np.asarray(samples).view(np.uint16) >> np.uint16(shift), np.uint16(255)).astype(np.uint8)


def _unwrap16(frames):
    """_unwrap for arrays of 2-byte samples: a uint16 numpy array, or a torch tensor of torch.uint16 (where the installed torch has
    it) or torch.int16 (the same bits); strides in BYTES.  Anything else: ValueError."""
    if _is_torch(frames):
        if str(frames.dtype) not in ('torch.uint16', 'torch.int16'):
            raise ValueError('frames must be uint16 (or int16 holding the same bits), not %s' % frames.dtype)
        on_device = frames.device.type == 'cuda'
        return (frames, True, tuple(frames.shape), tuple(2 * st for st in frames.stride()),
                frames.data_ptr(), on_device, frames.device.index if on_device else None)
    frames = np.asarray(frames)
    if frames.dtype != np.uint16:
        raise ValueError('frames must be uint16, not %s' % frames.dtype)
    return (frames, False, frames.shape, frames.strides, frames.ctypes.data, False, None)


def yuv16_frames_view(frames, pixel_format, matrix):
    """Describes the raw-video (N, rows, W) uint16 array of 16-bit planar / semi-planar YUV frames (numpy array, or torch tensor of
    uint16 / int16) as melf_process_yuv16* read it.  pixel_format, a name of YUV16_FORMATS: 4:2:0 'p010', 'p012', 'p016' (semi-planar,
    the value in the high bits), 'i010' / 'yuv420p10le', 'i012' / 'yuv420p12le', 'yuv420p16le' (planar, the value in the low bits)
    with rows = 3 H / 2; 4:2:2 'p210', 'p216', 'i210' / 'yuv422p10le', 'i212' / 'yuv422p12le', 'yuv422p16le' with rows = 2 H.  Rows
    0 .. H - 1 are Y; behind them the U plane and then the V plane, H >> sub_y rows of W / 2 samples each, or one plane of
    interleaved U V pairs, W samples a row.  The frame stride is honoured in place (frames[::2], frames[a:b]), and so is a
    row-padded view (frames[:, :, :w]) of the semi-planar formats, whose chroma row is one row of the array.  Anything else -- padded
    rows of a planar format (its chroma rows are half rows of the array), an element stride other than 1, negative strides -- is
    copied once to a packed array (Yuv16FramesView.copied).  matrix: a name of YUV_MATRIX_CODES or a code; there is no default:
    nearly all 10-bit material is BT.709, and the wrong matrix raises no error.  Not 16-bit samples, a shape that is not that of the
    format, an odd W (an odd H for 4:2:0), an unknown format or an unknown matrix: ValueError."""
    mcode = yuv_matrix_code(matrix)
    (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap16(frames)
    fmt = str(pixel_format).lower()
    if fmt not in YUV16_FORMATS:
        raise ValueError('pixel_format %r is not a 16-bit planar / semi-planar YUV layout (%s)' % (pixel_format, ', '.join(YUV16_FORMATS)))
    (sy, step, vfirst, shift) = YUV16_FORMATS[fmt]
    (frames, ptr, n, H, W, rp, c_pitch, u_off, v_off, fs, extent, copied) = _yuv_rows_layout(
        frames, is_torch, shape, strides, ptr, 2, 1, sy, step, vfirst, fmt, ' with an even W' + ' and an even H' * sy)
    return Yuv16FramesView(ptr, on_device, device, n, H, W, sy, step, shift, rp, c_pitch, u_off, v_off, fs, extent, copied, frames, mcode)


class PlaneView(NamedTuple):
    """One plane of one frame as melf_process_plane_list* read it (plane_view)."""
    ptr: int            # address of the plane's first sample
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    rows: int
    row_bytes: int      # bytes of a row's samples (an interleaved plane: of both)
    pitch: int          # bytes between rows
    in_place: bool      # False: the plane would have to be copied (an element stride other than 1, a negative or too small row stride)
    array: object       # what ptr points into: keep it alive while the call runs


def plane_view(plane, bps=1):
    """Describes one plane -- a 2-D (rows, samples) array, or (rows, pairs, 2) for an interleaved chroma plane -- of bps-byte
    samples (1: uint8; 2: uint16, or torch.int16 holding the same bits): a numpy array or torch tensor whose elements are contiguous
    along the last axis (and the pairs along the last two), with any row stride.  Not that dtype or not 2-D / (.., .., 2): ValueError."""
    (a, _is_t, shape, strides, ptr, on_device, device) = _unwrap(plane) if bps == 1 else _unwrap16(plane)
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 2)) or 0 in shape:
        raise ValueError('a plane must be (rows, samples) or, interleaved, (rows, pairs, 2), not %s' % (tuple(shape),))
    rows = shape[0]
    samples = shape[1] * (2 if len(shape) == 3 else 1)
    row_bytes = samples * bps
    contiguous = strides[-1] == bps or shape[-1] == 1
    if len(shape) == 3:
        contiguous = contiguous and (strides[1] == 2 * bps or shape[1] == 1)
    pitch = strides[0] if rows > 1 else row_bytes   # the stride of a dimension of size 1 is never stepped over
    in_place = bool(contiguous and row_bytes <= pitch <= 2 ** 31 - 1 and pitch % bps == 0)
    return PlaneView(int(ptr), on_device, device, int(rows), int(row_bytes), int(pitch), in_place, a)


class Yuv422_10FramesView(NamedTuple):
    """How the kernels read a batch of packed 10-bit YUV 4:2:2 frames in place (yuv422_10_frames_view)."""
    ptr: int            # address of frame 0's first group / macropixel
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    format: int         # YUV422_10_V210 / YUV422_10_Y210
    n: int
    H: int
    W: int
    row_pitch: int      # bytes between rows
    frame_stride: int   # bytes between frames
    extent: int         # bytes read from ptr: (n - 1) * frame_stride + (H - 1) * row_pitch + a row's groups / macropixels
    copied: bool        # the layout could not be described and the frames were copied once to a packed array
    array: object       # what ptr points into (the caller's array, or the copy): keep it alive while the call runs
    matrix: int         # YUV_BT* code of the colour conversion

    def descriptor(self):
        return MelfYuv422_10Frames(self.format, self.matrix, self.n, self.H, self.W, 0, self.row_pitch, self.frame_stride)


def _unwrap32(frames):
    """_unwrap for arrays of 4-byte words: a uint32 numpy array, or a torch tensor of torch.uint32 (where the installed torch has it)
    or torch.int32 (the same bits); strides in BYTES.  Anything else: ValueError."""
    if _is_torch(frames):
        if str(frames.dtype) not in ('torch.uint32', 'torch.int32'):
            raise ValueError('frames must be uint32 (or int32 holding the same bits), not %s' % frames.dtype)
        on_device = frames.device.type == 'cuda'
        return (frames, True, tuple(frames.shape), tuple(4 * st for st in frames.stride()),
                frames.data_ptr(), on_device, frames.device.index if on_device else None)
    frames = np.asarray(frames)
    if frames.dtype != np.uint32:
        raise ValueError('frames must be uint32, not %s' % frames.dtype)
    return (frames, False, frames.shape, frames.strides, frames.ctypes.data, False, None)


def v210_row_bytes(width):
    """Bytes of a v210 row of `width` pixels: ceil(width / 6) whole groups of 16 bytes."""
    return (width + 5) // 6 * 16


def yuv422_10_frames_view(frames, pixel_format, matrix, width=None):
    """Describes a batch of packed 10-bit YUV 4:2:2 frames (numpy array or torch tensor) as melf_process_yuv422_10* read it.
    pixel_format, a name of YUV422_10_FORMATS.  'v210': frames are (N, H, row_words) of uint32 (torch: int32 holding the same
    bits), a row being ceil(width / 6) groups of four words and whatever padding follows them (the conventional pitch is
    ((width + 47) // 48) * 32 words); width, the frames' width in pixels, is required: the array does not say it.  'y210' / 'y212' /
    'y216': frames are (N, H, W, 2) of uint16 (torch: int16 holding the same bits), the two words of pixel x being Y and, in turn,
    U or V; width, if given, must be W.  The frame stride and the row stride are honoured in place (frames[a:b], frames[::2], padded
    rows) where they are multiples of 16 (v210) / 8 (Y21x) bytes; any other layout -- an element stride, a row stride that is no such
    multiple, negative strides -- is copied once to a packed array (Yuv422_10FramesView.copied).  matrix: a name of YUV_MATRIX_CODES
    or a code; there is no default: nearly all 10-bit material is BT.709, and the wrong matrix raises no error.  A wrong dtype or
    rank, an odd or missing width, rows shorter than the width's groups, a base that is not 16- (v210) / 8-byte (Y21x) aligned, an
    unknown format or an unknown matrix: ValueError."""
    mcode = yuv_matrix_code(matrix)
    fmt = str(pixel_format).lower()
    if fmt not in YUV422_10_FORMATS:
        raise ValueError('pixel_format %r is not a packed 10-bit YUV 4:2:2 layout (%s)' % (pixel_format, ', '.join(YUV422_10_FORMATS)))
    code = YUV422_10_FORMATS[fmt]
    if code == YUV422_10_V210:
        (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap32(frames)
        if width is None:
            raise ValueError('v210 frames need width=: the row of words does not say how many pixels it holds')
        W = int(width)
        if len(shape) != 3 or shape[1] == 0 or W <= 0 or W % 2 != 0:
            raise ValueError('v210 frames must be (N, H, row_words) with an even width, not %s at width %r' % (shape, width))
        (n, H, words) = shape
        (row, align) = (v210_row_bytes(W), 16)
        if words * 4 < row:
            raise ValueError('v210 rows of %d words are shorter than the %d bytes of %d pixels' % (words, row, W))
        (fs, rp, es) = strides
        ok = es == 4
    else:
        (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap16(frames)
        if len(shape) != 4 or shape[3] != 2 or shape[1] == 0 or shape[2] == 0 or shape[2] % 2 != 0 or (width is not None and int(width) != shape[2]):
            raise ValueError('%s frames must be (N, H, W, 2) with an even W (and width, if given, W), not %s at width %r' % (fmt, shape, width))
        (n, H, W, _two) = shape
        (row, align) = (4 * W, 8)
        (fs, rp, ps, es) = strides
        ok = es == 2 and ps == 4
    if ptr % align != 0:
        raise ValueError('%s frames need a %d-byte aligned base' % (fmt, align))
    # strides of dimensions of size 1 are never stepped over: make them what a packed array has
    if H == 1:
        rp = row
    if n == 1:
        fs = (H - 1) * rp + row if rp > 0 else 0
    ok = ok and rp >= row and fs >= (H - 1) * rp + row and rp <= 2 ** 31 - 1 and (rp | fs) % align == 0
    if not ok:
        if code == YUV422_10_V210:
            frames = frames[:, :, :row // 4]   # the groups alone: a packed row of them is a multiple of 16 bytes
        (frames, ptr) = _packed_copy(frames, is_torch)
        (rp, fs) = (row, H * row)
    extent = (n - 1) * fs + (H - 1) * rp + row if n else 0
    return Yuv422_10FramesView(int(ptr), on_device, device, code, n, H, W, int(rp), int(fs), int(extent), not ok, frames, mcode)


class Packed32FramesView(NamedTuple):
    """How the kernels read a batch of 32-bit packed 4:4:4 frames in place (packed32_frames_view)."""
    ptr: int            # address of frame 0's first word
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    colour: int         # P32_YUV / P32_RGB
    pos: tuple          # low bit of the 8 bits read of Y, U, V / R, G, B
    n: int
    H: int
    W: int
    row_pitch: int      # bytes between rows
    frame_stride: int   # bytes between frames
    extent: int         # bytes read from ptr: (n - 1) * frame_stride + (H - 1) * row_pitch + 4 * W
    copied: bool        # the layout could not be described and the frames were copied once to a packed array
    array: object       # what ptr points into (the caller's array, or the copy): keep it alive while the call runs
    matrix: int         # YUV_BT* code of the colour conversion; 0 for P32_RGB

    def descriptor(self):
        return MelfPacked32Frames(self.colour, self.matrix, self.n, self.H, self.W, (C.c_int32 * 3)(*self.pos), self.row_pitch,
                                  self.frame_stride, 0, 0)


def packed32_frames_view(frames, pixel_format, matrix=None):
    """Describes a batch of 4:4:4 frames of one 32-bit word per pixel (numpy array or torch tensor) as melf_process_packed32* read
    it.  pixel_format: a name of PACKED32_FORMATS.  frames: (N, H, W) of uint32 (torch: int32 holding the same bits), a little-endian
    word per pixel; for the formats whose reads are whole bytes ('vuya', 'ayuv', 'uyva') also (N, H, W, 4) of uint8, the word's bytes
    in memory order.  The frame stride and the row stride are honoured in place (frames[a:b], frames[::2], frames[:, :, :w], padded
    rows) where the pixels are 4 bytes apart and the strides are multiples of 4; any other layout -- a pixel stride other than 4, a
    byte stride other than 1, negative strides -- is copied once to a packed array (Packed32FramesView.copied).  matrix: a name of
    YUV_MATRIX_CODES or a code for the YUV formats, where there is no default (None: ValueError) -- the wrong matrix raises no error;
    it must be None for the RGB formats.  A wrong dtype or rank, a base that is not 4-byte aligned, an unknown format or matrix:
    ValueError."""
    fmt = str(pixel_format).lower()
    if fmt not in PACKED32_FORMATS:
        raise ValueError('pixel_format %r is not a 32-bit packed 4:4:4 layout (%s)' % (pixel_format, ', '.join(PACKED32_FORMATS)))
    (colour, pos) = PACKED32_FORMATS[fmt]
    if colour == P32_YUV:
        if matrix is None:
            raise ValueError('%s frames need matrix=: there is no default, and the wrong matrix raises no error' % fmt)
        mcode = yuv_matrix_code(matrix)
    else:
        if matrix is not None:
            raise ValueError('%s frames are RGB: matrix must be None, not %r' % (fmt, matrix))
        mcode = 0
    as_bytes = (frames.dim() if _is_torch(frames) else np.ndim(frames)) == 4
    if as_bytes:
        if any(p % 8 for p in pos):
            raise ValueError('%s frames must be (N, H, W) of uint32: their reads are not whole bytes' % fmt)
        (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap(frames)
        if shape[3] != 4 or shape[1] == 0 or shape[2] == 0:
            raise ValueError('%s frames of uint8 must be (N, H, W, 4), not %s' % (fmt, shape))
        (n, H, W, _four) = shape
        (fs, rp, ps, es) = strides
        ok = es == 1
    else:
        (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap32(frames)
        if len(shape) != 3 or shape[1] == 0 or shape[2] == 0:
            raise ValueError('%s frames must be (N, H, W) of uint32, not %s' % (fmt, shape))
        (n, H, W) = shape
        (fs, rp, ps) = strides
        ok = True
    if ptr % 4 != 0:
        raise ValueError('%s frames need a 4-byte aligned base' % fmt)
    row = 4 * W
    # strides of dimensions of size 1 are never stepped over: make them what a packed array has
    if W == 1:
        ps = 4
    if H == 1:
        rp = row
    if n == 1:
        fs = (H - 1) * rp + row if rp > 0 else 0
    ok = ok and ps == 4 and rp >= row and fs >= (H - 1) * rp + row and rp <= 2 ** 31 - 1 and (rp | fs) % 4 == 0
    if not ok:
        (frames, ptr) = _packed_copy(frames, is_torch)
        (rp, fs) = (row, H * row)
    extent = (n - 1) * fs + (H - 1) * rp + row if n else 0
    return Packed32FramesView(int(ptr), on_device, device, colour, tuple(pos), n, H, W, int(rp), int(fs), int(extent), not ok, frames, mcode)


class PlanarFramesView(NamedTuple):
    """How the kernels read a batch of planar (channels-first) frames in place (planar_frames_view)."""
    ptr: int            # address of frame 0's first plane
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    n: int
    H: int
    W: int
    b_offset: int       # bytes from a frame's first byte to the first sample of its B / G / R plane
    g_offset: int
    r_offset: int
    row_pitch: int      # bytes between rows of a plane
    frame_stride: int   # bytes between frames
    extent: int         # bytes read from ptr: (n - 1) * frame_stride + max(offset) + (H - 1) * row_pitch + W
    copied: bool        # the layout could not be described and the frames were copied once to a packed (N, 3, H, W) array
    array: object       # what ptr points into (the caller's array, or the copy): keep it alive while the call runs

    def descriptor(self):
        return MelfPlanarFrames(self.n, self.H, self.W, 0, self.b_offset, self.g_offset, self.r_offset, self.row_pitch, self.frame_stride)


def planar_frames_view(frames, channel_order='rgb'):
    """Describes an (N, C, H, W) uint8 numpy array or torch tensor (channels first: what torch's decoders and pre-processing
    pipelines hold, ffmpeg's gbrp) as melf_process_planes* read it.  channel_order names the planes present, in the array's order:
    'rgb', 'bgr' or 'gbr' for C = 3, 'rgba' / 'rgbx' / 'bgra' / 'bgrx' for C = 4 (the 4th plane is never read).  Read in place: a
    unit stride along W, a row stride >= W, a plane stride that keeps the planes apart, any frame stride that holds a frame's
    planes -- contiguous NCHW, x[:, :3] of a 4-plane tensor, x[..., :h, :w], x[::2]; a channel order other than the caller's is
    a matter of channel_order, not of x[:, [2, 1, 0]].  Anything else -- a W stride other than 1 (a permuted NHWC tensor:
    frames_view reads those), negative strides, overlapping planes -- is copied once to a packed (N, 3, H, W) array
    (PlanarFramesView.copied).  Not uint8, not four-dimensional, a zero H or W, or a channel_order that does not name the array's C
    planes: ValueError."""
    (frames, is_torch, shape, strides, ptr, on_device, device) = _unwrap(frames)
    order = str(channel_order).lower()
    if order not in PLANAR_ORDERS:
        raise ValueError('channel_order %r is not one of %s' % (channel_order, ', '.join(PLANAR_ORDERS)))
    if len(shape) != 4 or shape[1] not in (3, 4) or shape[2] == 0 or shape[3] == 0:
        raise ValueError('planar frames must be (N, 3, H, W) or (N, 4, H, W), not %s' % (shape,))
    if shape[1] != len(order):
        raise ValueError('channel_order %r does not name the %d planes of the frames' % (channel_order, shape[1]))
    (n, _c, H, W) = shape
    (fs, ps, rp, es) = strides
    (ib, ig, ir) = (order.index('b'), order.index('g'), order.index('r'))
    # strides of dimensions of size 1 are never stepped over: make them what a packed array has
    if W == 1:
        es = 1
    if H == 1:
        rp = W
    span = (H - 1) * rp + W                       # bytes of one plane, first to last sample
    if n == 1:
        fs = max(ib, ig, ir) * ps + span if ps >= 0 else 0
    ok = es == 1 and W <= rp <= 2 ** 31 - 1 and ps >= span and fs >= max(ib, ig, ir) * ps + span
    if not ok:
        # the three colour planes, packed, in the caller's order (they are the first three of every order)
        (frames, ptr) = _packed_copy(frames[:, :3], is_torch)
        (rp, ps, fs) = (W, H * W, 3 * H * W)
        span = H * W
    extent = (n - 1) * fs + max(ib, ig, ir) * ps + span if n else 0
    return PlanarFramesView(int(ptr), on_device, device, n, H, W, int(ib * ps), int(ig * ps), int(ir * ps), int(rp), int(fs), int(extent),
                            not ok, frames)


class WideFramesView(NamedTuple):
    """How melf_process_wide* read a batch of RGB frames of wide samples in place (wide_frames_view)."""
    ptr: int            # address of frame 0's first sample (planar: of the lowest named plane's)
    on_device: bool     # True: a torch tensor on a GPU (ptr is a device address)
    device: Optional[int]
    sample_type: int    # WIDE_*
    layout: int         # WIDE_PACKED / WIDE_PLANAR
    pixel_format: int   # packed: PIX_*
    shift: int
    rounding: int       # ROUND_*
    scale: tuple        # B, G, R
    offset: tuple
    n: int
    H: int
    W: int
    b_offset: int       # planar: bytes from ptr to the first sample of frame 0's B / G / R plane
    g_offset: int
    r_offset: int
    row_pitch: int      # bytes between rows
    frame_stride: int   # bytes between frames
    extent: int         # bytes read from ptr
    copied: bool        # always False: a layout that cannot be described is a ValueError, not a copy
    array: object       # what ptr points into: keep it alive while the call runs

    def descriptor(self):
        return MelfWideFrames(self.sample_type, self.layout, self.pixel_format, self.shift, self.rounding, 0, (C.c_float * 3)(*self.scale),
                              (C.c_float * 3)(*self.offset), self.n, self.H, self.W, 0, self.b_offset, self.g_offset, self.r_offset,
                              self.row_pitch, self.frame_stride)


def narrow_wide(samples, scale=255.0, offset=0.0, rounding='nearest', shift=None):
    """The bytes melf_process_wide* read wide samples as, in numpy, exactly (include/meterelf_hip.h): uint16: min(s >> shift, 255);
    float16 / float32 (bfloat16: pass its values as float32): float32 x * scale, then + offset -- two roundings --, np.rint or
    np.floor, NaN to 0, clipped to 0 .. 255.  scale / offset broadcast against the samples."""
    a = np.asarray(samples)
    if a.dtype == np.uint16:
        return np.minimum(a >> np.uint16(shift), np.uint16(255)).astype(np.uint8)
    with np.errstate(all='ignore'):
        q = a.astype(np.float32) * np.asarray(scale, np.float32) + np.asarray(offset, np.float32)
        r = np.floor(q) if rounding == 'floor' else np.rint(q)
        return np.clip(np.where(np.isnan(r), np.float32(0), r), 0, 255).astype(np.uint8)


def _three(value, order, default, what):
    """scale / offset of wide_frames_view: a scalar or three values in the order of the frames' channels -> (B, G, R) floats"""
    if value is None:
        value = default
    v = np.asarray(value, np.float64).reshape(-1)
    if v.size not in (1, 3):
        raise ValueError('%s must be a scalar or three values, not %r' % (what, value))
    v = np.broadcast_to(v, (3,)).astype(np.float32)
    out = tuple(float(v[order.index(ch)]) for ch in 'bgr')
    if not all(np.isfinite(out)) or (what == 'scale' and max(abs(x) for x in out) > 2.0 ** 24):
        raise ValueError('%s must be finite%s, not %r' % (what, ', |scale| <= 2^24' if what == 'scale' else '', value))
    return out


def wide_frames_view(frames, layout, channel_order='rgb', scale=None, offset=None, rounding='nearest', shift=None):
    """Describes RGB frames of wide samples as melf_process_wide* read them: layout 'hwc' (N, H, W, C) or 'chw' (N, C, H, W), C = 3
    or 4, of uint16 (torch: uint16, or int16 holding the same bits), float16, bfloat16 (torch only) or float32; a numpy array or a
    torch tensor on the CPU or a GPU.  channel_order names the channels present in the array's order: 'rgb', 'bgr', 'rgba' / 'rgbx',
    'bgra' / 'bgrx', and for 'chw' also 'gbr' (the 4th is never converted).  Integer frames need shift (0 .. 8: the low bits dropped,
    8 for full 16-bit and MSB-aligned samples, 4 / 2 for 12 / 10 bits in the low bits) and take no scale, offset or rounding; float
    frames take no shift; scale / offset: a scalar or three values in the order of channel_order, defaults 255 and 0; rounding
    'nearest' or 'floor' (include/meterelf_hip.h has the rule; the wrong choice raises no error and moves samples by one).
    Strided views are taken in place when their strides fit the descriptor: unit stride along a pixel's samples ('hwc', pixels 3 or 4
    samples apart: x[..., :3] of a 4-channel tensor is read as the 4-sample format) or along W ('chw'), non-negative row, plane and
    frame strides that keep rows, planes and frames apart -- a channel slice x[:, :3], a spatial crop x[:, :, y0:, x0:], x[::2].
    Anything else is a ValueError: nothing is copied."""
    lay = str(layout).lower()
    if lay not in ('chw', 'hwc'):
        raise ValueError("layout %r is not 'chw' or 'hwc'" % (layout,))
    is_torch = _is_torch(frames)
    if not is_torch:
        frames = np.asarray(frames)
    tname = str(frames.dtype).replace('torch.', '')
    if tname not in WIDE_TYPES or (not is_torch and tname in ('int16', 'bfloat16')):
        raise ValueError('wide frames must be uint16, float16, bfloat16 or float32, not %s' % frames.dtype)
    stype = WIDE_TYPES[tname]
    ss = WIDE_SAMPLE_BYTES[stype]
    if is_torch:
        on_device = frames.device.type == 'cuda'
        (shape, strides, ptr, device) = (tuple(frames.shape), tuple(ss * st for st in frames.stride()), frames.data_ptr(),
                                         frames.device.index if on_device else None)
    else:
        (shape, strides, ptr, on_device, device) = (frames.shape, frames.strides, frames.ctypes.data, False, None)
    order = str(channel_order).lower()
    orders = WIDE_PACKED_ORDERS if lay == 'hwc' else PLANAR_ORDERS
    if order not in orders:
        raise ValueError('channel_order %r is not one of %s' % (channel_order, ', '.join(orders)))
    ci = 3 if lay == 'hwc' else 1
    if len(shape) != 4 or shape[ci] not in (3, 4) or 0 in shape[1:]:
        raise ValueError('wide %s frames must be %s with C = 3 or 4, not %s' % (lay, '(N, H, W, C)' if lay == 'hwc' else '(N, C, H, W)', shape,))
    if shape[ci] != len(order):
        raise ValueError('channel_order %r does not name the %d channels of the frames' % (channel_order, shape[ci]))
    if stype == WIDE_U16:
        if shift is None or int(shift) != shift or not 0 <= shift <= 8:
            raise ValueError('integer frames need shift = 0 .. 8 (the low bits dropped: 8 for 16-bit, 4 for 12-bit, 2 for 10-bit samples), not %r' % (shift,))
        if scale is not None or offset is not None or str(rounding).lower() != 'nearest':
            raise ValueError('integer frames take no scale, offset or rounding')
    elif shift is not None:
        raise ValueError('float frames take no shift')
    if str(rounding).lower() not in WIDE_ROUNDINGS:
        raise ValueError("rounding %r is not 'nearest' or 'floor'" % (rounding,))
    rgb3 = order[:3]
    (sc, of) = (_three(scale, rgb3, 255.0, 'scale'), _three(offset, rgb3, 0.0, 'offset'))
    n = shape[0]
    (b_off, g_off, r_off, code) = (0, 0, 0, 0)
    if lay == 'hwc':
        (_n, H, W, ch) = shape
        (fs, rp, ps, cs) = strides
        if ch == 3 and W > 1 and ps == 4 * ss:
            ch = 4                                   # a 3-channel view of 4-sample pixels: read the 4-sample format
        code = PIX_CODES[rgb3 + ('a' if ch == 4 else '')]
        if W == 1:
            ps = ch * ss
        if H == 1:
            rp = W * ch * ss
        span = (H - 1) * rp + W * ch * ss
        if n == 1:
            fs = span
        ok = cs == ss and ps == ch * ss and W * ch * ss <= rp <= 2 ** 31 - 1 and fs >= span
        if ok and n and ch == 4 and shape[3] == 3:
            # the unconverted 4th sample of the last pixel lies behind the view's own samples: it must belong to the same memory
            (lo, hi) = _owner_span(frames, is_torch)
            ok = lo <= ptr and ptr + (n - 1) * fs + span <= hi
    else:
        (_n, _c, H, W) = shape
        (fs, ps, rp, es) = strides
        (ib, ig, ir) = (order.index('b'), order.index('g'), order.index('r'))
        if W == 1:
            es = ss
        if H == 1:
            rp = W * ss
        span = (H - 1) * rp + W * ss
        if n == 1:
            fs = max(ib, ig, ir) * ps + span if ps >= 0 else 0
        ok = es == ss and W * ss <= rp <= 2 ** 31 - 1 and ps >= span and fs >= max(ib, ig, ir) * ps + span
        (b_off, g_off, r_off) = (ib * ps, ig * ps, ir * ps)
        span = max(ib, ig, ir) * ps + span
    if not ok or (ptr | rp | fs | b_off | g_off | r_off) % ss:
        raise ValueError('the strides %s (bytes) of these %s frames do not fit melf_wide_frames: they are not read in place, and nothing is '
                         'copied' % (strides, lay))
    extent = (n - 1) * fs + span if n else 0
    return WideFramesView(int(ptr), on_device, device, stype, WIDE_PLANAR if lay == 'chw' else WIDE_PACKED, code, int(shift or 0),
                          WIDE_ROUNDINGS[str(rounding).lower()], sc, of, n, H, W, int(b_off), int(g_off), int(r_off), int(rp), int(fs),
                          int(extent), False, frames)


def jpeg_probe(data):
    """(H, W, supported, reason) of a JPEG file's bytes; header parse only, no GPU."""
    L = lib()
    H, W, ok = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if isinstance(data, np.ndarray):
        p = _ptr(data)
    else:
        data = data if isinstance(data, bytes) else bytes(data)
        p = C.cast(C.c_char_p(data), C.c_void_p)  # no copy: the bytes object outlives the call
    check(L.melf_jpeg_probe(p, len(data), C.byref(H), C.byref(W), C.byref(ok)))
    return H.value, W.value, bool(ok.value), L.melf_last_error().decode()


def jpeg_probe_oriented(data):
    """(H, W, orientation, supported, reason) of a JPEG file's bytes, with the EXIF orientation taken instead of refused: H and W are
    the STORED size, orientation is 1..8 (1 when the tag is absent or invalid), supported is what jpeg_probe would say of the file
    without its tag.  The upright size is (W, H) for orientations 5-8.  Header parse only, no GPU."""
    L = lib()
    H, W, o, ok = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if isinstance(data, np.ndarray):
        p = _ptr(data)
    else:
        data = data if isinstance(data, bytes) else bytes(data)
        p = C.cast(C.c_char_p(data), C.c_void_p)  # no copy: the bytes object outlives the call
    check(L.melf_jpeg_probe_oriented(p, len(data), C.byref(H), C.byref(W), C.byref(o), C.byref(ok)))
    return H.value, W.value, o.value, bool(ok.value), L.melf_last_error().decode()


def jpeg_probe_oriented_batch(files):
    """jpeg_probe_oriented of many files' bytes in one call: (H, W, orientation, supported) int32 arrays; H and W are STORED sizes."""
    n = len(files)
    (H, W, o, ok) = (np.zeros(n, np.int32), np.zeros(n, np.int32), np.ones(n, np.int32), np.zeros(n, np.int32))
    if n:
        (ptrs, sizes, keep) = _file_table(files)
        check(lib().melf_jpeg_probe_oriented_batch(ptrs, sizes, n, _ptr(H), _ptr(W), _ptr(o), _ptr(ok)))
    return H, W, o, ok


JPEG_TAKE_ORIENTED = 1      # MELF_JPEG_TAKE_*: the switches a probe answers for
JPEG_TAKE_PROGRESSIVE = 2
JPEG_TAKE_SAMPLINGS = 4     # 4:4:0 and 4:1:1 files (melf_ctx_set_jpeg_samplings)
JPEG_TAKE_MULTISCAN = 32    # sequential files of three one-component scans (melf_ctx_set_jpeg_multiscan)
JPEG_TAKE_DEFAULT_TABLES = 16   # sequential files that leave Huffman tables 0 / 1 out: Motion-JPEG frames (melf_ctx_set_jpeg_default_tables)

# The JPEG switches of a context, one entry each: (name, the MELF_JPEG_TAKE_* flag a probe answers for it with -- None: no probe does --,
# what the switch does).  The library has melf_ctx_set_<name> / melf_ctx_get_<name>, Context has set_<name>(on) / <name>(), MeterReader
# the keyword argument, the attribute <name> and set_<name>(on); a new switch is a new entry here (and its line in _api.JPEG_SWITCH_ENV).
JPEG_SWITCHES = (
    ('jpeg_orientation', JPEG_TAKE_ORIENTED,
     """JPEG files with an EXIF orientation 2..8 are decoded upright by the jpeg_* calls of this context instead of coming back
     unsupported (melf_ctx_set_jpeg_orientation); H and W of those calls are then upright sizes.  Off by default."""),
    ('jpeg_progressive', JPEG_TAKE_PROGRESSIVE,
     """Progressive JPEG files (SOF2) of the subset include/meterelf_hip.h states are decoded by the jpeg_* calls of this context
     instead of coming back unsupported (melf_ctx_set_jpeg_progressive).  Off by default."""),
    ('jpeg_samplings', JPEG_TAKE_SAMPLINGS,
     """YCbCr 4:4:0 (luma 1x2) and 4:1:1 (luma 4x1) JPEG files are decoded by the jpeg_* calls of this context instead of coming
     back unsupported (melf_ctx_set_jpeg_samplings).  Off by default."""),
    ('jpeg_multiscan', JPEG_TAKE_MULTISCAN,
     """Sequential JPEG files sent as three scans of one component each are decoded by the jpeg_* calls of this context instead
     of coming back unsupported (melf_ctx_set_jpeg_multiscan).  Off by default."""),
    ('jpeg_default_tables', JPEG_TAKE_DEFAULT_TABLES,
     """Sequential JPEG files that leave Huffman tables 0 / 1 out (Motion-JPEG frames: no DHT segment) are decoded with the
     T.81 Annex K tables, as libjpeg-turbo does, instead of coming back unsupported (melf_ctx_set_jpeg_default_tables).  Off by default."""),
    ('jpeg_truncated', None,       # deliberately no probe flag: the headers do not show that a file ends early
     """Baseline JPEG files whose bytes stop inside the scan are completed by the jpeg_* calls of this context as libjpeg completes
     them -- the cut MCU from zero bits, mid grey behind it -- instead of coming back corrupt (melf_ctx_set_jpeg_truncated).  Off by
     default."""),
    ('jpeg_long_scans', None,      # no probe flag either: whether a scan is long does not show in what a probe reports
     """Baseline JPEG files without restart markers whose entropy-coded data exceed 4 MB (12 MP snapshots at high quality) are
     decoded by the jpeg_* calls of this context, chapter by chapter, instead of coming back unsupported
     (melf_ctx_set_jpeg_long_scans).  chapter_bytes: 0 = production (scans up to 4 MB take the ordinary kernels, longer ones the
     longest chapters the kernel addresses); > 0, for tests and tuning: every restart-less baseline scan longer than one chapter
     takes the chapter kernel, with chapters of that length rounded up to what the segment rule gives.  Off by default."""),
)


def jpeg_probe_flags(data, flags):
    """(H, W, orientation, supported, reason) of a JPEG file's bytes as the decode calls of a context with the switches `flags`
    (JPEG_TAKE_ORIENTED | JPEG_TAKE_PROGRESSIVE | JPEG_TAKE_SAMPLINGS | JPEG_TAKE_MULTISCAN | JPEG_TAKE_DEFAULT_TABLES) on answer from the headers: H and W are the STORED size, orientation is the EXIF code
    1..8 whether or not oriented files are taken.  With flags 0: jpeg_probe plus the orientation.  Header parse only, no GPU."""
    L = lib()
    H, W, o, ok = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if isinstance(data, np.ndarray):
        p = _ptr(data)
    else:
        data = data if isinstance(data, bytes) else bytes(data)
        p = C.cast(C.c_char_p(data), C.c_void_p)  # no copy: the bytes object outlives the call
    check(L.melf_jpeg_probe_flags(p, len(data), int(flags), C.byref(H), C.byref(W), C.byref(o), C.byref(ok)))
    return H.value, W.value, o.value, bool(ok.value), L.melf_last_error().decode()


def jpeg_probe_flags_batch(files, flags):
    """jpeg_probe_flags of many files' bytes in one call: (H, W, orientation, supported) int32 arrays; H and W are STORED sizes."""
    n = len(files)
    (H, W, o, ok) = (np.zeros(n, np.int32), np.zeros(n, np.int32), np.ones(n, np.int32), np.zeros(n, np.int32))
    if n:
        (ptrs, sizes, keep) = _file_table(files)
        check(lib().melf_jpeg_probe_flags_batch(ptrs, sizes, n, int(flags), _ptr(H), _ptr(W), _ptr(o), _ptr(ok)))
    return H, W, o, ok


def jpeg_probe_batch(files):
    """Header check of many files' bytes in one call: (H, W, supported) int32 arrays."""
    n = len(files)
    (H, W, ok) = (np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    if n:
        (ptrs, sizes, keep) = _file_table(files)
        check(lib().melf_jpeg_probe_batch(ptrs, sizes, n, _ptr(H), _ptr(W), _ptr(ok)))
    return H, W, ok


def _file_table(files):
    """list of bytes objects -> (pointer array, size array, keep-alive).  One ctypes array construction for the whole list
    (the per-file cast of a c_char_p cost 0.9 ms per 1024 files, a quarter of a melf_jpeg_process_batch call)."""
    n = len(files)
    keep = [f if isinstance(f, bytes) else bytes(f) for f in files]
    ptrs = (C.c_char_p * n)(*keep)          # holds references to the bytes objects; no copies
    sizes = np.fromiter(map(len, keep), dtype=np.uint64, count=n)
    return ptrs, _ptr(sizes), (keep, sizes)


file_table = _file_table


def _path_table(paths):
    """list of file names (str or bytes) -> (char** as a numpy array of addresses, keep-alive).  One join + one encode for the
    whole list instead of an os.fsencode and a ctypes conversion per name (0.45 -> 0.05 ms per 1024 names: the Python side
    of get_meter_values is one thread, and its per-chunk cost is what long lists wait for)."""
    n = len(paths)
    if n == 0:
        return np.zeros(1, np.uint64), None
    if all(type(p) is str for p in paths):
        blob = ('\0'.join(paths) + '\0').encode(sys.getfilesystemencoding(), 'surrogateescape')   # = os.fsencode, for all at once
    else:
        blob = b'\0'.join(os.fsencode(p) for p in paths) + b'\0'
    buf = np.frombuffer(blob, np.uint8)
    ends = np.flatnonzero(buf == 0)
    if len(ends) != n:   # a name with an embedded NUL: a C string would silently end there ('good.jpg\0x' would open good.jpg)
        raise ValueError('embedded null byte')   # what open() raises for such a name
    addr = np.empty(n, np.uint64)
    addr[0] = 0
    addr[1:] = ends[:-1] + 1
    addr += np.uint64(buf.ctypes.data)
    return addr, (blob, buf)


def files_open_probe(paths, device=0):
    """open() + close() of every path on the library's I/O pool: (milliseconds, threads).  Measurement aid."""
    (addr, keep) = _path_table(paths)
    ms = C.c_double(0.0)
    th = C.c_int(0)
    check(lib().melf_files_open_probe(C.c_void_p(addr.ctypes.data), len(paths), device, C.byref(ms), C.byref(th)))
    del keep
    return ms.value, th.value


def pack_blob(cparams, template):
    """params + template -> calibration blob (numpy uint8), masks built inside."""
    L = lib()
    template = np.ascontiguousarray(template, dtype=np.uint8)
    assert template.shape == (cparams.th, cparams.tw), (template.shape, cparams.th, cparams.tw)
    size = L.melf_blob_size(C.byref(cparams))
    if size == 0:
        raise HipError('libmeterelf_hip: %s' % L.melf_last_error().decode())
    blob = np.zeros(size, np.uint8)
    check(L.melf_blob_pack(C.byref(cparams), _ptr(template), _ptr(blob), size))
    return blob


def blob_params(blob):
    p = MelfParams()
    check(lib().melf_blob_params(_ptr(blob), blob.nbytes, C.byref(p)))
    return p


def build_dial_masks(cparams):
    out = np.zeros((cparams.ndials, 2, cparams.th, cparams.tw), np.uint8)
    check(lib().melf_build_dial_masks(C.byref(cparams), _ptr(out)))
    return out


GEN_TASK_DTYPE = np.dtype([(k, '<i4') for k in ('y0', 'rows', 'rows_computed', 'xb0', 'nxb', 'tile', 'slice', 'nslices', 'k_lo', 'k_hi',
                                                  'lds_bytes', 'reserved')])


def _match_info_dict(mi, gen_plan=False):
    d = {k: getattr(mi, k) for (k, _t) in MelfMatchInfo._fields_ if k != 'reserved'}
    d['kernel'] = MATCH_KERNEL_NAMES[mi.kernel]
    d['layout'] = ('rb%d%s%s' % (mi.rows_per_wave, '+pairs' if mi.pair_waves else '', '/k%d' % mi.reserved[2] if mi.reserved[2] > 1 else '')) if mi.kernel == 1 and not gen_plan else None
    if mi.kernel == 2 or gen_plan:   # the general kernel's plan: tile shape, slices, remainder columns
        (d['nd'], d['rows_pad'], d['blocks_per_tile'], d['slices'], d['v_columns'], d['v_blocks']) = tuple(mi.reserved)
        d['layout'] = 'r%dx%d/%d%s' % (mi.rows_per_wave, d['blocks_per_tile'], d['slices'], '+v%d' % d['v_columns'] if d['v_columns'] else '')
    else:
        d['th_pad'], d['rows_pad'], d['k_slices'] = mi.reserved[0], mi.reserved[1], max(1, mi.reserved[2])
    return d


def match_gen_plan_query(th, tw, rows, cols, n):
    """The general matrix-core kernel's plan for this shape and batch size (host logic, no GPU needed): (info dict -- 'kernel' is what
    DEFAULT dispatch launches for the shape --, structured array of one frame group's wave tasks)."""
    mi = MelfMatchInfo()
    nt = C.c_int32(0)
    check(lib().melf_match_gen_plan_query(th, tw, rows, cols, n, C.byref(mi), None, 0, C.byref(nt)))
    tasks = np.zeros(nt.value, GEN_TASK_DTYPE)
    check(lib().melf_match_gen_plan_query(th, tw, rows, cols, n, C.byref(mi), _ptr(tasks), nt.value, C.byref(nt)))
    d = _match_info_dict(mi, gen_plan=True)
    d['default_kernel'] = d.pop('kernel')
    return d, tasks


def match_layout_query(th, tw, rows, cols, n):
    """The tuned matrix-core kernel's wave layout for this shape and batch size (host logic, no GPU needed)."""
    mi = MelfMatchInfo()
    check(lib().melf_match_layout_query(th, tw, rows, cols, n, C.byref(mi)))
    return _match_info_dict(mi)


class Context:
    """One melf_ctx = one GPU's resident calibration state + workspaces."""

    def __init__(self, blob, device=0, blob_device_ptr=None):
        L = lib()
        self._h = C.c_void_p()
        self._L = L
        if blob_device_ptr is not None:
            check(L.melf_ctx_create(device, C.c_void_p(blob_device_ptr), int(blob.nbytes), 1, C.byref(self._h)))
        else:
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
            check(L.melf_ctx_create(device, _ptr(blob), blob.nbytes, 0, C.byref(self._h)))
        self.device = device
        self.params = MelfParams()
        check(L.melf_ctx_params(self._h, C.byref(self.params)))

    @classmethod
    def create_bcast(cls, blob, devices):
        """One context per listed GPU of THIS process, the blob sent to devices[0] and broadcast from there by RCCL
        (melf_ctx_create_bcast).  Devices must be distinct.  Returns the contexts in the order of `devices`."""
        L = lib()
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        n = len(devices)
        devs = (C.c_int * n)(*[int(d) for d in devices])
        handles = (C.c_void_p * n)()
        check(L.melf_ctx_create_bcast(devs, n, _ptr(blob), blob.nbytes, handles))
        out = []
        for (d, h) in zip(devices, handles):
            c = cls.__new__(cls)
            c._h = C.c_void_p(h)
            c._L = L
            c.device = int(d)
            c.params = MelfParams()
            check(L.melf_ctx_params(c._h, C.byref(c.params)))
            out.append(c)
        return out

    def sync(self):
        """Waits for the context's work on every caller stream and forgets the streams (call before destroying one)."""
        check(self._L.melf_ctx_sync(self._h))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._L.melf_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- whole path ---
    def process_batch(self, frames):
        """frames: (N, H, W, 3) uint8 BGR host array -> structured array of records."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        assert frames.ndim == 4 and frames.shape[3] == 3, frames.shape
        n, H, W, _ = frames.shape
        out = np.zeros(n, RESULT_DTYPE)
        if n:
            check(self._L.melf_process_batch(self._h, _ptr(frames), n, H, W, H * W * 3, _ptr(out)))
        return out

    def process_batch_dev(self, d_frames_ptr, n, H, W, frame_stride=None, d_results_ptr=None, want_host=True,
                          stream=None):
        """Frames already in HBM (device pointer as int).  Returns records when want_host."""
        out = np.zeros(n, RESULT_DTYPE) if want_host else None
        check(self._L.melf_process_batch_dev(
            self._h, C.c_void_p(d_frames_ptr), n, H, W, frame_stride or H * W * 3,
            C.c_void_p(d_results_ptr) if d_results_ptr else None,
            _ptr(out) if want_host else None, C.c_void_p(stream) if stream else None))
        return out

    def _host(self, entry, frames_ptr, desc):
        """A descriptor-taking host entry point (melf_process_frames / _yuv / _yuv422 / _yuv_planar / _planes) -> records."""
        out = np.zeros(desc.n, RESULT_DTYPE)
        check(entry(self._h, C.c_void_p(frames_ptr), C.byref(desc), _ptr(out)))
        return out

    def _dev(self, entry, d_frames_ptr, desc, d_results_ptr, want_host, stream):
        """Its *_dev form: frames in HBM (device pointer as int), as process_batch_dev.  Returns records when want_host."""
        out = np.zeros(desc.n, RESULT_DTYPE) if want_host else None
        check(entry(self._h, C.c_void_p(d_frames_ptr), C.byref(desc), C.c_void_p(d_results_ptr) if d_results_ptr else None,
                    _ptr(out) if want_host else None, C.c_void_p(stream) if stream else None))
        return out

    def process_frames(self, frames_ptr, pixel_format, n, H, W, row_pitch, frame_stride):
        """Host frames in any PIX_* layout (melf_process_frames; frames_view describes an array) -> records."""
        return self._host(self._L.melf_process_frames, frames_ptr, MelfFrames(pixel_format, n, H, W, row_pitch, frame_stride))

    def process_frames_dev(self, d_frames_ptr, pixel_format, n, H, W, row_pitch, frame_stride, d_results_ptr=None, want_host=True,
                           stream=None):
        """Frames in HBM in any PIX_* layout (melf_process_frames_dev, as process_batch_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_frames_dev, d_frames_ptr, MelfFrames(pixel_format, n, H, W, row_pitch, frame_stride),
                         d_results_ptr, want_host, stream)

    def process_yuv(self, frames_ptr, desc):
        """Host YUV 4:2:0 frames (melf_process_yuv; desc: a MelfYuvFrames, e.g. yuv_frames_view(...).descriptor()) -> records."""
        return self._host(self._L.melf_process_yuv, frames_ptr, desc)

    def process_yuv_dev(self, d_frames_ptr, desc, d_results_ptr=None, want_host=True, stream=None):
        """YUV 4:2:0 frames in HBM (melf_process_yuv_dev, as process_frames_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_yuv_dev, d_frames_ptr, desc, d_results_ptr, want_host, stream)

    def yuv_to_bgr(self, frames_ptr, desc):
        """The conversion alone (melf_yuv_to_bgr): host YUV 4:2:0 frames -> (n, H, W, 3) BGR."""
        out = np.empty((desc.n, desc.H, desc.W, 3), np.uint8)
        check(self._L.melf_yuv_to_bgr(self._h, C.c_void_p(frames_ptr), C.byref(desc), _ptr(out)))
        return out

    def process_yuv422(self, frames_ptr, desc):
        """Host packed YUV 4:2:2 frames (melf_process_yuv422; desc: a MelfYuv422Frames, e.g. yuv422_frames_view(...).descriptor())
        -> records."""
        return self._host(self._L.melf_process_yuv422, frames_ptr, desc)

    def process_yuv422_dev(self, d_frames_ptr, desc, d_results_ptr=None, want_host=True, stream=None):
        """Packed YUV 4:2:2 frames in HBM (melf_process_yuv422_dev, as process_frames_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_yuv422_dev, d_frames_ptr, desc, d_results_ptr, want_host, stream)

    def yuv422_to_bgr(self, frames_ptr, desc):
        """The conversion alone (melf_yuv422_to_bgr): host packed YUV 4:2:2 frames -> (n, H, W, 3) BGR."""
        out = np.empty((desc.n, desc.H, desc.W, 3), np.uint8)
        check(self._L.melf_yuv422_to_bgr(self._h, C.c_void_p(frames_ptr), C.byref(desc), _ptr(out)))
        return out

    def process_yuv_planar(self, frames_ptr, desc):
        """Host planar / semi-planar YUV frames (melf_process_yuv_planar; desc: a MelfYuvPlanarFrames, e.g.
        yuv_planar_frames_view(...).descriptor()) -> records."""
        return self._host(self._L.melf_process_yuv_planar, frames_ptr, desc)

    def process_yuv_planar_dev(self, d_frames_ptr, desc, d_results_ptr=None, want_host=True, stream=None):
        """Planar / semi-planar YUV frames in HBM (melf_process_yuv_planar_dev, as process_frames_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_yuv_planar_dev, d_frames_ptr, desc, d_results_ptr, want_host, stream)

    def yuv_planar_to_bgr(self, frames_ptr, desc):
        """The conversion alone (melf_yuv_planar_to_bgr): host planar / semi-planar YUV frames -> (n, H, W, 3) BGR."""
        out = np.empty((desc.n, desc.H, desc.W, 3), np.uint8)
        check(self._L.melf_yuv_planar_to_bgr(self._h, C.c_void_p(frames_ptr), C.byref(desc), _ptr(out)))
        return out

    def process_yuv16(self, frames_ptr, desc):
        """Host 16-bit planar / semi-planar YUV frames (melf_process_yuv16; desc: a MelfYuv16Frames, e.g.
        yuv16_frames_view(...).descriptor()) -> records."""
        return self._host(self._L.melf_process_yuv16, frames_ptr, desc)

    def process_yuv16_dev(self, d_frames_ptr, desc, d_results_ptr=None, want_host=True, stream=None):
        """16-bit planar / semi-planar YUV frames in HBM (melf_process_yuv16_dev, as process_frames_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_yuv16_dev, d_frames_ptr, desc, d_results_ptr, want_host, stream)

    def yuv16_to_bgr(self, frames_ptr, desc):
        """Reduction and conversion alone (melf_yuv16_to_bgr): host 16-bit planar / semi-planar YUV frames -> (n, H, W, 3) BGR."""
        out = np.empty((desc.n, desc.H, desc.W, 3), np.uint8)
        check(self._L.melf_yuv16_to_bgr(self._h, C.c_void_p(frames_ptr), C.byref(desc), _ptr(out)))
        return out

    def process_yuv422_10(self, frames_ptr, desc):
        """Host packed 10-bit YUV 4:2:2 frames (melf_process_yuv422_10; desc: a MelfYuv422_10Frames, e.g.
        yuv422_10_frames_view(...).descriptor()) -> records."""
        return self._host(self._L.melf_process_yuv422_10, frames_ptr, desc)

    def process_yuv422_10_dev(self, d_frames_ptr, desc, d_results_ptr=None, want_host=True, stream=None):
        """Packed 10-bit YUV 4:2:2 frames in HBM (melf_process_yuv422_10_dev, as process_frames_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_yuv422_10_dev, d_frames_ptr, desc, d_results_ptr, want_host, stream)

    def yuv422_10_to_bgr(self, frames_ptr, desc):
        """Unpacking and conversion alone (melf_yuv422_10_to_bgr): host packed 10-bit YUV 4:2:2 frames -> (n, H, W, 3) BGR."""
        out = np.empty((desc.n, desc.H, desc.W, 3), np.uint8)
        check(self._L.melf_yuv422_10_to_bgr(self._h, C.c_void_p(frames_ptr), C.byref(desc), _ptr(out)))
        return out

    def process_packed32(self, frames_ptr, desc):
        """Host 32-bit packed 4:4:4 frames (melf_process_packed32; desc: a MelfPacked32Frames, e.g.
        packed32_frames_view(...).descriptor()) -> records."""
        return self._host(self._L.melf_process_packed32, frames_ptr, desc)

    def process_packed32_dev(self, d_frames_ptr, desc, d_results_ptr=None, want_host=True, stream=None):
        """32-bit packed 4:4:4 frames in HBM (melf_process_packed32_dev, as process_frames_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_packed32_dev, d_frames_ptr, desc, d_results_ptr, want_host, stream)

    def packed32_to_bgr(self, frames_ptr, desc):
        """Unpacking and conversion alone (melf_packed32_to_bgr): host 32-bit packed 4:4:4 frames -> (n, H, W, 3) BGR."""
        out = np.empty((desc.n, desc.H, desc.W, 3), np.uint8)
        check(self._L.melf_packed32_to_bgr(self._h, C.c_void_p(frames_ptr), C.byref(desc), _ptr(out)))
        return out

    def process_planes(self, frames_ptr, desc):
        """Host planar frames (melf_process_planes; desc: a MelfPlanarFrames, e.g. planar_frames_view(...).descriptor()) -> records."""
        return self._host(self._L.melf_process_planes, frames_ptr, desc)

    def process_planes_dev(self, d_frames_ptr, desc, d_results_ptr=None, want_host=True, stream=None):
        """Planar frames in HBM (melf_process_planes_dev, as process_frames_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_planes_dev, d_frames_ptr, desc, d_results_ptr, want_host, stream)

    def process_wide(self, frames_ptr, desc):
        """Host RGB frames of wide samples (melf_process_wide; desc: a MelfWideFrames, e.g. wide_frames_view(...).descriptor()) ->
        records."""
        return self._host(self._L.melf_process_wide, frames_ptr, desc)

    def process_wide_dev(self, d_frames_ptr, desc, d_results_ptr=None, want_host=True, stream=None):
        """RGB frames of wide samples in HBM (melf_process_wide_dev, as process_frames_dev).  Returns records when want_host."""
        return self._dev(self._L.melf_process_wide_dev, d_frames_ptr, desc, d_results_ptr, want_host, stream)

    def wide_to_bgr(self, frames_ptr, desc):
        """The narrowing alone, through the GPU kernel (melf_wide_to_bgr): host frames of wide samples -> (n, H, W, 3) BGR."""
        out = np.empty((desc.n, desc.H, desc.W, 3), np.uint8)
        check(self._L.melf_wide_to_bgr(self._h, C.c_void_p(frames_ptr), C.byref(desc), _ptr(out)))
        return out

    # --- frames in separate allocations ---
    @staticmethod
    def _pointer_table(ptrs, desc):
        """The host array of frame pointers melf_process_frame_list* take (a NULL entry stays NULL: the library names it); a
        ctypes array made by an earlier call is taken as it is.  The library reads desc.n entries: fewer is a ValueError."""
        if len(ptrs) < desc.n:
            raise ValueError('the descriptor counts %d frames, the list holds %d pointers' % (desc.n, len(ptrs)))
        if isinstance(ptrs, C.Array):
            return ptrs
        return (C.c_void_p * len(ptrs))(*[int(p) or None for p in ptrs])

    def process_frame_list(self, family, desc, frame_ptrs):
        """Host frames in separate allocations (melf_process_frame_list) -> records.  family: LIST_FAMILIES' code or name; desc: the
        family's descriptor, its n the length of the list (frame_stride is not looked at); frame_ptrs: the frames' addresses."""
        family = LIST_FAMILIES.get(family, family)
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE)
        check(self._L.melf_process_frame_list(self._h, family, C.byref(desc), self._pointer_table(frame_ptrs, desc), _ptr(out)))
        return out

    def process_frame_list_dev(self, family, desc, d_frame_ptrs, d_results_ptr=None, want_host=True, stream=None):
        """Frames in separate allocations in HBM (melf_process_frame_list_dev, as process_frames_dev): d_frame_ptrs: their device
        addresses (the library copies the table before it returns).  Returns records when want_host."""
        family = LIST_FAMILIES.get(family, family)
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE) if want_host else None
        check(self._L.melf_process_frame_list_dev(self._h, family, C.byref(desc), self._pointer_table(d_frame_ptrs, desc),
                                                  C.c_void_p(d_results_ptr) if d_results_ptr else None, _ptr(out) if want_host else None,
                                                  C.c_void_p(stream) if stream else None))
        return out

    # --- a frame's planes in separate allocations ---
    @staticmethod
    def _plane_table(ptrs, desc, nplanes):
        """The host array of plane pointers melf_process_plane_list* take, frame-major: ptrs is flat (n * nplanes addresses) or one
        sequence of nplanes addresses per frame; a NULL entry stays NULL (the library names it).  Fewer than desc.n * nplanes: ValueError."""
        if isinstance(ptrs, C.Array):
            flat = ptrs
        else:
            flat = []
            for p in ptrs:
                flat.extend(p if isinstance(p, (tuple, list)) else (p,))
        if nplanes > 0 and len(flat) < desc.n * nplanes:
            raise ValueError('the descriptor counts %d frames of %d planes, the list holds %d pointers' % (desc.n, nplanes, len(flat)))
        return flat if isinstance(flat, C.Array) else (C.c_void_p * len(flat))(*[int(p) or None for p in flat])

    def process_plane_list(self, family, desc, plane_ptrs, nplanes):
        """Host frames whose planes lie in separate allocations (melf_process_plane_list) -> records.  family: LIST_FAMILIES' code or
        name ('yuv', 'yuv_planar', 'yuv16', 'planar'); desc: the family's descriptor, its n the length of the list, its plane offsets
        counted from each plane's own pointer; plane_ptrs: n * nplanes addresses, frame-major (slots: Y, U or interleaved chroma, V;
        B, G, R), flat or one tuple per frame."""
        family = LIST_FAMILIES.get(family, family)
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE)
        check(self._L.melf_process_plane_list(self._h, family, C.byref(desc), self._plane_table(plane_ptrs, desc, nplanes), nplanes, _ptr(out)))
        return out

    def process_plane_list_dev(self, family, desc, d_plane_ptrs, nplanes, d_results_ptr=None, want_host=True, stream=None):
        """The same for planes in HBM (melf_process_plane_list_dev, as process_frame_list_dev): d_plane_ptrs: their device addresses
        (the library copies the table before it returns).  Returns records when want_host."""
        family = LIST_FAMILIES.get(family, family)
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE) if want_host else None
        check(self._L.melf_process_plane_list_dev(self._h, family, C.byref(desc), self._plane_table(d_plane_ptrs, desc, nplanes), nplanes,
                                                  C.c_void_p(d_results_ptr) if d_results_ptr else None, _ptr(out) if want_host else None,
                                                  C.c_void_p(stream) if stream else None))
        return out

    # --- wide frames, and wide planes, in separate allocations ---
    def process_wide_list(self, desc, frame_ptrs):
        """Host frames of wide samples in separate allocations (melf_process_wide_list) -> records.  desc: a MelfWideFrames, its n the
        length of the list (frame_stride is not looked at); frame_ptrs: the frames' addresses."""
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE)
        check(self._L.melf_process_wide_list(self._h, C.byref(desc), self._pointer_table(frame_ptrs, desc), _ptr(out)))
        return out

    def process_wide_list_dev(self, desc, d_frame_ptrs, d_results_ptr=None, want_host=True, stream=None):
        """The same for frames in HBM (melf_process_wide_list_dev, as process_frame_list_dev).  Returns records when want_host."""
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE) if want_host else None
        check(self._L.melf_process_wide_list_dev(self._h, C.byref(desc), self._pointer_table(d_frame_ptrs, desc),
                                                 C.c_void_p(d_results_ptr) if d_results_ptr else None, _ptr(out) if want_host else None,
                                                 C.c_void_p(stream) if stream else None))
        return out

    def process_wide_plane_list(self, desc, plane_ptrs, nplanes=3):
        """Host planar frames of wide samples whose planes lie in separate allocations (melf_process_wide_plane_list) -> records.  desc:
        a planar MelfWideFrames, its n the length of the list, its plane offsets 0; plane_ptrs: n * 3 addresses, frame-major (B, G,
        R), flat or one tuple per frame."""
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE)
        check(self._L.melf_process_wide_plane_list(self._h, C.byref(desc), self._plane_table(plane_ptrs, desc, nplanes), nplanes, _ptr(out)))
        return out

    def process_wide_plane_list_dev(self, desc, d_plane_ptrs, nplanes=3, d_results_ptr=None, want_host=True, stream=None):
        """The same for planes in HBM (melf_process_wide_plane_list_dev, as process_plane_list_dev).  Returns records when want_host."""
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE) if want_host else None
        check(self._L.melf_process_wide_plane_list_dev(self._h, C.byref(desc), self._plane_table(d_plane_ptrs, desc, nplanes), nplanes,
                                                       C.c_void_p(d_results_ptr) if d_results_ptr else None, _ptr(out) if want_host else None,
                                                       C.c_void_p(stream) if stream else None))
        return out

    def wide_list_to_bgr(self, desc, ptrs, nplanes=0):
        """The narrowing alone, through the list kernels (melf_wide_list_to_bgr): host addresses of desc.n frames (nplanes 0) or of
        desc.n * 3 planes (nplanes 3), each uploaded into a device allocation of exactly its readable extent -> (n, H, W, 3) BGR."""
        out = np.empty((max(desc.n, 0), desc.H, desc.W, 3), np.uint8)
        table = self._plane_table(ptrs, desc, nplanes) if nplanes else self._pointer_table(ptrs, desc)
        check(self._L.melf_wide_list_to_bgr(self._h, C.byref(desc), table, nplanes, _ptr(out)))
        return out

    # --- frames stored rotated or mirrored ---
    def process_oriented(self, family, desc, orientation, frames_ptr):
        """Host frames stored rotated or mirrored (melf_process_oriented) -> records.  family: LIST_FAMILIES' code or name; desc: the
        family's descriptor of the STORED batch; orientation: ORIENTATIONS' code (1 .. 8) or name."""
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE)
        check(self._L.melf_process_oriented(self._h, LIST_FAMILIES.get(family, family), C.byref(desc), ORIENTATIONS.get(orientation, orientation),
                                            C.c_void_p(frames_ptr), _ptr(out)))
        return out

    def process_oriented_dev(self, family, desc, orientation, d_frames_ptr, d_results_ptr=None, want_host=True, stream=None):
        """The same for a stored batch in HBM (melf_process_oriented_dev, as process_frames_dev).  Returns records when want_host."""
        out = np.zeros(max(desc.n, 0), RESULT_DTYPE) if want_host else None
        check(self._L.melf_process_oriented_dev(self._h, LIST_FAMILIES.get(family, family), C.byref(desc), ORIENTATIONS.get(orientation, orientation),
                                                C.c_void_p(d_frames_ptr), C.c_void_p(d_results_ptr) if d_results_ptr else None,
                                                _ptr(out) if want_host else None, C.c_void_p(stream) if stream else None))
        return out

    def orient_frames(self, family, desc, orientation, frames_ptr, out_bytes):
        """The orientation alone (melf_orient_frames): host frames -> a uint8 array of out_bytes bytes holding desc.n oriented frames in
        the family's layout at tight pitches (include/meterelf_hip.h states the tight frame per family)."""
        out = np.zeros(out_bytes, np.uint8)
        check(self._L.melf_orient_frames(self._h, LIST_FAMILIES.get(family, family), C.byref(desc), ORIENTATIONS.get(orientation, orientation),
                                         C.c_void_p(frames_ptr), _ptr(out), out_bytes))
        return out

    def gather_frame_list_dev(self, family, desc, d_frame_ptrs, stream=None):
        """The gather kernel of process_frame_list_dev alone (melf_gather_frame_list_dev: the diagnostic build only) -> the bytes it
        read plus the bytes it wrote."""
        if not hasattr(self._L, 'melf_gather_frame_list_dev'):
            raise HipError('melf_gather_frame_list_dev is part of the diagnostic build only (make -C meterelf_amd/csrc diag; MELF_LIB_PATH)')
        moved = C.c_size_t(0)
        check(self._L.melf_gather_frame_list_dev(self._h, LIST_FAMILIES.get(family, family), C.byref(desc), self._pointer_table(d_frame_ptrs, desc),
                                                 C.c_void_p(stream) if stream else None, C.byref(moved)))
        return moved.value

    # --- stages ---
    def process_stream_dev(self, d_frames_ptr, nbatches, batch_stride, n, H, W, d_results_ptr, results_stride, frame_stride=None,
                           stream=None):
        """nbatches batches of n device-resident frames in one call; consecutive batches overlap on two lanes."""
        check(self._L.melf_process_stream_dev(self._h, C.c_void_p(d_frames_ptr), nbatches, batch_stride, n, H, W,
                                              frame_stride or H * W * 3, C.c_void_p(d_results_ptr), results_stride,
                                              C.c_void_p(stream) if stream else None))

    def bgr2hls(self, bgr):
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        rows, cols, _ = bgr.shape
        out = np.empty((rows, cols, 3), np.uint8)
        check(self._L.melf_bgr2hls(self._h, _ptr(bgr), rows, cols, cols * 3, _ptr(out)))
        return out

    def hls_inrange_close(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, H, W, _ = frames.shape
        out = np.empty((n, H, W), np.uint8)
        check(self._L.melf_hls_inrange_close(self._h, _ptr(frames), n, H, W, _ptr(out)))
        return out

    def hls_inrange_close_dev(self, d_frames_ptr, n, H, W, d_masks_ptr, stream=None):
        check(self._L.melf_hls_inrange_close_dev(self._h, C.c_void_p(d_frames_ptr), n, H, W,
                                                  C.c_void_p(d_masks_ptr), C.c_void_p(stream) if stream else None))

    def stream_probe_dev(self, d_in_ptr, in_bytes, d_out_ptr, chunks_per_block=0, stream=None):
        if not hasattr(self._L, 'melf_stream_probe_dev'):
            raise HipError('melf_stream_probe_dev is part of the diagnostic build only (make -C meterelf_amd/csrc diag; MELF_LIB_PATH)')
        """Measurement aid: one bare 3:1 stream launch over device buffers (include/meterelf_hip.h); d_out is overwritten."""
        check(self._L.melf_stream_probe_dev(self._h, C.c_void_p(d_in_ptr), C.c_size_t(in_bytes), C.c_void_p(d_out_ptr),
                                             int(chunks_per_block), C.c_void_p(stream) if stream else None))

    def match_ccoeff(self, images, want_map=False):
        images = np.ascontiguousarray(images, dtype=np.uint8)
        n, rows, cols = images.shape
        mv = np.zeros(n, np.float32)
        mx = np.zeros(n, np.int32)
        my = np.zeros(n, np.int32)
        rmap = None
        if want_map:
            rmap = np.zeros((n, rows - self.params.th + 1, cols - self.params.tw + 1), np.float32)
        check(self._L.melf_match_ccoeff(self._h, _ptr(images), n, rows, cols, _ptr(mv), _ptr(mx), _ptr(my),
                                        _ptr(rmap) if want_map else None))
        return mv, mx, my, rmap

    def read_dials(self, dials_hls):
        dials_hls = np.ascontiguousarray(dials_hls, dtype=np.uint8)
        n = dials_hls.shape[0]
        assert dials_hls.shape[1:] == (self.params.th, self.params.tw, 3), dials_hls.shape
        out = np.zeros(n, RESULT_DTYPE)
        check(self._L.melf_read_dials(self._h, _ptr(dials_hls), n, _ptr(out)))
        return out

    def masks(self):
        p = self.params
        out = np.zeros((p.ndials, 2, p.th, p.tw), np.uint8)
        check(self._L.melf_ctx_get_masks(self._h, _ptr(out)))
        return out

    # --- calibration stages ---
    def aligned_average(self, frames, match_x, match_y, align_x, align_y):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        (n, H, W, _) = frames.shape
        p = self.params
        (rows, cols) = (min(p.rect_y1, H) - min(p.rect_y0, H), min(p.rect_x1, W) - min(p.rect_x0, W))
        mx = np.ascontiguousarray(match_x, dtype=np.int32)
        my = np.ascontiguousarray(match_y, dtype=np.int32)
        out = np.empty((rows, cols, 3), np.uint8)
        check(self._L.melf_aligned_average(self._h, _ptr(frames), n, H, W, H * W * 3, _ptr(mx), _ptr(my),
                                           int(align_x), int(align_y), _ptr(out)))
        return out

    def inrange(self, img, lo, hi):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        (rows, cols, _) = img.shape
        lo = np.ascontiguousarray(lo, dtype=np.int32)
        hi = np.ascontiguousarray(hi, dtype=np.int32)
        out = np.empty((rows, cols), np.uint8)
        check(self._L.melf_inrange(self._h, _ptr(img), rows, cols, _ptr(lo), _ptr(hi), _ptr(out)))
        return out

    def fused_table_ties(self):
        n = C.c_int(0)
        check(self._L.melf_ctx_fused_table_ties(self._h, C.byref(n)))
        return n.value

    def fused_variant(self):
        """Which fused-mask kernel body this context's needle bounds select, from what, and what the last launch ran
        (include/meterelf_hip.h, melf_ctx_fused_variant): last_body -1 = the float-path kernel, -2 = no launch yet;
        last_queue_slot -1 = static split."""
        (v, a) = (C.c_int(0), C.c_int(0))
        (noniv, last) = ((C.c_int * 3)(), (C.c_int * 2)())
        check(self._L.melf_ctx_fused_variant(self._h, C.byref(v), C.byref(a), noniv, last))
        return dict(variant=v.value, active_sectors=a.value, noniv=tuple(noniv), last_body=last[0], last_queue_slot=last[1])

    # --- measurement ---
    def jpeg_decode(self, files, H, W):
        """cv2.imread for a batch of JPEG files' bytes: (frames n x H x W x 3 BGR u8, status n)."""
        n = len(files)
        out = np.zeros((n, H, W, 3), np.uint8)
        status = np.zeros(n, np.int32)
        if n:
            (ptrs, sizes, keep) = _file_table(files)
            check(self._L.melf_jpeg_decode_batch(self._h, ptrs, sizes, n, H, W, _ptr(out), 0, _ptr(status)))
        return out, status

    def jpeg_decode_dev(self, files, H, W, d_frames_ptr):
        """Same, into device memory (n*H*W*3 bytes at d_frames_ptr); returns the status array."""
        n = len(files)
        status = np.zeros(n, np.int32)
        if n:
            (ptrs, sizes, keep) = _file_table(files)
            check(self._L.melf_jpeg_decode_batch(self._h, ptrs, sizes, n, H, W, C.c_void_p(d_frames_ptr), 1, _ptr(status)))
        return status

    def jpeg_process_batch(self, files, H, W, table=None):
        """JPEG bytes -> (result records, decode status); decode and reading both on the GPU.  table: file_table(files) made
        earlier (a caller that sends the same list again -- a benchmark -- then pays for the call alone, as a compiled host
        would, not for 1024 ctypes conversions)."""
        n = len(files)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        status = np.zeros(n, np.int32)
        if n:
            (ptrs, sizes, keep) = table if table is not None else _file_table(files)
            check(self._L.melf_jpeg_process_batch(self._h, ptrs, sizes, n, H, W, _ptr(out), _ptr(status)))
        return out, status

    def jpeg_process_files(self, paths):
        """File names -> (records, status, (H, W) of the batch): files are read, decoded and read out inside the
        library; status 3 = another frame size (call again with those), 1 / 2 / 4 = not for the GPU decoder."""
        n = len(paths)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        status = np.zeros(n, np.int32)
        (H, W) = (C.c_int32(0), C.c_int32(0))
        if n:
            (addr, keep) = _path_table(paths)
            check(self._L.melf_jpeg_process_files(self._h, _ptr(addr), n, C.byref(H), C.byref(W), _ptr(out), _ptr(status)))
        return out, status, (H.value, W.value)

    def jpeg_process_files_begin(self, paths):
        """Starts jpeg_process_files(paths) on a thread of the library and returns at once; jpeg_process_files_end()
        waits for the oldest call begun.  Up to FILES_IN_FLIGHT_MAX calls in flight per context (one reading its files, one
        preparing and enqueueing, one waiting for its kernels), no other call on the context in between."""
        n = len(paths)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        status = np.zeros(n, np.int32)
        hw = (C.c_int32(0), C.c_int32(0))
        (addr, keep) = _path_table(paths)
        check(self._L.melf_jpeg_process_files_begin(self._h, _ptr(addr), n, C.byref(hw[0]), C.byref(hw[1]), _ptr(out), _ptr(status)))
        if getattr(self, '_files_pending', None) is None:
            self._files_pending = []
        self._files_pending.append((out, status, hw, addr, keep))  # everything the library points into, alive until its _end

    def jpeg_process_files_end(self):
        (out, status, hw, _arr, _enc) = self._files_pending.pop(0)  # the library forgets the call whatever it returns
        check(self._L.melf_jpeg_process_files_end(self._h))
        return out, status, (hw[0].value, hw[1].value)

    def files_in_flight(self):
        return len(getattr(self, '_files_pending', None) or ())

    # set_jpeg_orientation(on) / jpeg_orientation() and so on, one pair per entry of JPEG_SWITCHES: _add_jpeg_switch below the class

    def jpeg_truncated_files(self, reset=False):
        """Files this context's calls completed under that rule since the last reset (melf_ctx_jpeg_truncated_files)."""
        n = C.c_int64(0)
        check(self._L.melf_ctx_jpeg_truncated_files(self._h, C.byref(n), int(bool(reset))))
        return int(n.value)

    def set_frames_resident(self, on):
        """Promise that the frames of every process_batch_dev call are complete in HBM when the call is made: a call's prep
        kernels then run under the previous call's dials kernel (melf_ctx_set_frames_resident)."""
        check(self._L.melf_ctx_set_frames_resident(self._h, int(bool(on))))

    def last_match(self):
        """Kernel and wave layout of the most recent template-match launch: dict with 'kernel' ('dot4' / 'mfma' / 'gen'),
        'layout' (tuned kernel: 'rb<rows per wave>' + '+pairs' when pairs of waves share a map row), and the raw fields."""
        mi = MelfMatchInfo()
        check(self._L.melf_ctx_last_match(self._h, C.byref(mi)))
        return _match_info_dict(mi)

    def last_dials(self):
        """The dial-reader kernel of the most recent launch (melf_ctx_last_dials): dict with 'family' (a name of DIALS_FAMILIES,
        None before the first launch), 'nr' (window rows a lane requests up front) and 'ws_max' (the context's largest window)."""
        (nr, fam, ws) = (C.c_int(0), C.c_int(0), C.c_int(0))
        check(self._L.melf_ctx_last_dials(self._h, C.byref(nr), C.byref(fam), C.byref(ws)))
        names = DIALS_FAMILIES + DIALS16_FAMILIES + DIALS10_FAMILIES + DIALS32_FAMILIES   # (the later families' values go on from the twelve's)
        return dict(family=names[fam.value] if fam.value >= 0 else None, nr=nr.value, ws_max=ws.value)

    def set_profiling(self, on):
        check(self._L.melf_ctx_set_profiling(self._h, int(on)))  # False/0 off, True/1 every kernel, 2 only k_match

    def files_stats(self, reset=True):
        """Host-time breakdown of the file-name calls since the last reset (include/meterelf_hip.h: melf_ctx_files_stats)."""
        out = np.zeros(10, np.float64)
        check(self._L.melf_ctx_files_stats(self._h, _ptr(out), 1 if reset else 0))
        keys = ('calls', 'files', 'ms_read', 'ms_turn_wait', 'ms_enqueue', 'ms_gpu_wait', 'io_threads', 'host_threads', 'cores', 'devices_in_process')
        return dict(zip(keys, (float(v) for v in out)))

    def timings(self):
        ms = np.zeros(K_COUNT, np.float64)
        cnt = np.zeros(K_COUNT, np.int64)
        check(self._L.melf_ctx_timings(self._h, _ptr(ms), _ptr(cnt)))
        return {self._L.melf_kernel_name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(K_COUNT)}


def _add_jpeg_switch(name, doc):
    def set_switch(self, on):
        check(getattr(self._L, 'melf_ctx_set_' + name)(self._h, int(bool(on))))

    def get_switch(self):
        on = C.c_int(0)
        check(getattr(self._L, 'melf_ctx_get_' + name)(self._h, C.byref(on)))
        return bool(on.value)
    set_switch.__doc__ = doc
    (set_switch.__name__, get_switch.__name__) = ('set_' + name, name)
    setattr(Context, 'set_' + name, set_switch)
    setattr(Context, name, get_switch)


for (_name, _flag, _doc) in JPEG_SWITCHES:
    _add_jpeg_switch(_name, _doc)


def _set_jpeg_long_scans(self, on, chapter_bytes=0):
    check(self._L.melf_ctx_set_jpeg_long_scans(self._h, int(bool(on)), int(chapter_bytes)))


def _jpeg_long_scans(self):
    (on, k) = (C.c_int(0), C.c_int(0))
    check(self._L.melf_ctx_get_jpeg_long_scans(self._h, C.byref(on), C.byref(k)))
    return bool(on.value)


def _jpeg_long_chapter_bytes(self):
    """The chapter length in force (melf_ctx_get_jpeg_long_scans): 4 091 904 in production."""
    (on, k) = (C.c_int(0), C.c_int(0))
    check(self._L.melf_ctx_get_jpeg_long_scans(self._h, C.byref(on), C.byref(k)))
    return int(k.value)


# the one switch with a second argument replaces the generic pair
_set_jpeg_long_scans.__doc__ = JPEG_SWITCHES[-1][2]
(_set_jpeg_long_scans.__name__, _jpeg_long_scans.__name__, _jpeg_long_chapter_bytes.__name__) = ('set_jpeg_long_scans', 'jpeg_long_scans', 'jpeg_long_chapter_bytes')
Context.set_jpeg_long_scans = _set_jpeg_long_scans
Context.jpeg_long_scans = _jpeg_long_scans
Context.jpeg_long_chapter_bytes = _jpeg_long_chapter_bytes
