"""MeterReader: the batched GPU engine behind the reference-shaped API.

One MeterReader owns one melf_ctx (one GPU).  Frames go in as uint8 BGR arrays
(N, H, W, 3); records come back as a numpy structured array (_hip.RESULT_DTYPE)
and are turned into the reference's dicts / exceptions by result_to_python().
"""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from . import _debug, _hip
from ._params import Params
from ._types import Rect
from .exceptions import (
    DialAngleDeterminingError, DialsNotFoundError, ImageProcessingError, NeedleContoursNotFoundError)


def load_template(params: Params) -> np.ndarray:
    """cv2.imread(dials_file, IMREAD_GRAYSCALE) (reference: meterelf/_image.py:72-81).

    A grey file is taken as it is.  For a colour file OpenCV 3.4 lets the file format's own library make the grey image:
    libpng for PNG (png_set_rgb_to_gray with 0.299 / 0.587: libpng 1.6 truncates them to the 15-bit coefficients 9797 / 19234 and
    gives blue the rest, 3737, and does NOT round the sum -- checked against libpng itself, tests/test_host_logic.py; palettes
    expanded to RGB first), libjpeg for JPEG (the decoder is asked for JCS_GRAYSCALE: the Y plane itself); every other format is
    decoded to BGR and goes through cvtColor's 14-bit weights (R 4899, G 9617, B 1868).  Pillow's convert('L') is none of
    these (other weights, truncation)."""
    from PIL import Image
    try:
        with Image.open(params.dials_file) as im:
            fmt = (im.format or '').upper()
            if im.mode == 'L':
                template = np.ascontiguousarray(np.asarray(im, dtype=np.uint8))
            elif im.mode == '1':
                template = np.ascontiguousarray(np.asarray(im.convert('L'), dtype=np.uint8))
            elif fmt == 'JPEG' and im.mode in ('RGB', 'YCbCr'):
                im.draft('L', im.size)      # libjpeg's grayscale output: the luma plane, no colour conversion
                template = np.ascontiguousarray(np.asarray(im.convert('L'), dtype=np.uint8))
            else:
                rgb = np.asarray(im.convert('RGB'), dtype=np.int64)
                (r, g, b) = (rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2])
                if fmt == 'PNG':
                    grey = (r * 9797 + g * 19234 + b * 3737) >> 15
                else:
                    grey = (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14
                template = np.ascontiguousarray(grey.astype(np.uint8))
    except Exception:
        raise IOError("Cannot read dials template: {}".format(params.dials_file))
    assert template.shape == params.dials_template_size
    return template


def make_blob(params: Params, meter_rect: Optional[Rect] = None) -> np.ndarray:
    return _hip.pack_blob(params.to_c(meter_rect), load_template(params))


def result_to_python(rec, dial_names: List[str], filename: str = '') -> Tuple[Dict[str, float], Optional[ImageProcessingError]]:
    """One record -> (meter_values dict, error) exactly as get_meter_value would
    return / raise (reference: meterelf/_reading.py:98-115, _image.py:62-64)."""
    status = int(rec['status'])
    if status == _hip.FRAME_OK:
        values = {name: float(rec['pos'][i]) for (i, name) in enumerate(dial_names)}
        if len(dial_names) == 4:
            values['value'] = float(rec['value'])
        return values, None
    if status == _hip.FRAME_DIALS_NOT_FOUND:
        return {}, DialsNotFoundError(filename, extra_info={'match val': float(rec['match_val'])})
    if status == _hip.FRAME_NEEDLE_CONTOURS_NOT_FOUND:
        return {}, NeedleContoursNotFoundError(extra_info={'dial': dial_names[int(rec['failed_dial'])]})
    if status == _hip.FRAME_ANGLE_UNDETERMINED:
        mask = int(rec['unreadable_mask'])
        bad = [name for (i, name) in enumerate(dial_names) if mask >> i & 1]
        extra_info = {}
        if _debug.DEBUG:
            # meterelf/_reading.py:98-104: the dials that WERE read, sorted by name, before 'unreadable dials'
            read = sorted((name, float(rec['pos'][i])) for (i, name) in enumerate(dial_names) if not mask >> i & 1)
            extra_info['dial positions'] = ' (' + ' | '.join('{}: {:.2f}'.format(k, v) for (k, v) in read) + ')'
        extra_info['unreadable dials'] = ', '.join(bad)
        return {}, DialAngleDeterminingError(filename, extra_info=extra_info)
    raise RuntimeError('unknown frame status {}'.format(status))


def records_to_python(records: np.ndarray, ok, dial_names: List[str], filenames: List[str]) -> list:
    """result_to_python over a whole record array: one (meter_values, error) per record, None where `ok[i]` is
    false.  The columns are converted to Python objects once per array instead of field by field per record
    (numpy scalar access costs more than everything else the API does per file)."""
    status = records['status'].tolist()
    pos = records['pos'][:, :len(dial_names)].tolist()
    value = records['value'].tolist()
    four = len(dial_names) == 4
    out: list = []
    for i in range(len(status)):
        if not ok[i]:
            out.append(None)
        elif status[i] == _hip.FRAME_OK:
            values = dict(zip(dial_names, pos[i]))
            if four:
                values['value'] = value[i]
            out.append((values, None))
        else:
            out.append(result_to_python(records[i], dial_names, filenames[i]))
    return out


def records_to_items(records: np.ndarray, ok, dial_names: List[str], filenames: List[str], make) -> list:
    """records_to_python fused with the construction of the API's result objects: make(filename, value, error,
    meter_values) per record, None where `ok[i]` is false.  The common case -- four dials, the frame read -- is ONE
    list comprehension over the columns (the per-file cost of get_meter_values is what bounds it on long lists)."""
    status = records['status'].tolist()
    value = records['value'].tolist()
    if len(dial_names) != 4:
        return [None if not o else make(f, mv.get('value'), err, mv)
                for (f, o, (mv, err)) in zip(filenames, ok, ((result_to_python(records[i], dial_names, filenames[i]) if ok[i] else ({}, None))
                                                             for i in range(len(status))))]
    (n0, n1, n2, n3) = dial_names
    (p0, p1, p2, p3) = (records['pos'][:, k].tolist() for k in range(4))
    good = _hip.FRAME_OK
    out = [make(f, v, None, {n0: a, n1: b, n2: c, n3: d, 'value': v}) if (o and s == good) else None
           for (f, o, s, v, a, b, c, d) in zip(filenames, ok, status, value, p0, p1, p2, p3)]
    for (i, item) in enumerate(out):
        if item is None and ok[i]:
            (mv, err) = result_to_python(records[i], dial_names, filenames[i])
            out[i] = make(filenames[i], mv.get('value'), err, mv)
    return out


class MeterReader:
    def __init__(self, params: Params, device: int = 0, blob: Optional[np.ndarray] = None, ctx: Optional['_hip.Context'] = None,
                 jpeg_orientation: bool = False, jpeg_progressive: bool = False, jpeg_samplings: bool = False,
                 jpeg_multiscan: bool = False, jpeg_default_tables: bool = False, jpeg_truncated: bool = False,
                 jpeg_long_scans: bool = False) -> None:
        """jpeg_long_scans: the read_jpeg_* methods decode baseline JPEG files without restart markers whose entropy-coded data exceed 4 MB
        (12 MP and larger snapshots at high quality) on the GPU, chapter by chapter, byte for byte like libjpeg, instead of leaving them
        to the caller's host decoder, which is the default.
        jpeg_truncated: the read_jpeg_* methods complete a baseline JPEG file whose bytes stop inside the scan (a snapshot still being
        written, an upload that lost its connection) as libjpeg does -- the MCU in progress from zero bits, mid grey behind it -- instead
        of handing it back as undecodable, which is the default.
        jpeg_default_tables: the read_jpeg_* methods decode sequential JPEG files that leave Huffman tables 0 / 1 out (Motion-JPEG frames of
        UVC webcams and AVI MJPG streams: no DHT segment) with the T.81 Annex K tables, as libjpeg-turbo does, instead of leaving them to
        the caller's host decoder, which is the default.
        jpeg_multiscan: the read_jpeg_* methods decode sequential JPEG files sent as three scans of one component each on the GPU, byte
        for byte like libjpeg, instead of leaving them to the caller's host decoder, which is the default.
        jpeg_samplings: the read_jpeg_* methods decode YCbCr 4:4:0 and 4:1:1 JPEG files (a losslessly rotated 4:2:2 file; DV-derived
        encoders) on the GPU, byte for byte like libjpeg, instead of leaving them to the caller's host decoder, which is the default.
        jpeg_progressive: the read_jpeg_* methods decode progressive JPEG files (the subset include/meterelf_hip.h states) on the
        GPU instead of leaving them to the caller's host decoder, which is the default.
        jpeg_orientation: the read_jpeg_* methods decode JPEG files that carry an EXIF orientation 2..8 on the GPU, upright (as
        cv2.imread returns them), instead of leaving them to the caller's host decoder (None / ok false), which is the default."""
        self.params = params
        self.device = device
        self.dial_names = params.dial_names
        self.blob = blob if blob is not None else make_blob(params)
        self.ctx = ctx if ctx is not None else _hip.Context(self.blob, device)   # ctx: created elsewhere from the same blob (broadcast)
        self._crop_ctx: Dict[Tuple[int, int], _hip.Context] = {}
        self._begun: list = []      # read_jpeg_paths_begin: path lists in flight, oldest first
        self._collected: list = []  # their results taken out of the library early (drain_jpeg_paths), oldest first
        asked = dict(jpeg_orientation=jpeg_orientation, jpeg_progressive=jpeg_progressive, jpeg_samplings=jpeg_samplings,
                     jpeg_multiscan=jpeg_multiscan, jpeg_default_tables=jpeg_default_tables, jpeg_truncated=jpeg_truncated,
                     jpeg_long_scans=jpeg_long_scans)
        for (name, _flag, _doc) in _hip.JPEG_SWITCHES:      # the attribute jpeg_<switch>: what the context was last told
            setattr(self, name, False)
            if asked[name]:
                self._set_jpeg_switch(name, True)

    def _set_jpeg_switch(self, name: str, on: bool) -> None:
        getattr(self.ctx, 'set_' + name)(on)
        setattr(self, name, bool(on))

    def set_jpeg_long_scans(self, on: bool, chapter_bytes: int = 0) -> None:
        """The switch of the constructor's jpeg_long_scans, on a reader with nothing in flight (melf_ctx_set_jpeg_long_scans);
        chapter_bytes > 0, for tests and tuning, chooses the chapter length."""
        self.ctx.set_jpeg_long_scans(on, chapter_bytes)
        self.jpeg_long_scans = bool(on)

    def set_jpeg_truncated(self, on: bool) -> None:
        """The switch of the constructor's jpeg_truncated, on a reader with nothing in flight (melf_ctx_set_jpeg_truncated)."""
        self._set_jpeg_switch('jpeg_truncated', on)

    def set_jpeg_multiscan(self, on: bool) -> None:
        """The switch of the constructor's jpeg_multiscan, on a reader with nothing in flight (melf_ctx_set_jpeg_multiscan)."""
        self._set_jpeg_switch('jpeg_multiscan', on)

    def set_jpeg_default_tables(self, on: bool) -> None:
        """The switch of the constructor's jpeg_default_tables, on a reader with nothing in flight (melf_ctx_set_jpeg_default_tables)."""
        self._set_jpeg_switch('jpeg_default_tables', on)

    def set_jpeg_samplings(self, on: bool) -> None:
        """The switch of the constructor's jpeg_samplings, on a reader with nothing in flight (melf_ctx_set_jpeg_samplings)."""
        self._set_jpeg_switch('jpeg_samplings', on)

    def set_jpeg_progressive(self, on: bool) -> None:
        """The switch of the constructor's jpeg_progressive, on a reader with nothing in flight (melf_ctx_set_jpeg_progressive)."""
        self._set_jpeg_switch('jpeg_progressive', on)

    def set_jpeg_orientation(self, on: bool) -> None:
        """The switch of the constructor's jpeg_orientation, on a reader with nothing in flight (melf_ctx_set_jpeg_orientation)."""
        self._set_jpeg_switch('jpeg_orientation', on)

    def close(self) -> None:
        self.ctx.close()
        for c in self._crop_ctx.values():
            c.close()
        self._crop_ctx.clear()

    def read_frames(self, frames: np.ndarray) -> np.ndarray:
        """Full camera frames (N, H, W, 3) BGR -> records."""
        return self.ctx.process_batch(frames)

    def _read_view(self, v, out, host_call, dev_call):
        """What the read_*_frames methods share once the frames are described (v: a *FramesView): host frames -> host_call();
        frames on this reader's GPU -> dev_call(...) on torch.cuda.current_stream, the records into out where one is given."""
        if not v.on_device:
            if out is not None:
                raise ValueError('out= takes the records of device frames only')
            return host_call()
        import torch
        if v.device != self.device:
            raise ValueError('frames are on cuda:%s, the reader on cuda:%d' % (v.device, self.device))
        stream = torch.cuda.current_stream(self.device)
        if out is None:
            return dev_call(stream=stream.cuda_stream)
        if (not _hip._is_torch(out) or out.dtype != torch.uint8 or out.device != v.array.device or not out.is_contiguous()
                or tuple(out.shape) != (v.n, _hip.RESULT_DTYPE.itemsize)):
            raise ValueError('out must be a contiguous uint8 tensor of shape (%d, %d) on %s' % (v.n, _hip.RESULT_DTYPE.itemsize, v.array.device))
        if v.copied:
            v.array.record_stream(stream)   # the packed copy lives until the stream has passed the call's kernels
        dev_call(d_results_ptr=out.data_ptr(), want_host=False, stream=stream.cuda_stream)
        return out

    def read_frame_views(self, frames, pixel_format: str = 'bgr', out=None):
        """Full camera frames in the layout the caller has -> records, equal to read_frames() of the packed BGR frames made from
        them (melf_process_frames*).  frames: (N, H, W, C) uint8, a numpy array / torch CPU tensor (host path) or a torch tensor
        on this reader's GPU (enqueued on torch.cuda.current_stream); pixel_format 'bgr', 'rgb' (C = 3), 'bgra', 'rgba' (C = 4,
        the 4th byte ignored); padded rows and frames and rgba[..., :3]-style views are read in place (_hip.frames_view).
        out: a uint8 device tensor (N, RESULT_DTYPE.itemsize) on the same GPU that receives the records without synchronising
        the stream (device frames only); returns it.  Otherwise returns the records.
        Channels-first (N, C, H, W) frames: read_planar_frames reads them in place; a permuted view of them is copied here."""
        v = _hip.frames_view(frames, pixel_format)
        geom = (v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride)
        return self._read_view(v, out, lambda: self.ctx.process_frames(v.ptr, *geom),
                               lambda **kw: self.ctx.process_frames_dev(v.ptr, *geom, **kw))

    def read_yuv_frames(self, frames, pixel_format: str = 'nv12', matrix='bt601', out=None):
        """YUV 4:2:0 video frames -> records, equal to read_frames() of the packed BGR frames that the integer conversion of
        include/meterelf_hip.h makes of them under `matrix` (melf_process_yuv*); the planes are read in place, no conversion pass.
        matrix: what the frames are encoded with, a name of _hip.YUV_MATRIX_CODES or a code -- 'bt709' for H.264 / HEVC of an HD IP
        camera as a hardware decoder leaves it in NV12; 'bt601-full' for MJPEG webcams and phone cameras decoded by ffmpeg (yuvj420p)
        or delivered raw over UVC; 'bt709-full' for screen and capture pipelines; 'bt601' (the default: limited range, what
        cv2.cvtColor(COLOR_YUV2BGR_NV12) assumes).  The wrong matrix shifts hue and lightness, which is what the dials are read from.
        frames: the conventional (N, H * 3 // 2, W) uint8 array, a numpy array / torch CPU tensor (host path) or a torch tensor on
        this reader's GPU (enqueued on torch.cuda.current_stream); pixel_format 'nv12', 'i420' or 'yv12' (_hip.yuv_frames_view says
        which layouts are read in place).  out: a uint8 device tensor (N, RESULT_DTYPE.itemsize) on the same GPU that receives the
        records without synchronising the stream (device frames only); returns it.  Otherwise returns the records."""
        v = _hip.yuv_frames_view(frames, pixel_format, matrix)
        desc = v.descriptor()
        return self._read_view(v, out, lambda: self.ctx.process_yuv(v.ptr, desc), lambda **kw: self.ctx.process_yuv_dev(v.ptr, desc, **kw))

    def read_yuv422_frames(self, frames, pixel_format: str = 'yuyv', matrix='bt601', out=None):
        """Packed YUV 4:2:2 frames (UVC / V4L2 YUYV, capture-card UYVY, YVYU) -> records, equal to read_frames() of the packed BGR
        frames that the integer conversion of include/meterelf_hip.h makes of them under `matrix` (melf_process_yuv422*); the
        macropixels are read in place, no conversion pass.  matrix as for read_yuv_frames: 'bt601-full' for MJPEG webcams and phone
        cameras (ffmpeg's yuvj422p, raw UVC), 'bt709' for HD capture cards and decoders, 'bt709-full' for screen and capture
        pipelines, 'bt601' (the default) limited range as cv2 assumes.  frames: the conventional (N, H, W, 2) uint8 array, a numpy
        array / torch CPU tensor (host path) or a torch tensor on this reader's GPU (enqueued on torch.cuda.current_stream); pixel_format
        'yuyv' (or 'yuy2'), 'uyvy' or 'yvyu' (_hip.yuv422_frames_view says which layouts are read in place).  out: a uint8 device
        tensor (N, RESULT_DTYPE.itemsize) on the same GPU that receives the records without synchronising the stream (device
        frames only); returns it.  Otherwise returns the records."""
        v = _hip.yuv422_frames_view(frames, pixel_format, matrix)
        desc = v.descriptor()
        return self._read_view(v, out, lambda: self.ctx.process_yuv422(v.ptr, desc), lambda **kw: self.ctx.process_yuv422_dev(v.ptr, desc, **kw))

    def read_yuv_planar_frames(self, frames, pixel_format: str = 'i422', matrix='bt601', out=None):
        """Planar and semi-planar YUV frames of the other chroma subsamplings -- 4:2:2 as software MJPEG decoders leave a webcam's
        frames ('i422': ffmpeg's yuv422p / yuvj422p; 'yv16'; 'nv16' / 'nv61' of Rockchip and V4L2 decoders), 4:4:4 of screen capture
        and high-quality JPEG ('i444', 'yv24', 'nv24', 'nv42'), 4:4:0 ('i440'), and Android's 'nv21' -- -> records, equal to
        read_frames() of the packed BGR frames that the integer conversion of include/meterelf_hip.h makes of them under `matrix`
        with the nearest chroma sample (melf_process_yuv_planar*); the planes are read in place, no conversion pass.  'nv12', 'i420'
        and 'yv12' are taken too and give read_yuv_frames' records.  matrix as for read_yuv_frames ('bt601-full' for yuvj422p /
        yuvj444p).  frames: the raw-video (N, rows, W) uint8 array, rows = 2 H (4:2:2, 4:4:0), 3 H (4:4:4) or 3 H / 2 (4:2:0), for
        'i444' / 'yv24' also (N, 3, H, W); a numpy array / torch CPU tensor (host path) or a torch tensor on this reader's GPU
        (enqueued on torch.cuda.current_stream); _hip.yuv_planar_frames_view says which layouts are read in place.  out: a uint8
        device tensor (N, RESULT_DTYPE.itemsize) on the same GPU that receives the records without synchronising the stream (device
        frames only); returns it.  Otherwise returns the records."""
        v = _hip.yuv_planar_frames_view(frames, pixel_format, matrix)
        desc = v.descriptor()
        return self._read_view(v, out, lambda: self.ctx.process_yuv_planar(v.ptr, desc),
                               lambda **kw: self.ctx.process_yuv_planar_dev(v.ptr, desc, **kw))

    def read_yuv16_frames(self, frames, pixel_format: str, matrix, out=None):
        """Planar and semi-planar YUV frames of 10, 12 or 16 bits per sample -- 'p010' as a hardware HEVC / AV1 Main10 decoder leaves
        a camera stream, 'i010' / 'yuv420p10le' as ffmpeg's software decoders do, 'p210' / 'p216' of capture cards, the 12- and 16-bit
        and 4:2:2 siblings (_hip.YUV16_FORMATS) -- -> records, equal to read_yuv_planar_frames() of the 8-bit frames whose samples are
        min(s >> shift, 255), the format's shift dropping the low bits (melf_process_yuv16*); the 16-bit planes are read in place, no
        reduction or conversion pass.  matrix has no default: nearly all 10-bit material is 'bt709', and the wrong matrix raises no
        error -- it shifts hue and lightness, which is what the dials are read from.  frames: the raw-video (N, rows, W) array of
        uint16, rows = 3 H / 2 (4:2:0) or 2 H (4:2:2): a numpy array / torch CPU tensor (host path) or a torch tensor on this
        reader's GPU (enqueued on torch.cuda.current_stream), torch.uint16 where the installed torch has it, or torch.int16 holding
        the same bits; _hip.yuv16_frames_view says which layouts are read in place.  out: a uint8 device tensor (N,
        RESULT_DTYPE.itemsize) on the same GPU that receives the records without synchronising the stream (device frames only);
        returns it.  Otherwise returns the records."""
        v = _hip.yuv16_frames_view(frames, pixel_format, matrix)
        desc = v.descriptor()
        return self._read_view(v, out, lambda: self.ctx.process_yuv16(v.ptr, desc),
                               lambda **kw: self.ctx.process_yuv16_dev(v.ptr, desc, **kw))

    def read_yuv422_10_frames(self, frames, pixel_format: str, matrix, width=None, out=None):
        """Packed 10-bit YUV 4:2:2 frames -- 'v210', the native 10-bit format of SDI / HDMI capture cards, or 'y210' / 'y212' / 'y216'
        as hardware 4:2:2 10-bit decoders leave them (_hip.YUV422_10_FORMATS) -- -> records, equal to read_yuv422_frames() of the 8-bit
        YUYV frames whose samples are the top 8 bits of each sample (melf_process_yuv422_10*); the packed frames are read in place, no
        unpack pass.  matrix has no default, as for read_yuv16_frames.  frames: 'v210' (N, H, row_words) of uint32 with width= the
        frames' width in pixels (required); 'y21x' (N, H, W, 2) of uint16: a numpy array / torch CPU tensor (host path) or a torch
        tensor on this reader's GPU (enqueued on torch.cuda.current_stream), torch.int32 / torch.int16 holding the same bits where the
        installed torch has no unsigned type; _hip.yuv422_10_frames_view says which layouts are read in place.  out: a uint8 device
        tensor (N, RESULT_DTYPE.itemsize) on the same GPU that receives the records without synchronising the stream (device frames
        only); returns it.  Otherwise returns the records."""
        v = _hip.yuv422_10_frames_view(frames, pixel_format, matrix, width)
        desc = v.descriptor()
        return self._read_view(v, out, lambda: self.ctx.process_yuv422_10(v.ptr, desc),
                               lambda **kw: self.ctx.process_yuv422_10_dev(v.ptr, desc, **kw))

    def read_packed32_frames(self, frames, pixel_format: str, matrix=None, out=None):
        """4:4:4 frames of one 32-bit word per pixel -- 'vuya' / 'ayuv' / 'uyva' (8-bit), 'y410' / 'xv30' / 'v30x' (10-bit YUV) as
        hardware 4:4:4 decoders deliver them, 'x2rgb10' / 'x2bgr10' (10-bit RGB) as scan-out, desktop duplication and camera ISPs do
        (_hip.PACKED32_FORMATS) -- -> records, equal to read_yuv_planar_frames() of the 8-bit 'i444' frames whose samples are the top
        8 bits of each field (YUV), or to read_frames() of the BGR frames of those (RGB) (melf_process_packed32*); the words are read
        in place, no unpack pass.  matrix is required for the YUV formats (no default, as for read_yuv16_frames) and must be None for
        the RGB ones.  frames: (N, H, W) of uint32, or (N, H, W, 4) of uint8 for the byte formats: a numpy array / torch CPU tensor
        (host path) or a torch tensor on this reader's GPU (enqueued on torch.cuda.current_stream), torch.int32 holding the same bits
        where the installed torch has no unsigned type; _hip.packed32_frames_view says which layouts are read in place.  out: a uint8
        device tensor (N, RESULT_DTYPE.itemsize) on the same GPU that receives the records without synchronising the stream (device
        frames only); returns it.  Otherwise returns the records."""
        v = _hip.packed32_frames_view(frames, pixel_format, matrix)
        desc = v.descriptor()
        return self._read_view(v, out, lambda: self.ctx.process_packed32(v.ptr, desc),
                               lambda **kw: self.ctx.process_packed32_dev(v.ptr, desc, **kw))

    def read_planar_frames(self, frames, channel_order: str = 'rgb', out=None):
        """Planar, channels-first frames (N, 3, H, W) / (N, 4, H, W) uint8 -> records, equal to read_frames() of the packed BGR
        frames with the same samples (melf_process_planes*); the planes are read in place, no interleaved copy is made.  frames: a
        numpy array / torch CPU tensor (host path) or a torch tensor on this reader's GPU (enqueued on torch.cuda.current_stream);
        channel_order names the planes present: 'rgb', 'bgr', 'gbr', 'rgba', 'rgbx', 'bgra' or 'bgrx' (_hip.planar_frames_view says
        which layouts are read in place).  out: a uint8 device tensor (N, RESULT_DTYPE.itemsize) on the same GPU that receives the
        records without synchronising the stream (device frames only); returns it.  Otherwise returns the records."""
        v = _hip.planar_frames_view(frames, channel_order)
        desc = v.descriptor()
        return self._read_view(v, out, lambda: self.ctx.process_planes(v.ptr, desc), lambda **kw: self.ctx.process_planes_dev(v.ptr, desc, **kw))

    def read_wide_frames(self, frames, layout: str, channel_order: str = 'rgb', scale=None, offset=None, rounding: str = 'nearest',
                         shift=None, out=None):
        """RGB frames of wide samples -- uint16 (RGB16 / BGR12 of machine-vision SDKs, ffmpeg's rgb48le / gbrp10le .., decoded 16-bit
        PNG and TIFF) or float16, bfloat16, float32 (the image tensors of a torch program, often still under a Normalize(mean, std))
        -- -> records, equal to read_frame_views() (layout 'hwc': (N, H, W, C)) or read_planar_frames() (layout 'chw': (N, C, H, W))
        of the 8-bit frames whose samples are the narrowed ones (melf_process_wide*; _hip.narrow_wide restates the rule in numpy);
        only the meter_rect crop of the wide frames is read, in place, and no 8-bit frame is formed.  Integer frames: shift is required
        and has no default -- min(s >> shift, 255): 8 for full 16-bit and MSB-aligned samples, 4 for 12 bits and 2 for 10 bits in the
        low bits; torch.int16 holding the same bits is taken.  Float frames: shift must be None; the byte is
        round(x * scale + offset) in float32, two roundings, clipped to 0 .. 255 (NaN: 0); scale and offset a scalar or three values
        in the order of channel_order, defaults 255 and 0; scale = std * 255, offset = mean * 255 undoes a Normalize; rounding
        'nearest' (ties to even, torch.round) or 'floor' (with scale 255.999: torchvision's convert_image_dtype; with 255:
        .mul(255).byte()).  The wrong choice raises no error: it moves samples by one, and with them what the dials are read from.
        frames: a numpy array / torch CPU tensor (host path: the host threads narrow the crop while they stage it) or a torch tensor
        on this reader's GPU (enqueued on torch.cuda.current_stream); strided views -- a channel slice of a 4-channel tensor, a
        spatial crop -- are read in place when their strides fit (_hip.wide_frames_view), anything else is a ValueError before the
        library is called.  out: a uint8 device tensor (N, RESULT_DTYPE.itemsize) on the same GPU that receives the records without
        synchronising the stream (device frames only); returns it.  Otherwise returns the records."""
        v = _hip.wide_frames_view(frames, layout, channel_order, scale, offset, rounding, shift)
        desc = v.descriptor()
        return self._read_view(v, out, lambda: self.ctx.process_wide(v.ptr, desc), lambda **kw: self.ctx.process_wide_dev(v.ptr, desc, **kw))

    # layout of read_frame_list: (the batch method's view function, whether it takes a matrix and with which default)
    _LIST_VIEWS = {
        'views': ('frames_view', None), 'yuv': ('yuv_frames_view', 'bt601'), 'yuv422': ('yuv422_frames_view', 'bt601'),
        'yuv_planar': ('yuv_planar_frames_view', 'bt601'), 'yuv16': ('yuv16_frames_view', ''), 'yuv422_10': ('yuv422_10_frames_view', ''),
        'packed32': ('packed32_frames_view', ''), 'planar': ('planar_frames_view', None),
    }

    def read_frame_list(self, frames, layout: str, pixel_format: str, matrix=None, width=None, out=None):
        """Frames in separate allocations -- the surfaces of a decoder's pool, a list of tensors from a video reader -- -> records,
        equal to the batch method's on one array holding the same frames in list order (melf_process_frame_list*), without the
        torch.stack or the copies that would make that array: one kernel gathers the meter crop's rows of every frame, and only
        those, into a staged batch which the reading kernels take.  layout names the family by its batch method: 'views'
        (read_frame_views), 'yuv' (read_yuv_frames), 'yuv422', 'yuv_planar', 'yuv16', 'yuv422_10', 'packed32', 'planar'
        (read_planar_frames; pixel_format is its channel_order); pixel_format, matrix and width are that method's, with its defaults.
        frames: a sequence whose elements each have the shape of ONE frame of that method's array (the documented shape without
        the leading N): numpy arrays / torch CPU tensors (host path), or torch tensors on this reader's GPU (enqueued on
        torch.cuda.current_stream).  Every element is described by the method's _hip.*_frames_view as frame[None]; all must agree
        in everything but the address.  ValueError: host and device elements mixed, an element on another device, elements that
        differ (the message says which and in what), an element the view would have to copy (a layout the descriptor cannot
        express).  out: as for the batch methods, a uint8 device tensor (len(frames), RESULT_DTYPE.itemsize)."""
        if layout not in self._LIST_VIEWS:
            raise ValueError('layout %r is none of %s' % (layout, ', '.join(sorted(self._LIST_VIEWS))))
        (view_name, default_matrix) = self._LIST_VIEWS[layout]
        args = [pixel_format]
        if default_matrix is not None:
            args.append(matrix if matrix is not None or default_matrix == '' else default_matrix)
        elif matrix is not None:
            raise ValueError('layout %r takes no matrix' % layout)
        if layout == 'yuv422_10':
            args.append(width)
        elif width is not None:
            raise ValueError('layout %r takes no width' % layout)
        frames = list(frames)
        views = []
        for (i, f) in enumerate(frames):
            if not (_hip._is_torch(f) or isinstance(f, np.ndarray)):
                f = np.asarray(f)
            v = getattr(_hip, view_name)(f[None], *args)
            if v.copied:
                raise ValueError('frame %d of the list has a layout the %r descriptor cannot express (it would have to be copied)' % (i, layout))
            if views:
                if v.on_device != views[0].on_device:
                    raise ValueError('frame %d of the list is in %s memory, frame 0 in %s memory' % ((i,) + tuple(
                        'device' if w.on_device else 'host' for w in (v, views[0]))))
                for name in v._fields:
                    if name not in ('ptr', 'array', 'on_device') and getattr(v, name) != getattr(views[0], name):
                        raise ValueError('frame %d of the list differs from frame 0 in %s: %r, not %r' % (i, name, getattr(v, name), getattr(views[0], name)))
            views.append(v)
        n = len(views)
        if n == 0:
            return out if out is not None else np.zeros(0, _hip.RESULT_DTYPE)
        v0 = views[0]
        desc = v0.descriptor() if hasattr(v0, 'descriptor') else _hip.MelfFrames(v0.pixel_format, 1, v0.H, v0.W, v0.row_pitch, v0.frame_stride)
        desc.n = n
        ptrs = [v.ptr for v in views]
        return self._read_view(v0._replace(n=n), out, lambda: self.ctx.process_frame_list(layout, desc, ptrs),
                               lambda **kw: self.ctx.process_frame_list_dev(layout, desc, ptrs, **kw))

    def read_oriented_frames(self, frames, layout: str, pixel_format: str, orientation, matrix=None, out=None):
        """Frames that are stored rotated or mirrored -- the raw frames of a camera mounted on its side, video whose rotation sits
        in the container's display matrix -- -> records, equal to the batch method's on the upright frames a viewer shows (what
        cv2.imread makes of a file with that EXIF orientation), without the torch.rot90(frames, ..).contiguous() or flip that
        would make them (melf_process_oriented*): one kernel writes the meter crop of every frame upright into a staged batch,
        reading only the crop's samples.  frames: the STORED batch, in the shape the layout's own batch method documents; layout,
        pixel_format and matrix resolve as in read_frame_list ('views', 'yuv', 'yuv_planar', 'yuv16', 'packed32', 'planar'; the
        packed 4:2:2 layouts cannot be oriented in place).  orientation: the EXIF code 1 .. 8 or its name -- 'normal', 'mirror',
        'rot180', 'flip', 'transpose', 'rot90cw', 'transverse', 'rot90ccw'; a stream's "rotate 90 / 180 / 270 degrees clockwise to
        display" is 'rot90cw' / 'rot180' / 'rot90ccw'.  The meter_rect is taken on the upright frame.  numpy arrays / torch CPU
        tensors take the host path, torch tensors on this reader's GPU are enqueued on torch.cuda.current_stream; out: as for the
        batch methods.  ValueError: an unknown orientation, a layout or chroma subsampling that cannot be oriented (codes 5 .. 8
        need sub_x == sub_y), a view that would have to copy."""
        if layout not in self._LIST_VIEWS:
            raise ValueError('layout %r is none of %s' % (layout, ', '.join(sorted(self._LIST_VIEWS))))
        if layout in ('yuv422', 'yuv422_10'):
            raise ValueError('layout %r cannot be oriented in place: a mirrored macropixel is not a permutation of equal-sized elements' % layout)
        code = _hip.ORIENTATIONS.get(orientation.lower()) if isinstance(orientation, str) else orientation
        if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or not 1 <= code <= 8:
            raise ValueError('orientation %r is none of 1 .. 8 or %s' % (orientation, ', '.join(_hip.ORIENTATIONS)))
        code = int(code)
        (view_name, default_matrix) = self._LIST_VIEWS[layout]
        args = [pixel_format]
        if default_matrix is not None:
            args.append(matrix if matrix is not None or default_matrix == '' else default_matrix)
        elif matrix is not None:
            raise ValueError('layout %r takes no matrix' % layout)
        v = getattr(_hip, view_name)(frames, *args)
        if v.copied:
            raise ValueError('the frames have a layout the %r descriptor cannot express (they would have to be copied)' % layout)
        desc = v.descriptor() if hasattr(v, 'descriptor') else _hip.MelfFrames(v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride)
        if code >= 5:
            (sx, sy) = (getattr(desc, 'sub_x', 1), getattr(desc, 'sub_y', 1)) if layout in ('yuv_planar', 'yuv16') else (1, 1)
            if sx != sy:
                raise ValueError('orientation %r transposes the frame: %r chroma is not subsampled alike in both directions' % (orientation, pixel_format))
        return self._read_view(v, out, lambda: self.ctx.process_oriented(layout, desc, code, v.ptr),
                               lambda **kw: self.ctx.process_oriented_dev(layout, desc, code, v.ptr, **kw))

    _PLANE_LAYOUTS = ('yuv', 'yuv_planar', 'yuv16', 'planar')

    class _PlaneListView(NamedTuple):
        """What _read_view looks at, for a list of planes"""
        on_device: bool
        device: Optional[int]
        n: int
        array: object
        copied: bool = False

    @staticmethod
    def _plane_list_format(layout, pixel_format, matrix):
        """(bytes per sample, sub_x, sub_y, interleaved, V first, shift, matrix code) of a format name of the layout's batch method"""
        fmt = str(pixel_format).lower()
        if layout == 'planar':
            if matrix is not None:
                raise ValueError("layout 'planar' takes no matrix")
            if fmt not in ('rgb', 'bgr', 'gbr'):
                raise ValueError("channel_order %r does not name three planes (rgb, bgr, gbr)" % (pixel_format,))
            return (1, 0, 0, False, False, 0, 0)
        if layout == 'yuv16':
            mcode = _hip.yuv_matrix_code(matrix)
            if fmt not in _hip.YUV16_FORMATS:
                raise ValueError('pixel_format %r is not a 16-bit planar / semi-planar YUV layout (%s)' % (pixel_format, ', '.join(_hip.YUV16_FORMATS)))
            (sy, step, vfirst, shift) = _hip.YUV16_FORMATS[fmt]
            return (2, 1, sy, step == 2, vfirst, shift, mcode)
        mcode = _hip.yuv_matrix_code('bt601' if matrix is None else matrix)
        if layout == 'yuv':
            if fmt not in _hip.YUV_CODES:
                raise ValueError('pixel_format %r is not a YUV 4:2:0 layout (nv12, i420, yv12)' % (pixel_format,))
            return (1, 1, 1, fmt == 'nv12', fmt == 'yv12', 0, mcode)
        if fmt not in _hip.YUV_PLANAR_FORMATS:
            raise ValueError('pixel_format %r is not a planar / semi-planar YUV layout (%s)' % (pixel_format, ', '.join(_hip.YUV_PLANAR_FORMATS)))
        (sx, sy, step, vfirst) = _hip.YUV_PLANAR_FORMATS[fmt]
        return (1, sx, sy, step == 2, vfirst, 0, mcode)

    def read_plane_list(self, frames, layout: str, pixel_format: str, matrix=None, out=None):
        """Frames whose PLANES lie in separate allocations -- libav's AVFrame (data[0..2], linesize[0..2]), V4L2 multi-planar capture
        (NV12M: one buffer per plane), (y, uv) or (r, g, b) held as separate tensors -- -> records, equal to the batch method's on one
        array holding the same samples in list order (melf_process_plane_list*), without concatenating any frame's planes: one kernel
        gathers the meter crop's rows of every plane, and only those, into a staged batch which the reading kernels take.
        layout: 'yuv' (read_yuv_frames), 'yuv_planar', 'yuv16' or 'planar' (read_planar_frames; pixel_format is its channel_order,
        'rgb', 'bgr' or 'gbr'); pixel_format and matrix are that method's, with its defaults.
        frames: a sequence of tuples of 2-D planes, in the order in which the format name stores them (cutting one frame of the batch
        method's array at its plane boundaries yields the tuple): 'i420' (Y, U, V); 'yv12' / 'yv16' / 'yv24' (Y, V, U); 'nv12' /
        'nv21' / 'p010' and the like (Y, C), C the interleaved plane of shape (Hc, Wc * 2) or (Hc, Wc, 2); 'planar': the three planes
        in channel_order.  A plane is a numpy array / torch CPU tensor (host path) or a torch tensor on this reader's GPU (enqueued on
        torch.cuda.current_stream): uint8, or uint16 / int16 for 'yuv16'; its elements contiguous along the last axis, any row stride.
        All Y planes share one pitch, all chroma planes (U and V alike) another; R, G and B share theirs.  ValueError, naming frame,
        plane and field: a wrong plane count, host and device planes mixed, a plane on another device, differing pitches or shapes,
        shapes that are not the format's subsampling, a plane that would have to be copied.  out: as for the batch methods, a uint8
        device tensor (len(frames), RESULT_DTYPE.itemsize)."""
        if layout not in self._PLANE_LAYOUTS:
            raise ValueError('layout %r is none of %s' % (layout, ', '.join(self._PLANE_LAYOUTS)))
        (bps, sx, sy, semi, vfirst, shift, mcode) = self._plane_list_format(layout, pixel_format, matrix)
        nplanes = 2 if semi else 3
        frames = list(frames)
        n = len(frames)
        if n == 0:
            return out if out is not None else np.zeros(0, _hip.RESULT_DTYPE)
        # tuple position -> plane slot of the C ABI (Y, U or interleaved chroma, V; B, G, R)
        if layout == 'planar':
            order = str(pixel_format).lower()
            slot_of = [('bgr').index(ch) for ch in order]
        else:
            slot_of = [0, 2, 1] if (vfirst and not semi) else list(range(nplanes))
        pitch_name = ['row_pitch'] * 3 if layout == 'planar' else ['y_pitch', 'c_pitch', 'c_pitch']
        first = None          # frame 0's views by slot
        table = []
        alive = []            # every plane's view (and with it the array its address points into, a converted one included)
        for (i, planes) in enumerate(frames):
            planes = tuple(planes) if isinstance(planes, (tuple, list)) else (planes,)
            if len(planes) != nplanes:
                raise ValueError('frame %d of the list has %d planes, %r / %r frames have %d' % (i, len(planes), layout, pixel_format, nplanes))
            views = [None] * nplanes
            for (k, p) in enumerate(planes):
                if not (_hip._is_torch(p) or isinstance(p, np.ndarray)):
                    p = np.asarray(p)
                try:
                    views[slot_of[k]] = (k, _hip.plane_view(p, bps))
                except ValueError as e:
                    raise ValueError('frame %d, plane %d of the list: %s' % (i, k, e)) from None
            if first is None:
                first = views
                (H, W) = (first[0][1].rows, first[0][1].row_bytes // bps)
                if (sx and W % 2) or (sy and H % 2):
                    raise ValueError('frame 0, plane 0 of the list: shape (%d, %d) is odd where %r subsamples the chroma' % (H, W, pixel_format))
                crows = H >> sy
                cbytes = (W >> sx) * (2 if semi else 1) * bps
                want_shape = [(H, W * bps)] + [(crows, cbytes)] * (nplanes - 1) if layout != 'planar' else [(H, W)] * 3
            for (slot, (k, v)) in enumerate(views):
                where = 'frame %d, plane %d of the list' % (i, k)
                (k0, v0) = first[0]
                if v.on_device != v0.on_device:
                    raise ValueError('%s is in %s memory, frame 0, plane %d in %s memory' % (
                        where, 'device' if v.on_device else 'host', k0, 'device' if v0.on_device else 'host'))
                if v.device != v0.device:
                    raise ValueError('%s is on cuda:%s, frame 0, plane %d on cuda:%s' % (where, v.device, k0, v0.device))
                if (v.rows, v.row_bytes) != want_shape[slot]:
                    raise ValueError('%s differs in shape: %d rows of %d bytes, not the %d rows of %d bytes that %r frames of %d x %d have' % (
                        where, v.rows, v.row_bytes, want_shape[slot][0], want_shape[slot][1], pixel_format, W, H))
                if not v.in_place:
                    raise ValueError('%s has a layout the descriptor cannot express (it would have to be copied): its elements must be '
                                     'contiguous along the last axis and its rows a non-negative stride apart' % where)
                ref = first[1 if slot == 2 else slot][1] if layout != 'planar' else first[0][1]
                if v.pitch != ref.pitch:
                    raise ValueError('%s differs in %s: %d, not %d' % (where, pitch_name[slot], v.pitch, ref.pitch))
                table.append(v.ptr)
                alive.append(v)
        (y_pitch, c_pitch) = (first[0][1].pitch, first[1][1].pitch)
        if layout == 'planar':
            desc = _hip.MelfPlanarFrames(n, H, W, 0, 0, 0, 0, y_pitch, 0)
        else:
            (u_off, v_off) = ((bps, 0) if vfirst else (0, bps)) if semi else (0, 0)
            if layout == 'yuv':
                desc = _hip.MelfYuvFrames(_hip.YUV_NV12 if semi else _hip.YUV_I420, mcode, n, H, W, 0, y_pitch, c_pitch, u_off, v_off, 0)
            elif layout == 'yuv_planar':
                desc = _hip.MelfYuvPlanarFrames(mcode, n, H, W, sx, sy, 2 if semi else 1, 0, y_pitch, c_pitch, u_off, v_off, 0)
            else:
                desc = _hip.MelfYuv16Frames(mcode, n, H, W, sy, 2 if semi else 1, shift, 0, y_pitch, c_pitch, u_off, v_off, 0)
        v0 = first[0][1]
        view = self._PlaneListView(v0.on_device, v0.device, n, v0.array)
        # the closures hold `alive`: the table is addresses only, and what np.asarray made of an array-like has no other owner
        return self._read_view(view, out, lambda alive=alive: self.ctx.process_plane_list(layout, desc, table, nplanes),
                               lambda alive=alive, **kw: self.ctx.process_plane_list_dev(layout, desc, table, nplanes, **kw))

    def read_wide_frame_list(self, frames, layout: str, channel_order: str = 'rgb', scale=None, offset=None, rounding: str = 'nearest',
                             shift=None, out=None):
        """Frames of wide samples in separate allocations -- one (H, W, 3) uint16 array per decoded 16-bit PNG or TIFF, one RGB16
        buffer per frame of a camera SDK, a list of float16 / float32 (3, H, W) tensors from a Dataset or a video reader -- ->
        records, equal to read_wide_frames() on one array holding the same frames in list order (melf_process_wide_list*), without
        the torch.stack that would make that array: the narrowing kernel takes each frame's address from a table and reads only its
        meter crop.  frames: a sequence whose elements are each ONE frame, (H, W, C) for layout 'hwc', (C, H, W) for 'chw': numpy
        arrays / torch CPU tensors (host path), or torch tensors on this reader's GPU (enqueued on torch.cuda.current_stream).
        channel_order, scale, offset, rounding and shift are read_wide_frames'.  Every element is described by
        _hip.wide_frames_view as frame[None]; all must agree in everything but the address.  ValueError: host and device elements
        mixed, an element on another device, elements that differ (the message says which and in what), an element whose strides
        the descriptor cannot express (nothing is copied).  out: as for the batch methods, a uint8 device tensor (len(frames),
        RESULT_DTYPE.itemsize)."""
        frames = list(frames)
        views = []
        for (i, f) in enumerate(frames):
            if not (_hip._is_torch(f) or isinstance(f, np.ndarray)):
                f = np.asarray(f)
            if f.ndim != 3:
                raise ValueError('frame %d of the list must be one frame, %s, not of shape %s' % (
                    i, '(C, H, W)' if str(layout).lower() == 'chw' else '(H, W, C)', tuple(f.shape)))
            try:
                v = _hip.wide_frames_view(f[None], layout, channel_order, scale, offset, rounding, shift)
            except ValueError as e:
                raise ValueError('frame %d of the list: %s' % (i, e)) from None
            if views:
                if v.on_device != views[0].on_device:
                    raise ValueError('frame %d of the list is in %s memory, frame 0 in %s memory' % ((i,) + tuple(
                        'device' if w.on_device else 'host' for w in (v, views[0]))))
                for name in v._fields:
                    if name not in ('ptr', 'array', 'on_device') and getattr(v, name) != getattr(views[0], name):
                        raise ValueError('frame %d of the list differs from frame 0 in %s: %r, not %r' % (i, name, getattr(v, name), getattr(views[0], name)))
            views.append(v)
        n = len(views)
        if n == 0:
            return out if out is not None else np.zeros(0, _hip.RESULT_DTYPE)
        desc = views[0].descriptor()
        desc.n = n
        ptrs = [v.ptr for v in views]
        # the closures hold `views`: the table is addresses only, and what np.asarray made of an array-like has no other owner
        return self._read_view(views[0]._replace(n=n), out, lambda views=views: self.ctx.process_wide_list(desc, ptrs),
                               lambda views=views, **kw: self.ctx.process_wide_list_dev(desc, ptrs, **kw))

    def read_wide_plane_list(self, frames, channel_order: str = 'rgb', scale=None, offset=None, rounding: str = 'nearest', shift=None,
                             out=None):
        """Planar frames of wide samples whose PLANES lie in separate allocations -- libav's gbrp10le / gbrp12le / gbrp16le AVFrame
        (data[0..2], linesize[0..2]: channel_order 'gbr'), (r, g, b) held as separate float tensors -- -> records, equal to
        read_wide_frames(layout='chw') on one array holding the same samples in list order (melf_process_wide_plane_list*), without
        stacking any frame's planes.  frames: a sequence of 3-tuples of 2-D (H, W) planes in the order channel_order names them
        ('rgb', 'bgr' or 'gbr'): numpy arrays / torch CPU tensors (host path) or torch tensors on this reader's GPU (enqueued on
        torch.cuda.current_stream), of uint16 (torch: or int16 holding the same bits), float16, bfloat16 or float32, their samples
        contiguous along W, any row stride; all planes share dtype, shape and row stride.  scale / offset: a scalar or three values
        in the order of channel_order; they, rounding and shift are read_wide_frames'.  ValueError, naming frame and plane: a wrong
        plane count, host and device planes mixed, a plane on another device, differing dtype, shape or row stride, a plane whose
        strides the descriptor cannot express (nothing is copied).  out: as for the batch methods, a uint8 device tensor
        (len(frames), RESULT_DTYPE.itemsize)."""
        order = str(channel_order).lower()
        if order not in ('rgb', 'bgr', 'gbr'):
            raise ValueError('channel_order %r does not name three planes (rgb, bgr, gbr)' % (channel_order,))
        frames = list(frames)
        n = len(frames)
        if n == 0:
            return out if out is not None else np.zeros(0, _hip.RESULT_DTYPE)
        slot_of = ['bgr'.index(ch) for ch in order]   # tuple position -> plane slot of the C ABI (B, G, R)
        first = None      # frame 0, plane 0: (its view, its dtype)
        table = []
        alive = []        # every plane's view (and with it the array its address points into, a converted one included)
        for (i, planes) in enumerate(frames):
            planes = tuple(planes) if isinstance(planes, (tuple, list)) else (planes,)
            if len(planes) != 3:
                raise ValueError('frame %d of the list has %d planes, wide planar frames have 3' % (i, len(planes)))
            slots = [None] * 3
            for (k, p) in enumerate(planes):
                where = 'frame %d, plane %d of the list' % (i, k)
                if not (_hip._is_torch(p) or isinstance(p, np.ndarray)):
                    p = np.asarray(p)
                if p.ndim != 2:
                    raise ValueError('%s must be a 2-D (H, W) plane, not of shape %s' % (where, tuple(p.shape)))
                try:
                    v = self._wide_plane_view(p, scale, offset, rounding, shift, order)
                except ValueError as e:
                    raise ValueError('%s: %s' % (where, e)) from None
                if first is None:
                    first = (v, str(p.dtype))
                else:
                    (v0, dt0) = first
                    if v.on_device != v0.on_device:
                        raise ValueError('%s is in %s memory, frame 0, plane 0 in %s memory' % (
                            where, 'device' if v.on_device else 'host', 'device' if v0.on_device else 'host'))
                    if v.device != v0.device:
                        raise ValueError('%s is on cuda:%s, frame 0, plane 0 on cuda:%s' % (where, v.device, v0.device))
                    for (name, a, b) in (('dtype', str(p.dtype), dt0), ('shape', (v.H, v.W), (v0.H, v0.W)), ('row_pitch', v.row_pitch, v0.row_pitch)):
                        if a != b:
                            raise ValueError('%s differs from frame 0, plane 0 in %s: %r, not %r' % (where, name, a, b))
                slots[slot_of[k]] = v.ptr
                alive.append(v)
            table.extend(slots)
        v0 = first[0]
        desc = v0._replace(n=n, b_offset=0, g_offset=0, r_offset=0, frame_stride=0).descriptor()
        view = self._PlaneListView(v0.on_device, v0.device, n, v0.array)
        return self._read_view(view, out, lambda alive=alive: self.ctx.process_wide_plane_list(desc, table, 3),
                               lambda alive=alive, **kw: self.ctx.process_wide_plane_list_dev(desc, table, 3, **kw))

    @staticmethod
    def _wide_plane_view(plane, scale, offset, rounding, shift, order):
        """One 2-D plane of wide samples as a WideFramesView of layout 'chw' (n = 1; its plane offsets mean nothing): the sample
        type, H, W, row_pitch and the address are the plane's; the rule and its argument checks are wide_frames_view's, taken from
        a one-pixel stand-in of the same dtype and channel order.  A plane the descriptor cannot express is a ValueError."""
        is_torch = _hip._is_torch(plane)
        tname = str(plane.dtype).replace('torch.', '')
        if tname not in _hip.WIDE_TYPES or (not is_torch and tname in ('int16', 'bfloat16')):
            raise ValueError('wide frames must be uint16, float16, bfloat16 or float32, not %s' % plane.dtype)
        ss = _hip.WIDE_SAMPLE_BYTES[_hip.WIDE_TYPES[tname]]
        (H, W) = tuple(plane.shape)
        if H == 0 or W == 0:
            raise ValueError('a plane must be (H, W) with H, W > 0, not %s' % ((H, W),))
        strides = tuple(ss * st for st in plane.stride()) if is_torch else plane.strides
        (rp, es) = strides
        # strides of dimensions of size 1 are never stepped over: make them what a packed plane has
        if W == 1:
            es = ss
        if H == 1:
            rp = W * ss
        ptr = plane.data_ptr() if is_torch else plane.ctypes.data
        if es != ss or not W * ss <= rp <= 2 ** 31 - 1 or (ptr | rp) % ss:
            raise ValueError('the strides %s (bytes) of this plane do not fit melf_wide_frames: it is not read in place, and nothing is '
                             'copied' % (strides,))
        # (a numpy stand-in also for torch's own types: integer samples take the checks of uint16, float samples those of float16)
        stand_in = np.zeros((1, 3, 1, 1), np.uint16 if _hip.WIDE_TYPES[tname] == _hip.WIDE_U16 else np.float16)
        rule = _hip.wide_frames_view(stand_in, 'chw', order, scale, offset, rounding, shift)
        on_device = is_torch and plane.device.type == 'cuda'
        return rule._replace(ptr=int(ptr), on_device=on_device, device=plane.device.index if on_device else None,
                             sample_type=_hip.WIDE_TYPES[tname], H=H, W=W, row_pitch=int(rp), array=plane)

    def read_crops(self, crops: np.ndarray) -> np.ndarray:
        """Already meter_rect-cropped images (the reference's bgr_image injection)."""
        (_n, h, w, _c) = crops.shape
        ctx = self._crop_ctx.get((h, w))
        if ctx is None:
            blob = make_blob(self.params, Rect((0, 0), (w, h)))
            ctx = self._crop_ctx[(h, w)] = _hip.Context(blob, self.device)
        return ctx.process_batch(crops)

    def read_jpeg_files(self, files: List[bytes]) -> List[Optional[np.void]]:
        """JPEG files' bytes -> records, decoded and read on the GPU (melf_jpeg_process_batch).
        None for a file the GPU decoder does not take (not a baseline JPEG, corrupt): the caller
        decodes that one on the host."""
        out: List[Optional[np.void]] = [None] * len(files)
        groups: Dict[Tuple[int, int], List[int]] = {}
        flags = sum(flag for (name, flag, _doc) in _hip.JPEG_SWITCHES if flag and getattr(self, name))   # what the context's switches make the library take
        if flags:
            (hs, ws, orient, oks) = _hip.jpeg_probe_flags_batch(files, flags)
            if self.jpeg_orientation:    # by UPRIGHT size: what the library takes as H and W once that switch is on
                (hs, ws) = (np.where(orient >= 5, ws, hs), np.where(orient >= 5, hs, ws))
        else:
            (hs, ws, oks) = _hip.jpeg_probe_batch(files)
        for i in np.flatnonzero(oks):
            groups.setdefault((int(hs[i]), int(ws[i])), []).append(int(i))
        for ((h, w), idxs) in groups.items():
            (recs, status) = self.ctx.jpeg_process_batch([files[i] for i in idxs], h, w)
            for (k, i) in enumerate(idxs):
                if status[k] == _hip.JPEG_OK:
                    out[i] = recs[k]
        return out

    def read_jpeg_paths_batch(self, paths: List[str]) -> Tuple[np.ndarray, np.ndarray]:
        """File names -> (records, ok) (melf_jpeg_process_files: the library reads the files itself).  ok[i] is
        false for a file the GPU decoder does not take (unreadable, not a baseline JPEG, corrupt): the caller's
        host branch."""
        records = np.zeros(len(paths), _hip.RESULT_DTYPE)
        ok = np.zeros(len(paths), bool)
        todo = np.arange(len(paths))
        while len(todo):
            (recs, status, _hw) = self.ctx.jpeg_process_files([paths[i] for i in todo])
            status = np.asarray(status)
            good = status == _hip.JPEG_OK
            records[todo[good]] = recs[good]
            ok[todo[good]] = True
            again = todo[status == _hip.JPEG_SIZE_MISMATCH]
            if len(again) == len(todo):
                break  # cannot happen (the first accepted file defines the size); never loop forever
            todo = again
        return records, ok

    def read_jpeg_paths_begin(self, paths: List[str]) -> None:
        """read_jpeg_paths_batch in two halves: the library works on `paths` on its own thread until
        read_jpeg_paths_end() collects (records, ok) of the OLDEST list begun.  Up to _hip.FILES_IN_FLIGHT_MAX lists may be in
        flight (a later one's files are read while an earlier one decodes); nothing else may use this reader while any is --
        drain_jpeg_paths() first."""
        paths = list(paths)
        self.ctx.jpeg_process_files_begin(paths)
        self._begun.append(paths)

    def jpeg_paths_in_flight(self) -> int:
        return len(self._begun) + len(self._collected)

    def _collect_one(self):
        paths = self._begun.pop(0)
        (recs, status, _hw) = self.ctx.jpeg_process_files_end()
        status = np.asarray(status)
        ok = status == _hip.JPEG_OK
        records = np.zeros(len(paths), _hip.RESULT_DTYPE)
        records[ok] = recs[ok]
        return (paths, records, ok, np.flatnonzero(status == _hip.JPEG_SIZE_MISMATCH))

    def drain_jpeg_paths(self) -> None:
        """Waits for every list in flight and keeps the results for read_jpeg_paths_end(): afterwards the context is
        free for other calls (host-decoded frames, files of another frame size)."""
        while self._begun:
            self._collected.append(self._collect_one())

    def discard_jpeg_paths(self) -> None:
        """Waits for every list in flight and forgets the results (a consumer that stopped early)."""
        self.drain_jpeg_paths()
        self._collected.clear()

    def read_jpeg_paths_end(self) -> Tuple[np.ndarray, np.ndarray]:
        (paths, records, ok, again) = self._collected.pop(0) if self._collected else self._collect_one()
        if len(again):  # files of another frame size: their own call(s), now -- with the context to ourselves
            self.drain_jpeg_paths()
            (r2, ok2) = self.read_jpeg_paths_batch([paths[i] for i in again])
            records[again] = r2
            ok[again] = ok2
        return records, ok

    def read_jpeg_paths(self, paths: List[str]) -> List[Optional[np.void]]:
        """The same as a list: a record, or None where the caller has to decode on the host."""
        (records, ok) = self.read_jpeg_paths_batch(paths)
        return [records[i] if ok[i] else None for i in range(len(paths))]

    def read_many(self, images: List[np.ndarray], cropped: Optional[List[bool]] = None) -> List[np.void]:
        """Heterogeneous list of frames: grouped by shape, one batched call per group."""
        cropped = cropped or [False] * len(images)
        groups: Dict[Tuple[bool, Tuple[int, ...]], List[int]] = {}
        for (i, img) in enumerate(images):
            groups.setdefault((cropped[i], img.shape), []).append(i)
        out: List[Optional[np.void]] = [None] * len(images)
        for ((is_crop, _shape), idxs) in groups.items():
            batch = np.stack([images[i] for i in idxs])
            recs = self.read_crops(batch) if is_crop else self.read_frames(batch)
            for (k, i) in enumerate(idxs):
                out[i] = recs[k]
        return out  # type: ignore


_readers: Dict[int, MeterReader] = {}


def get_reader(params: Params) -> MeterReader:
    """Per-Params cache, like the reference's id(params)-keyed caches
    (meterelf/_image.py:69-81, meterelf/_dial_data.py:11-19)."""
    r = _readers.get(id(params))
    if r is None or r.params is not params:
        r = _readers[id(params)] = MeterReader(params)
    return r
