"""Support for tests/test_frame_list.py (melf_process_frame_list*, MeterReader.read_frame_list): every family with every format name
its view function accepts, the array a caller would hold made from BGR frames by the existing builders, and device frames in
separate allocations.  New support lives here; tests/frame_cases.py and the *_cases.py modules are used as they are."""
import ctypes as C
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import p10_cases as p10  # noqa: E402
from tests import p32_cases as p32  # noqa: E402
from tests import yuv16_cases as y16  # noqa: E402

# layout of read_frame_list -> the family's C entry points (host; + '_dev') and its batch method
ENTRY = {'views': 'melf_process_frames', 'yuv': 'melf_process_yuv', 'yuv422': 'melf_process_yuv422', 'yuv_planar': 'melf_process_yuv_planar',
         'yuv16': 'melf_process_yuv16', 'yuv422_10': 'melf_process_yuv422_10', 'packed32': 'melf_process_packed32', 'planar': 'melf_process_planes'}
METHOD = {'views': 'read_frame_views', 'yuv': 'read_yuv_frames', 'yuv422': 'read_yuv422_frames', 'yuv_planar': 'read_yuv_planar_frames',
          'yuv16': 'read_yuv16_frames', 'yuv422_10': 'read_yuv422_10_frames', 'packed32': 'read_packed32_frames', 'planar': 'read_planar_frames'}
M10 = 3   # BT.709 limited for the 10-bit material, as the *_cases modules have it

# every format name each family's view function accepts
FORMATS = ([('views', f) for f in _hip.PIX_CODES] + [('yuv', f) for f in _hip.YUV_CODES] + [('yuv422', f) for f in _hip.YUV422_CODES]
           + [('yuv_planar', f) for f in _hip.YUV_PLANAR_FORMATS] + [('yuv16', f) for f in _hip.YUV16_FORMATS]
           + [('yuv422_10', f) for f in _hip.YUV422_10_FORMATS] + [('packed32', f) for f in _hip.PACKED32_FORMATS]
           + [('planar', f) for f in _hip.PLANAR_ORDERS])
# one format per family (host lists, the Python child)
ONE_PER_FAMILY = [('views', 'rgba'), ('yuv', 'nv12'), ('yuv422', 'uyvy'), ('yuv_planar', 'nv24'), ('yuv16', 'p010'), ('yuv422_10', 'v210'),
                  ('packed32', 'y410'), ('planar', 'gbr')]
# one format per distinct shape of the row runs (per-frame ends of mappings)
RUN_SHAPES = [('views', 'bgr'), ('views', 'bgra'), ('yuv', 'nv12'), ('yuv', 'i420'), ('yuv422', 'yuyv'), ('yuv_planar', 'i422'), ('yuv_planar', 'nv24'),
              ('yuv16', 'p010'), ('yuv422_10', 'v210'), ('yuv422_10', 'y210'), ('packed32', 'y410'), ('planar', 'rgb')]


class Source:
    """BGR frames and, made once each and shared, their planes at a chroma subsampling under a matrix (frame_cases.bgr_to_yuv)."""

    def __init__(self, bgr):
        self.bgr = bgr
        self.bgr.setflags(write=False)
        self._yuv = {}

    def yuv(self, sx, sy, matrix=None):
        key = (sx, sy, matrix)
        if key not in self._yuv:
            self._yuv[key] = fc.bgr_to_yuv(self.bgr, sx, sy, matrix)
        return self._yuv[key]


def make(src, layout, fmt, rng):
    """(the contiguous array of all frames a caller would hold, view(array) -> the family's *FramesView, read_frame_list's keyword
    arguments) of src's frames in format fmt of the family `layout`."""
    if layout == 'views':
        arr = np.ascontiguousarray(fc.to_layout(src.bgr, fmt.replace('x', 'a'), 0, rng)[0])
        return arr, lambda a: _hip.frames_view(a, fmt), {}
    if layout == 'yuv':
        return fc.conventional420(*src.yuv(1, 1), fmt, 0, rng), lambda a: _hip.yuv_frames_view(a, fmt, 'bt601'), {}
    if layout == 'yuv422':
        return fc.conventional422(*src.yuv(1, 0), 'yuyv' if fmt == 'yuy2' else fmt, 0, rng), lambda a: _hip.yuv422_frames_view(a, fmt, 'bt601'), {}
    if layout == 'yuv_planar':
        (sx, sy, _step, _vf) = _hip.YUV_PLANAR_FORMATS[fmt]
        return fc.conventional_yuv_planar(*src.yuv(sx, sy), fmt, 0, rng), lambda a: _hip.yuv_planar_frames_view(a, fmt, 'bt601'), {}
    if layout == 'yuv16':
        sy = _hip.YUV16_FORMATS[fmt][0]
        arr = y16.conventional16(*y16.widen_planes(src.yuv(1, sy, M10), fmt, rng), fmt, 0, rng)
        return arr, lambda a: _hip.yuv16_frames_view(a, fmt, 'bt709'), {'matrix': 'bt709'}
    if layout == 'yuv422_10':
        arr = p10.conventional10(*src.yuv(1, 0, M10), 'v210' if fmt == 'v210' else 'y210', 0, rng)
        width = getattr(arr, 'width', None)
        return np.asarray(arr), lambda a: _hip.yuv422_10_frames_view(a, fmt, 'bt709', width=width), {'matrix': 'bt709', 'width': width}
    if layout == 'packed32':
        kind = p32.kind_of(fmt)
        planes = src.yuv(0, 0, M10) if kind == 'yuv' else (src.bgr,)
        matrix = p32.matrix_of(fmt, 'bt709')
        arr = np.ascontiguousarray(p32.conventional32(*planes, fmt, 0, rng))
        return arr, lambda a: _hip.packed32_frames_view(a, fmt, matrix), ({'matrix': matrix} if matrix else {})
    assert layout == 'planar'
    return fc.to_planes(src.bgr, fmt, rng), lambda a: _hip.planar_frames_view(a, fmt), {}


def reference_bgr(src, layout, fmt):
    """The packed BGR frames whose read_frames records the family's contract names for make(src, layout, fmt)'s frames: the frames
    themselves for the RGB families, the header's integer conversion of the samples for the YUV ones."""
    if layout in ('views', 'planar') or (layout == 'packed32' and p32.kind_of(fmt) == 'rgb'):
        return src.bgr
    if layout == 'yuv_planar':
        (sx, sy, m) = _hip.YUV_PLANAR_FORMATS[fmt][:2] + (None,)
    elif layout == 'yuv16':
        (sx, sy, m) = (1, _hip.YUV16_FORMATS[fmt][0], M10)
    else:
        (sx, sy, m) = {'yuv': (1, 1, None), 'yuv422': (1, 0, None), 'yuv422_10': (1, 0, M10), 'packed32': (0, 0, M10)}[layout]
    return fc.yuv_to_bgr(*src.yuv(sx, sy, m), sx, sy, 0 if m is None else m)


def descriptor(v):
    """The C descriptor of a *FramesView."""
    return v.descriptor() if hasattr(v, 'descriptor') else _hip.MelfFrames(v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride)


def frame_extent(v):
    """Bytes of ONE frame of the view: FrameLayout::extent of its descriptor as a one-frame batch."""
    return v.extent - (v.n - 1) * v.frame_stride


def dev_batch(ctx, layout, d_ptr, desc, **kw):
    """The family's melf_process_*_dev call on a contiguous batch."""
    return ctx._dev(getattr(ctx._L, ENTRY[layout] + '_dev'), d_ptr, desc, kw.pop('d_results_ptr', None), kw.pop('want_host', True), kw.pop('stream', None))


def host_batch(ctx, layout, ptr, desc):
    return ctx._host(getattr(ctx._L, ENTRY[layout]), ptr, desc)


class DevFrames:
    """The frames of a view, each a device allocation of its own of exactly one frame's extent (frame_cases.DevBuf), allocated in
    shuffled order with spacer allocations of differing sizes between them, so that no two frames are one stride apart by accident of
    the allocator.  at_end: each copy ends where its allocation ends (DevBuf.at_end), at base phase `phase` modulo 4."""

    def __init__(self, v, rng, at_end=False, phase=None):
        ext = frame_extent(v)
        self.bufs = [None] * v.n
        self.spacers = []
        blank = np.zeros(8192, np.uint8)
        for (k, i) in enumerate(rng.permutation(v.n)):
            src = v.ptr + int(i) * v.frame_stride
            self.bufs[int(i)] = fc.DevBuf.at_end(src, ext, phase) if at_end else fc.DevBuf(src, ext)
            self.spacers.append(fc.DevBuf(blank.ctypes.data, 256 + 1024 * (k % 7)))
        self.ptrs = [b.d.value for b in self.bufs]

    def spread(self):
        """the differences between consecutive frames' addresses"""
        return [b - a for (a, b) in zip(self.ptrs, self.ptrs[1:])]

    def free(self):
        for b in self.bufs + self.spacers:
            b.free()


@functools.lru_cache(maxsize=None)
def synth_source(n=33, seed=21):
    """n fixture-size frames of frame_cases.synth (every ninth constant: 29 of 33 read), as a Source shared by the tests."""
    import glob
    from meterelf_amd._image import imread_bgr
    frames = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(fc.GOLDEN, 'sample-images1', '*.jpg')))]
    return Source(fc.synth(frames, n, seed))


def pointer_table(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)
