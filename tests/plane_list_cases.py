"""Support for tests/test_plane_list.py (melf_process_plane_list*, MeterReader.read_plane_list): the planes of a contiguous batch
cut apart -- every plane of every frame with its own address and readable extent, and the descriptor whose plane offsets count from
the plane's own pointer --, and device planes in separate allocations.  New support lives here; tests/frame_cases.py and
tests/frame_list_cases.py are used as they are."""
import ctypes as C
import os
import sys
from typing import NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import frame_list_cases as flc  # noqa: E402
from tests import yuv16_cases as y16  # noqa: E402

LAYOUTS = ('yuv', 'yuv_planar', 'yuv16', 'planar')
# every format name of the four layouts' view functions
FORMATS = [lf for lf in flc.FORMATS if lf[0] in LAYOUTS]
# one format per distinct shape of the row runs and order of the planes
SHAPES = [('yuv', 'nv12'), ('yuv', 'yv12'), ('yuv_planar', 'i422'), ('yuv_planar', 'nv42'), ('yuv16', 'p010'), ('yuv16', 'i210'), ('planar', 'gbr')]


class Batch(NamedTuple):
    """A contiguous batch in host memory as the family's batch call takes it"""
    ptr: int
    desc: object      # the family's C descriptor
    extent: int       # bytes from ptr to the last sample of the last frame
    keep: object      # what ptr points into


def batch(src, layout, fmt, rng, n=None, padded=False):
    """src's first n frames (flc.Source) as a contiguous batch of format fmt of the family `layout`.  padded: Y and chroma pitches
    padded differently (for 'planar': padded rows), gaps between the planes and behind a frame."""
    n = len(src.bgr) if n is None else n
    if not padded:
        (arr, view, _kw) = flc.make(src, layout, fmt, rng)
        v = view(arr[:n])
        assert not v.copied and v.n == n
        return Batch(v.ptr, flc.descriptor(v), v.extent, (arr, v))
    if layout == 'yuv':
        (buf, d) = fc.pitched420(*(p[:n] for p in src.yuv(1, 1)), fmt, y_pad=5, c_pad=3, gap=7, stride_pad=9, rng=rng)
        return Batch(buf.ctypes.data, d, fc.extent420(d), buf)
    if layout == 'yuv_planar':
        (sx, sy, _step, _vf) = _hip.YUV_PLANAR_FORMATS[fmt]
        (raw, d, lead) = fc.pitched_yuv_planar(*(p[:n] for p in src.yuv(sx, sy)), fmt, y_pad=5, c_pad=3, gap=7, stride_pad=9, rng=rng)
        return Batch(raw.ctypes.data + lead, d, fc.extent_yuv_planar(d), raw)
    if layout == 'yuv16':
        sy = _hip.YUV16_FORMATS[fmt][0]
        planes = y16.widen_planes(tuple(p[:n] for p in src.yuv(1, sy, flc.M10)), fmt, rng)
        (raw, d, lead) = y16.pitched16(*planes, fmt, y_pad=6, c_pad=10, gap=4, stride_pad=8, rng=rng)
        return Batch(raw.ctypes.data + lead, d, y16.extent16(d), raw)
    assert layout == 'planar'
    (buf, d) = fc.pitched_planes(src.bgr[:n], fmt, row_pad=5, gaps=(0, 3, 6), stride_pad=9, rng=rng)
    return Batch(buf.ctypes.data, d, fc.extent_planes(d), buf)


class Cut(NamedTuple):
    """A contiguous batch cut at its plane boundaries"""
    desc: object      # the plane list's descriptor: the batch's with the plane offsets counted from each plane's own pointer
    nplanes: int
    offsets: tuple    # per slot: the plane's first byte in a frame of the batch
    extents: tuple    # per slot: the bytes readable from the plane's pointer
    frame_stride: int
    n: int


def cut(layout, desc):
    """The plane slots of the C ABI (Y, U or interleaved chroma, V; B, G, R) of a contiguous batch's descriptor."""
    d = type(desc).from_buffer_copy(desc)
    fs = desc.frame_stride
    d.frame_stride = 0   # not looked at
    if layout == 'planar':
        span = (desc.H - 1) * desc.row_pitch + desc.W
        offsets = (desc.b_offset, desc.g_offset, desc.r_offset)
        (d.b_offset, d.g_offset, d.r_offset) = (0, 0, 0)
        return Cut(d, 3, offsets, (span,) * 3, fs, desc.n)
    if layout == 'yuv':
        (bps, sx, sy, semi) = (1, 1, 1, desc.format == _hip.YUV_NV12)
    elif layout == 'yuv_planar':
        (bps, sx, sy, semi) = (1, desc.sub_x, desc.sub_y, desc.c_step == 2)
    else:
        (bps, sx, sy, semi) = (2, 1, desc.sub_y, desc.c_step == 2)
    y_ext = (desc.H - 1) * desc.y_pitch + desc.W * bps
    c_ext = ((desc.H >> sy) - 1) * desc.c_pitch + (desc.W >> sx) * (2 if semi else 1) * bps
    if semi:
        lo = min(desc.u_offset, desc.v_offset)
        (d.u_offset, d.v_offset) = (desc.u_offset - lo, desc.v_offset - lo)
        return Cut(d, 2, (0, lo), (y_ext, c_ext), fs, desc.n)
    (d.u_offset, d.v_offset) = (0, 0)
    return Cut(d, 3, (0, desc.u_offset, desc.v_offset), (y_ext, c_ext, c_ext), fs, desc.n)


def host_addresses(b, c):
    """[frame][slot] -> the host address of that plane inside the contiguous batch b"""
    return [[b.ptr + i * c.frame_stride + off for off in c.offsets] for i in range(c.n)]


class DevPlanes:
    """Every plane of every frame of a batch a device allocation of its own of exactly the plane's extent (frame_cases.DevBuf),
    allocated in shuffled order with spacer allocations of differing sizes between them.  ptrs: the flat, frame-major table;
    at(i, k): the address of plane slot k of frame i."""

    def __init__(self, b, c, rng):
        host = host_addresses(b, c)
        self.nplanes = c.nplanes
        self.bufs = [None] * (c.n * c.nplanes)
        self.spacers = []
        blank = np.zeros(8192, np.uint8)
        for (j, q) in enumerate(rng.permutation(c.n * c.nplanes)):
            (i, k) = divmod(int(q), c.nplanes)
            self.bufs[int(q)] = fc.DevBuf(host[i][k], c.extents[k])
            self.spacers.append(fc.DevBuf(blank.ctypes.data, 256 + 1024 * (j % 7)))
        self.ptrs = [buf.d.value for buf in self.bufs]

    def at(self, i, k):
        return self.ptrs[i * self.nplanes + k]

    def spread(self, k):
        """the differences between consecutive frames' addresses of plane slot k"""
        col = self.ptrs[k::self.nplanes]
        return [q - p for (p, q) in zip(col, col[1:])]

    def free(self):
        for buf in self.bufs + self.spacers:
            buf.free()


def frame_bytes(b, c):
    """The batch as an (n, bytes of one frame) array of its own: a copy, frame i the bytes of frame i up to its last sample"""
    ext = b.extent - (c.n - 1) * c.frame_stride
    flat = np.lib.stride_tricks.as_strided(np.frombuffer((C.c_uint8 * b.extent).from_address(b.ptr), np.uint8), shape=(c.n, ext),
                                           strides=(c.frame_stride, 1))
    return np.array(flat)


def rotated(b, c, slots):
    """A contiguous batch of b's geometry (frames packed one frame's extent apart, rounded up to 16) whose plane slots `slots` are those
    of the NEXT frame of b, the others b's own: (array, address, descriptor, extent)."""
    flat = frame_bytes(b, c)
    out = flat.copy()
    for k in slots:
        (lo, hi) = (c.offsets[k], c.offsets[k] + c.extents[k])
        out[:, lo:hi] = np.roll(flat[:, lo:hi], -1, axis=0)
    ext = flat.shape[1]
    stride = (ext + 15) // 16 * 16
    packed = np.zeros((c.n, stride), np.uint8)
    packed[:, :ext] = out
    d = type(b.desc).from_buffer_copy(b.desc)
    d.frame_stride = stride
    return packed, packed.ctypes.data, d, (c.n - 1) * stride + ext
