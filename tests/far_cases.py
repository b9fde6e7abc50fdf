"""Support for tests/test_far_addresses.py: frames, rows and planes that lie 2 GiB, 4 GiB and more from the base pointer.

FarArena is ONE device allocation of several GiB, filled with 0x80 (a frame of 0x80 reads FRAME_DIALS_NOT_FOUND), into which a test
copies only the few hundred KB its frames occupy and which remembers what was written; HostTwin is the same span of host memory, an
anonymous mapping whose untouched pages read as zeros, for the host-fed entry points.  The rest is generic over the eight families
(frame_list_cases' names): tight one-frame buffers from the existing builders, the BGR frame a frame of filler bytes decodes to,
the descriptors and the copies of the three placements, and the precondition that a load whose offset wrapped at 2^31 or 2^32 finds
filler.  New support lives here; tests/frame_cases.py and the *_cases.py modules are used as they are."""
import ctypes as C
import mmap
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import frame_list_cases as flc  # noqa: E402
from tests import oriented_cases as oc  # noqa: E402
from tests import p10_cases as p10  # noqa: E402
from tests import p32_cases as p32  # noqa: E402
from tests import yuv16_cases as y16  # noqa: E402

GIB = 1 << 30
ARENA_MAX = 9 * GIB
FILL = 0x80
WRAPS = (1 << 31, 1 << 32)

# the families and the format lists their own test modules go through
FORMATS = {
    'views': ('bgr', 'rgb', 'bgra', 'rgba'), 'yuv': fc.F420.formats, 'yuv422': fc.F422.formats, 'yuv_planar': tuple(fc.YUV_PLANAR_FORMATS),
    'yuv16': y16.DISTINCT, 'yuv422_10': p10.FORMATS, 'packed32': p32.FORMATS, 'planar': fc.PLANAR.formats,
}
LAYOUTS = tuple(FORMATS)


def dial_family(layout, fmt):
    """The dial reader's kernel family (melf_ctx_last_dials) that reads frames of this format."""
    if layout == 'views':
        return {'bgr': 'bgr', 'rgb': 'packed3'}.get(fmt, 'packed4')
    if layout == 'yuv':
        return 'nv12' if fmt == 'nv12' else 'i420'
    if layout == 'yuv_planar':
        (sx, _sy, step, _vf) = fc.YUV_PLANAR_FORMATS[fmt]
        return 'yp_sub%d_step%d' % (sx, step)
    if layout == 'yuv16':
        return 'yuv16_step%d' % y16.FORMATS[fmt][1]
    if layout == 'yuv422_10':
        return 'v210' if fmt == 'v210' else 'y210'
    if layout == 'packed32':
        return 'p32' + p32.kind_of(fmt)
    return {'yuv422': 'p422', 'planar': 'planar'}[layout]


# ---------------------------------------------------------------------------------------------------------------- memory ---
class FarArena:
    """One hipMalloc of nbytes bytes (at most 9 GiB) filled with 0x80; put / put_rows copy host bytes to an offset and are
    remembered; reset() turns what was written back into filler.  The caller frees it in a finally."""
    FILL = FILL

    def __init__(self, nbytes):
        assert 0 < nbytes <= ARENA_MAX, nbytes
        self.hip = fc.hip_rt()
        self.nbytes = nbytes
        self.base = C.c_void_p()
        self._written = []
        rc = self.hip.hipMalloc(C.byref(self.base), C.c_size_t(nbytes))
        if rc != 0 or not self.base.value:
            self.base = C.c_void_p()
            pytest.fail('hipMalloc of %d bytes (%.1f GiB) failed with error %d: the far-address tests need one allocation of that size '
                        '(an MI355X has 288 GB)' % (nbytes, nbytes / GIB, rc))
        rc = self.hip.hipMemset(self.base, FILL, C.c_size_t(nbytes))
        if rc == 0:
            rc = self.hip.hipDeviceSynchronize()
        if rc != 0:
            self.free()
            pytest.fail('hipMemset of the %d-byte arena failed with error %d' % (nbytes, rc))

    @property
    def ptr(self):
        return self.base.value

    def put(self, offset, host_bytes):
        """One hipMemcpy of a contiguous uint8 array to base + offset."""
        a = np.ascontiguousarray(host_bytes).reshape(-1).view(np.uint8)
        assert 0 <= offset and offset + a.nbytes <= self.nbytes, (offset, a.nbytes, self.nbytes)
        assert self.hip.hipMemcpy(C.c_void_p(self.base.value + offset), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        self._written.append((offset, offset + a.nbytes))

    def put_rows(self, offset, pitch, rows):
        """rows (nrows, row bytes) uint8: row r to base + offset + r * pitch, one hipMemcpy per row."""
        for (r, row) in enumerate(rows):
            self.put(offset + r * pitch, row)

    def written(self):
        """The intervals [lo, hi) written so far, sorted."""
        return sorted(self._written)

    def reset(self):
        """What was written becomes filler again."""
        for (lo, hi) in self._written:
            assert self.hip.hipMemset(C.c_void_p(self.base.value + lo), FILL, C.c_size_t(hi - lo)) == 0
        assert self.hip.hipDeviceSynchronize() == 0
        self._written = []

    def free(self):
        if self.base.value:
            self.hip.hipFree(self.base)
            self.base = C.c_void_p()


class HostTwin:
    """The same span in host memory: an anonymous private mapping (no page is backed until it is written; what was never written
    reads as zeros), wrapped as a uint8 array.  The interface of FarArena, FILL 0."""
    FILL = 0

    def __init__(self, nbytes):
        flags = mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, 'MAP_NORESERVE', 0)
        self.map = mmap.mmap(-1, nbytes, flags=flags)
        self.bytes = np.frombuffer(self.map, np.uint8)
        self.nbytes = nbytes
        self._written = []

    @property
    def ptr(self):
        return self.bytes.ctypes.data

    def put(self, offset, host_bytes):
        a = np.ascontiguousarray(host_bytes).reshape(-1).view(np.uint8)
        assert 0 <= offset and offset + a.nbytes <= self.nbytes
        self.bytes[offset:offset + a.nbytes] = a
        self._written.append((offset, offset + a.nbytes))

    def put_rows(self, offset, pitch, rows):
        for (r, row) in enumerate(rows):
            self.put(offset + r * pitch, row)

    def written(self):
        return sorted(self._written)

    def reset(self):
        for (lo, hi) in self._written:
            self.bytes[lo:hi] = 0
        self._written = []

    def free(self):
        self.bytes = None
        self.map.close()


def overlaps(written, lo, hi):
    return any(a < hi and lo < b for (a, b) in written)


def assert_wraps_find_filler(written, far):
    """The precondition of every far placement: for every interval of `far` (written intervals whose samples a kernel must fetch)
    that starts at or beyond 2^31 / 2^32, the same interval taken modulo that power -- where a load whose offset was cut to 31 or 32
    bits would go -- meets nothing that was written: it reads filler and cannot give the frame's record.  Returns how many wrapped
    intervals were looked at."""
    looked = 0
    for (lo, hi) in far:
        assert overlaps(written, lo, hi), ('not written', lo, hi)
        for m in WRAPS:
            if lo >= m:
                assert not overlaps(written, lo % m, lo % m + hi - lo), ('a load wrapped at 2^%d meets written bytes' % (m.bit_length() - 1), lo, hi)
                looked += 1
    return looked


# ---------------------------------------------------------------------------------------------------------------- frames ---
def tight_batch(src, layout, fmt, rng):
    """src's frames (flc.Source) as ONE tight batch of format fmt from the family's pitched builder: no padding, the frames one
    frame's extent apart.  Returns (uint8 array of n * frame_stride bytes, the family's descriptor); frame i is
    bytes[i * frame_stride:(i + 1) * frame_stride].  The BGR frames its records must equal: flc.reference_bgr(src, layout, fmt)."""
    if layout == 'views':
        (buf, args) = fc.pitched_packed(src.bgr, fmt, 0, rng)
        return buf, _hip.MelfFrames(*args)
    if layout == 'yuv':
        (buf, d) = fc.pitched420(*src.yuv(1, 1), fmt, rng=rng)
    elif layout == 'yuv422':
        (buf, d) = fc.pitched422(*src.yuv(1, 0), fmt, rng=rng)
    elif layout == 'yuv_planar':
        (sx, sy, _step, _vf) = fc.YUV_PLANAR_FORMATS[fmt]
        (buf, d, _lead) = fc.pitched_yuv_planar(*src.yuv(sx, sy), fmt, rng=rng)
    elif layout == 'yuv16':
        planes = y16.widen_planes(src.yuv(1, y16.FORMATS[fmt][0], flc.M10), fmt, rng)
        (raw, d, _lead) = y16.pitched16(*planes, fmt, rng=rng, matrix=flc.M10)
        buf = raw.view(np.uint8)
    elif layout == 'yuv422_10':
        (buf, d) = p10.pitched10(*src.yuv(1, 0, flc.M10), fmt, rng=rng, matrix=flc.M10)
    elif layout == 'packed32':
        planes = src.yuv(0, 0, flc.M10) if p32.kind_of(fmt) == 'yuv' else (src.bgr,)
        (buf, d) = p32.pitched32(*planes, fmt, rng=rng, matrix=flc.M10)
    else:
        assert layout == 'planar'
        (buf, d) = fc.pitched_planes(src.bgr, fmt, rng=rng)
    assert buf.nbytes == d.n * d.frame_stride, (layout, fmt, buf.nbytes, d.n, d.frame_stride)
    return buf, d


def filler_bgr(layout, fmt, H, W, value):
    """The (1, H, W, 3) BGR frame whose read_frames record a frame of bytes `value` must give in this format: the samples the
    format's own unpacking (the *_cases modules' inverses) makes of such bytes, through the header's conversion."""
    word = value * 0x01010101
    if layout in ('views', 'planar'):
        return np.full((1, H, W, 3), value, np.uint8)
    if layout in ('yuv', 'yuv422', 'yuv_planar'):
        (sx, sy) = {'yuv': (1, 1), 'yuv422': (1, 0)}.get(layout) or fc.YUV_PLANAR_FORMATS[fmt][:2]
        return fc.yuv_to_bgr(np.full((1, H, W), value, np.uint8), np.full((1, H >> sy, W >> sx), value, np.uint8),
                             np.full((1, H >> sy, W >> sx), value, np.uint8), sx, sy, 0)
    if layout == 'yuv16':
        (sy, _step, _vf, shift) = y16.FORMATS[fmt]
        s = int(y16.reduce16(np.array([value * 257], np.uint16), shift)[0])
        return fc.yuv_to_bgr(np.full((1, H, W), s, np.uint8), np.full((1, H >> sy, W // 2), s, np.uint8), np.full((1, H >> sy, W // 2), s, np.uint8),
                             1, sy, flc.M10)
    if layout == 'yuv422_10':
        if fmt == 'v210':
            planes = p10.unpack_v210(np.full((1, H, 4 * p10.v210_groups(W)), word, np.uint32), W)
        else:
            planes = p10.unpack_y210(np.full((1, H, W, 2), value * 257, np.uint16))
        return fc.yuv_to_bgr(*planes, 1, 0, flc.M10)
    assert layout == 'packed32'
    reads = p32.unpack32(np.full((1, H, W), word, np.uint32), p32.pos_of(fmt))
    if p32.kind_of(fmt) == 'yuv':
        return fc.yuv_to_bgr(*reads, 0, 0, flc.M10)
    return np.ascontiguousarray(np.stack([reads[2], reads[1], reads[0]], axis=-1))


def planes_of(layout, d):
    """The planes of one frame of descriptor d in memory order: (offset, rows, bytes of a row, pitch)."""
    if layout == 'yuv422':
        return [(0, d.H, 2 * d.W, d.row_pitch)]
    if layout == 'yuv422_10':
        return [(0, d.H, p10.v210_row_bytes(d.W) if d.format == _hip.YUV422_10_V210 else 4 * d.W, d.row_pitch)]
    return sorted((off, rows, cols * eb, pitch) for (off, rows, cols, eb, pitch, _f) in oc.plane_table(layout, d))


def frame_extent(layout, d):
    return max(off + (rows - 1) * pitch + row for (off, rows, row, pitch) in planes_of(layout, d))


# ------------------------------------------------------------------------------------------------------------ placements ---
A_FRAMES = fc.ENDS_FRAMES          # 33: the second prep frame group holds one frame
A_STRIDE = (1 << 27) + 4096        # a multiple of 16 (v210); frame 16 starts beyond 2^31, frame 32 beyond 2^32
A_FIRST = 16                       # the frames in front of it stay filler: what a wrapped offset of a far frame would find
B_PITCH = (1 << 25) + 64           # rows >= 64 start beyond 2^31, >= 128 beyond 2^32, >= 192 beyond 3 * 2^31
B_ROWS = 252
C_OFFSETS = (0, (1 << 32) + 64, (1 << 33) + 128)


def far_frames_desc(d):
    """Placement A: the tight descriptor d as A_FRAMES frames A_STRIDE apart."""
    new = oc.copy_desc(d)
    (new.n, new.frame_stride) = (A_FRAMES, A_STRIDE)
    return new


def put_far_frames(mem, buf, d):
    """Placement A: the frames of the tight batch (buf, d) -- its frame k is frame A_FIRST + k -- at their far places.  Returns
    the intervals written."""
    fs = d.frame_stride
    assert d.n == A_FRAMES - A_FIRST
    far = []
    for k in range(d.n):
        at = (A_FIRST + k) * A_STRIDE
        mem.put(at, buf[k * fs:(k + 1) * fs])
        far.append((at, at + fs))
    return far


def far_rows_desc(layout, d):
    """Placement B: the tight one-frame descriptor d with the rows of its first plane (the packed plane, the Y plane) B_PITCH
    apart and the chroma planes behind it, as tight as they were.  Returns (descriptor, offset of the chroma planes' first byte in
    the tight frame or None, the same in the far frame)."""
    planes = planes_of(layout, d)
    new = oc.copy_desc(d)
    assert d.n == 1 and d.H == B_ROWS and planes[0][0] == 0
    setattr(new, 'y_pitch' if hasattr(d, 'y_pitch') else 'row_pitch', B_PITCH)
    end0 = (d.H - 1) * B_PITCH + planes[0][2]
    if len(planes) == 1:
        new.frame_stride = (end0 + 15) // 16 * 16
        return new, None, None
    (c_tight, c_far) = (planes[1][0], (end0 + 15) // 16 * 16)
    (new.u_offset, new.v_offset) = (d.u_offset - c_tight + c_far, d.v_offset - c_tight + c_far)
    new.frame_stride = (c_far + frame_extent(layout, d) - c_tight + 15) // 16 * 16
    return new, c_tight, c_far


def put_far_rows(mem, layout, buf, d, c_tight, c_far):
    """Placement B: the one tight frame (buf, d) with its first plane's rows B_PITCH apart (one copy per row) and everything behind
    that plane as one copy at c_far.  Returns the intervals written that lie beyond 2^31."""
    (_off, rows, row_bytes, pitch) = planes_of(layout, d)[0]
    mem.put_rows(0, B_PITCH, np.lib.stride_tricks.as_strided(buf, shape=(rows, row_bytes), strides=(pitch, 1)))
    if c_tight is not None:
        mem.put(c_far, buf[c_tight:frame_extent(layout, d)])
    return [(lo, hi) for (lo, hi) in mem.written() if lo >= WRAPS[0]]
