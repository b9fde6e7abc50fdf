"""What the tests of the 32-bit packed 4:4:4 frames (test_packed32_frames, test_packed32_dials) share, on top of tests.frame_cases:
the layout restated in numpy (the packer and its inverse), the caller's array and the pitched-buffer builder -- every ignored bit
random --, a Family record per colour kind so that the shared bodies of frame_cases run on the new frames, and the expected records
from the existing paths.

The contract (include/meterelf_hip.h): a pixel is one little-endian 32-bit word with three 8-bit reads s8_k = (word >> pos[k]) & 255.
YUV: the reads are Y, U, V and the records equal those of melf_process_yuv_planar(_dev) on the 8-bit i444 frame of the s8, and so
those of melf_process_batch on the BGR frame the integer conversion (frame_cases.yuv_to_bgr at sub_x = sub_y = 0) makes of it.  RGB:
the reads are R, G, B and the records equal those of melf_process_batch on the BGR frame of the s8."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402

# the layouts, restated from the bit table of include/meterelf_hip.h (drm_fourcc.h, ffmpeg's pixfmt.h): name -> (kind, pos of
# Y, U, V / R, G, B); aliases name the same layout
TABLE = {
    'vuya': ('yuv', (16, 8, 0)), 'ayuv': ('yuv', (8, 16, 24)), 'uyva': ('yuv', (8, 0, 16)), 'y410': ('yuv', (12, 2, 22)),
    'v30x': ('yuv', (14, 4, 24)), 'x2rgb10': ('rgb', (22, 12, 2)), 'x2bgr10': ('rgb', (2, 12, 22)),
}
ALIASES = {'vuyx': 'vuya', 'xv30': 'y410', 'xrgb2101010': 'x2rgb10', 'xbgr2101010': 'x2bgr10', 'r10g10b10a2': 'x2bgr10'}
YUV_FORMATS = tuple(f for (f, (k, _p)) in TABLE.items() if k == 'yuv')
RGB_FORMATS = tuple(f for (f, (k, _p)) in TABLE.items() if k == 'rgb')
FORMATS = YUV_FORMATS + RGB_FORMATS
MATRIX = 3   # BT.709 limited: what nearly all 10-bit material is


def kind_of(fmt):
    return TABLE[ALIASES.get(fmt, fmt)][0]


def pos_of(fmt):
    return TABLE[ALIASES.get(fmt, fmt)][1]


def matrix_of(fmt, matrix=MATRIX):
    """The matrix argument of the view and of the reader: the YUV formats', None for RGB."""
    return matrix if kind_of(fmt) == 'yuv' else None


def pack32(reads, pos, rng):
    """Three (n, H, W) uint8 planes in read order (Y, U, V / R, G, B) -> (n, H, W) uint32 words: read k at bits pos[k] .. pos[k] + 7,
    EVERY other bit random (alpha / X bits, the low bits of 10-bit fields)."""
    words = rng.integers(0, 2 ** 32, size=reads[0].shape, dtype=np.uint32)
    for (p8, p) in zip(reads, pos):
        words &= ~np.uint32(255 << p)
        words |= p8.astype(np.uint32) << np.uint32(p)
    return words


def unpack32(words, pos):
    """The inverse: -> the three reads, s8_k = (word >> pos[k]) & 255."""
    w = np.asarray(words).view(np.uint32)
    return tuple(((w >> np.uint32(p)) & np.uint32(255)).astype(np.uint8) for p in pos)


def reads_of(src, fmt):
    """The reads of a family's source in the descriptor's order: (Y, U, V) as they are, (bgr,) -> (R, G, B)."""
    if kind_of(fmt) == 'yuv':
        return src
    (bgr,) = src
    return (bgr[..., 2], bgr[..., 1], bgr[..., 0])


def conventional32(*args):
    """(*source, fmt, pad, rng) -> the array a caller would hold: (n, H, W) uint32, a [:, :, :W] view of an array whose rows are
    `pad` words longer (random filling)."""
    (src, fmt, pad, rng) = (args[:-3], args[-3], args[-2], args[-1])
    rng = rng if rng is not None else np.random.default_rng(0)
    reads = reads_of(src, fmt)
    (n, H, W) = reads[0].shape
    full = rng.integers(0, 2 ** 32, size=(n, H, W + pad), dtype=np.uint32)
    full[:, :, :W] = pack32(reads, pos_of(fmt), rng)
    return full[:, :, :W]


def descriptor(fmt, matrix, n, H, W, rp, fs, pos=None):
    (colour, p) = _hip.PACKED32_FORMATS[fmt]
    return _hip.MelfPacked32Frames(colour, matrix if colour == _hip.P32_YUV else 0, n, H, W, (_hip.C.c_int32 * 3)(*(pos or p)), rp, fs, 0, 0)


def pitched32(*args, row_pad=0, stride_pad=0, rng=None, matrix=MATRIX):
    """(*source, fmt) -> a byte buffer of exactly the descriptor's extent: rows row_pad bytes longer than their words, stride_pad
    bytes behind a frame (multiples of 4), random filling: (buffer, MelfPacked32Frames)."""
    (src, fmt) = (args[:-1], args[-1])
    rng = rng if rng is not None else np.random.default_rng(0)
    assert row_pad % 4 == 0 and stride_pad % 4 == 0
    reads = reads_of(src, fmt)
    (n, H, W) = reads[0].shape
    rows = np.ascontiguousarray(pack32(reads, pos_of(fmt), rng)).view(np.uint8).reshape(n, H, 4 * W)
    row = 4 * W
    rp = row + row_pad
    end = (H - 1) * rp + row
    fs = end + stride_pad
    raw = rng.integers(0, 256, size=(n - 1) * fs + end + 16, dtype=np.uint8)
    buf = raw[-raw.ctypes.data % 16:][:(n - 1) * fs + end]   # 16-byte aligned in host memory
    assert buf.ctypes.data % 16 == 0
    for f in range(n):
        np.lib.stride_tricks.as_strided(buf[f * fs:], shape=(H, row), strides=(rp, 1))[...] = rows[f]
    return buf, descriptor(fmt, matrix, n, H, W, rp, fs)


def extent32(d):
    return (d.n - 1) * d.frame_stride + (d.H - 1) * d.row_pitch + 4 * d.W


def view32(arr, fmt, matrix=MATRIX):
    return _hip.packed32_frames_view(arr, fmt, matrix_of(fmt, matrix))


def family(kind, matrix=MATRIX):
    """The fc.Family of one colour kind: 'yuv' (source (Y, U, V) at full resolution) or 'rgb' (source (bgr,))."""
    yuv = kind == 'yuv'
    return fc.Family(
        formats=YUV_FORMATS if yuv else RGB_FORMATS, view=lambda a, fmt: view32(a, fmt, matrix), host='process_packed32',
        dev='process_packed32_dev', read='read_packed32_frames', conventional=conventional32,
        pitched=lambda *a, **kw: pitched32(*a, matrix=matrix, **kw), desc_extent=extent32,
        from_bgr=(lambda bgr: fc.bgr_to_yuv(bgr, 0, 0, matrix)) if yuv else (lambda bgr: (bgr,)),
        bgr_of=(lambda Y, U, V: fc.yuv_to_bgr(Y, U, V, 0, 0, matrix)) if yuv else (lambda bgr: bgr),
        devbuf=fc.DevBuf, sub=(0, 0), check_pad=lambda fmt: 1, check_pitch=lambda k: dict(row_pad=4, stride_pad=4 * (k + 1)),
        resident_sync_call=True)


F32 = {'yuv': family('yuv'), 'rgb': family('rgb')}


class BoundReader:
    """A MeterReader whose read_packed32_frames(frames, fmt) passes the matrix the format needs: the shared bodies of frame_cases
    call a family's reader method with the array and the format name alone."""

    def __init__(self, reader, matrix=MATRIX):
        (self._reader, self._matrix) = (reader, matrix)

    def __getattr__(self, name):
        return getattr(self._reader, name)

    def read_packed32_frames(self, frames, fmt, **kw):
        return self._reader.read_packed32_frames(frames, fmt, matrix_of(fmt, self._matrix), **kw)


def want_8bit(reader, src, kind, matrix=MATRIX):
    """The expected records, from the EXISTING paths: 'yuv': read_yuv_planar_frames of the 8-bit i444 frames of the samples, 'rgb':
    read_frames of the BGR frames; both equal read_frames of the family's bgr_of (asserted)."""
    if kind == 'yuv':
        want = reader.read_yuv_planar_frames(fc.conventional_yuv_planar(*src, 'i444', 0, None), 'i444', matrix)
        assert reader.read_frames(fc.yuv_to_bgr(*src, 0, 0, matrix)).tobytes() == want.tobytes()
    else:
        want = reader.read_frames(np.ascontiguousarray(src[0]))
    return want
