"""What the tests of the packed 10-bit YUV 4:2:2 frames (test_yuv422_10_frames, test_yuv422_10_dials) share, on top of
tests.frame_cases: the two layouts restated in numpy (packers and their inverses), the pitched-buffer builder, a Family record so
that the shared bodies of frame_cases run on the new family, and the comparison every GPU test makes.

The contract (include/meterelf_hip.h): every sample is read as its top 8 bits -- v210: s8 = (field >> 2) & 255 of a 10-bit field,
Y210 / Y212 / Y216: s8 = s >> 8 of a 16-bit word -- and the records equal those of melf_process_yuv422(_dev) on the 8-bit YUYV frame
with the same n, H, W and matrix whose samples are the s8, and so those of melf_process_batch on the BGR frame the integer
conversion (frame_cases.yuv_to_bgr) makes of it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402

FORMATS = ('v210', 'y210')
MATRIX = 3   # BT.709 limited: what nearly all 10-bit material is

# v210: where the samples of pair q of a group lie, (word, bit offset) -- the table of include/meterelf_hip.h, written out
V210_TABLE = {
    0: dict(y0=(0, 10), y1=(1, 0), u=(0, 0), v=(0, 20)),
    1: dict(y0=(1, 20), y1=(2, 10), u=(1, 10), v=(2, 0)),
    2: dict(y0=(3, 0), y1=(3, 20), u=(2, 20), v=(3, 10)),
}


def v210_groups(W):
    return (W + 5) // 6


def v210_row_bytes(W):
    return v210_groups(W) * 16


def v210_pitch(W):
    """The conventional pitch of a v210 row, in bytes."""
    return (W + 47) // 48 * 128


def pack_v210(Y8, U8, V8, rng, garbage=False):
    """(n, H, W) Y and (n, H, W / 2) U, V uint8 -> (n, H, 4 * ceil(W / 6)) uint32 v210 words: field = s8 << 2 | two random low
    bits.  garbage: bits 30-31 of every word are random and so are the fields of pixels >= W in a row's last group (zero
    otherwise)."""
    (n, H, W) = Y8.shape
    assert W % 2 == 0 and U8.shape == V8.shape == (n, H, W // 2)
    G = v210_groups(W)

    def fields(p8, count):
        f = np.zeros((n, H, count), np.uint32)
        if garbage:
            f[...] = rng.integers(0, 1024, size=f.shape, dtype=np.uint32)
        k = p8.shape[2]
        f[:, :, :k] = (p8.astype(np.uint32) << 2) | rng.integers(0, 4, size=p8.shape, dtype=np.uint32)
        return f
    (Yf, Uf, Vf) = (fields(Y8, 6 * G), fields(U8, 3 * G), fields(V8, 3 * G))
    words = np.zeros((n, H, G, 4), np.uint32)
    if garbage:
        words |= rng.integers(0, 4, size=words.shape, dtype=np.uint32) << 30
    for (q, t) in V210_TABLE.items():
        for (key, plane) in (('y0', Yf[:, :, 2 * q::6]), ('y1', Yf[:, :, 2 * q + 1::6]), ('u', Uf[:, :, q::3]), ('v', Vf[:, :, q::3])):
            (w, bit) = t[key]
            words[:, :, :, w] |= plane << bit
    return words.reshape(n, H, 4 * G)


def unpack_v210(words, W):
    """The inverse: (n, H, >= 4 * ceil(W / 6)) uint32 -> (Y8, U8, V8), s8 = (field >> 2) & 255."""
    (n, H, _) = words.shape
    G = v210_groups(W)
    g = np.asarray(words)[:, :, :4 * G].reshape(n, H, G, 4).astype(np.uint32)
    (Y, U, V) = (np.zeros((n, H, 6 * G), np.uint8), np.zeros((n, H, 3 * G), np.uint8), np.zeros((n, H, 3 * G), np.uint8))
    for (q, t) in V210_TABLE.items():
        def s8(key):
            (w, bit) = t[key]
            return (((g[:, :, :, w] >> bit) & 1023) >> 2).astype(np.uint8)
        Y[:, :, 2 * q::6] = s8('y0')
        Y[:, :, 2 * q + 1::6] = s8('y1')
        U[:, :, q::3] = s8('u')
        V[:, :, q::3] = s8('v')
    return Y[:, :, :W], U[:, :, :W // 2], V[:, :, :W // 2]


def pack_y210(Y8, U8, V8, rng):
    """-> (n, H, W, 2) uint16, the words of a macropixel Y0 U Y1 V: the sample in the high byte, a random low byte (Y210 keeps
    6 low bits zero, Y212 4, Y216 none: under truncation the three are one format, and random bits cover them all)."""
    (n, H, W) = Y8.shape
    out = rng.integers(0, 256, size=(n, H, W, 2), dtype=np.uint16)
    out[..., 0] |= Y8.astype(np.uint16) << 8
    out[:, :, 0::2, 1] |= U8.astype(np.uint16) << 8
    out[:, :, 1::2, 1] |= V8.astype(np.uint16) << 8
    return out


def unpack_y210(words):
    w = np.asarray(words).view(np.uint16)
    return (w[..., 0] >> 8).astype(np.uint8), (w[:, :, 0::2, 1] >> 8).astype(np.uint8), (w[:, :, 1::2, 1] >> 8).astype(np.uint8)


class WithWidth(np.ndarray):
    """A v210 array that remembers its width in pixels (the array of words does not say it)."""
    width = None


def conventional10(Y, U, V, fmt, pad=0, rng=None, garbage=True):
    """The array a caller would hold: v210 (n, H, row_words) uint32 at the conventional pitch plus `pad` groups; y210 (n, H, W, 2)
    uint16, a [:, :, :W] view of an array whose rows are `pad` macropixels longer."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W) = Y.shape
    if fmt == 'v210':
        packed = pack_v210(Y, U, V, rng, garbage)
        full = rng.integers(0, 2 ** 32, size=(n, H, v210_pitch(W) // 4 + 4 * pad), dtype=np.uint32)
        full[:, :, :packed.shape[2]] = packed
        out = full.view(WithWidth)
        out.width = W
        return out
    full = rng.integers(0, 65536, size=(n, H, W + 2 * pad, 2), dtype=np.uint16)
    full[:, :, :W] = pack_y210(Y, U, V, rng)
    return full[:, :, :W]


def view10(arr, fmt, matrix=MATRIX):
    return _hip.yuv422_10_frames_view(arr, fmt, matrix, width=getattr(arr, 'width', None))


def pitched10(Y, U, V, fmt, row_pad=0, stride_pad=0, rng=None, matrix=MATRIX, garbage=True):
    """A byte buffer of exactly the descriptor's extent: rows row_pad bytes longer than their groups / macropixels, stride_pad
    bytes behind a frame (both multiples of 16 for v210, of 8 for y210), random filling: (buffer, MelfYuv422_10Frames)."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W) = Y.shape
    align = 16 if fmt == 'v210' else 8
    assert row_pad % align == 0 and stride_pad % align == 0
    rows = (pack_v210(Y, U, V, rng, garbage) if fmt == 'v210' else pack_y210(Y, U, V, rng)).reshape(n, H, -1).view(np.uint8)
    row = rows.shape[2]
    assert row == (v210_row_bytes(W) if fmt == 'v210' else 4 * W)
    rp = row + row_pad
    end = (H - 1) * rp + row
    fs = end + stride_pad
    raw = rng.integers(0, 256, size=(n - 1) * fs + end + 16, dtype=np.uint8)
    buf = raw[-raw.ctypes.data % 16:][:(n - 1) * fs + end]   # 16-byte aligned in host memory
    assert buf.ctypes.data % 16 == 0
    for f in range(n):
        np.lib.stride_tricks.as_strided(buf[f * fs:], shape=(H, row), strides=(rp, 1))[...] = rows[f]
    return buf, _hip.MelfYuv422_10Frames(_hip.YUV422_10_FORMATS[fmt], matrix, n, H, W, 0, rp, fs)


def extent10(d):
    row = v210_row_bytes(d.W) if d.format == _hip.YUV422_10_V210 else 4 * d.W
    return (d.n - 1) * d.frame_stride + (d.H - 1) * d.row_pitch + row


def family(matrix=MATRIX):
    return fc.Family(
        formats=FORMATS, view=lambda a, fmt: view10(a, fmt, matrix), host='process_yuv422_10', dev='process_yuv422_10_dev',
        read='read_yuv422_10_frames', conventional=conventional10,
        pitched=lambda *a, **kw: pitched10(*a, matrix=matrix, **kw), desc_extent=extent10,
        from_bgr=lambda bgr: fc.bgr_to_yuv(bgr, 1, 0, matrix), bgr_of=lambda Y, U, V: fc.yuv_to_bgr(Y, U, V, 1, 0, matrix),
        devbuf=fc.DevBuf, sub=(1, 0), check_pad=lambda fmt: 1, check_pitch=lambda k: dict(row_pad=16 - 8 * k, stride_pad=32),   # (k: the format's position: one group, one macropixel)
        resident_sync_call=True)


F10 = family()


def want_8bit(reader, src8, matrix=MATRIX):
    """The expected records, from the 8-bit side: read_yuv422_frames of the YUYV frames of the samples; they equal read_frames of
    the BGR frames frame_cases.yuv_to_bgr makes of them (asserted)."""
    want = reader.read_yuv422_frames(fc.packed422(*src8, 'yuyv'), 'yuyv', matrix)
    assert reader.read_frames(fc.yuv_to_bgr(*src8, 1, 0, matrix)).tobytes() == want.tobytes()
    return want


def read_all(ctx, ptr, desc, extent, devbuf=fc.DevBuf, host=True):
    """(records of the device path on a device buffer of exactly `extent` bytes, of the host path or None, the dial family the
    device call ran)."""
    assert extent == extent10(desc)
    buf = devbuf(ptr, extent)
    try:
        dev = ctx.process_yuv422_10_dev(buf.d.value, desc)
        fam = ctx.last_dials()['family']
    finally:
        buf.free()
    return dev, (ctx.process_yuv422_10(ptr, desc) if host else None), fam


def check_identity(ctx, ptr, desc, extent, want, tag, **kw):
    (dev, host, fam) = read_all(ctx, ptr, desc, extent, **kw)
    assert fam == ('v210' if desc.format == _hip.YUV422_10_V210 else 'y210'), (tag, fam)
    assert dev.tobytes() == want.tobytes(), (tag, 'device', int((dev != want).sum()))
    if host is not None:
        assert host.tobytes() == want.tobytes(), (tag, 'host', int((host != want).sum()))
