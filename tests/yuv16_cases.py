"""What the tests of the 16-bit YUV frames (test_yuv16_frames, test_yuv16_dials) share, on top of tests.frame_cases: the reduction
restated, widening of 8-bit planes to 16-bit samples, the layout builders, the 8-bit descriptor of the same geometry, and the
comparison every GPU test makes.

The contract (include/meterelf_hip.h): a sample s is read as s8 = min(s >> shift, 255), and the records equal those of
melf_process_yuv_planar(_dev) on the 8-bit frame of the same geometry whose samples are s8.  Every byte quantity of a 16-bit
descriptor is even, so that 8-bit frame is the 16-bit buffer reduced sample by sample -- padding and all -- under the descriptor with
every byte quantity halved (desc8_of): nothing else has to be built to get the expected side."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402

FORMATS = _hip.YUV16_FORMATS          # name: (sub_y, c_step, V first, shift)
# one name per distinct (sub_y, c_step, shift): the aliases differ in nothing the library sees
DISTINCT = ('p010', 'p210', 'i010', 'i210', 'i012', 'i212', 'yuv420p16le', 'yuv422p16le')


def reduce16(s, shift):
    """The reduction restated: uint16 samples -> uint8, min(s >> shift, 255)."""
    s = np.asarray(s, dtype=np.uint16).astype(np.uint32) >> shift
    return np.where(s > 255, 255, s).astype(np.uint8)


def widen(p8, shift, rng, garbage=False):
    """uint8 samples -> uint16 samples that reduce to them: the value in bits shift .. shift + 7, the `shift` dropped low bits random.
    garbage (LSB-aligned data, shift < 8): one sample in eight also carries random bits above the value -- out of spec; those reduce
    to 255 (the clamp), which the expected side gets from reduce16 like everything else."""
    s = p8.astype(np.uint16) << shift
    if shift:
        s |= rng.integers(0, 1 << shift, size=p8.shape, dtype=np.uint16)
    if garbage:
        assert shift < 8
        hit = rng.integers(0, 8, size=p8.shape) == 0
        s[hit] |= (rng.integers(1, 1 << (8 - shift), size=int(hit.sum()), dtype=np.uint16) << (8 + shift)).astype(np.uint16)
    return s


def widen_planes(src8, fmt, rng, garbage=False):
    shift = FORMATS[fmt][3]
    return tuple(widen(p, shift, rng, garbage) for p in src8)


def rows_of(fmt, H):
    return H + (H >> FORMATS[fmt][0])


def conventional16(Y, U, V, fmt, pad=0, rng=None):
    """The raw-video (N, rows, W) uint16 array of 16-bit planes in layout fmt; pad > 0: a [:, :, :W] view of an array whose rows are
    pad samples longer (random filling) -- semi-planar layouts only (a planar chroma row is half a row of the array)."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (sy, step, vfirst, _shift) = FORMATS[fmt]
    (n, H, W) = Y.shape
    full = rng.integers(0, 65536, size=(n, rows_of(fmt, H), W + pad), dtype=np.uint16)
    out = full[:, :, :W]
    out[:, :H] = Y
    (first, second) = (V, U) if vfirst else (U, V)
    if step == 2:
        out[:, H:, 0::2] = first
        out[:, H:, 1::2] = second
    else:
        assert pad == 0
        q = (H >> sy) * (W // 2)
        flat = out.reshape(n, -1)
        flat[:, H * W:H * W + q] = first.reshape(n, -1)
        flat[:, H * W + q:] = second.reshape(n, -1)
    return out


def pitched16(Y, U, V, fmt, y_pad=0, c_pad=0, gap=0, stride_pad=0, rng=None, matrix=3, lead=0, vfirst=None):
    """A buffer of exactly the descriptor's extent (+ lead bytes in front of the base) with padded pitches: (uint16 array whose
    bytes are the buffer, MelfYuv16Frames, lead).  Every pad counts BYTES and is even; gap: bytes between the planes' spans."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (sy, step, vf, shift) = FORMATS[fmt]
    vfirst = vf if vfirst is None else vfirst
    assert (y_pad | c_pad | gap | stride_pad | lead) % 2 == 0
    (n, H, W) = Y.shape
    (ch, cw) = (H >> sy, (W // 2) * step)                # chroma rows, samples of a chroma row (semi-planar: of both)
    (yp, cp) = (W + y_pad // 2, cw + c_pad // 2)         # in samples from here on
    c0 = (H - 1) * yp + W + gap // 2
    if step == 2:
        (uo, vo) = (c0 + 1, c0) if vfirst else (c0, c0 + 1)
        end = c0 + (ch - 1) * cp + cw
    else:
        c1 = c0 + (ch - 1) * cp + cw + gap // 2
        (uo, vo) = (c1, c0) if vfirst else (c0, c1)
        end = c1 + (ch - 1) * cp + cw
    fs = end + stride_pad // 2
    raw = rng.integers(0, 65536, size=lead // 2 + (n - 1) * fs + end, dtype=np.uint16)
    buf = raw[lead // 2:]
    for f in range(n):
        o = f * fs
        np.lib.stride_tricks.as_strided(buf[o:], shape=(H, W), strides=(2 * yp, 2))[...] = Y[f]
        np.lib.stride_tricks.as_strided(buf[o + uo:], shape=(ch, W // 2), strides=(2 * cp, 2 * step))[...] = U[f]
        np.lib.stride_tricks.as_strided(buf[o + vo:], shape=(ch, W // 2), strides=(2 * cp, 2 * step))[...] = V[f]
    desc = _hip.MelfYuv16Frames(matrix, n, H, W, sy, step, shift, 0, 2 * yp, 2 * cp, 2 * uo, 2 * vo, 2 * fs)
    return raw, desc, lead


def extent16(d):
    """Bytes from the base to the end of the last frame's last sample."""
    ch = d.H >> d.sub_y
    last = max(d.u_offset, d.v_offset) + (ch - 1) * d.c_pitch + ((d.W // 2 - 1) * d.c_step + 1) * 2
    return (d.n - 1) * d.frame_stride + last


def desc8_of(d):
    """The 8-bit descriptor (melf_process_yuv_planar*) of the same geometry: every byte quantity halved."""
    return _hip.MelfYuvPlanarFrames(d.matrix, d.n, d.H, d.W, 1, d.sub_y, d.c_step, 0, d.y_pitch // 2, d.c_pitch // 2, d.u_offset // 2,
                                    d.v_offset // 2, d.frame_stride // 2)


def samples_at(ptr, extent):
    """The uint16 samples of the `extent` bytes at host address ptr (a copy)."""
    return np.frombuffer((C.c_uint8 * extent).from_address(ptr), np.uint16).copy()


def want_8bit(ctx, ptr, desc, extent):
    """The expected records: melf_process_yuv_planar_dev on the reduced buffer, a device buffer of exactly its extent."""
    b8 = reduce16(samples_at(ptr, extent), desc.shift)
    d8 = desc8_of(desc)
    assert b8.nbytes == fc.extent_yuv_planar(d8) == extent // 2
    buf = fc.DevBuf(b8.ctypes.data, b8.nbytes)
    try:
        return ctx.process_yuv_planar_dev(buf.d.value, d8)
    finally:
        buf.free()


def read_all(ctx, ptr, desc, extent, devbuf=fc.DevBuf, phase=None, host=True):
    """(records of melf_process_yuv16_dev on a device buffer of exactly `extent` bytes, of melf_process_yuv16 or None, the dial
    family the device call ran)."""
    assert extent == extent16(desc)
    buf = devbuf(ptr, extent) if phase is None else devbuf(ptr, extent, phase)
    try:
        dev = ctx.process_yuv16_dev(buf.d.value, desc)
        fam = ctx.last_dials()['family']
    finally:
        buf.free()
    return dev, (ctx.process_yuv16(ptr, desc) if host else None), fam


def check_identity(ctx, ptr, desc, extent, tag, want=None, **kw):
    """The 16-bit device and host paths against the 8-bit path on the reduced buffer, as bytes.  Returns the expected records."""
    if want is None:
        want = want_8bit(ctx, ptr, desc, extent)
    (dev, host, fam) = read_all(ctx, ptr, desc, extent, **kw)
    assert fam == 'yuv16_step%d' % desc.c_step, (tag, fam)
    assert dev.tobytes() == want.tobytes(), (tag, 'device', int((dev != want).sum()))
    if host is not None:
        assert host.tobytes() == want.tobytes(), (tag, 'host')
    return want


def planes_of(bgr, fmt, matrix=None):
    """Test input: the 8-bit (Y, U, V) planes of BGR frames at the format's subsampling (frame_cases.bgr_to_yuv)."""
    return fc.bgr_to_yuv(bgr, 1, FORMATS[fmt][0], matrix)


def bgr_of(src8, fmt, matrix):
    return fc.yuv_to_bgr(*src8, 1, FORMATS[fmt][0], matrix)
