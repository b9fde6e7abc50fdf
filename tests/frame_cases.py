"""What the frame-format tests share: the fixtures' readers, device buffers of exact extent (DevBuf: two placements), frame synthesis, the integer YUV -> BGR
conversion of include/meterelf_hip.h restated once, the layout builders of every family, a record per family that names its entry
points, and the test bodies that are the same for every family once those names are given.

The files that use it -- test_pixel_formats, test_planar_frames, test_yuv_frames, test_yuv422_frames, test_yuv_matrices,
test_yuv_planar_frames, test_host_staging, test_dials_instantiations -- keep their contracts, their CPU tests, their case lists and
every literal (seeds, pads, gaps, batch sizes, thresholds); a test there calls a body here with its family and those literals.

Device frames without torch come from the HIP runtime the library is bound to (tests.helpers.hip_runtime).  The torch paths run in
a child process, `python tests/frame_cases.py torch <family>`, that imports torch before the package loads the library, as a torch
program does (bench.py): a process that loaded the library first holds a second HIP runtime once torch loads its own, and torch's
streams would be foreign to it.
"""
import ctypes as C
import functools
import glob
import os
import shutil
import subprocess
import sys
from typing import Callable, NamedTuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402


# ---------------------------------------------------------------------------------------------------- readers and buffers ---
@pytest.fixture(scope='module')
def env():
    """Per fixture set: its parameter file, parameters, frames and a reader.  Module-scoped: every file that imports it gets
    readers of its own."""
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    from meterelf_amd._image import imread_bgr
    out = {}
    for sd in ('sample-images1', 'sample-images2'):
        pfile = os.path.join(GOLDEN, sd, 'params.yml')
        params = _params.load(pfile)
        frames = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(GOLDEN, sd, '*.jpg')))]
        out[sd] = dict(pfile=pfile, params=params, frames=frames, reader=MeterReader(params))
    yield out
    for e in out.values():
        e['reader'].close()


def hip_rt():
    from tests.helpers import hip_runtime
    return hip_runtime()


class DevBuf:
    """Device copy of `nbytes` bytes at host address `ptr`.  Two placements, which are not interchangeable (what lies behind the
    copy differs, and so what a load past the extent would hit):

    DevBuf(ptr, nbytes): an allocation of exactly nbytes bytes, the copy at its start.
    DevBuf.at_end(ptr, nbytes, phase=None): an allocation of whole 4 KiB pages, the copy ending where it ends.  phase 0..3: the
    copy's address has that residue modulo 4 instead, as close to the allocation's end as that allows (at most 3 bytes of it left
    behind the copy)."""

    def __init__(self, ptr, nbytes, _at_end=False, _phase=None):
        self.hip = hip_rt()
        self.base = C.c_void_p()
        alloc = (nbytes + 3 + 4095) // 4096 * 4096 if _at_end else max(nbytes, 1)
        assert self.hip.hipMalloc(C.byref(self.base), C.c_size_t(alloc)) == 0
        at = alloc - nbytes if _at_end else 0
        if _phase is not None:
            at -= (self.base.value + at - _phase) % 4
        assert at >= 0
        self.d = C.c_void_p(self.base.value + at)
        assert self.hip.hipMemcpy(self.d, C.c_void_p(ptr), C.c_size_t(nbytes), 1) == 0

    @classmethod
    def at_end(cls, ptr, nbytes, phase=None):
        return cls(ptr, nbytes, True, phase)

    def free(self):
        self.hip.hipFree(self.base)


def synth(frames, n, seed):
    """n shifted + noisy fixture frames, every 9th a constant frame (Dials not found)."""
    rng = np.random.default_rng(seed)
    shapes = [f.shape for f in frames]
    base = [f for f in frames if f.shape == max(set(shapes), key=shapes.count)]   # the fixture's frame size
    out = np.empty((n,) + base[0].shape, np.uint8)
    for i in range(n):
        if i % 9 == 4:
            out[i] = 128
            continue
        (dx, dy) = rng.integers(-8, 9, size=2)
        img = np.roll(base[i % len(base)], (int(dy), int(dx)), axis=(0, 1)).astype(np.int16)
        img += rng.integers(-2, 3, size=img.shape).astype(np.int16)
        out[i] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def params_with_rect(tmp_path, sd, rect, tag):
    """The parameters of fixture set sd with meter_rect (x0, y0, x1, y1)."""
    import yaml
    from meterelf_amd import _params
    src = os.path.join(GOLDEN, sd)
    with open(os.path.join(src, 'params.yml')) as fp:
        data = yaml.safe_load(fp)
    data['meter_rect'] = {'top_left': [rect[0], rect[1]], 'bottom_right': [rect[2], rect[3]]}
    d = tmp_path / tag
    d.mkdir()
    with open(d / 'params.yml', 'w') as fp:
        yaml.safe_dump(data, fp)
    shutil.copy(os.path.join(src, 'dials_gray.png'), d / 'dials_gray.png')
    return _params.load(str(d / 'params.yml'))


# ------------------------------------------------------------------------------------------------ stand-alone programs ---
def build_and_run(tmp_path, cxx, src, name, extra, san):
    """src as a stand-alone program, plain and under the host sanitizers `san`: both exit 0 and print `failures 0`.  Returns
    the plain run's output."""
    out = None
    for (tag, flags) in (('plain', ['-O2']), ('san', ['-O1', '-g', '-fno-sanitize-recover=all'] + san)):
        exe = str(tmp_path / (name + '_' + tag))
        subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror'] + extra + flags + ['-o', exe, src])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        assert p.returncode == 0, (tag, p.stdout[-2000:], p.stderr[-4000:])
        assert b'failures 0' in p.stdout, p.stdout
        print(tag, p.stdout.decode().strip())
        out = out or p.stdout.decode()
    return out


# ------------------------------------------------------------------------------------------------- the conversion, restated ---
# matrix code: (YOFF, CY, CRV, CGV, CGU, CBU) of include/meterelf_hip.h's table
MATRIX = {
    0: (16, 1220542, 1673527, -852492, -409993, 2116026),
    2: (0, 1048576, 1470104, -748826, -360853, 1858077),
    3: (16, 1220945, 1879825, -558796, -223607, 2215014),
    4: (0, 1048576, 1651297, -490864, -196424, 1945738),
}
# matrix code: (Kr, Kb, limited range) of the standard
STANDARD = {0: (0.299, 0.114, True), 2: (0.299, 0.114, False), 3: (0.2126, 0.0722, True), 4: (0.2126, 0.0722, False)}


def yuv_to_bgr(Y, U, V, sub_x, sub_y, matrix=0):
    """Y (..., H, W), U and V (..., H >> sub_y, W >> sub_x) uint8 -> (..., H, W, 3) uint8 BGR: the header's integer arithmetic
    (>> is the arithmetic shift) under matrix code `matrix`, with the NEAREST chroma sample: pixel (x, y) uses
    U[y >> sub_y][x >> sub_x] and V[..].  The expected side of every YUV comparison.

        yy = max(Y - YOFF, 0) * CY        u = U - 128        v = V - 128
        R = clamp((yy + (1 << 19) + CRV * v)           >> 20, 0, 255)
        G = clamp((yy + (1 << 19) + CGV * v + CGU * u) >> 20, 0, 255)
        B = clamp((yy + (1 << 19) + CBU * u)           >> 20, 0, 255)

    Every sum stays below 2^30 (test_yuv_matrices.py::test_conversion_bounds_all_triples), so int32 holds it."""
    (yoff, cy, crv, cgv, cgu, cbu) = MATRIX[matrix]
    yy = np.maximum(Y.astype(np.int32) - yoff, 0) * cy + (1 << 19)

    def up(p):
        p = p.astype(np.int32) - 128
        if sub_y:
            p = np.repeat(p, 2, axis=-2)
        if sub_x:
            p = np.repeat(p, 2, axis=-1)
        return p
    (u, v) = (up(U), up(V))
    out = np.empty(Y.shape + (3,), np.uint8)
    out[..., 2] = np.clip((yy + crv * v) >> 20, 0, 255)
    out[..., 1] = np.clip((yy + cgv * v + cgu * u) >> 20, 0, 255)
    out[..., 0] = np.clip((yy + cbu * u) >> 20, 0, 255)
    return out


def _ycbcr(bgr, matrix):
    """Full-resolution float64 (y, u, v) of BGR frames.  matrix None: BT.601 limited range from the three-decimal constants, as the
    format files have always made their input; a matrix code: from Kr and Kb of STANDARD[code] (test_yuv_matrices.py).  For
    BT.601 limited the two differ in the last bit of a few chroma samples."""
    f = bgr.astype(np.float64)
    (b, g, r) = (f[..., 0], f[..., 1], f[..., 2])
    if matrix is None:
        return (16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0, 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0,
                128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0)
    (kr, kb, limited) = STANDARD[matrix]
    yl = kr * r + (1.0 - kr - kb) * g + kb * b
    (pb, pr) = ((b - yl) / (2.0 * (1.0 - kb)), (r - yl) / (2.0 * (1.0 - kr)))
    if limited:
        return 16.0 + yl * 219.0 / 255.0, 128.0 + pb * 224.0 / 255.0, 128.0 + pr * 224.0 / 255.0
    return yl, 128.0 + pb, 128.0 + pr


def bgr_to_yuv(bgr, sub_x, sub_y, matrix=None):
    """Test input only, nothing is compared against it: (..., H, W, 3) BGR -> Y (..., H, W), U and V (..., H >> sub_y, W >> sub_x)
    uint8: float64 RGB -> YUV (_ycbcr), the mean of each chroma block, round half up, clip.  Batches go in chunks of 16 frames."""
    def q(p):
        return np.clip(np.floor(p + 0.5), 0, 255).astype(np.uint8)

    def mean(p):
        if sub_x and sub_y:
            return (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]) / 4.0
        if sub_y:
            return (p[..., 0::2, :] + p[..., 1::2, :]) / 2.0
        if sub_x:
            return (p[..., 0::2] + p[..., 1::2]) / 2.0
        return p
    if bgr.ndim == 4 and len(bgr) > 16:
        parts = [bgr_to_yuv(bgr[i:i + 16], sub_x, sub_y, matrix) for i in range(0, len(bgr), 16)]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    (y, u, v) = _ycbcr(bgr, matrix)
    return q(y), q(mean(u)), q(mean(v))


# ------------------------------------------------------------------------------------------------------- layout builders ---
PACKED_ORDER = {'bgr': [0, 1, 2], 'rgb': [2, 1, 0], 'bgra': [0, 1, 2], 'rgba': [2, 1, 0]}
YUV_PLANAR_FORMATS = getattr(_hip, 'YUV_PLANAR_FORMATS', {})   # name: (sub_x, sub_y, c_step, V first)


def to_layout(bgr, fmt, pad=0, rng=None, view3=False):
    """Packed pixels: the frames `bgr` (N, H, W, 3) in layout `fmt`, rows padded by `pad` pixels (a [:, :, :W] view of a wider
    array), the 4th byte random; view3: a 4-byte layout handed over as its 3-channel view (rgba[..., :3])."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W, _) = bgr.shape
    ch = 4 if fmt in ('bgra', 'rgba') else 3
    full = rng.integers(0, 256, size=(n, H, W + pad, ch), dtype=np.uint8)
    full[:, :, :W, :3] = bgr[..., PACKED_ORDER[fmt]]
    out = full[:, :, :W]
    if view3 and ch == 4:
        return out[..., :3], fmt[:3]
    return out, fmt


def read_packed_dev(ctx, v, **kw):
    """Packed pixels: the records of the device path for the view v of host frames, from an allocation of its extent with the copy at
    its start (the runtime rounds the allocation up to whole pages: what lies behind the copy is mapped; buffer_ends places copies
    where the mapping ends)."""
    buf = DevBuf(v.ptr, v.extent)
    try:
        return ctx.process_frames_dev(buf.d.value, v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride, **kw)
    finally:
        buf.free()


def pitched_packed(bgr, fmt, row_pad=0, rng=None):
    """Packed pixels: a byte buffer of exactly the descriptor's extent, rows row_pad bytes longer than W pixels (a multiple of 4
    for the 4-byte layouts), the frames back to back (frame_stride = one frame's extent: the last row unpadded), random filling:
    (buffer, the arguments of process_frames_dev behind the pointer)."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W, _c) = bgr.shape
    px = to_layout(bgr, fmt, 0, rng)[0]
    ch = px.shape[-1]
    assert ch == 3 or row_pad % 4 == 0
    rp = W * ch + row_pad
    fs = (H - 1) * rp + W * ch
    buf = rng.integers(0, 256, size=n * fs, dtype=np.uint8)
    for f in range(n):
        np.lib.stride_tricks.as_strided(buf[f * fs:], shape=(H, W * ch), strides=(rp, 1))[...] = px[f].reshape(H, W * ch)
    return buf, (getattr(_hip, 'PIX_' + fmt.upper()), n, H, W, rp, fs)


def conventional420(Y, U, V, fmt, pad=0, rng=None):
    """4:2:0: the (N, H * 3 // 2, W) array of the planes in layout fmt ('nv12' / 'i420' / 'yv12'); pad > 0: a [:, :, :W] view of
    an array whose rows are pad bytes longer (random filling)."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W) = Y.shape
    full = rng.integers(0, 256, size=(n, H * 3 // 2, W + pad), dtype=np.uint8)
    out = full[:, :, :W]
    out[:, :H] = Y
    if fmt == 'nv12':
        out[:, H:, 0::2] = U
        out[:, H:, 1::2] = V
    else:
        assert pad == 0
        (first, second) = (V, U) if fmt == 'yv12' else (U, V)
        q = H * W // 4
        flat = out.reshape(n, -1)
        flat[:, H * W:H * W + q] = first.reshape(n, -1)
        flat[:, H * W + q:] = second.reshape(n, -1)
    return out


def pitched420(Y, U, V, fmt, y_pad=0, c_pad=0, gap=0, stride_pad=0, rng=None, matrix=0):
    """4:2:0: a byte buffer of exactly the descriptor's extent with padded pitches: (buffer, MelfYuvFrames).  gap: bytes between
    the planes; yv12: V before U."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W) = Y.shape
    nv12 = fmt == 'nv12'
    (yp, cw) = (W + y_pad, W if nv12 else W // 2)
    cp = cw + c_pad
    c0 = H * yp + gap
    if nv12:
        c0 += c0 & 1   # NV12: u_offset is even
        (uo, vo, end) = (c0, c0 + 1, c0 + (H // 2 - 1) * cp + cw)
    else:
        c1 = c0 + (H // 2) * cp + gap
        (uo, vo) = (c1, c0) if fmt == 'yv12' else (c0, c1)
        end = c1 + (H // 2 - 1) * cp + cw
    fs = end + stride_pad
    buf = rng.integers(0, 256, size=(n - 1) * fs + end, dtype=np.uint8)
    for f in range(n):
        o = f * fs
        for y in range(H):
            buf[o + y * yp:o + y * yp + W] = Y[f, y]
        for y in range(H // 2):
            if nv12:
                buf[o + uo + y * cp:o + uo + y * cp + W:2] = U[f, y]
                buf[o + vo + y * cp:o + vo + y * cp + W - 1:2] = V[f, y]
            else:
                buf[o + uo + y * cp:o + uo + y * cp + cw] = U[f, y]
                buf[o + vo + y * cp:o + vo + y * cp + cw] = V[f, y]
    return buf, _hip.MelfYuvFrames(_hip.YUV_CODES[fmt], matrix, n, H, W, 0, yp, cp, uo, vo, fs)


def extent420(d):
    nv12 = d.format == _hip.YUV_NV12
    last = max(d.u_offset, d.v_offset) + (d.H // 2 - 1) * d.c_pitch + (d.W - 1 if nv12 else d.W // 2)
    return (d.n - 1) * d.frame_stride + last


def fill422(out, Y, U, V, fmt):
    """Writes the samples into out (..., H, W, 2) in layout fmt.  Bytes of a macropixel (pixels 2 k, 2 k + 1 of a row):
    yuyv: Y0 U Y1 V    uyvy: U Y0 V Y1    yvyu: Y0 V Y1 U"""
    assert fmt in ('yuyv', 'uyvy', 'yvyu')
    (yb, cb) = (1, 0) if fmt == 'uyvy' else (0, 1)
    (first, second) = (V, U) if fmt == 'yvyu' else (U, V)
    out[..., yb] = Y
    out[..., 0::2, cb] = first
    out[..., 1::2, cb] = second
    return out


def packed422(Y, U, V, fmt):
    (n, H, W) = Y.shape
    return fill422(np.empty((n, H, W, 2), np.uint8), Y, U, V, fmt)


def conventional422(Y, U, V, fmt, pad=0, rng=None):
    """Packed 4:2:2: the (N, H, W, 2) array of the samples in layout fmt; pad > 0: a [:, :, :W] view of an array whose rows are
    pad pixels longer (random filling; pad even, so that the rows stay 4-byte aligned)."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W) = Y.shape
    assert pad % 2 == 0
    full = rng.integers(0, 256, size=(n, H, W + pad, 2), dtype=np.uint8)
    return fill422(full[:, :, :W], Y, U, V, fmt)


def pitched422(Y, U, V, fmt, row_pad=0, stride_pad=0, rng=None, matrix=0):
    """Packed 4:2:2: a byte buffer of exactly the descriptor's extent with padded rows and a padded frame stride: (buffer,
    MelfYuv422Frames).  row_pad, stride_pad: bytes, multiples of 4."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W) = Y.shape
    assert row_pad % 4 == 0 and stride_pad % 4 == 0
    rp = 2 * W + row_pad
    end = (H - 1) * rp + 2 * W
    fs = end + stride_pad
    buf = rng.integers(0, 256, size=(n - 1) * fs + end, dtype=np.uint8)
    assert buf.ctypes.data % 4 == 0
    rows = packed422(Y, U, V, fmt).reshape(n, H, 2 * W)
    for f in range(n):
        for y in range(H):
            o = f * fs + y * rp
            buf[o:o + 2 * W] = rows[f, y]
    return buf, _hip.MelfYuv422Frames(_hip.YUV422_CODES[fmt], matrix, n, H, W, 0, rp, fs)


def extent422(d):
    return (d.n - 1) * d.frame_stride + (d.H - 1) * d.row_pitch + 2 * d.W


def rows_of(fmt, H):
    (sx, sy, _step, _vf) = YUV_PLANAR_FORMATS[fmt]
    return H + 2 * (H >> sy) // (1 << sx)


def conventional_yuv_planar(Y, U, V, fmt, pad=0, rng=None):
    """Planar / semi-planar YUV: the raw-video (N, rows, W) array of the planes in layout fmt; pad > 0: a [:, :, :W] view of an
    array whose rows are pad bytes longer (random filling) -- only for the layouts whose chroma rows are whole rows of the array."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (sx, sy, step, vfirst) = YUV_PLANAR_FORMATS[fmt]
    (n, H, W) = Y.shape
    (ch, cw) = (H >> sy, W >> sx)
    rows = rows_of(fmt, H)
    full = rng.integers(0, 256, size=(n, rows, W + pad), dtype=np.uint8)
    out = full[:, :, :W]
    out[:, :H] = Y
    (first, second) = (V, U) if vfirst else (U, V)
    if step == 2:
        if cw * 2 == W:
            out[:, H:, 0::2] = first
            out[:, H:, 1::2] = second
        else:   # 4:4:4: a chroma row is two rows of the array
            assert pad == 0
            c = out[:, H:].reshape(n, ch, 2 * cw)
            c[:, :, 0::2] = first
            c[:, :, 1::2] = second
    elif cw == W:
        out[:, H:H + ch] = first
        out[:, H + ch:] = second
    else:
        assert pad == 0
        flat = out.reshape(n, -1)
        flat[:, H * W:H * W + ch * cw] = first.reshape(n, -1)
        flat[:, H * W + ch * cw:] = second.reshape(n, -1)
    return out


def pitched_yuv_planar(Y, U, V, fmt, y_pad=0, c_pad=0, gap=0, stride_pad=0, rng=None, matrix=0, lead=0):
    """Planar / semi-planar YUV: a byte buffer of exactly the descriptor's extent (+ lead bytes in front of the base) with padded
    pitches: (buffer, MelfYuvPlanarFrames, base offset).  gap: bytes between the planes -- it sets the chroma planes' byte phase
    against Y."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (sx, sy, step, vfirst) = YUV_PLANAR_FORMATS[fmt]
    (n, H, W) = Y.shape
    (ch, cw) = (H >> sy, (W >> sx) * step)
    (yp, cp) = (W + y_pad, cw + c_pad)
    c0 = H * yp - y_pad + gap
    if step == 2:
        (uo, vo) = (c0 + 1, c0) if vfirst else (c0, c0 + 1)
        end = c0 + (ch - 1) * cp + cw
    else:
        c1 = c0 + (ch - 1) * cp + cw + gap
        (uo, vo) = (c1, c0) if vfirst else (c0, c1)
        end = c1 + (ch - 1) * cp + cw
    fs = end + stride_pad
    raw = rng.integers(0, 256, size=lead + (n - 1) * fs + end, dtype=np.uint8)
    buf = raw[lead:]
    for f in range(n):
        o = f * fs
        for y in range(H):
            buf[o + y * yp:o + y * yp + W] = Y[f, y]
        for y in range(ch):
            buf[o + uo + y * cp:o + uo + y * cp + step * (cw // step - 1) + 1:step] = U[f, y]
            buf[o + vo + y * cp:o + vo + y * cp + step * (cw // step - 1) + 1:step] = V[f, y]
    desc = _hip.MelfYuvPlanarFrames(matrix, n, H, W, sx, sy, step, 0, yp, cp, uo, vo, fs)
    return raw, desc, lead


def extent_yuv_planar(d):
    ch = d.H >> d.sub_y
    last = max(d.u_offset, d.v_offset) + (ch - 1) * d.c_pitch + ((d.W >> d.sub_x) - 1) * d.c_step + 1
    return (d.n - 1) * d.frame_stride + last


def to_planes(bgr, order, rng=None):
    """Planar RGB: (n, H, W, 3) BGR -> the (n, C, H, W) array whose planes are in `order`; a 4th plane ('a' / 'x') is random."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W, _c) = bgr.shape
    out = rng.integers(0, 256, size=(n, len(order), H, W), dtype=np.uint8)
    for (k, ch) in enumerate(order):
        if ch in 'bgr':
            out[:, k] = bgr[..., 'bgr'.index(ch)]
    return out


def pitched_planes(bgr, order='rgb', row_pad=0, gaps=(0, 0, 0), stride_pad=0, rng=None):
    """Planar RGB: a byte buffer of exactly the descriptor's extent: the three planes in `order`, rows row_pad bytes longer than
    W, gaps[k] bytes in front of plane k (gaps[0]: from the frame's first byte), stride_pad bytes behind a frame's last sample;
    random filling.  Returns (buffer, MelfPlanarFrames)."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W, _c) = bgr.shape
    rp = W + row_pad
    span = (H - 1) * rp + W
    off = {}
    at = 0
    for (k, ch) in enumerate(order):
        at += gaps[k]
        off[ch] = at
        at += span
    fs = at + stride_pad
    buf = rng.integers(0, 256, size=(n - 1) * fs + at, dtype=np.uint8)
    for ch in 'bgr':
        plane = bgr[..., 'bgr'.index(ch)]
        for f in range(n):
            dst = np.lib.stride_tricks.as_strided(buf[f * fs + off[ch]:], shape=(H, W), strides=(rp, 1))
            dst[...] = plane[f]
    desc = _hip.MelfPlanarFrames(n, H, W, 0, off['b'], off['g'], off['r'], rp, fs)
    return buf, desc


def extent_planes(d):
    return (d.n - 1) * d.frame_stride + max(d.b_offset, d.g_offset, d.r_offset) + (d.H - 1) * d.row_pitch + d.W


# ------------------------------------------------------------------------------------------------------------- families ---
class Family(NamedTuple):
    """What the shared bodies below differ in from family to family: the entry points, the layout builders, and what
    check_formats and resident_lanes_two_streams do for this family alone.  The source of a family's frames is a tuple: (Y, U, V)
    planes for the YUV families, (bgr,) for planar RGB."""
    formats: tuple               # the format names the file's tests go through
    view: Callable               # _hip.*_frames_view(array, fmt)
    host: str                    # Context: records of host frames (ptr, descriptor)
    dev: str                     # Context: records of device frames (device ptr, descriptor)
    read: str                    # MeterReader: records of an array or tensor
    conventional: Callable       # (*source, fmt, pad, rng) -> the array a caller would hold
    pitched: Callable            # (*source, fmt, rng=, **pads) -> (byte buffer of exactly the extent, descriptor)
    desc_extent: Callable        # descriptor -> bytes from the base to the last sample
    from_bgr: Callable           # BGR frames -> source (test input only)
    bgr_of: Callable             # (*source) -> the packed BGR frames the records must equal
    devbuf: Callable             # DevBuf or DevBuf.at_end
    check_pad: Callable          # check_formats: fmt -> the row padding of its conventional array
    check_pitch: Callable        # check_formats: k (the format's position) -> the pads of its pitched buffer
    sub: tuple = (0, 0)          # (sub_x, sub_y) of the chroma planes
    resident_sync_call: bool = False   # resident_lanes_two_streams: a synchronous call on every buffer first


F420 = Family(
    formats=('nv12', 'i420'), view=_hip.yuv_frames_view, host='process_yuv', dev='process_yuv_dev',
    read='read_yuv_frames', conventional=conventional420, pitched=pitched420, desc_extent=extent420,
    from_bgr=lambda bgr: bgr_to_yuv(bgr, 1, 1), bgr_of=lambda Y, U, V: yuv_to_bgr(Y, U, V, 1, 1), devbuf=DevBuf, sub=(1, 1),
    check_pad=lambda fmt: 10 if fmt == 'nv12' else 0, check_pitch=lambda k: dict(y_pad=7, c_pad=5, gap=3, stride_pad=11))

F422 = Family(
    formats=('yuyv', 'uyvy', 'yvyu'), view=_hip.yuv422_frames_view, host='process_yuv422',
    dev='process_yuv422_dev', read='read_yuv422_frames', conventional=conventional422, pitched=pitched422,
    desc_extent=extent422, from_bgr=lambda bgr: bgr_to_yuv(bgr, 1, 0), bgr_of=lambda Y, U, V: yuv_to_bgr(Y, U, V, 1, 0),
    devbuf=DevBuf, sub=(1, 0), check_pad=lambda fmt: 0, check_pitch=lambda k: dict(row_pad=12, stride_pad=20),
    resident_sync_call=True)

PLANAR = Family(
    formats=('rgb', 'bgr', 'gbr'), view=_hip.planar_frames_view, host='process_planes', dev='process_planes_dev',
    read='read_planar_frames', conventional=lambda bgr, order, pad, rng: to_planes(bgr, order, rng),
    pitched=lambda bgr, order, rng=None, **kw: pitched_planes(bgr, order[:3], rng=rng, **kw), desc_extent=extent_planes,
    from_bgr=lambda bgr: (bgr,), bgr_of=lambda bgr: bgr, devbuf=DevBuf.at_end, check_pad=lambda order: 0,
    check_pitch=lambda k: dict(row_pad=5 + k, gaps=(k, 1 + k, 6 - k), stride_pad=7 + k), resident_sync_call=True)


def yuv_planar(sub_x, sub_y, matrix=0):
    """The planar / semi-planar YUV family at one chroma subsampling (a format name implies its own; from_bgr and bgr_of need it)."""
    return Family(
        formats=tuple(f for (f, v) in YUV_PLANAR_FORMATS.items() if v[:2] == (sub_x, sub_y)),
        view=_hip.yuv_planar_frames_view, host='process_yuv_planar', dev='process_yuv_planar_dev', read='read_yuv_planar_frames',
        conventional=conventional_yuv_planar,
        pitched=lambda *a, **kw: pitched_yuv_planar(*a, **kw)[:2], desc_extent=extent_yuv_planar,
        from_bgr=lambda bgr: bgr_to_yuv(bgr, sub_x, sub_y), bgr_of=lambda Y, U, V: yuv_to_bgr(Y, U, V, sub_x, sub_y, matrix),
        devbuf=DevBuf, sub=(sub_x, sub_y), check_pad=lambda fmt: 0, check_pitch=lambda k: dict(y_pad=7, c_pad=5, gap=3, stride_pad=11))


def with_matrix(fam, code):
    """fam read under matrix `code`: its input encoded with that standard, its view, pitched descriptor and expected BGR under it."""
    (sx, sy) = fam.sub
    return fam._replace(
        view=lambda a, fmt: fam.view(a, fmt, code), pitched=lambda *a, **kw: fam.pitched(*a, matrix=code, **kw),
        from_bgr=lambda bgr: bgr_to_yuv(bgr, sx, sy, code), bgr_of=lambda Y, U, V: yuv_to_bgr(Y, U, V, sx, sy, code))


# -------------------------------------------------------------------------------------------------------- shared bodies ---
def read_both(fam, reader, ptr, desc, extent, phase=None):
    """Records of the host path and of the device path: a device copy of exactly `extent` bytes, placed by the family's devbuf -- plain
    DevBuf: at the start of an allocation the runtime rounds up to whole pages, so a load past the extent stays inside mapped
    memory; DevBuf.at_end: ending where the allocation ends (buffer_ends does that for every family)."""
    assert extent == fam.desc_extent(desc)
    host = getattr(reader.ctx, fam.host)(ptr, desc)
    buf = fam.devbuf(ptr, extent) if phase is None else fam.devbuf(ptr, extent, phase)
    try:
        dev = getattr(reader.ctx, fam.dev)(buf.d.value, desc)
    finally:
        buf.free()
    return host, dev


def check_formats(fam, reader, src, tag, rng, formats, want=None):
    """Every format named, as the conventional array and as a pitched buffer, through the reader, the host and the device entry
    point, against read_frames of the BGR frames the family's contract names.  Returns those records."""
    if want is None:
        want = reader.read_frames(fam.bgr_of(*src))
    wb = want.tobytes()
    for (k, fmt) in enumerate(formats):
        arr = fam.conventional(*src, fmt, fam.check_pad(fmt), rng)
        assert getattr(reader, fam.read)(arr, fmt).tobytes() == wb, (tag, fmt, 'reader')
        v = fam.view(arr, fmt)
        assert not v.copied
        (host, dev) = read_both(fam, reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == wb, (tag, fmt, 'host')
        assert dev.tobytes() == wb, (tag, fmt, 'device')
        (buf, desc) = fam.pitched(*src, fmt, rng=rng, **fam.check_pitch(k))
        (host, dev) = read_both(fam, reader, buf.ctypes.data, desc, buf.nbytes)
        assert host.tobytes() == wb, (tag, fmt, 'pitched host')
        assert dev.tobytes() == wb, (tag, fmt, 'pitched device')
    return want


def as_conventional(fam, pad_of):
    """each_match_kernel: format k of a source as its conventional array with pad_of(fmt) padding."""
    def layout(src, k, fmt, rng):
        arr = fam.conventional(*src, fmt, pad_of(fmt), rng)
        v = fam.view(arr, fmt)
        assert not v.copied
        return v.ptr, v.descriptor(), v.extent, arr
    return layout


def as_pitched(fam, pads_of):
    """each_match_kernel: format k of a source as a pitched buffer with the pads pads_of(k)."""
    def layout(src, k, fmt, rng):
        (buf, desc) = fam.pitched(*src, fmt, rng=rng, **pads_of(k))
        return buf.ctypes.data, desc, buf.nbytes, buf
    return layout


def each_match_kernel(e, monkeypatch, kind, kernel, groups, n, seed, rng_seed, min_not_found, min_ok):
    """n synthetic frames with match kernel `kind` forced: for every (family, formats, layout) of groups, the host and the device
    entry point against read_frames of the family's BGR frames, and melf_ctx_last_match naming `kernel` after every call."""
    from meterelf_amd import MeterReader
    bgr = synth(e['frames'], n, seed)
    monkeypatch.setenv('MELF_MATCH', kind)
    r = MeterReader(e['params'])
    try:
        rng = np.random.default_rng(rng_seed)
        for (fam, formats, layout) in groups:
            src = fam.from_bgr(bgr)
            want = r.read_frames(fam.bgr_of(*src))
            assert r.ctx.last_match()['kernel'] == kernel
            assert (want['status'] == _hip.FRAME_DIALS_NOT_FOUND).sum() >= min_not_found
            assert (want['status'] == _hip.FRAME_OK).sum() >= min_ok
            for (k, fmt) in enumerate(formats):
                (ptr, desc, extent, _keep) = layout(src, k, fmt, rng)
                assert extent == fam.desc_extent(desc)
                assert getattr(r.ctx, fam.host)(ptr, desc).tobytes() == want.tobytes(), (kind, fmt, 'host')
                assert r.ctx.last_match()['kernel'] == kernel
                buf = fam.devbuf(ptr, extent)
                try:
                    assert getattr(r.ctx, fam.dev)(buf.d.value, desc).tobytes() == want.tobytes(), (kind, fmt, 'device')
                finally:
                    buf.free()
                assert r.ctx.last_match()['kernel'] == kernel
    finally:
        r.close()


def fixture_frames(fam, e, sd, count, min_ok, check):
    """Every fixture frame of set sd through check (the file's check_formats); at least min_ok of them read OK on the BGR side."""
    assert len(e['frames']) == count
    rng = np.random.default_rng(count)
    shapes = {}
    for fr in e['frames']:
        shapes.setdefault(fr.shape, []).append(fr)
    ok = 0
    for (shape, group) in shapes.items():
        want = check(e['reader'], fam.from_bgr(np.stack(group)), '%s %s' % (sd, shape), rng)
        ok += int((want['status'] == _hip.FRAME_OK).sum())
    print('%s: %d of %d converted frames read OK' % (sd, ok, count))
    assert ok >= min_ok, ok   # the comparison is one of readings, not of failures


def odd_geometry(fam, e, tmp_path, cases, check, n, seed, rng_seed, min_ok):
    """meter_rect (50, 160)-(300, 410) moved by (dx, dy) and resized by (dw, dh) for every case; the frames are shifted by as
    much, so that the meter stays inside.  check(reader, source, tag, rng, k) is the file's check_formats for case k."""
    from meterelf_amd import MeterReader
    src = synth(e['frames'], n, seed)
    rng = np.random.default_rng(rng_seed)
    for (k, (dx, dy, dw, dh)) in enumerate(cases):
        params = params_with_rect(tmp_path, 'sample-images1', (50 + dx, 160 + dy, 300 + dx + dw, 410 + dy + dh), 'odd%d' % k)
        bgr = np.roll(src, (dy, dx), axis=(1, 2))
        r = MeterReader(params)
        try:
            want = check(r, fam.from_bgr(bgr), (dx, dy, dw, dh), rng, k)
            assert (want['status'] == _hip.FRAME_OK).sum() > min_ok, (dx, dy, dw, dh)
        finally:
            r.close()


def frame_edges(fam, reader, src, rng, n, sizes, check, min_ok):
    """The first n frames cut to each (H, W) of sizes: meter_rect (50, 160)-(300, 410) reaching the right and bottom frame edges,
    and past them (numpy clamp)."""
    for (H, W) in sizes:
        want = check(reader, fam.from_bgr(np.ascontiguousarray(src[:n, :H, :W])), (H, W), rng)
        assert (want['status'] == _hip.FRAME_OK).sum() >= min_ok, (H, W)


def batch_sizes(fam, reader, src, rng, sizes, formats_of, check, min_ok):
    """The first n frames for every n of sizes, in the formats formats_of(k), against the leading records of one call on all."""
    planes = fam.from_bgr(src)
    want = reader.read_frames(fam.bgr_of(*planes))
    assert (want['status'] == _hip.FRAME_OK).sum() > min_ok
    for (k, n) in enumerate(sizes):
        check(reader, tuple(p[:n] for p in planes), n, rng, formats=formats_of(k), want=want[:n])


def random_yuv_frames(fam, e, check, n, seed):
    """Uniform random Y, U, V bytes: every clamp of the conversion is hit, in every kernel that converts."""
    rng = np.random.default_rng(seed)
    (H, W) = e['frames'][2].shape[:2]
    (sx, sy) = fam.sub
    (Y, U, V) = (rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H >> sy, W >> sx), dtype=np.uint8),
                 rng.integers(0, 256, (n, H >> sy, W >> sx), dtype=np.uint8))
    bgr = fam.bgr_of(Y, U, V)
    assert (bgr == 0).any() and (bgr == 255).any()
    # half of the frames carry a fixture's meter, so that the dial reader runs on them (random chroma under it)
    (Yf, _, _) = fam.from_bgr(np.stack(e['frames'][2:2 + n // 2]))
    Y[::2] = Yf
    U[::2] = 128 + (U[::2].astype(np.int16) - 128) // 16
    V[::2] = 128 + (V[::2].astype(np.int16) - 128) // 16
    want = check(e['reader'], (Y, U, V), 'random', rng)
    assert (want['status'] != _hip.FRAME_DIALS_NOT_FOUND).sum() >= n // 4


def resident_calls(r, nframes, calls, rounds, pick):
    """melf_ctx_set_frames_resident(1) and two caller streams: call pick(i) of calls for i in range(rounds), the streams
    alternating, each call's records into its own slice of one device array; every slice equals the call's wanted bytes.
    calls: (function taking d_results_ptr, want_host and stream; wanted bytes)."""
    hip = hip_rt()
    rsz = _hip.RESULT_DTYPE.itemsize
    streams = [C.c_void_p(), C.c_void_p()]
    d_res = C.c_void_p()
    try:
        for s in streams:
            assert hip.hipStreamCreate(C.byref(s)) == 0
        assert hip.hipMalloc(C.byref(d_res), C.c_size_t(rounds * nframes * rsz)) == 0
        r.ctx.set_frames_resident(True)
        for i in range(rounds):
            calls[pick(i)][0](d_results_ptr=d_res.value + i * nframes * rsz, want_host=False, stream=streams[i % 2].value)
        r.ctx.sync()
        got = np.zeros(rounds * nframes, _hip.RESULT_DTYPE)
        assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), d_res, C.c_size_t(got.nbytes), 2) == 0
        for i in range(rounds):
            assert got[i * nframes:(i + 1) * nframes].tobytes() == calls[pick(i)][1], i
        r.ctx.set_frames_resident(False)
    finally:
        if d_res.value:
            hip.hipFree(d_res)
        for s in streams:
            if s.value:
                hip.hipStreamDestroy(s)


def resident_lanes_two_streams(fam, e, formats, pads_of, n, seed, min_ok, keep_host):
    """Pitched device buffers of the formats named (pads pads_of(k)), read in turn by eight resident calls on two streams: every
    call's records equal a synchronous call's.  keep_host: the pitched host buffers stay allocated to the end, as the 4:2:0 and
    4:2:2 files hold them; planar RGB lets each go after its (synchronous) upload, so that the next is built where it lay."""
    from meterelf_amd import MeterReader
    src = fam.from_bgr(synth(e['frames'], n, seed))
    r = MeterReader(e['params'])
    bufs = []
    try:
        want = r.read_frames(fam.bgr_of(*src))
        assert (want['status'] == _hip.FRAME_OK).sum() > min_ok
        calls = []
        keep = []
        for (k, fmt) in enumerate(formats):
            (buf, desc) = fam.pitched(*src, fmt, rng=np.random.default_rng(k), **pads_of(k))
            if keep_host:
                keep.append(buf)
            bufs.append(fam.devbuf(buf.ctypes.data, buf.nbytes))
            if fam.resident_sync_call:
                assert getattr(r.ctx, fam.dev)(bufs[-1].d.value, desc).tobytes() == want.tobytes(), fmt
            calls.append((functools.partial(getattr(r.ctx, fam.dev), bufs[-1].d.value, desc), want.tobytes()))
        resident_calls(r, n, calls, 8, lambda i: i % 4)
    finally:
        r.close()
        for b in bufs:
            b.free()


MATCH_KINDS = (('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4'))   # MELF_MATCH, the kernel melf_ctx_last_match names
ENDS_FRAMES = 33                                                       # a second frame group of one frame
ENDS_CASES = (((410, 300), (0, 0)), ((412, 302), (1, 1)))              # frames cut to (H, W), meter_rect moved by (dx, dy)


@functools.lru_cache(maxsize=None)
def corner_frames(n=ENDS_FRAMES):
    """(frames, mx, my): n same-sized sample-images1 frames that read OK, each rolled so that the dials template matches at the
    bottom-right corner of the crop of meter_rect (50, 160)-(300, 410): match position (mx, my) = (crop_cols - tw, crop_rows - th).
    Where the frames come from: the oracle's match positions of the fixture frames (no GPU)."""
    from meterelf_amd._image import imread_bgr
    from oracle import pyoracle as po
    sd = os.path.join(GOLDEN, 'sample-images1')
    op = po.Params(os.path.join(sd, 'params.yml'))
    (th, tw) = op.template_size
    (mx, my) = (250 - tw, 250 - th)
    frames = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(sd, '*.jpg')))]
    shapes = [f.shape for f in frames]
    same = np.stack([f for f in frames if f.shape == max(set(shapes), key=shapes.count)][:n + 12])
    out = []
    for (fr, o) in zip(same, po.process_frames(same, op)):
        if o.status == 0 and len(out) < n:
            out.append(np.roll(fr, (my - o.match_y, mx - o.match_x), axis=(0, 1)))
    assert len(out) == n
    out = np.stack(out)
    out.setflags(write=False)
    return out, mx, my


def family_ends(fam, formats=None):
    """buffer_ends' arguments for a Family: two pitched buffers per format, without padding and with the rows, pitches and gaps of
    the family's check_pitch, neither with stride padding."""
    def layouts(src, k, fmt, rng):
        pads = dict(fam.check_pitch(k), stride_pad=0)
        none = {key: (0, 0, 0) if isinstance(v, tuple) else 0 for (key, v) in pads.items()}
        return [fam.pitched(*src, fmt, rng=rng, **kw) for kw in (none, pads)]
    return dict(formats=formats or fam.formats, from_bgr=fam.from_bgr, bgr_of=fam.bgr_of, layouts=layouts,
                read_dev=lambda ctx, d, desc: getattr(ctx, fam.dev)(d, desc),
                nframes_stride=lambda desc: (desc.n, desc.frame_stride))


def buffer_ends(monkeypatch, tmp_path, formats, from_bgr, bgr_of, layouts, read_dev, nframes_stride, phases_of):
    """Device buffers that end where their allocation ends (DevBuf.at_end), at every base phase phases_of(fmt) the family's check
    accepts, read through the device entry point: a load past the descriptor's extent leaves the mapping.  The frames
    (corner_frames) are cut so that meter_rect ends on the frame's last row and column, (410, 300), or starts at an odd origin and
    ends one pixel short of both, (412, 302) with the rect moved by (1, 1); the template matches at the crop's bottom-right corner
    (asserted from the records), so the dial windows' last rows and columns are the crop's.  Buffers: layouts(src, k, fmt, rng), a
    list of (byte buffer of exactly the extent, descriptor) without stride padding (asserted), for 1 and for 33 frames; the last
    frame reads FRAME_OK (asserted).  Under each match kernel (MELF_MATCH fast, gen, dot4; melf_ctx_last_match asserted after
    every call) the records equal, byte for byte, read_frames of the family's BGR frames under that kernel."""
    from meterelf_amd import MeterReader
    (base, mx, my) = corner_frames()
    rng = np.random.default_rng(ENDS_FRAMES)
    for (case, ((H, W), (dx, dy))) in enumerate(ENDS_CASES):
        params = params_with_rect(tmp_path, 'sample-images1', (50 + dx, 160 + dy, 300 + dx, 410 + dy), 'ends%d' % case)
        src = from_bgr(np.ascontiguousarray(np.roll(base, (dy, dx), axis=(1, 2))[:, :H, :W]))
        readers = []
        try:
            for (kind, kernel) in MATCH_KINDS:
                monkeypatch.setenv('MELF_MATCH', kind)
                r = MeterReader(params)
                want = r.read_frames(bgr_of(*src))
                assert r.ctx.last_match()['kernel'] == kernel
                assert [(int(x), int(y)) for (x, y) in zip(want['match_x'], want['match_y'])] == [(mx, my)] * ENDS_FRAMES, (H, W, kind)
                assert int(want['status'][0]) == int(want['status'][-1]) == _hip.FRAME_OK, (H, W, kind)
                readers.append((r, kernel, want))
            for n in (1, ENDS_FRAMES):
                for (k, fmt) in enumerate(formats):
                    for (buf, desc) in layouts(tuple(p[:n] for p in src), k, fmt, rng):
                        (dn, fs) = nframes_stride(desc)
                        assert dn == n and buf.nbytes == n * fs, (fmt, 'stride padding')
                        for phase in phases_of(fmt):
                            d = DevBuf.at_end(buf.ctypes.data, buf.nbytes, phase)
                            try:
                                assert d.d.value % 4 == phase
                                for (r, kernel, want) in readers:
                                    got = read_dev(r.ctx, d.d.value, desc)
                                    assert r.ctx.last_match()['kernel'] == kernel
                                    assert got.tobytes() == want[:n].tobytes(), (H, W, n, fmt, phase, kernel)
                            finally:
                                d.free()
        finally:
            for (r, _k, _w) in readers:
                r.close()


def first_bytes(monkeypatch, tmp_path, formats, from_bgr, bgr_of, layouts, read_dev, x0s):
    """A base that is not 4-byte aligned (phases 1 .. 3) and meter_rect in the frame's first row from column x0 of x0s.  For the
    columns from which a window would reach the base's dword, launch_match_prep sends the whole launch down the prep kernel's
    sample-by-sample path (melf_prep_addr.h: prep_window_readable); this test checks that the RECORDS of that path, and of the
    window path at the columns next to it, are byte for byte those of read_frames of the family's BGR frames, under the two
    matrix-core match kernels (they read what the prep kernel wrote), three frames.  It cannot see where a load starts: the bytes
    before an unaligned base share a mapped dword with it.  That no window starts before the base is what
    tests/prep_bounds_main.cpp sweeps, with the launcher's own function."""
    from meterelf_amd import MeterReader
    (base, _mx, _my) = corner_frames()
    rng = np.random.default_rng(3)
    for x0 in x0s:
        params = params_with_rect(tmp_path, 'sample-images1', (x0, 0, x0 + 250, 250), 'first%d' % x0)
        src = from_bgr(np.ascontiguousarray(np.roll(base[:3], (-160, x0 - 50), axis=(1, 2))[:, :252, :x0 + 252 - (x0 & 1)]))
        for (kind, kernel) in MATCH_KINDS[:2]:
            monkeypatch.setenv('MELF_MATCH', kind)
            r = MeterReader(params)
            try:
                want = r.read_frames(bgr_of(*src))
                assert (want['status'] == _hip.FRAME_OK).all(), (x0, kind)
                for (k, fmt) in enumerate(formats):
                    (buf, desc) = layouts(src, k, fmt, rng)[0]
                    for phase in (1, 2, 3):
                        d = DevBuf.at_end(buf.ctypes.data, buf.nbytes, phase)
                        try:
                            assert d.d.value % 4 == phase
                            assert read_dev(r.ctx, d.d.value, desc).tobytes() == want.tobytes(), (x0, fmt, phase, kind)
                            assert r.ctx.last_match()['kernel'] == kernel
                        finally:
                            d.free()
            finally:
                r.close()


def launch_counts(ctx):
    """test_argument_errors_launch_nothing: the launches per kernel so far (under melf_ctx_set_profiling(1))."""
    return {k: cnt for (k, (_ms, cnt)) in ctx.timings().items()}


# ------------------------------------------------------------------------------------------------------ the torch child ---
TORCH_OK = {'packed': b'torch path ok', 'yuv': b'torch yuv path ok', 'yuv422': b'torch yuv422 path ok',
            'planar': b'torch planar path ok', 'yuv_planar': b'torch planar yuv path ok', 'yuv_matrix': b'torch yuv matrix path ok'}


def run_torch_child(family):
    """The torch checks of `family` in a fresh process that imports torch first (the module docstring says why): its exit status
    and its '... path ok' line."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.abspath(__file__), 'torch', family], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and TORCH_OK[family] in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


class _Torch:
    """torch (imported before the package loads the library: one HIP runtime in the process), a reader on GPU 0 and n synthetic
    sample-images1 frames."""

    def __init__(self, n, seed):
        import torch
        from meterelf_amd import MeterReader, _params
        from meterelf_amd._image import imread_bgr
        self.torch = torch
        params = _params.load(os.path.join(GOLDEN, 'sample-images1', 'params.yml'))
        frames = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(GOLDEN, 'sample-images1', '*.jpg')))]
        self.bgr = synth(frames, n, seed)
        self.reader = MeterReader(params, device=0)
        self.dev = torch.device('cuda', 0)
        self.rsz = _hip.RESULT_DTYPE.itemsize

    def records(self, n):
        return self.torch.empty((n, self.rsz), dtype=self.torch.uint8, device=self.dev)

    def three_ways(self, read, t, host, want, tag):
        """read(frames, out=None) of the device tensor t, of the host tensor host() (made only now, after the device read: a
        t.cpu() ahead of it changes how many copy kernels the runtime launches), and of t with out=."""
        assert read(t).tobytes() == want.tobytes(), tag
        # host tensors take the host path
        assert read(host()).tobytes() == want.tobytes(), tag
        # out=: records into a device tensor on the current stream, nothing synchronised
        out = self.records(len(want))
        assert read(t, out=out) is out
        self.torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), (tag, 'out')

    def two_streams(self, read_i, want):
        """Resident frames, two caller streams, out= on each: read_i(i, out) for six calls."""
        torch = self.torch
        self.reader.ctx.set_frames_resident(True)
        (sa, sb) = (torch.cuda.Stream(self.dev), torch.cuda.Stream(self.dev))
        outs = []
        torch.cuda.synchronize()
        for i in range(6):
            with torch.cuda.stream(sa if i % 2 == 0 else sb):
                o = self.records(len(want))
                read_i(i, o)
                outs.append(o)
        torch.cuda.synchronize()
        for o in outs:
            assert o.cpu().numpy().tobytes() == want.tobytes()
        self.reader.ctx.set_frames_resident(False)


def _torch_packed():
    T = _Torch(128, 9)
    (torch, reader, dev, bgr) = (T.torch, T.reader, T.dev, T.bgr)
    want = reader.read_frames(bgr)
    assert (want['status'] == _hip.FRAME_OK).sum() > 64
    rng = np.random.default_rng(1)
    for fmt in ('bgr', 'rgb', 'bgra', 'rgba'):
        for pad in (0, 11):
            (arr, f) = to_layout(bgr, fmt, pad, rng)
            full = torch.from_numpy(arr.base).to(dev)
            t = full[:, :, :bgr.shape[2]]
            assert not _hip.frames_view(t, f).copied
            T.three_ways(lambda x, **kw: reader.read_frame_views(x, f, **kw), t, lambda: torch.from_numpy(np.ascontiguousarray(arr)), want,
                         (fmt, pad))
    # a 3-channel view of RGBA pixels, and a buffer of exactly the descriptor's extent (torch.as_strided)
    (arr, f) = to_layout(bgr, 'rgba', 6, rng, view3=True)
    v = _hip.frames_view(arr, f)
    flat = torch.from_numpy(np.frombuffer((C.c_uint8 * v.extent).from_address(v.ptr), np.uint8).copy()).to(dev)
    t = torch.as_strided(flat, arr.shape, (v.frame_stride, v.row_pitch, 4, 1))
    assert _hip.frames_view(t, f).pixel_format == _hip.PIX_RGBA
    assert reader.read_frame_views(t, f).tobytes() == want.tobytes()
    tb = torch.from_numpy(to_layout(bgr, 'bgra', 3, rng)[0].base).to(dev)[:, :, :bgr.shape[2]]
    T.two_streams(lambda i, o: reader.read_frame_views(tb, 'bgra', out=o), want)
    # a tensor on another device than the reader's is an error
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            reader.read_frame_views(t.to(torch.device('cuda', 1)), f)
    reader.ctx.sync()
    reader.close()


def _torch_yuv(fam, formats, pads_of, strided, wide_pad, lanes):
    """4:2:0 and packed 4:2:2.  strided: the format read as every other frame; wide_pad: the row padding (pixels) that its view
    cannot describe; lanes: the padded format that alternates with it on the two streams."""
    T = _Torch(128, 9)
    (torch, reader, dev) = (T.torch, T.reader, T.dev)
    read = getattr(reader, fam.read)
    src = fam.from_bgr(T.bgr)
    want = reader.read_frames(fam.bgr_of(*src))
    assert (want['status'] == _hip.FRAME_OK).sum() > 64
    rng = np.random.default_rng(1)
    W = src[0].shape[2]
    for fmt in formats:
        for pad in pads_of(fmt):
            arr = fam.conventional(*src, fmt, pad, rng)
            full = torch.from_numpy(arr.base if pad else arr).to(dev)
            t = full[:, :, :W]
            assert not fam.view(t, fmt).copied
            T.three_ways(lambda x, **kw: read(x, fmt, **kw), t, lambda: torch.from_numpy(np.ascontiguousarray(arr)), want, (fmt, pad))
    # every other frame in place; rows padded so that the view cannot describe them go through one packed copy
    t = torch.from_numpy(fam.conventional(*src, strided)).to(dev)
    assert not fam.view(t[::2], strided).copied
    assert read(t[::2], strided).tobytes() == want[::2].tobytes()
    wide = torch.zeros(t.shape[:2] + (W + wide_pad,) + t.shape[3:], dtype=torch.uint8, device=dev)
    wide[:, :, :W] = t
    assert fam.view(wide[:, :, :W], strided).copied
    out = T.records(len(want))
    read(wide[:, :, :W], strided, out=out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        read(t.cpu(), strided, out=out)   # out= takes device frames only
    tn = torch.from_numpy(fam.conventional(*src, lanes, 4, rng).base).to(dev)[:, :, :W]
    T.two_streams(lambda i, o: read(tn if i % 3 else t, lanes if i % 3 else strided, out=o), want)
    reader.ctx.sync()
    reader.close()


def _torch_planar():
    T = _Torch(128, 9)
    (torch, reader, dev, bgr) = (T.torch, T.reader, T.dev, T.bgr)
    want = reader.read_frames(bgr)
    assert (want['status'] == _hip.FRAME_OK).sum() > 64
    rng = np.random.default_rng(1)
    (n, H, W, _c) = bgr.shape
    for order in ('rgb', 'bgr', 'gbr', 'rgba', 'bgrx'):
        t = torch.from_numpy(to_planes(bgr, order, rng)).to(dev)
        assert t.is_contiguous() and not _hip.planar_frames_view(t, order).copied
        T.three_ways(lambda x, **kw: reader.read_planar_frames(x, order, **kw), t, t.cpu, want, order)
    # the NCHW batch a torch pipeline holds: what the interleaved route gives, without the interleaved copy
    t = torch.from_numpy(to_planes(bgr, 'rgb')).to(dev)
    assert _hip.frames_view(t.permute(0, 2, 3, 1), 'rgb').copied            # today's route copies (unchanged)
    assert reader.read_frame_views(t.permute(0, 2, 3, 1), 'rgb').tobytes() == want.tobytes()
    # x[:, :3] of a 4-plane tensor, every other frame, a crop of a larger tensor: in place
    t4 = torch.from_numpy(to_planes(bgr, 'rgba', rng)).to(dev)
    assert not _hip.planar_frames_view(t4[:, :3], 'rgb').copied
    assert reader.read_planar_frames(t4[:, :3], 'rgb').tobytes() == want.tobytes()
    assert not _hip.planar_frames_view(t[::2], 'rgb').copied
    assert reader.read_planar_frames(t[::2], 'rgb').tobytes() == want[::2].tobytes()
    big = torch.randint(0, 256, (n, 3, H + 3, W + 5), dtype=torch.uint8, device=dev)
    big[:, :, 2:2 + H, 1:1 + W] = t
    view = big[:, :, 2:2 + H, 1:1 + W]
    v = _hip.planar_frames_view(view, 'rgb')
    assert not v.copied and v.row_pitch == W + 5 and v.ptr == big.data_ptr() + 2 * (W + 5) + 1
    assert reader.read_planar_frames(view, 'rgb').tobytes() == want.tobytes()
    # a permuted NHWC tensor goes through one packed copy, with out= too
    nhwc = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1])).to(dev)
    assert _hip.planar_frames_view(nhwc.permute(0, 3, 1, 2), 'rgb').copied
    out = T.records(n)
    reader.read_planar_frames(nhwc.permute(0, 3, 1, 2), 'rgb', out=out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        reader.read_planar_frames(t.cpu(), 'rgb', out=out)   # out= takes device frames only
    with pytest.raises(ValueError):
        reader.read_planar_frames(t, 'rgba')
    T.two_streams(lambda i, o: reader.read_planar_frames(view if i % 3 else t4, 'rgb' if i % 3 else 'rgba', out=o), want)
    reader.ctx.sync()
    reader.close()


def _torch_yuv_planar():
    T = _Torch(96, 9)
    (torch, reader, dev, bgr) = (T.torch, T.reader, T.dev, T.bgr)
    rng = np.random.default_rng(1)
    W = bgr.shape[2]
    for fmt in ('i422', 'nv16', 'nv61', 'i444', 'nv24', 'i440', 'nv21'):
        (sx, sy, step, _vf) = YUV_PLANAR_FORMATS[fmt]
        (Y, U, V) = bgr_to_yuv(bgr, sx, sy)
        want = reader.read_frames(yuv_to_bgr(Y, U, V, sx, sy, 2))
        assert (want['status'] == _hip.FRAME_OK).sum() > 48

        def read(x, **kw):
            return reader.read_yuv_planar_frames(x, fmt, 'bt601-full', **kw)
        for pad in ((0, 12) if (W >> sx) * step == W else (0,)):
            arr = conventional_yuv_planar(Y, U, V, fmt, pad, rng)
            t = torch.from_numpy(arr.base if pad else arr).to(dev)[:, :, :W]
            assert not _hip.yuv_planar_frames_view(t, fmt).copied
            T.three_ways(read, t, lambda: torch.from_numpy(np.ascontiguousarray(arr)), want, (fmt, pad))
        if fmt == 'i444':
            # the (N, 3, H, W) shape, every other frame, in place
            t4 = torch.from_numpy(np.stack([Y, U, V], axis=1)).to(dev)
            assert not _hip.yuv_planar_frames_view(t4[::2], fmt).copied
            assert read(t4[::2]).tobytes() == want[::2].tobytes()
        if fmt == 'i422':
            # padded rows of a layout whose chroma rows are half rows: one packed copy, on the device
            wide = torch.zeros((len(Y), 2 * Y.shape[1], W + 8), dtype=torch.uint8, device=dev)
            wide[:, :, :W] = torch.from_numpy(conventional_yuv_planar(Y, U, V, fmt)).to(dev)
            assert _hip.yuv_planar_frames_view(wide[:, :, :W], fmt).copied
            out = T.records(len(Y))
            read(wide[:, :, :W], out=out)
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == want.tobytes()
            with pytest.raises(ValueError):
                reader.read_yuv_planar_frames(conventional_yuv_planar(Y, U, V, fmt), fmt, out=out)   # out= with host frames
    reader.close()


def _torch_yuv_matrix():
    T = _Torch(64, 9)
    (torch, reader, dev) = (T.torch, T.reader, T.dev)
    seen = set()
    for (name, code) in (('bt709', 3), ('bt601-full', 2), ('bt709-full', 4)):
        (p420, p422) = (bgr_to_yuv(T.bgr, 1, 1, 3), bgr_to_yuv(T.bgr, 1, 0, 3))   # the same bytes under each matrix
        (n, _H, W) = p420[0].shape
        want0 = reader.read_frames(yuv_to_bgr(*p420, 1, 1, code))
        want2 = reader.read_frames(yuv_to_bgr(*p422, 1, 0, code))
        assert (want0['status'] == _hip.FRAME_OK).sum() > 32
        seen.add(want0.tobytes())
        full = torch.from_numpy(conventional420(*p420, 'nv12', 12).base).to(dev)
        t = full[:, :, :W]
        assert not _hip.yuv_frames_view(t, 'nv12', name).copied
        assert reader.read_yuv_frames(t, 'nv12', matrix=name).tobytes() == want0.tobytes(), name
        assert reader.read_yuv_frames(t, 'nv12', code).tobytes() == want0.tobytes(), name
        out = T.records(n)
        assert reader.read_yuv_frames(t, 'nv12', matrix=name, out=out) is out
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want0.tobytes(), (name, 'out')
        t2 = torch.from_numpy(packed422(*p422, 'uyvy')).to(dev)
        assert reader.read_yuv422_frames(t2, 'uyvy', matrix=name).tobytes() == want2.tobytes(), name
        out2 = T.records(n)
        assert reader.read_yuv422_frames(t2, 'uyvy', matrix=code, out=out2) is out2
        torch.cuda.synchronize()
        assert out2.cpu().numpy().tobytes() == want2.tobytes(), (name, 'out 4:2:2')
        # host tensors take the host path
        assert reader.read_yuv422_frames(t2.cpu(), 'uyvy', matrix=name).tobytes() == want2.tobytes(), name
    assert len(seen) == 3
    reader.close()


TORCH_MAIN = {
    'packed': _torch_packed,
    'yuv': lambda: _torch_yuv(F420, ('nv12', 'i420', 'yv12'), lambda fmt: (0, 12) if fmt == 'nv12' else (0,), 'i420', 8, 'nv12'),
    'yuv422': lambda: _torch_yuv(F422, F422.formats, lambda fmt: (0, 12), 'uyvy', 1, 'yuyv'),
    'planar': _torch_planar,
    'yuv_planar': _torch_yuv_planar,
    'yuv_matrix': _torch_yuv_matrix,
}

if __name__ == '__main__' and len(sys.argv) == 3 and sys.argv[1] == 'torch':
    TORCH_MAIN[sys.argv[2]]()
    print(TORCH_OK[sys.argv[2]].decode())
