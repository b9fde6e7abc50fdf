"""YUV 4:2:0 video frames -- NV12, I420, YV12 -- read in place (melf_process_yuv, melf_process_yuv_dev, melf_yuv_to_bgr,
_hip.yuv_frames_view, MeterReader.read_yuv_frames).

The contract: the records of a YUV frame are byte-identical to read_frames() of the packed BGR frame that the conversion below
makes of it.  The conversion (include/meterelf_hip.h; the constants of cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420), BT.601 limited
range), in integers, >> arithmetic:

    chroma: the nearest sample, no interpolation: pixel (x, y) uses U[y >> 1][x >> 1], V[y >> 1][x >> 1]
    yy = max(Y - 16, 0) * 1220542          u = U - 128          v = V - 128
    R = clamp((yy + (1 << 19) + 1673527 * v)              >> 20, 0, 255)
    G = clamp((yy + (1 << 19) -  852492 * v - 409993 * u) >> 20, 0, 255)
    B = clamp((yy + (1 << 19) + 2116026 * u)              >> 20, 0, 255)

yuv420_to_bgr below is its numpy restatement: the expected side of every comparison.  bgr_to_yuv420 (float BT.601 limited-range
RGB -> YUV, 2 x 2 chroma mean, round half up, clip) only makes test input from the BGR fixtures; nothing is compared against it.

CPU tests: the descriptor against the header, yuv_frames_view's mapping of numpy arrays and torch CPU tensors, the restatement
against hand-derived triples, the new kernels' code-object notes.  GPU tests: the conversion kernel for all 2^24 triples, records
against the BGR path of the converted frames on the fixtures, with every match kernel, at odd crop origins, at the frame edges, at
1080p, over lanes and streams, with torch tensors (in a child process that imports torch first: tests/test_pixel_formats.py says why).
"""
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402

FORMATS = ('nv12', 'i420')


# ------------------------------------------------------------------------------------------------- the conversion, restated ---
def yuv420_to_bgr(Y, U, V):
    """Y (..., H, W), U and V (..., H / 2, W / 2) uint8 -> (..., H, W, 3) uint8 BGR: the module docstring's arithmetic."""
    yy = np.maximum(Y.astype(np.int32) - 16, 0) * 1220542 + (1 << 19)
    u = np.repeat(np.repeat(U.astype(np.int32) - 128, 2, axis=-2), 2, axis=-1)
    v = np.repeat(np.repeat(V.astype(np.int32) - 128, 2, axis=-2), 2, axis=-1)
    out = np.empty(Y.shape + (3,), np.uint8)
    out[..., 2] = np.clip((yy + 1673527 * v) >> 20, 0, 255)
    out[..., 1] = np.clip((yy - 852492 * v - 409993 * u) >> 20, 0, 255)
    out[..., 0] = np.clip((yy + 2116026 * u) >> 20, 0, 255)
    return out


def bgr_to_yuv420(bgr):
    """Test input only: (..., H, W, 3) BGR -> Y, U, V planes (float BT.601 limited range, 2 x 2 chroma mean, round half up)."""
    f = bgr.astype(np.float64)
    (b, g, r) = (f[..., 0], f[..., 1], f[..., 2])
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0

    def mean22(p):
        return (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]) / 4.0

    def q(p):
        return np.clip(np.floor(p + 0.5), 0, 255).astype(np.uint8)
    return q(y), q(mean22(u)), q(mean22(v))


def conventional(Y, U, V, fmt, pad=0, rng=None):
    """The (N, H * 3 // 2, W) array of the planes in layout fmt ('nv12' / 'i420' / 'yv12'); pad > 0: a [:, :, :W] view of an
    array whose rows are pad bytes longer (random filling)."""
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


def pitched(Y, U, V, fmt, y_pad=0, c_pad=0, gap=0, stride_pad=0, rng=None):
    """A byte buffer of exactly the descriptor's extent with padded pitches: (buffer, MelfYuvFrames).  gap: bytes between the
    planes; yv12: V before U."""
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
    desc = _hip.MelfYuvFrames(_hip.YUV_CODES[fmt], _hip.YUV_BT601_LIMITED, n, H, W, 0, yp, cp, uo, vo, fs)
    return buf, desc


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_yuv_struct_matches_header(tmp_path):
    fields = ('format', 'matrix', 'n', 'H', 'W', 'reserved', 'y_pitch', 'c_pitch', 'u_offset', 'v_offset', 'frame_stride')
    src = tmp_path / 'yuv.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(melf_yuv_frames));\n'
                   + ''.join('printf(" %%zu", offsetof(melf_yuv_frames, %s));\n' % f for f in fields)
                   + 'printf(" %d %d %d\\n", MELF_YUV_NV12, MELF_YUV_I420, MELF_YUV_BT601_LIMITED);return 0;}\n')
    exe = tmp_path / 'yuv'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfYuvFrames
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in fields] + [_hip.YUV_NV12, _hip.YUV_I420, _hip.YUV_BT601_LIMITED]
    for name in ('melf_process_yuv', 'melf_process_yuv_dev', 'melf_yuv_to_bgr'):
        assert name in _hip.EXPORTS


def _arrays():
    yield np.zeros
    try:
        import torch
    except ImportError:
        return
    yield lambda shape, dtype: torch.zeros(shape, dtype=torch.uint8 if dtype == np.uint8 else torch.int16)


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_yuv_frames_view_layouts(kind):
    makers = list(_arrays())
    if kind == 'torch' and len(makers) < 2:
        pytest.skip('torch is not installed')
    z = makers[0 if kind == 'numpy' else 1]

    def addr(a):
        return a.ctypes.data if kind == 'numpy' else a.data_ptr()
    (n, H, W) = (5, 8, 12)
    R = H * 3 // 2
    a = z((n, R, W), np.uint8)
    # packed
    v = _hip.yuv_frames_view(a, 'nv12')
    assert (v.format, v.n, v.H, v.W, v.y_pitch, v.c_pitch, v.u_offset, v.v_offset, v.frame_stride, v.extent, v.copied, v.on_device) == \
           (_hip.YUV_NV12, n, H, W, W, W, H * W, H * W + 1, R * W, n * R * W, False, False)
    v = _hip.yuv_frames_view(a, 'i420')
    assert (v.format, v.y_pitch, v.c_pitch, v.u_offset, v.v_offset, v.frame_stride, v.extent, v.copied) == \
           (_hip.YUV_I420, W, W // 2, H * W, H * W + H * W // 4, R * W, n * R * W, False)
    v = _hip.yuv_frames_view(a, 'yv12')
    assert (v.format, v.u_offset, v.v_offset, v.copied) == (_hip.YUV_I420, H * W + H * W // 4, H * W, False)
    d = v.descriptor()
    assert (d.format, d.matrix, d.n, d.H, d.W, d.y_pitch, d.c_pitch, d.u_offset, d.v_offset, d.frame_stride) == \
           (_hip.YUV_I420, 0, n, H, W, W, W // 2, v.u_offset, v.v_offset, R * W)
    # NV12, padded rows: the strides describe it, the extent stops at the last sample
    v = _hip.yuv_frames_view(a[:, :, :8], 'nv12')
    assert (v.W, v.y_pitch, v.c_pitch, v.u_offset, v.v_offset, v.frame_stride, v.extent, v.copied) == \
           (8, W, W, H * W, H * W + 1, R * W, (n - 1) * R * W + (R - 1) * W + 8, False)
    # every other frame, a frame-range slice: in place, both families
    for fmt in ('nv12', 'i420', 'yv12'):
        v = _hip.yuv_frames_view(a[::2], fmt)
        assert (v.n, v.frame_stride, v.extent, v.copied, v.ptr) == (3, 2 * R * W, 4 * R * W + R * W, False, addr(a))
        v = _hip.yuv_frames_view(a[1:4], fmt)
        assert (v.n, v.frame_stride, v.extent, v.copied, v.ptr) == (3, R * W, 3 * R * W, False, addr(a) + R * W)
    # I420 with padded rows: the chroma rows are no longer half rows of the array: one packed copy
    v = _hip.yuv_frames_view(a[:, :, :8], 'i420')
    assert (v.W, v.y_pitch, v.c_pitch, v.u_offset, v.frame_stride, v.extent, v.copied) == (8, 8, 4, H * 8, R * 8, n * R * 8, True)
    assert v.ptr != addr(a)
    # rejected: dtype, rank, odd H, odd W, unknown names (the packed-pixel names among them)
    with pytest.raises(ValueError):
        _hip.yuv_frames_view(z((n, R, W), np.int16), 'nv12')
    with pytest.raises(ValueError):
        _hip.yuv_frames_view(z((n, R, W, 1), np.uint8), 'nv12')
    with pytest.raises(ValueError):
        _hip.yuv_frames_view(z((n, 7, W), np.uint8), 'nv12')      # H = 5
    with pytest.raises(ValueError):
        _hip.yuv_frames_view(z((n, R, 11), np.uint8), 'i420')
    for bad in ('nv21', 'bgr', 'yuv', ''):
        with pytest.raises(ValueError):
            _hip.yuv_frames_view(a, bad)


def test_conversion_restatement_hand_derived():
    """yuv420_to_bgr against triples worked out by hand from the docstring's formulas."""
    def one(y, u, v):
        px = yuv420_to_bgr(np.full((2, 2), y, np.uint8), np.full((1, 1), u, np.uint8), np.full((1, 1), v, np.uint8))
        assert (px == px[0, 0]).all()
        return tuple(int(c) for c in px[0, 0])   # (B, G, R)
    assert one(16, 128, 128) == (0, 0, 0)
    # yy = 219 * 1220542 = 267298698; + 524288 = 267822986; >> 20 = 255 (255 * 2^20 = 267386880 <= 267822986 < 256 * 2^20)
    assert one(235, 128, 128) == (255, 255, 255)
    assert one(0, 128, 128) == (0, 0, 0)           # Y below 16 is 16
    # mid grey: yy = 110 * 1220542 = 134259620; + 524288 = 134783908; >> 20 = 128
    assert one(126, 128, 128) == (128, 128, 128)
    # R saturates high: v = 127: 134783908 + 1673527 * 127 = 347321837 >> 20 = 331 -> 255
    #   G: 134783908 - 852492 * 127 = 26517424 >> 20 = 25;  B: u = 0 -> 128
    assert one(126, 128, 255) == (128, 25, 255)
    # R saturates low: v = -128: 134783908 - 214211456 < 0 -> 0;  G: 134783908 + 109118976 = 243902884 >> 20 = 232
    assert one(126, 128, 0) == (128, 232, 0)
    # B saturates high: u = 127: 134783908 + 2116026 * 127 = 403519210 >> 20 = 384 -> 255;  G: 134783908 - 409993 * 127 = 82714797 >> 20 = 78
    assert one(126, 255, 128) == (255, 78, 128)
    # B saturates low: u = -128: negative -> 0;  G: 134783908 + 409993 * 128 = 187263012 >> 20 = 178
    assert one(126, 0, 128) == (0, 178, 128)
    # G saturates high: u = v = -128 on a bright Y: yy = 204 * 1220542 + 524288 = 249514856; G: + 109118976 + 52479104 = 411112936 >> 20 = 392
    #   -> 255;  R: 249514856 - 214211456 = 35303400 >> 20 = 33;  B: 249514856 - 270851328 < 0 -> 0
    assert one(220, 0, 0) == (0, 255, 33)
    # G saturates low: u = v = 127 on a dark Y: yy = 14 * 1220542 + 524288 = 17611876; G: - 108266484 - 52069111 < 0 -> 0;
    #   R: 17611876 + 212537929 = 230149805 >> 20 = 219;  B: 17611876 + 268735302 = 286347178 >> 20 = 273 -> 255
    assert one(30, 255, 255) == (255, 0, 219)
    # arithmetic shift of a negative sum floors: v = -1 on Y = 16: R: (524288 - 1673527) = -1149239 >> 20 = -2 -> 0;
    #   G: 524288 + 852492 = 1376780 >> 20 = 1;  B: 524288 >> 20 = 0
    assert one(16, 128, 127) == (0, 1, 0)


def test_yuv_kernels_metadata():
    """The kernels that read YUV frames are in the library, without scratch; the dial readers within k_dials' register count."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    names = ('k_lplane_yuv', 'k_match_yuv', 'k_yneedle', 'k_yuv2bgr')
    new = {k: d for (k, d) in meta.items() if any(s in k for s in names)}
    assert [sum(s in k for k in new) for s in names] == [2, 2, 12, 2]
    dials_vgpr = max(d['vgpr_count'] for (k, d) in meta.items() if 'k_dials' in k)
    for (k, d) in new.items():
        assert d.get('private_segment_fixed_size', 0) == 0 and d.get('vgpr_spill_count', 0) == 0, (k, d)
        if 'k_yneedle' in k:
            assert d['vgpr_count'] <= dials_vgpr, (k, d)


# ------------------------------------------------------------------------------------------------------------- GPU ---------
@pytest.fixture(scope='module')
def env():
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    from meterelf_amd._image import imread_bgr
    out = {}
    for sd in ('sample-images1', 'sample-images2'):
        params = _params.load(os.path.join(GOLDEN, sd, 'params.yml'))
        frames = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(GOLDEN, sd, '*.jpg')))]
        out[sd] = dict(params=params, frames=frames, reader=MeterReader(params))
    yield out
    for e in out.values():
        e['reader'].close()


def _hip_rt():
    from tests.helpers import hip_runtime
    return hip_runtime()


class DevBuf:
    """Device copy of `nbytes` bytes at host address `ptr`, allocated to exactly that size."""

    def __init__(self, ptr, nbytes):
        self.hip = _hip_rt()
        self.d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.d), C.c_size_t(max(nbytes, 1))) == 0
        assert self.hip.hipMemcpy(self.d, C.c_void_p(ptr), C.c_size_t(nbytes), 1) == 0

    def free(self):
        self.hip.hipFree(self.d)


def _desc_extent(d):
    nv12 = d.format == _hip.YUV_NV12
    last = max(d.u_offset, d.v_offset) + (d.H // 2 - 1) * d.c_pitch + (d.W - 1 if nv12 else d.W // 2)
    return (d.n - 1) * d.frame_stride + last


def _read_both(reader, ptr, desc, extent):
    """Records of the host path and of the device path (a device buffer of exactly `extent` bytes)."""
    assert extent == _desc_extent(desc)
    host = reader.ctx.process_yuv(ptr, desc)
    buf = DevBuf(ptr, extent)
    try:
        dev = reader.ctx.process_yuv_dev(buf.d.value, desc)
    finally:
        buf.free()
    return host, dev


def _check_formats(reader, Y, U, V, tag, rng, formats=('nv12', 'i420', 'yv12'), want=None):
    """Every format, conventional and pitched, host and device, against read_frames of the converted frames."""
    if want is None:
        want = reader.read_frames(yuv420_to_bgr(Y, U, V))
    wb = want.tobytes()
    for fmt in formats:
        arr = conventional(Y, U, V, fmt, 10 if fmt == 'nv12' else 0, rng)
        assert reader.read_yuv_frames(arr, fmt).tobytes() == wb, (tag, fmt, 'reader')
        v = _hip.yuv_frames_view(arr, fmt)
        assert not v.copied
        (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == wb, (tag, fmt, 'host')
        assert dev.tobytes() == wb, (tag, fmt, 'device')
        (buf, desc) = pitched(Y, U, V, fmt, y_pad=7, c_pad=5, gap=3, stride_pad=11, rng=rng)
        (host, dev) = _read_both(reader, buf.ctypes.data, desc, buf.nbytes)
        assert host.tobytes() == wb, (tag, fmt, 'pitched host')
        assert dev.tobytes() == wb, (tag, fmt, 'pitched device')
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', FORMATS)
def test_yuv_to_bgr_all_triples(env, fmt):
    """melf_yuv_to_bgr == the numpy restatement for all 2^24 (Y, U, V): one 4096 x 4096 frame whose 2 x 2 blocks share chroma --
    block b has (U, V) = (b & 255, (b >> 8) & 255) and the four Y values 4 (b >> 16) .. + 3."""
    ctx = env['sample-images1']['reader'].ctx
    b = np.arange(2048 * 2048, dtype=np.uint32).reshape(2048, 2048)
    U = (b & 255).astype(np.uint8)[None]
    V = ((b >> 8) & 255).astype(np.uint8)[None]
    k = (b >> 16).astype(np.uint8) * 4
    Y = np.empty((1, 4096, 4096), np.uint8)
    Y[0, 0::2, 0::2] = k
    Y[0, 0::2, 1::2] = k + 1
    Y[0, 1::2, 0::2] = k + 2
    Y[0, 1::2, 1::2] = k + 3
    seen = np.zeros(1 << 24, bool)
    uv = (V[0].astype(np.uint32) << 16) | (U[0].astype(np.uint32) << 8)
    for plane in (Y[0, 0::2, 0::2], Y[0, 0::2, 1::2], Y[0, 1::2, 0::2], Y[0, 1::2, 1::2]):
        seen[(uv | plane).ravel()] = True
    assert seen.all()
    v = _hip.yuv_frames_view(conventional(Y, U, V, fmt), fmt)
    got = ctx.yuv_to_bgr(v.ptr, v.descriptor())
    want = yuv420_to_bgr(Y, U, V)
    bad = np.flatnonzero((got != want).any(axis=-1).ravel())
    assert bad.size == 0, (fmt, bad.size, bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', ('nv12', 'i420', 'yv12'))
def test_yuv_to_bgr_padded_pitches(env, fmt):
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(5)
    (n, H, W) = (3, 38, 50)
    (Y, U, V) = (rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H // 2, W // 2), dtype=np.uint8),
                 rng.integers(0, 256, (n, H // 2, W // 2), dtype=np.uint8))
    (buf, desc) = pitched(Y, U, V, fmt, y_pad=9, c_pad=3, gap=5, stride_pad=13, rng=rng)
    assert np.array_equal(ctx.yuv_to_bgr(buf.ctypes.data, desc), yuv420_to_bgr(Y, U, V))


@pytest.mark.gpu
@pytest.mark.parametrize('sd,count,min_ok', [('sample-images1', 81, 79), ('sample-images2', 223, 223)])
def test_fixture_frames(env, sd, count, min_ok):
    e = env[sd]
    assert len(e['frames']) == count
    rng = np.random.default_rng(count)
    shapes = {}
    for fr in e['frames']:
        shapes.setdefault(fr.shape, []).append(fr)
    ok = 0
    for (shape, group) in shapes.items():
        (Y, U, V) = bgr_to_yuv420(np.stack(group))
        want = _check_formats(e['reader'], Y, U, V, '%s %s' % (sd, shape), rng)
        ok += int((want['status'] == _hip.FRAME_OK).sum())
    assert ok >= min_ok, ok   # the comparison is one of readings, not of failures


def _synth(frames, n, seed):
    """n shifted + noisy fixture frames, every 9th a constant frame (Dials not found): as tests/test_pixel_formats.py."""
    rng = np.random.default_rng(seed)
    shapes = [f.shape for f in frames]
    base = [f for f in frames if f.shape == max(set(shapes), key=shapes.count)]
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


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')])
def test_each_match_kernel(env, monkeypatch, kind, kernel):
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    (Y, U, V) = bgr_to_yuv420(_synth(e['frames'], 256, 5))
    monkeypatch.setenv('MELF_MATCH', kind)
    r = MeterReader(e['params'])
    try:
        want = r.read_frames(yuv420_to_bgr(Y, U, V))
        assert r.ctx.last_match()['kernel'] == kernel
        assert (want['status'] == _hip.FRAME_DIALS_NOT_FOUND).sum() >= 28 and (want['status'] == _hip.FRAME_OK).sum() >= 128
        rng = np.random.default_rng(7)
        for fmt in FORMATS:
            arr = conventional(Y, U, V, fmt, 6 if fmt == 'nv12' else 0, rng)
            v = _hip.yuv_frames_view(arr, fmt)
            assert r.ctx.process_yuv(v.ptr, v.descriptor()).tobytes() == want.tobytes(), (kind, fmt, 'host')
            assert r.ctx.last_match()['kernel'] == kernel
            buf = DevBuf(v.ptr, v.extent)
            try:
                assert r.ctx.process_yuv_dev(buf.d.value, v.descriptor()).tobytes() == want.tobytes(), (kind, fmt, 'device')
            finally:
                buf.free()
            assert r.ctx.last_match()['kernel'] == kernel
    finally:
        r.close()


def _params_with_rect(tmp_path, sd, rect, tag):
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


@pytest.mark.gpu
def test_odd_geometry(env, tmp_path):
    """meter_rect (50, 160)-(300, 410) moved to odd x0, odd y0, both, and given an odd width and height; the frames are shifted
    by as much, so that the meter stays inside."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    src = _synth(e['frames'], 40, 3)
    rng = np.random.default_rng(13)
    for (k, (dx, dy, dw, dh)) in enumerate(((1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, -1, -1), (1, 1, -1, -1), (3, 5, 1, 1))):
        params = _params_with_rect(tmp_path, 'sample-images1', (50 + dx, 160 + dy, 300 + dx + dw, 410 + dy + dh), 'odd%d' % k)
        bgr = np.roll(src, (dy, dx), axis=(1, 2))
        (Y, U, V) = bgr_to_yuv420(bgr)
        r = MeterReader(params)
        try:
            want = _check_formats(r, Y, U, V, (dx, dy, dw, dh), rng)
            assert (want['status'] == _hip.FRAME_OK).sum() > 20, (dx, dy, dw, dh)
        finally:
            r.close()


@pytest.mark.gpu
def test_frame_edges_and_batch_sizes(env):
    """meter_rect (50, 160)-(300, 410) reaching the right and bottom frame edges, and past them (numpy clamp), device buffers of
    exactly the descriptor's extent (every _read_both); batch sizes around the 32-frame group."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(11)
    src = _synth(e['frames'], 70, 3)
    for (H, W) in ((410, 300), (400, 290)):
        (Y, U, V) = bgr_to_yuv420(np.ascontiguousarray(src[:12, :H, :W]))
        want = _check_formats(reader, Y, U, V, (H, W), rng)
        assert (want['status'] == _hip.FRAME_OK).sum() >= 6, (H, W)
    (Y, U, V) = bgr_to_yuv420(src)
    want = reader.read_frames(yuv420_to_bgr(Y, U, V))
    assert (want['status'] == _hip.FRAME_OK).sum() > 40
    for n in (1, 31, 33, 70):
        _check_formats(reader, Y[:n], U[:n], V[:n], n, rng, formats=FORMATS, want=want[:n])


@pytest.mark.gpu
def test_random_frames(env):
    """Uniform random Y, U, V bytes: every clamp of the conversion is hit, in every kernel that converts."""
    e = env['sample-images1']
    rng = np.random.default_rng(99)
    (H, W) = e['frames'][2].shape[:2]
    n = 40
    (Y, U, V) = (rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H // 2, W // 2), dtype=np.uint8),
                 rng.integers(0, 256, (n, H // 2, W // 2), dtype=np.uint8))
    bgr = yuv420_to_bgr(Y, U, V)
    assert (bgr == 0).any() and (bgr == 255).any()
    # half of the frames carry a fixture's meter, so that the dial reader runs on them (random chroma under it)
    (Yf, _, _) = bgr_to_yuv420(np.stack(e['frames'][2:2 + n // 2]))
    Y[::2] = Yf
    U[::2] = 128 + (U[::2].astype(np.int16) - 128) // 16
    V[::2] = 128 + (V[::2].astype(np.int16) - 128) // 16
    want = _check_formats(e['reader'], Y, U, V, 'random', rng, formats=FORMATS)
    assert (want['status'] != _hip.FRAME_DIALS_NOT_FOUND).sum() >= n // 4


@pytest.mark.gpu
def test_1080p_six_dials_nv12_padded(env, tmp_path):
    """The configuration of tests/test_pixel_formats.py::test_1080p_six_dials_bgra_padded as NV12 with padded pitches."""
    import yaml
    from meterelf_amd import MeterReader, _params
    src = os.path.join(GOLDEN, 'sample-images1')
    with open(os.path.join(src, 'params.yml')) as fp:
        data = yaml.safe_load(fp)
    data['meter_rect'] = {'top_left': [1210, 420], 'bottom_right': [1460, 670]}
    extra = []
    for (k, nd) in enumerate(data['needle_data'][:2]):
        nd2 = dict(nd)
        nd2['name'] = '1.%d' % k
        nd2['center'] = [nd['center'][0] + 0.4, nd['center'][1] - 0.3]
        extra.append(nd2)
    data['needle_data'] = data['needle_data'] + extra
    with open(tmp_path / 'params.yml', 'w') as fp:
        yaml.safe_dump(data, fp)
    shutil.copy(os.path.join(src, 'dials_gray.png'), tmp_path / 'dials_gray.png')
    params = _params.load(str(tmp_path / 'params.yml'))
    assert len(params.dial_names) == 6
    rng = np.random.default_rng(1080)
    good = env['sample-images1']['frames'][2:7]
    frames = rng.integers(0, 256, size=(len(good), 1080, 1920, 3), dtype=np.uint8)
    for (i, f) in enumerate(good):
        frames[i, 420:670, 1210:1460] = f[160:410, 50:300]
    (Y, U, V) = bgr_to_yuv420(frames)
    reader = MeterReader(params)
    try:
        want = reader.read_frames(yuv420_to_bgr(Y, U, V))
        assert (want['status'] == _hip.FRAME_OK).any()
        arr = conventional(Y, U, V, 'nv12', 64, rng)
        v = _hip.yuv_frames_view(arr, 'nv12')
        assert not v.copied and v.y_pitch == 1920 + 64
        (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()
    finally:
        reader.close()


@pytest.mark.gpu
def test_resident_lanes_two_streams(env):
    """melf_ctx_set_frames_resident(1) and two caller streams, formats alternating: every call's records equal a synchronous call's."""
    from meterelf_amd import MeterReader
    e = env['sample-images2']
    hip = _hip_rt()
    (Y, U, V) = bgr_to_yuv420(_synth(e['frames'], 96, 21))
    rsz = _hip.RESULT_DTYPE.itemsize
    r = MeterReader(e['params'])
    bufs = []
    streams = [C.c_void_p(), C.c_void_p()]
    d_res = C.c_void_p()
    try:
        want = r.read_frames(yuv420_to_bgr(Y, U, V))
        assert (want['status'] == _hip.FRAME_OK).sum() > 48
        descs = []
        keep = []
        for (k, fmt) in enumerate(('nv12', 'i420', 'yv12', 'nv12')):
            (buf, desc) = pitched(Y, U, V, fmt, y_pad=4 * k, c_pad=2 * k, gap=k, stride_pad=k, rng=np.random.default_rng(k))
            keep.append(buf)
            bufs.append(DevBuf(buf.ctypes.data, buf.nbytes))
            descs.append(desc)
        for s in streams:
            assert hip.hipStreamCreate(C.byref(s)) == 0
        assert hip.hipMalloc(C.byref(d_res), C.c_size_t(8 * len(Y) * rsz)) == 0
        r.ctx.set_frames_resident(True)
        for i in range(8):
            r.ctx.process_yuv_dev(bufs[i % 4].d.value, descs[i % 4], d_results_ptr=d_res.value + i * len(Y) * rsz, want_host=False,
                                  stream=streams[i % 2].value)
        r.ctx.sync()
        got = np.zeros(8 * len(Y), _hip.RESULT_DTYPE)
        assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), d_res, C.c_size_t(got.nbytes), 2) == 0
        for i in range(8):
            assert got[i * len(Y):(i + 1) * len(Y)].tobytes() == want.tobytes(), i
        r.ctx.set_frames_resident(False)
    finally:
        r.close()
        for b in bufs:
            b.free()
        if d_res.value:
            hip.hipFree(d_res)
        for s in streams:
            if s.value:
                hip.hipStreamDestroy(s)


@pytest.mark.gpu
def test_argument_errors_launch_nothing(env):
    e = env['sample-images1']
    ctx = e['reader'].ctx
    L = _hip.lib()
    (Y, U, V) = bgr_to_yuv420(np.stack(e['frames'][2:6]))
    (n, H, W) = Y.shape
    arr = conventional(Y, U, V, 'nv12')
    buf = DevBuf(arr.ctypes.data, arr.nbytes)
    try:
        ctx.set_profiling(1)
        before = {k: cnt for (k, (_ms, cnt)) in ctx.timings().items()}
        out = np.zeros(n, _hip.RESULT_DTYPE)
        bgr_out = np.zeros((n, H, W, 3), np.uint8)
        F = _hip.MelfYuvFrames
        (NV, I4) = (_hip.YUV_NV12, _hip.YUV_I420)
        fs = H * W * 3 // 2
        q = H * W // 4
        bad = [
            F(2, 0, n, H, W, 0, W, W, H * W, H * W + 1, fs),                   # unknown format
            F(-1, 0, n, H, W, 0, W, W, H * W, H * W + 1, fs),
            F(NV, 1, n, H, W, 0, W, W, H * W, H * W + 1, fs),                  # unknown matrix
            F(NV, 0, n, H - 1, W, 0, W, W, H * W, H * W + 1, fs),              # odd H
            F(NV, 0, n, H, W - 1, 0, W, W, H * W, H * W + 1, fs),              # odd W
            F(NV, 0, n, H, W, 0, W - 1, W, H * W, H * W + 1, fs),              # y_pitch too small
            F(NV, 0, n, H, W, 0, W, W - 2, H * W, H * W + 1, fs),              # c_pitch too small
            F(I4, 0, n, H, W, 0, W, W // 2 - 1, H * W, H * W + q, fs),
            F(NV, 0, n, H, W, 0, W, W, H * W, H * W + 1, fs - 1),              # stride too small
            F(I4, 0, n, H, W, 0, W, W // 2, H * W, H * W + q, fs - 1),
            F(NV, 0, n, H, W, 0, W, W, H * W - 2, H * W - 1, fs),              # chroma overlaps the Y plane
            F(I4, 0, n, H, W, 0, W, W // 2, H * W - 1, H * W + q, fs),
            F(I4, 0, n, H, W, 0, W, W // 2, H * W + q, 0, fs),
            F(NV, 0, n, H, W, 0, W, W, H * W, H * W + 2, fs),                  # NV12: V not beside U
            F(NV, 0, n, H, W, 0, W + 1, W, H * (W + 1) - 1, H * (W + 1), fs + H),   # NV12: odd u_offset
            F(NV, 0, n, 0, W, 0, W, W, H * W, H * W + 1, fs),                  # bad shape
            F(NV, 0, -1, H, W, 0, W, W, H * W, H * W + 1, fs),
        ]
        for f in bad:
            key = (f.format, f.matrix, f.n, f.H, f.W, f.y_pitch, f.c_pitch, f.u_offset, f.v_offset, f.frame_stride)
            assert L.melf_process_yuv_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(f), None, _hip._ptr(out), None) == -1, key
            assert L.melf_last_error().decode()
            assert L.melf_process_yuv(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(out)) == -1, key
            assert L.melf_last_error().decode()
            assert L.melf_yuv_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(bgr_out)) == -1, key
            assert L.melf_last_error().decode()
        assert L.melf_process_yuv_dev(ctx._h, C.c_void_p(buf.d.value), None, None, _hip._ptr(out), None) == -1
        assert L.melf_process_yuv(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(out)) == -1
        assert L.melf_yuv_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(bgr_out)) == -1
        good = F(NV, 0, n, H, W, 0, W, W, H * W, H * W + 1, fs)
        assert L.melf_process_yuv_dev(ctx._h, None, C.byref(good), None, _hip._ptr(out), None) == -1   # NULL frames
        assert {k: cnt for (k, (_ms, cnt)) in ctx.timings().items()} == before
        # a good descriptor runs
        assert L.melf_process_yuv_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
        assert {k: cnt for (k, (_ms, cnt)) in ctx.timings().items()} != before
        assert out.tobytes() == e['reader'].read_frames(yuv420_to_bgr(Y, U, V)).tobytes()
    finally:
        ctx.set_profiling(0)
        buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_yuv_frames with torch tensors, in a child process that imports torch first."""
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.abspath(__file__), 'torch'], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch yuv path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


def _torch_main():
    import torch  # before the package loads the library: one HIP runtime in the process
    from meterelf_amd import MeterReader, _params
    from meterelf_amd._image import imread_bgr
    params = _params.load(os.path.join(GOLDEN, 'sample-images1', 'params.yml'))
    files = sorted(glob.glob(os.path.join(GOLDEN, 'sample-images1', '*.jpg')))
    frames = [imread_bgr(f) for f in files]
    (Y, U, V) = bgr_to_yuv420(_synth(frames, 128, 9))
    reader = MeterReader(params, device=0)
    dev = torch.device('cuda', 0)
    want = reader.read_frames(yuv420_to_bgr(Y, U, V))
    assert (want['status'] == _hip.FRAME_OK).sum() > 64
    rsz = _hip.RESULT_DTYPE.itemsize
    rng = np.random.default_rng(1)
    W = Y.shape[2]
    for fmt in ('nv12', 'i420', 'yv12'):
        for pad in ((0, 12) if fmt == 'nv12' else (0,)):
            arr = conventional(Y, U, V, fmt, pad, rng)
            full = torch.from_numpy(arr.base if pad else arr).to(dev)
            t = full[:, :, :W]
            assert not _hip.yuv_frames_view(t, fmt).copied
            assert reader.read_yuv_frames(t, fmt).tobytes() == want.tobytes(), (fmt, pad)
            # host tensors take the host path
            assert reader.read_yuv_frames(torch.from_numpy(np.ascontiguousarray(arr)), fmt).tobytes() == want.tobytes(), (fmt, pad)
            # out=: records into a device tensor on the current stream, nothing synchronised
            out = torch.empty((len(Y), rsz), dtype=torch.uint8, device=dev)
            assert reader.read_yuv_frames(t, fmt, out=out) is out
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == want.tobytes(), (fmt, pad, 'out')
    # every other frame in place; I420 with padded rows goes through one packed copy
    t = torch.from_numpy(conventional(Y, U, V, 'i420')).to(dev)
    assert not _hip.yuv_frames_view(t[::2], 'i420').copied
    assert reader.read_yuv_frames(t[::2], 'i420').tobytes() == want[::2].tobytes()
    wide = torch.zeros((len(Y), Y.shape[1] * 3 // 2, W + 8), dtype=torch.uint8, device=dev)
    wide[:, :, :W] = t
    assert _hip.yuv_frames_view(wide[:, :, :W], 'i420').copied
    out = torch.empty((len(Y), rsz), dtype=torch.uint8, device=dev)
    reader.read_yuv_frames(wide[:, :, :W], 'i420', out=out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # resident frames, two caller streams, out= on each
    reader.ctx.set_frames_resident(True)
    (sa, sb) = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    outs = []
    tn = torch.from_numpy(conventional(Y, U, V, 'nv12', 4, rng).base).to(dev)[:, :, :W]
    torch.cuda.synchronize()
    for i in range(6):
        with torch.cuda.stream(sa if i % 2 == 0 else sb):
            o = torch.empty((len(Y), rsz), dtype=torch.uint8, device=dev)
            reader.read_yuv_frames(tn if i % 3 else t, 'nv12' if i % 3 else 'i420', out=o)
            outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
        assert o.cpu().numpy().tobytes() == want.tobytes()
    reader.ctx.set_frames_resident(False)
    reader.ctx.sync()
    reader.close()
    print('torch yuv path ok')


if __name__ == '__main__' and sys.argv[1:] == ['torch']:
    _torch_main()
