"""Packed YUV 4:2:2 frames -- YUYV (YUY2), UYVY, YVYU -- read in place (melf_process_yuv422, melf_process_yuv422_dev,
melf_yuv422_to_bgr, _hip.yuv422_frames_view, MeterReader.read_yuv422_frames).

The contract: the records of a 4:2:2 frame are byte-identical to read_frames() of the packed BGR frame that the conversion below
makes of it.  The conversion (include/meterelf_hip.h; the constants of cv2.cvtColor(COLOR_YUV2BGR_YUY2 / _UYVY / _YVYU), BT.601
limited range), in integers, >> arithmetic:

    chroma: the two pixels of a macropixel share its U and V: pixel (x, y) uses U[y][x >> 1], V[y][x >> 1]
    yy = max(Y - 16, 0) * 1220542          u = U - 128          v = V - 128
    R = clamp((yy + (1 << 19) + 1673527 * v)              >> 20, 0, 255)
    G = clamp((yy + (1 << 19) -  852492 * v - 409993 * u) >> 20, 0, 255)
    B = clamp((yy + (1 << 19) + 2116026 * u)              >> 20, 0, 255)

    bytes of a macropixel (pixels 2 k, 2 k + 1 of a row):  yuyv: Y0 U Y1 V    uyvy: U Y0 V Y1    yvyu: Y0 V Y1 U

yuv_to_bgr(Y, U, V, 1, 0) of tests/frame_cases.py is its numpy restatement (yuv422_to_bgr here; U and V repeated twice along x):
the expected side of every comparison.  bgr_to_yuv422 (float BT.601 limited-range RGB -> YUV, the mean of each horizontal pixel
pair for chroma, round half up, clip) only makes test input from the BGR fixtures; nothing is compared against it.

CPU tests: the descriptor against the header, yuv422_frames_view's mapping of numpy arrays and torch CPU tensors, the restatement
against hand-derived triples and byte positions, the new kernels' code-object notes.  GPU tests: the conversion kernel for all
2^24 triples at both pixels of a macropixel, records against the BGR path of the converted frames on the fixtures, with every
match kernel, at every parity of the crop, at the frame edges, at 1080p, over lanes and streams, with torch tensors (in a child
process that imports torch first: tests/frame_cases.py says why).  Every device copy has exactly the descriptor's
extent; test_buffer_ends places the copies where their allocation ends, so that a load past the extent leaves the mapping (the
other tests' copies start their allocation, which the runtime rounds up to whole pages).
"""
import ctypes as C
import functools
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
from tests import frame_cases as fc  # noqa: E402
from tests.frame_cases import DevBuf, F422, conventional422 as conventional, env, pitched422 as pitched  # noqa: E402,F401

FORMATS = F422.formats
yuv422_to_bgr = F422.bgr_of        # the conversion above, restated (tests/frame_cases.py: yuv_to_bgr)
bgr_to_yuv422 = F422.from_bgr      # test input only


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_yuv422_struct_matches_header(tmp_path):
    fields = ('format', 'matrix', 'n', 'H', 'W', 'reserved', 'row_pitch', 'frame_stride')
    src = tmp_path / 'yuv422.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(melf_yuv422_frames));\n'
                   + ''.join('printf(" %%zu", offsetof(melf_yuv422_frames, %s));\n' % f for f in fields)
                   + 'printf(" %d %d %d %d %d\\n", MELF_YUV422_YUYV, MELF_YUV422_UYVY, MELF_YUV422_YVYU, MELF_YUV_BT601_LIMITED, '
                     'MELF_ABI_VERSION);return 0;}\n')
    exe = tmp_path / 'yuv422'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfYuv422Frames
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in fields] + [_hip.YUV422_YUYV, _hip.YUV422_UYVY, _hip.YUV422_YVYU,
                                                                          _hip.YUV_BT601_LIMITED, 3]
    assert C.sizeof(F) == 40
    for name in ('melf_process_yuv422', 'melf_process_yuv422_dev', 'melf_yuv422_to_bgr'):
        assert name in _hip.EXPORTS
    assert (_hip.YUV422_CODES['yuyv'], _hip.YUV422_CODES['yuy2'], _hip.YUV422_CODES['uyvy'], _hip.YUV422_CODES['yvyu']) == (0, 0, 1, 2)


def _arrays():
    yield np.zeros
    try:
        import torch
    except ImportError:
        return
    yield lambda shape, dtype: torch.zeros(shape, dtype=torch.uint8 if dtype == np.uint8 else torch.int16)


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_yuv422_frames_view_layouts(kind):
    makers = list(_arrays())
    if kind == 'torch' and len(makers) < 2:
        pytest.skip('torch is not installed')
    z = makers[0 if kind == 'numpy' else 1]

    def addr(a):
        return a.ctypes.data if kind == 'numpy' else a.data_ptr()
    (n, H, W) = (5, 7, 12)   # H odd: 4:2:2 has no vertical subsampling
    a = z((n, H, W, 2), np.uint8)
    assert addr(a) % 4 == 0
    fs = H * W * 2
    # packed, every name
    for (name, code) in (('yuyv', 0), ('yuy2', 0), ('YUYV', 0), ('uyvy', 1), ('yvyu', 2)):
        v = _hip.yuv422_frames_view(a, name)
        assert (v.format, v.n, v.H, v.W, v.row_pitch, v.frame_stride, v.extent, v.copied, v.on_device, v.ptr) == \
               (code, n, H, W, 2 * W, fs, n * fs, False, False, addr(a))
    assert _hip.yuv422_frames_view(a).format == _hip.YUV422_YUYV   # the default
    d = _hip.yuv422_frames_view(a, 'uyvy').descriptor()
    assert (d.format, d.matrix, d.n, d.H, d.W, d.reserved, d.row_pitch, d.frame_stride) == (1, 0, n, H, W, 0, 2 * W, fs)
    # padded rows: the strides describe it, the extent stops at the last sample
    v = _hip.yuv422_frames_view(a[:, :, :8], 'yuyv')
    assert (v.W, v.row_pitch, v.frame_stride, v.extent, v.copied, v.ptr) == (8, 2 * W, fs, (n - 1) * fs + (H - 1) * 2 * W + 16, False, addr(a))
    # a crop that starts at an even pixel and at any row: in place
    v = _hip.yuv422_frames_view(a[:, 1:, 2:10], 'yvyu')
    assert (v.H, v.W, v.row_pitch, v.frame_stride, v.copied, v.ptr) == (H - 1, 8, 2 * W, fs, False, addr(a) + 2 * W + 4)
    # every other frame, a frame-range slice, one frame: in place
    v = _hip.yuv422_frames_view(a[::2], 'uyvy')
    assert (v.n, v.frame_stride, v.extent, v.copied, v.ptr) == (3, 2 * fs, 4 * fs + fs, False, addr(a))
    v = _hip.yuv422_frames_view(a[1:4], 'uyvy')
    assert (v.n, v.frame_stride, v.extent, v.copied, v.ptr) == (3, fs, 3 * fs, False, addr(a) + fs)
    v = _hip.yuv422_frames_view(a[2:3, :, :8], 'uyvy')
    assert (v.n, v.row_pitch, v.extent, v.copied, v.ptr) == (1, 2 * W, (H - 1) * 2 * W + 16, False, addr(a) + 2 * fs)
    v = _hip.yuv422_frames_view(a[:0], 'yuyv')
    assert (v.n, v.extent) == (0, 0)

    def copied(view, W_):
        v = _hip.yuv422_frames_view(view, 'yuyv')
        assert v.copied and v.ptr % 4 == 0 and (v.W, v.row_pitch, v.frame_stride) == (W_, 2 * W_, v.H * W_ * 2), view.shape
        assert v.extent == v.n * v.frame_stride
        return v
    # copied once: a crop that starts at an odd pixel (the base is no longer 4-byte aligned)
    v = copied(a[:, :, 1:9], 8)
    assert v.ptr != addr(a)
    # copied: a row pitch that is not a multiple of 4 (W + 1 pixels per row, a W-pixel view)
    b = z((n, H, W + 1, 2), np.uint8)
    copied(b[:, :, :W], W)
    # copied: a frame stride that is not a multiple of 4 (odd H of the wider array times an odd pitch is excluded above; here H x
    # (W + 1) x 2 bytes = 7 x 26: a multiple of 2 only) even with whole rows
    if kind == 'numpy':
        flat = np.zeros(n * (fs + 2), np.uint8)
        c = np.lib.stride_tricks.as_strided(flat, shape=(n, H, W, 2), strides=(fs + 2, 2 * W, 2, 1))
        copied(c, W)
        # an element stride other than 1, a pixel stride other than 2 (every other pixel)
        wide = np.zeros((n, H, W, 4), np.uint8)
        copied(wide[..., ::2], W)
        copied(np.zeros((n, H, 2 * W, 2), np.uint8)[:, :, ::2], W)
        # negative strides
        copied(a[::-1], W)
        copied(a[:, ::-1], W)
    else:
        import torch
        wide = torch.zeros((n, H, W, 4), dtype=torch.uint8)
        copied(wide[..., ::2], W)
        copied(torch.zeros((n, H, 2 * W, 2), dtype=torch.uint8)[:, :, ::2], W)
    # the copy holds the caller's bytes
    if kind == 'numpy':
        src = np.arange(n * H * W * 2, dtype=np.uint32).astype(np.uint8).reshape(n, H, W, 2)
        v = _hip.yuv422_frames_view(src[:, :, 1:9], 'yuyv')
        assert v.copied and np.array_equal(np.asarray(v.array), src[:, :, 1:9])
    # rejected: dtype, rank, last dimension, odd W, empty frames, unknown names (the other families' names among them)
    with pytest.raises(ValueError):
        _hip.yuv422_frames_view(z((n, H, W, 2), np.int16), 'yuyv')
    with pytest.raises(ValueError):
        _hip.yuv422_frames_view(z((n, H, 2 * W), np.uint8), 'yuyv')
    with pytest.raises(ValueError):
        _hip.yuv422_frames_view(z((1, n, H, W, 2), np.uint8), 'yuyv')
    for last in (1, 3, 4):
        with pytest.raises(ValueError):
            _hip.yuv422_frames_view(z((n, H, W, last), np.uint8), 'yuyv')
    with pytest.raises(ValueError):
        _hip.yuv422_frames_view(z((n, H, 11, 2), np.uint8), 'uyvy')
    with pytest.raises(ValueError):
        _hip.yuv422_frames_view(z((n, H, 0, 2), np.uint8), 'uyvy')
    with pytest.raises(ValueError):
        _hip.yuv422_frames_view(z((n, 0, W, 2), np.uint8), 'uyvy')
    for bad in ('nv12', 'i420', 'yv12', 'nv16', 'bgr', 'yuv', 'vyuy', ''):
        with pytest.raises(ValueError):
            _hip.yuv422_frames_view(a, bad)
    # and the other views do not take these names
    for name in ('yuyv', 'yuy2', 'uyvy', 'yvyu'):
        with pytest.raises(ValueError):
            _hip.yuv_frames_view(z((n, 12, W), np.uint8), name)
        with pytest.raises(ValueError):
            _hip.frames_view(z((n, H, W, 3), np.uint8), name)


def test_conversion_restatement_hand_derived():
    """yuv422_to_bgr against triples worked out by hand from the docstring's formulas, the chroma sharing, and the byte
    positions of the three formats."""
    def one(y, u, v):
        px = yuv422_to_bgr(np.full((3, 2), y, np.uint8), np.full((3, 1), u, np.uint8), np.full((3, 1), v, np.uint8))
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
    # arithmetic shift of a negative sum floors: v = -1 on Y = 16: R: (524288 - 1673527) = -1149239 >> 20 = -2 -> 0;
    #   G: 524288 + 852492 = 1376780 >> 20 = 1;  B: 524288 >> 20 = 0
    assert one(16, 128, 127) == (0, 1, 0)
    # one row of two macropixels: (Y 126 | 235, U 128, V 255) and (Y 126 | 16, U 0, V 128).  The two pixels of a macropixel get
    # the same chroma, the neighbouring macropixel another; nothing is shared between rows.
    #   pixel 1: yy = 267822986: R + 1673527 * 127 -> 255;  G: 267822986 - 108266484 = 159556502 >> 20 = 152;  B: 255
    #   pixel 3: Y = 16: yy = 524288: B: - 2116026 * 128 < 0 -> 0;  G: 524288 + 52479104 = 53003392 >> 20 = 50;  R: 524288 >> 20 = 0
    Y = np.array([[126, 235, 126, 16], [16, 16, 16, 16]], np.uint8)
    U = np.array([[128, 0], [128, 128]], np.uint8)
    V = np.array([[255, 128], [128, 128]], np.uint8)
    px = yuv422_to_bgr(Y, U, V)
    assert [tuple(int(c) for c in p) for p in px[0]] == [(128, 25, 255), (255, 152, 255), (0, 178, 128), (0, 50, 0)]
    assert (px[1] == 0).all()
    # the byte positions: the row above as bytes, per format
    for (fmt, row) in (('yuyv', [126, 128, 235, 255, 126, 0, 16, 128]), ('uyvy', [128, 126, 255, 235, 0, 126, 128, 16]),
                       ('yvyu', [126, 255, 235, 128, 126, 128, 16, 0])):
        arr = conventional(Y[None], U[None], V[None], fmt)
        assert arr.shape == (1, 2, 4, 2) and arr[0, 0].ravel().tolist() == row, fmt
        (buf, desc) = pitched(Y[None], U[None], V[None], fmt, row_pad=4, stride_pad=8)
        assert (desc.row_pitch, desc.frame_stride, buf.size) == (12, 28, 20) and buf[:8].tolist() == row and buf[12:20].tolist() == arr[0, 1].ravel().tolist()
    # bgr_to_yuv422 makes plausible input (not an expected value of anything): grey stays grey
    (y, u, v) = bgr_to_yuv422(np.full((1, 2, 4, 3), 128, np.uint8))
    assert y.shape == (1, 2, 4) and u.shape == (1, 2, 2) and (u == 128).all() and (v == 128).all() and (y == 126).all()


def test_yuv422_kernels_metadata():
    """The kernels that read 4:2:2 frames are in the library, one instantiation per body (the byte order is a runtime value),
    without scratch; the dial readers within k_dials' register count."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    names = ('k_p422_lplane', 'k_p422_match', 'k_p422_needle', 'k_p422_to_bgr')
    new = {k: d for (k, d) in meta.items() if any(s in k for s in names)}
    assert [sum(s in k for k in new) for s in names] == [1, 1, 6, 1]
    dials_vgpr = max(d['vgpr_count'] for (k, d) in meta.items() if 'k_dials' in k)
    for (k, d) in new.items():
        assert d.get('private_segment_fixed_size', 0) == 0 and d.get('vgpr_spill_count', 0) == 0, (k, d)
        if 'k_p422_needle' in k:
            assert d['vgpr_count'] <= dials_vgpr, (k, d)


# ------------------------------------------------------------------------------------------------------------- GPU ---------
_read_both = functools.partial(fc.read_both, F422)


def _check_formats(reader, Y, U, V, tag, rng, formats=FORMATS, want=None):
    """Every format, conventional and pitched, host and device, against read_frames of the converted frames."""
    return fc.check_formats(F422, reader, (Y, U, V), tag, rng, formats, want)


def _check_source(reader, src, tag, rng, **kw):
    return _check_formats(reader, *src, tag, rng, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', FORMATS)
def test_yuv422_to_bgr_all_triples(env, fmt):
    """melf_yuv422_to_bgr == the numpy restatement for all 2^24 (Y, U, V), each at the even and at the odd pixel of a macropixel:
    one 4096 x 8192 frame, macropixel b has (U, V) = (b & 255, (b >> 8) & 255), Y0 = b >> 16 and Y1 = 255 - Y0."""
    ctx = env['sample-images1']['reader'].ctx
    b = np.arange(4096 * 4096, dtype=np.uint32).reshape(4096, 4096)
    U = (b & 255).astype(np.uint8)[None]
    V = ((b >> 8) & 255).astype(np.uint8)[None]
    Y = np.empty((1, 4096, 8192), np.uint8)
    Y[0, :, 0::2] = (b >> 16).astype(np.uint8)
    Y[0, :, 1::2] = 255 - (b >> 16).astype(np.uint8)
    uv = (V[0].astype(np.uint32) << 16) | (U[0].astype(np.uint32) << 8)
    for plane in (Y[0, :, 0::2], Y[0, :, 1::2]):   # the coverage, at the even and at the odd pixel
        seen = np.zeros(1 << 24, bool)
        seen[(uv | plane).ravel()] = True
        assert seen.all()
    v = _hip.yuv422_frames_view(conventional(Y, U, V, fmt), fmt)
    assert not v.copied
    got = ctx.yuv422_to_bgr(v.ptr, v.descriptor())
    want = yuv422_to_bgr(Y, U, V)
    bad = np.flatnonzero((got != want).any(axis=-1).ravel())
    assert bad.size == 0, (fmt, bad.size, bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', FORMATS)
def test_yuv422_to_bgr_padded_pitch_and_stride(env, fmt):
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(5)
    (n, H, W) = (3, 37, 50)
    (Y, U, V) = (rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H, W // 2), dtype=np.uint8),
                 rng.integers(0, 256, (n, H, W // 2), dtype=np.uint8))
    (buf, desc) = pitched(Y, U, V, fmt, row_pad=12, stride_pad=36, rng=rng)
    assert np.array_equal(ctx.yuv422_to_bgr(buf.ctypes.data, desc), yuv422_to_bgr(Y, U, V))
    arr = conventional(Y, U, V, fmt, 6, rng)
    v = _hip.yuv422_frames_view(arr[::2], fmt)
    assert not v.copied and v.row_pitch == 2 * (W + 6)
    assert np.array_equal(ctx.yuv422_to_bgr(v.ptr, v.descriptor()), yuv422_to_bgr(Y[::2], U[::2], V[::2]))


@pytest.mark.gpu
@pytest.mark.parametrize('sd,count,min_ok', [('sample-images1', 81, 79), ('sample-images2', 223, 222)])
def test_fixture_frames(env, sd, count, min_ok):  # noqa: F811
    fc.fixture_frames(F422, env[sd], sd, count, min_ok, _check_source)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')])
def test_each_match_kernel(env, monkeypatch, kind, kernel):  # noqa: F811
    layout = fc.as_conventional(F422, lambda fmt: 6)
    fc.each_match_kernel(env['sample-images1'], monkeypatch, kind, kernel, [(F422, FORMATS, layout)], n=256, seed=5, rng_seed=7,
                         min_not_found=28, min_ok=128)


@pytest.mark.gpu
def test_odd_geometry(env, tmp_path):  # noqa: F811
    """meter_rect (50, 160)-(300, 410) moved to all four parities of (x0, y0), and given sizes of all four parities (the far edge
    of the crop odd or even whatever the origin); the frames are shifted by as much, so that the meter stays inside."""
    cases = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0),       # origins at the four parities of (x, y), even sizes
             (0, 0, -1, 0), (0, 0, 0, -1), (0, 0, -1, -1),                  # sizes at the other three parities: far edge odd
             (1, 1, -1, -1), (1, 0, 1, 1), (3, 5, 1, 1), (1, 2, 2, 1))      # odd origin with an even / odd far edge
    fc.odd_geometry(F422, env['sample-images1'], tmp_path, cases,
                    lambda r, src, tag, rng, k: _check_source(r, src, tag, rng, formats=(FORMATS[k % 3], FORMATS[(k + 1) % 3])),
                    n=40, seed=3, rng_seed=13, min_ok=20)


@pytest.mark.gpu
def test_frame_edges_and_batch_sizes(env):  # noqa: F811
    """meter_rect (50, 160)-(300, 410) reaching the right and bottom frame edges, and past them (numpy clamp), with an odd frame
    height, device copies of exactly the descriptor's extent at the start of their allocation (every _read_both; what lies behind
    them is mapped: test_buffer_ends places them at its end); batch sizes around the 32-frame group and above the 128 frames of a
    host-path chunk."""
    e = env['sample-images1']
    rng = np.random.default_rng(11)
    src = fc.synth(e['frames'], 131, 3)
    fc.frame_edges(F422, e['reader'], src, rng, 12, ((410, 300), (399, 290), (405, 298)), _check_source, min_ok=6)
    fc.batch_sizes(F422, e['reader'], src, rng, (1, 31, 32, 33, 131), lambda k: (FORMATS[k % 3],), _check_source, min_ok=80)


@pytest.mark.gpu
def test_buffer_ends(env, monkeypatch, tmp_path):  # noqa: F811
    """tests/frame_cases.py: buffer_ends -- pitched buffers of exactly the descriptor's extent that end where their allocation ends,
    at every base phase the descriptor check accepts, the match at the crop's bottom-right corner, 1 and 33 frames, every match
    kernel."""
    fc.buffer_ends(monkeypatch, tmp_path, **fc.family_ends(F422), phases_of=lambda fmt: (0,))


@pytest.mark.gpu
def test_random_frames(env):  # noqa: F811
    """Uniform random Y, U, V bytes: every clamp of the conversion is hit, in every kernel that converts."""
    fc.random_yuv_frames(F422, env['sample-images1'], _check_source, n=40, seed=99)


@pytest.mark.gpu
def test_1080p_six_dials_uyvy_padded(env, tmp_path):
    """The configuration of tests/test_pixel_formats.py::test_1080p_six_dials_bgra_padded as UYVY with a padded pitch."""
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
    (Y, U, V) = bgr_to_yuv422(frames)
    reader = MeterReader(params)
    try:
        want = reader.read_frames(yuv422_to_bgr(Y, U, V))
        assert (want['status'] == _hip.FRAME_OK).any()
        arr = conventional(Y, U, V, 'uyvy', 32, rng)
        v = _hip.yuv422_frames_view(arr, 'uyvy')
        assert not v.copied and v.row_pitch == 2 * (1920 + 32)
        (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()
    finally:
        reader.close()


@pytest.mark.gpu
def test_resident_lanes_two_streams(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1) and two caller streams, formats alternating: every call's records equal a synchronous call's."""
    fc.resident_lanes_two_streams(F422, env['sample-images2'], ('yuyv', 'uyvy', 'yvyu', 'uyvy'),
                                  lambda k: dict(row_pad=4 * k, stride_pad=8 * k), n=96, seed=21, min_ok=48,
                                  keep_host=True)


@pytest.mark.gpu
def test_argument_errors_launch_nothing(env):
    e = env['sample-images1']
    ctx = e['reader'].ctx
    L = _hip.lib()
    (Y, U, V) = bgr_to_yuv422(np.stack(e['frames'][2:6]))
    (n, H, W) = Y.shape
    # two spare bytes in front, so that a misaligned base lies inside the buffers
    host = np.zeros(n * H * W * 2 + 4, np.uint8)
    assert host.ctypes.data % 4 == 0
    host[:n * H * W * 2] = conventional(Y, U, V, 'yuyv').ravel()
    buf = DevBuf(host.ctypes.data, host.nbytes)
    try:
        ctx.set_profiling(1)
        before = fc.launch_counts(ctx)
        out = np.zeros(n, _hip.RESULT_DTYPE)
        bgr_out = np.zeros((n, H, W, 3), np.uint8)
        F = _hip.MelfYuv422Frames
        (rp, fs) = (2 * W, 2 * W * H)
        bad = [
            F(3, 0, n, H, W, 0, rp, fs),                     # unknown format
            F(-1, 0, n, H, W, 0, rp, fs),
            F(0, 1, n, H, W, 0, rp, fs),                     # unknown matrix
            F(0, 0, n, H, W - 1, 0, rp, fs),                 # odd W
            F(1, 0, n, H, W, 0, rp - 4, fs),                 # pitch too small
            F(2, 0, n, H, W, 0, rp, fs - 4),                 # stride too small
            F(0, 0, n, H, W - 2, 0, rp - 2, fs),             # misaligned pitch
            F(0, 0, n, H - 1, W, 0, rp, fs - 2),             # misaligned stride
            F(0, 0, n, 0, W, 0, rp, fs),                     # bad shape
            F(0, 0, n, H, 0, 0, rp, fs),
            F(0, 0, n, -1, W, 0, rp, fs),
            F(0, 0, -1, H, W, 0, rp, fs),
        ]

        def all_fail(dptr, hptr, fref, key):
            assert L.melf_process_yuv422_dev(ctx._h, dptr, fref, None, _hip._ptr(out), None) == -1, key
            assert L.melf_last_error().decode()
            assert L.melf_process_yuv422(ctx._h, hptr, fref, _hip._ptr(out)) == -1, key
            assert L.melf_last_error().decode()
            assert L.melf_yuv422_to_bgr(ctx._h, hptr, fref, _hip._ptr(bgr_out)) == -1, key
            assert L.melf_last_error().decode()
        for f in bad:
            all_fail(C.c_void_p(buf.d.value), C.c_void_p(host.ctypes.data), C.byref(f),
                     (f.format, f.matrix, f.n, f.H, f.W, f.row_pitch, f.frame_stride))
        good = F(0, 0, n, H, W, 0, rp, fs)
        all_fail(C.c_void_p(buf.d.value), C.c_void_p(host.ctypes.data), None, 'NULL descriptor')
        all_fail(None, None, C.byref(good), 'NULL frames')
        all_fail(C.c_void_p(buf.d.value + 2), C.c_void_p(host.ctypes.data + 2), C.byref(good), 'misaligned base')
        # n == 0 passes, whatever the pointers
        empty = F(0, 0, 0, H, W, 0, rp, fs)
        assert L.melf_process_yuv422_dev(ctx._h, None, C.byref(empty), None, None, None) == 0
        assert L.melf_process_yuv422(ctx._h, None, C.byref(empty), None) == 0
        assert L.melf_yuv422_to_bgr(ctx._h, None, C.byref(empty), None) == 0
        assert fc.launch_counts(ctx) == before
        # a good descriptor runs
        assert L.melf_process_yuv422_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
        assert fc.launch_counts(ctx) != before
        assert out.tobytes() == e['reader'].read_frames(yuv422_to_bgr(Y, U, V)).tobytes()
    finally:
        ctx.set_profiling(0)
        buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_yuv422_frames with torch tensors, in a child process that imports torch first."""
    fc.run_torch_child('yuv422')
