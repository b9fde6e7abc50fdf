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

yuv_to_bgr(Y, U, V, 1, 1) of tests/frame_cases.py is its numpy restatement (yuv420_to_bgr here): the expected side of every
comparison.  bgr_to_yuv420 (float BT.601 limited-range RGB -> YUV, 2 x 2 chroma mean, round half up, clip) only makes test input
from the BGR fixtures; nothing is compared against it.

CPU tests: the descriptor against the header, yuv_frames_view's mapping of numpy arrays and torch CPU tensors, the restatement
against hand-derived triples, the new kernels' code-object notes.  GPU tests: the conversion kernel for all 2^24 triples, records
against the BGR path of the converted frames on the fixtures, with every match kernel, at odd crop origins, at the frame edges, at
1080p, over lanes and streams, with torch tensors (in a child process that imports torch first: tests/frame_cases.py says why).
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
from tests.frame_cases import DevBuf, F420, conventional420 as conventional, env, pitched420 as pitched  # noqa: E402,F401

FORMATS = F420.formats
yuv420_to_bgr = F420.bgr_of        # the conversion above, restated (tests/frame_cases.py: yuv_to_bgr)
bgr_to_yuv420 = F420.from_bgr      # test input only


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
_read_both = functools.partial(fc.read_both, F420)


def _check_formats(reader, Y, U, V, tag, rng, formats=('nv12', 'i420', 'yv12'), want=None):
    """Every format, conventional and pitched, host and device, against read_frames of the converted frames."""
    return fc.check_formats(F420, reader, (Y, U, V), tag, rng, formats, want)


def _check_source(reader, src, tag, rng, **kw):
    return _check_formats(reader, *src, tag, rng, **kw)


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
def test_fixture_frames(env, sd, count, min_ok):  # noqa: F811
    fc.fixture_frames(F420, env[sd], sd, count, min_ok, _check_source)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')])
def test_each_match_kernel(env, monkeypatch, kind, kernel):  # noqa: F811
    layout = fc.as_conventional(F420, lambda fmt: 6 if fmt == 'nv12' else 0)
    fc.each_match_kernel(env['sample-images1'], monkeypatch, kind, kernel, [(F420, FORMATS, layout)], n=256, seed=5, rng_seed=7,
                         min_not_found=28, min_ok=128)


@pytest.mark.gpu
def test_odd_geometry(env, tmp_path):  # noqa: F811
    """meter_rect (50, 160)-(300, 410) moved to odd x0, odd y0, both, and given an odd width and height; the frames are shifted
    by as much, so that the meter stays inside."""
    cases = ((1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, -1, -1), (1, 1, -1, -1), (3, 5, 1, 1))
    fc.odd_geometry(F420, env['sample-images1'], tmp_path, cases, lambda r, src, tag, rng, k: _check_source(r, src, tag, rng),
                    n=40, seed=3, rng_seed=13, min_ok=20)


@pytest.mark.gpu
def test_frame_edges_and_batch_sizes(env):  # noqa: F811
    """meter_rect (50, 160)-(300, 410) reaching the right and bottom frame edges, and past them (numpy clamp), device copies of
    exactly the descriptor's extent at the start of their allocation (every _read_both; what lies behind them is mapped:
    test_buffer_ends places them at its end); batch sizes around the 32-frame group."""
    e = env['sample-images1']
    rng = np.random.default_rng(11)
    src = fc.synth(e['frames'], 70, 3)
    fc.frame_edges(F420, e['reader'], src, rng, 12, ((410, 300), (400, 290)), _check_source, min_ok=6)
    fc.batch_sizes(F420, e['reader'], src, rng, (1, 31, 33, 70), lambda k: FORMATS, _check_source, min_ok=40)


@pytest.mark.gpu
def test_buffer_ends(env, monkeypatch, tmp_path):  # noqa: F811
    """tests/frame_cases.py: buffer_ends -- pitched buffers of exactly the descriptor's extent that end where their allocation ends,
    at every base phase the descriptor check accepts, the match at the crop's bottom-right corner, 1 and 33 frames, every match
    kernel."""
    fc.buffer_ends(monkeypatch, tmp_path, **fc.family_ends(F420, ('nv12', 'i420', 'yv12')),
                   phases_of=lambda fmt: (0, 1, 2, 3))


@pytest.mark.gpu
def test_first_bytes_unaligned_base(env, monkeypatch, tmp_path):  # noqa: F811
    """tests/frame_cases.py: first_bytes -- a base at byte phases 1 .. 3 and the meter crop at the frame's first row and first
    columns, where the launcher sends the prep kernel down its sample-by-sample path: the records are the BGR path's.  (Where the
    loads start is swept on the CPU, tests/prep_bounds_main.cpp.)"""
    args = fc.family_ends(F420, ('nv12', 'i420', 'yv12'))
    del args['nframes_stride']   # (buffer_ends' check of the frame stride)
    fc.first_bytes(monkeypatch, tmp_path, **args, x0s=(0, 3, 4))


@pytest.mark.gpu
def test_random_frames(env):  # noqa: F811
    """Uniform random Y, U, V bytes: every clamp of the conversion is hit, in every kernel that converts."""
    fc.random_yuv_frames(F420, env['sample-images1'], functools.partial(_check_source, formats=FORMATS), n=40, seed=99)


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
def test_resident_lanes_two_streams(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1) and two caller streams, formats alternating: every call's records equal a synchronous call's."""
    fc.resident_lanes_two_streams(F420, env['sample-images2'], ('nv12', 'i420', 'yv12', 'nv12'),
                                  lambda k: dict(y_pad=4 * k, c_pad=2 * k, gap=k, stride_pad=k), n=96, seed=21, min_ok=48,
                                  keep_host=True)


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
        before = fc.launch_counts(ctx)
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
        assert fc.launch_counts(ctx) == before
        # a good descriptor runs
        assert L.melf_process_yuv_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
        assert fc.launch_counts(ctx) != before
        assert out.tobytes() == e['reader'].read_frames(yuv420_to_bgr(Y, U, V)).tobytes()
    finally:
        ctx.set_profiling(0)
        buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_yuv_frames with torch tensors, in a child process that imports torch first."""
    fc.run_torch_child('yuv')
