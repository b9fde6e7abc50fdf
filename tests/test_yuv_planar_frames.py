"""melf_process_yuv_planar* / melf_yuv_planar_to_bgr: planar and semi-planar YUV frames of any 8-bit chroma subsampling -- 4:2:2
(I422, YV16, NV16, NV61), 4:4:4 (I444, YV24, NV24, NV42), 4:4:0 (I440) and 4:2:0 (NV21; NV12, I420 and YV12 again) -- read in place.

The contract (include/meterelf_hip.h): the records are byte-identical to melf_process_batch on the packed BGR frame that the
header's integer conversion makes of each frame under the descriptor's matrix, with the NEAREST chroma sample: pixel (x, y) uses
U[y >> sub_y][x >> sub_x] and V[..]; U of pixel (x, y) is the byte at frame + u_offset + (y >> sub_y) * c_pitch + (x >> sub_x) *
c_step.  yuv_to_bgr of tests/frame_cases.py (yuv_planar_to_bgr here) restates that in numpy; every GPU test compares against
read_frames of its output.

The reference (meterelf/_image.py:46-55) has cv2.imread and nothing else: it never sees such frames.  These layouts are what the
sources of the 'bt601-full' / 'bt709-full' matrices deliver (software MJPEG decoders: yuvj422p; screen capture: 4:4:4; V4L2 /
Rockchip decoders: NV16; Android's camera: NV21).
"""
import ctypes as C
import functools
import os
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
from tests.frame_cases import (DevBuf, conventional420, conventional_yuv_planar as conventional, env,  # noqa: E402,F401
                               extent_yuv_planar as _desc_extent, pitched420, pitched_yuv_planar as pitched, rows_of)

FORMATS = fc.YUV_PLANAR_FORMATS
NAMES = ('i422', 'yv16', 'nv16', 'nv61', 'i444', 'yv24', 'nv24', 'nv42', 'i440', 'nv21', 'nv12', 'i420', 'yv12')
SUBSAMPLINGS = {'422': (1, 0), '444': (0, 0), '440': (0, 1), '420': (1, 1)}
yuv_planar_to_bgr = fc.yuv_to_bgr   # (Y, U, V, sub_x, sub_y, matrix=0): the header's conversion, restated
bgr_to_yuv = fc.bgr_to_yuv          # (bgr, sub_x, sub_y): test input only
yuv420_to_bgr = fc.F420.bgr_of


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_struct_matches_header(tmp_path):
    fields = ('matrix', 'n', 'H', 'W', 'sub_x', 'sub_y', 'c_step', 'reserved', 'y_pitch', 'c_pitch', 'u_offset', 'v_offset', 'frame_stride')
    src = tmp_path / 'yuvp.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(melf_yuv_planar_frames));\n'
                   + ''.join('printf(" %%zu", offsetof(melf_yuv_planar_frames, %s));\n' % f for f in fields)
                   + 'printf(" %d\\n", MELF_ABI_VERSION);return 0;}\n')
    exe = tmp_path / 'yuvp'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfYuvPlanarFrames
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in fields] + [3]
    for name in ('melf_process_yuv_planar', 'melf_process_yuv_planar_dev', 'melf_yuv_planar_to_bgr'):
        assert name in _hip.EXPORTS


def test_format_table():
    assert tuple(FORMATS) == NAMES
    assert {k: v[:2] for (k, v) in FORMATS.items()} == {
        'i422': (1, 0), 'yv16': (1, 0), 'nv16': (1, 0), 'nv61': (1, 0), 'i444': (0, 0), 'yv24': (0, 0), 'nv24': (0, 0), 'nv42': (0, 0),
        'i440': (0, 1), 'nv21': (1, 1), 'nv12': (1, 1), 'i420': (1, 1), 'yv12': (1, 1)}
    assert [k for (k, v) in FORMATS.items() if v[2] == 2] == ['nv16', 'nv61', 'nv24', 'nv42', 'nv21', 'nv12']
    assert [k for (k, v) in FORMATS.items() if v[3]] == ['yv16', 'nv61', 'yv24', 'nv42', 'nv21', 'yv12']


def _makers():
    yield lambda a: a
    try:
        import torch
    except ImportError:
        return
    yield torch.from_numpy


@pytest.mark.parametrize('fmt', NAMES)
def test_view_layouts(fmt):
    """The descriptor and the extent of the conventional array, for numpy arrays and torch CPU tensors: exact values, in place."""
    (sx, sy, step, vfirst) = FORMATS[fmt]
    (n, H, W) = (3, 8, 12)
    (ch, cw) = (H >> sy, (W >> sx) * step)
    rows = rows_of(fmt, H)
    assert rows == {(1, 0): 2 * H, (0, 0): 3 * H, (0, 1): 2 * H, (1, 1): 3 * H // 2}[(sx, sy)]
    for make in _makers():
        base = np.zeros((n, rows, W), np.uint8)
        v = _hip.yuv_planar_frames_view(make(base), fmt, 'bt709')
        assert not v.copied and v.ptr == base.ctypes.data and not v.on_device and v.matrix == 3
        assert (v.n, v.H, v.W, v.sub_x, v.sub_y, v.c_step, v.y_pitch, v.frame_stride) == (n, H, W, sx, sy, step, W, rows * W)
        assert v.c_pitch == cw
        if step == 2:
            assert (v.u_offset, v.v_offset) == ((H * W + 1, H * W) if vfirst else (H * W, H * W + 1))
        else:
            (a, b) = (H * W, H * W + ch * cw)
            assert (v.u_offset, v.v_offset) == ((b, a) if vfirst else (a, b))
        assert v.extent == n * rows * W == _desc_extent(v.descriptor())
        d = v.descriptor()
        assert (d.matrix, d.n, d.H, d.W, d.sub_x, d.sub_y, d.c_step, d.reserved) == (3, n, H, W, sx, sy, step, 0)
        # every other frame, and a slice of frames: in place
        v2 = _hip.yuv_planar_frames_view(make(base)[::2], fmt)
        assert not v2.copied and v2.n == 2 and v2.frame_stride == 2 * rows * W and v2.extent == 3 * rows * W and v2.matrix == 0
        v3 = _hip.yuv_planar_frames_view(make(base)[1:], fmt)
        assert not v3.copied and v3.ptr == base.ctypes.data + rows * W and v3.extent == 2 * rows * W
        # padded rows: in place where a chroma row is one row of the array, one packed copy otherwise
        wide = np.zeros((n, rows, W + 5), np.uint8)
        vw = _hip.yuv_planar_frames_view(make(wide)[:, :, :W], fmt)
        if cw == W:
            assert not vw.copied and vw.ptr == wide.ctypes.data and (vw.y_pitch, vw.c_pitch) == (W + 5, W + 5)
            assert min(vw.u_offset, vw.v_offset) == H * (W + 5) and vw.frame_stride == rows * (W + 5)
            assert vw.extent == (n - 1) * rows * (W + 5) + (rows - 1) * (W + 5) + W == _desc_extent(vw.descriptor())
        else:
            assert vw.copied and vw.ptr != wide.ctypes.data and (vw.y_pitch, vw.c_pitch, vw.frame_stride) == (W, cw, rows * W)
        # an element stride of 2: copied
        assert _hip.yuv_planar_frames_view(make(np.zeros((n, rows, 2 * W), np.uint8))[:, :, ::2], fmt).copied
        # n == 0
        assert _hip.yuv_planar_frames_view(make(base)[:0], fmt).extent == 0


def test_view_444_as_planes():
    (n, H, W) = (2, 6, 7)
    for make in _makers():
        base = np.zeros((n, 3, H, W), np.uint8)
        for (fmt, uo, vo) in (('i444', H * W, 2 * H * W), ('yv24', 2 * H * W, H * W)):
            v = _hip.yuv_planar_frames_view(make(base), fmt, 'bt601-full')
            assert not v.copied and (v.H, v.W, v.sub_x, v.sub_y, v.c_step, v.matrix) == (H, W, 0, 0, 1, 2)
            assert (v.y_pitch, v.c_pitch, v.u_offset, v.v_offset, v.frame_stride, v.extent) == (W, W, uo, vo, 3 * H * W, n * 3 * H * W)
        big = np.zeros((n, 4, H + 2, W + 3), np.uint8)
        v = _hip.yuv_planar_frames_view(make(big)[:, :3, :H, :W], 'i444')
        ps = (H + 2) * (W + 3)
        assert not v.copied and (v.y_pitch, v.c_pitch, v.u_offset, v.v_offset, v.frame_stride) == (W + 3, W + 3, ps, 2 * ps, 4 * ps)
        assert v.extent == 4 * ps + 2 * ps + (H - 1) * (W + 3) + W == _desc_extent(v.descriptor())
        nhwc = make(np.zeros((n, H, W, 3), np.uint8))
        chw = nhwc.transpose(0, 3, 1, 2) if isinstance(nhwc, np.ndarray) else nhwc.permute(0, 3, 1, 2)
        assert _hip.yuv_planar_frames_view(chw, 'i444').copied       # an element stride of 3
        with pytest.raises(ValueError):
            _hip.yuv_planar_frames_view(make(base), 'i422')          # four dimensions: 4:4:4 planar only
        with pytest.raises(ValueError):
            _hip.yuv_planar_frames_view(make(base), 'nv24')
        with pytest.raises(ValueError):
            _hip.yuv_planar_frames_view(make(np.zeros((n, 4, H, W), np.uint8)), 'i444')


def test_view_errors():
    z = np.zeros
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 16, 8), np.uint8), 'yuyv')              # not a name of the family
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 16, 8), np.uint8), 'i422', 'bt2020')    # unknown matrix
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 16, 8), np.uint8), 'i422', 1)           # code 1 is never assigned
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 16, 8), np.int8), 'i422')               # not uint8
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((16, 8), np.uint8), 'i422')                 # not three-dimensional
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 15, 8), np.uint8), 'i422')              # rows not 2 H
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 16, 7), np.uint8), 'i422')              # odd W with horizontal subsampling
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 16, 7), np.uint8), 'nv16')
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 14, 8), np.uint8), 'i440')              # odd H (7) with vertical subsampling
    with pytest.raises(ValueError):
        _hip.yuv_planar_frames_view(z((1, 16, 8), np.uint8), 'i444')              # rows not 3 H


def test_view_accepts_what_the_subsampling_allows():
    v = _hip.yuv_planar_frames_view(np.zeros((1, 9, 8), np.uint8), 'nv21')
    assert (v.H, v.W, v.u_offset, v.v_offset, v.c_pitch) == (6, 8, 49, 48, 8)
    # odd W is fine where the chroma is not subsampled horizontally, odd H where not vertically
    v = _hip.yuv_planar_frames_view(np.zeros((1, 21, 7), np.uint8), 'i444')
    assert (v.H, v.W) == (7, 7)
    v = _hip.yuv_planar_frames_view(np.zeros((1, 14, 8), np.uint8), 'i422')
    assert (v.H, v.W, v.c_pitch) == (7, 8, 4)


def test_read_yuv_frames_still_rejects_nv21():
    with pytest.raises(ValueError):
        _hip.yuv_frames_view(np.zeros((1, 12, 8), np.uint8), 'nv21')
    assert not _hip.yuv_planar_frames_view(np.zeros((1, 12, 8), np.uint8), 'nv21').copied   # the new view takes the same array


def test_restatement_equals_420_restatement():
    """The 4:2:0 file's restatement is the shared yuv_to_bgr at (1, 1) since the two were made one function; what is left to
    check is that the package's table gives nv12 that subsampling."""
    rng = np.random.default_rng(4)
    (Y, U, V) = (rng.integers(0, 256, (2, 12, 20), dtype=np.uint8), rng.integers(0, 256, (2, 6, 10), dtype=np.uint8),
                 rng.integers(0, 256, (2, 6, 10), dtype=np.uint8))
    (sx, sy) = FORMATS['nv12'][:2]   # the package's table says what 4:2:0 is
    assert np.array_equal(yuv_planar_to_bgr(Y, U, V, sx, sy, 0), yuv420_to_bgr(Y, U, V))


@pytest.mark.parametrize('name', sorted(SUBSAMPLINGS))
def test_restatement_hand_written_4x4(name):
    """A 4 x 4 frame, a distinct chroma value per sample: every pixel is the hand-derived conversion of (its Y, the chroma sample at
    (y >> sub_y, x >> sub_x)), worked out per pixel with Python integers."""
    (sx, sy) = SUBSAMPLINGS[name]
    assert FORMATS[{'422': 'i422', '444': 'i444', '440': 'i440', '420': 'i420'}[name]][:2] == (sx, sy)   # the package's table agrees
    Y = (16 + 13 * np.arange(16)).astype(np.uint8).reshape(4, 4)
    (ch, cw) = (4 >> sy, 4 >> sx)
    U = (40 + 11 * np.arange(ch * cw)).astype(np.uint8).reshape(ch, cw)
    V = (230 - 9 * np.arange(ch * cw)).astype(np.uint8).reshape(ch, cw)
    assert len(set(U.ravel())) == ch * cw and len(set(V.ravel())) == ch * cw
    got = yuv_planar_to_bgr(Y, U, V, sx, sy, 0)
    for y in range(4):
        for x in range(4):
            (u, v) = (int(U[y >> sy, x >> sx]) - 128, int(V[y >> sy, x >> sx]) - 128)
            yy = max(int(Y[y, x]) - 16, 0) * 1220542 + (1 << 19)
            want = (min(max((yy + 2116026 * u) >> 20, 0), 255), min(max((yy - 852492 * v - 409993 * u) >> 20, 0), 255),
                    min(max((yy + 1673527 * v) >> 20, 0), 255))
            assert tuple(int(c) for c in got[y, x]) == want, (name, x, y)
    # two pixels by hand: (0, 0): Y 16, U 40, V 230 -> yy = 524288; B: 524288 + 2116026 * -88 < 0 -> 0;
    #   G: 524288 - 852492 * 102 - 409993 * -88 = -50350512 -> 0; R: 524288 + 1673527 * 102 = 171224042 >> 20 = 163
    assert tuple(int(c) for c in got[0, 0]) == (0, 0, 163)
    # (3, 3) at 4:4:4: Y 211, U 40 + 165 = 205, V 230 - 135 = 95: yy = 195 * 1220542 + 524288 = 238529978;
    #   B: + 2116026 * 77 = 401463980 >> 20 = 382 -> 255; G: - 852492 * -33 - 409993 * 77 = 235092753 >> 20 = 224;
    #   R: + 1673527 * -33 = 183303587 >> 20 = 174
    if name == '444':
        assert tuple(int(c) for c in got[3, 3]) == (255, 224, 174)


def test_kernels_metadata():
    """The kernels that read these frames are in the library: no scratch, no spills; the dial readers within k_dials' VGPR count."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    names = ('k_yp_lplane', 'k_yp_match', 'k_yp_needle', 'k_yp_to_bgr')
    new = {k: d for (k, d) in meta.items() if any(s in k for s in names)}
    assert [sum(s in k for k in new) for s in names] == [4, 1, 24, 1]
    dials_vgpr = max(d['vgpr_count'] for (k, d) in meta.items() if 'k_dials' in k)
    for (k, d) in new.items():
        assert d.get('private_segment_fixed_size', 0) == 0 and d.get('vgpr_spill_count', 0) == 0, (k, d)
        if 'k_yp_needle' in k:
            assert d['vgpr_count'] <= dials_vgpr, (k, d)


# ------------------------------------------------------------------------------------------------------------- GPU ---------
_read_both = functools.partial(fc.read_both, fc.yuv_planar(1, 0))   # (the entry points are those of every subsampling)


def _check_formats(reader, bgr, tag, rng, formats=NAMES, pitch=True):
    """Every format named: the frames forward-converted to its subsampling, as the conventional array and as a pitched buffer with
    odd pads and gaps, host and device, against read_frames of the restated conversion.  Returns {subsampling: want}."""
    wants = {}
    planes = {}
    for fmt in formats:
        (sx, sy, step, _vf) = FORMATS[fmt]
        if (sx, sy) not in planes:
            planes[(sx, sy)] = bgr_to_yuv(bgr, sx, sy)
            wants[(sx, sy)] = reader.read_frames(yuv_planar_to_bgr(*planes[(sx, sy)], sx, sy))
        (Y, U, V) = planes[(sx, sy)]
        wb = wants[(sx, sy)].tobytes()
        pad = 10 if (Y.shape[2] >> sx) * step == Y.shape[2] else 0
        arr = conventional(Y, U, V, fmt, pad, rng)
        assert reader.read_yuv_planar_frames(arr, fmt).tobytes() == wb, (tag, fmt, 'reader')
        v = _hip.yuv_planar_frames_view(arr, fmt)
        assert not v.copied
        (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == wb, (tag, fmt, 'host')
        assert dev.tobytes() == wb, (tag, fmt, 'device')
        if pitch:
            (raw, desc, _lead) = pitched(Y, U, V, fmt, y_pad=7, c_pad=5, gap=3, stride_pad=11, rng=rng)
            (host, dev) = _read_both(reader, raw.ctypes.data, desc, raw.nbytes)
            assert host.tobytes() == wb, (tag, fmt, 'pitched host')
            assert dev.tobytes() == wb, (tag, fmt, 'pitched device')
    return wants


# the eight forms of the chroma fetch: sub_x x c_step x the order of U and V; with the matrix each runs under and its sub_y
FORMS = [('i422', 0), ('yv16', 2), ('nv16', 0), ('nv61', 3), ('i444', 0), ('yv24', 4), ('nv24', 0), ('nv42', 0),
         ('i440', 0), ('nv21', 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('fmt,matrix', FORMS)
def test_to_bgr_all_triples(env, fmt, matrix):
    """melf_yuv_planar_to_bgr == the restatement for all 2^24 (Y, U, V): 2048 x 2048 chroma samples, sample b = (U, V) =
    (b & 255, (b >> 8) & 255), whose row band sets the base Y value k = 4 (b >> 16).  The pixels of a sample's block carry
    k + their position in it; where a block has fewer than four pixels, 4 / (pixels per block) frames over the same chroma carry
    the remaining values, so that k .. k + 3 all occur with every (U, V) and every position of a block is converted."""
    ctx = env['sample-images1']['reader'].ctx
    (sx, sy, _step, _vf) = FORMATS[fmt]
    b = np.arange(2048 * 2048, dtype=np.uint32).reshape(2048, 2048)
    U = (b & 255).astype(np.uint8)[None]
    V = ((b >> 8) & 255).astype(np.uint8)[None]
    (H, W) = (2048 << sy, 2048 << sx)
    if (sx, sy) == (1, 1):
        k = ((b >> 16).astype(np.uint8) * 4)
        Y = np.empty((1, H, W), np.uint8)
        (Y[0, 0::2, 0::2], Y[0, 0::2, 1::2], Y[0, 1::2, 0::2], Y[0, 1::2, 1::2]) = (k, k + 1, k + 2, k + 3)
        need = 1
    else:
        # fewer than four pixels per sample: four frames' worth of Y values over the same chroma (4 / pixels-per-sample frames)
        need = 4 >> (sx + sy)
        k = ((b >> 16).astype(np.uint8) * 4)
        Y = np.empty((need, H, W), np.uint8)
        for i in range(need):
            if sx:
                (Y[i, :, 0::2], Y[i, :, 1::2]) = (k + 2 * i, k + 2 * i + 1)
            elif sy:
                (Y[i, 0::2, :], Y[i, 1::2, :]) = (k + 2 * i, k + 2 * i + 1)
            else:
                Y[i] = k + i
        (U, V) = (np.repeat(U, need, axis=0), np.repeat(V, need, axis=0))
    seen = np.zeros(1 << 24, bool)
    uvf = ((V.astype(np.uint32) << 16) | (U.astype(np.uint32) << 8))
    for i in range(need):
        for oy in range(1 << sy):
            for ox in range(1 << sx):
                seen[(uvf[i] | Y[i, oy::1 << sy, ox::1 << sx]).ravel()] = True
    assert seen.all()
    v = _hip.yuv_planar_frames_view(conventional(Y, U, V, fmt), fmt, matrix)
    assert not v.copied
    got = ctx.yuv_planar_to_bgr(v.ptr, v.descriptor())
    want = yuv_planar_to_bgr(Y, U, V, sx, sy, matrix)
    bad = np.flatnonzero((got != want).any(axis=-1).ravel())
    assert bad.size == 0, (fmt, bad.size, bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', NAMES)
def test_to_bgr_padded_pitches(env, fmt):
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(5)
    (sx, sy, _step, _vf) = FORMATS[fmt]
    (n, H, W) = (3, 38, 50)
    (Y, U, V) = (rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H >> sy, W >> sx), dtype=np.uint8),
                 rng.integers(0, 256, (n, H >> sy, W >> sx), dtype=np.uint8))
    (raw, desc, _lead) = pitched(Y, U, V, fmt, y_pad=9, c_pad=3, gap=5, stride_pad=13, rng=rng, matrix=4)
    assert np.array_equal(ctx.yuv_planar_to_bgr(raw.ctypes.data, desc), yuv_planar_to_bgr(Y, U, V, sx, sy, 4))


@pytest.mark.gpu
@pytest.mark.parametrize('sd,count', [('sample-images1', 81), ('sample-images2', 223)])
def test_fixture_frames(env, sd, count):
    """Every fixture frame under every format name; at least three quarters of each set read OK on the BGR side (the floor of
    tests/test_yuv_matrices.py).  The counts are printed."""
    e = env[sd]
    assert len(e['frames']) == count
    rng = np.random.default_rng(count)
    shapes = {}
    for fr in e['frames']:
        shapes.setdefault(fr.shape, []).append(fr)
    ok = {}
    for (shape, group) in shapes.items():
        wants = _check_formats(e['reader'], np.stack(group), '%s %s' % (sd, shape), rng)
        for (key, want) in wants.items():
            ok[key] = ok.get(key, 0) + int((want['status'] == _hip.FRAME_OK).sum())
    print('%s: frames read OK per (sub_x, sub_y): %s' % (sd, ok))
    assert len(ok) == 4
    for (key, cnt) in ok.items():
        assert 4 * cnt >= 3 * count, (key, cnt)


@pytest.mark.gpu
def test_420_equals_existing_entry_points(env):
    """nv12 / i420 / yv12 through the new entry point == melf_process_yuv on the same bytes (other kernels: an independent
    cross-check); nv21 == nv12 of the swapped chroma."""
    e = env['sample-images1']
    reader = e['reader']
    (Y, U, V) = bgr_to_yuv(fc.synth(e['frames'], 70, 3), 1, 1)
    want = reader.read_frames(yuv420_to_bgr(Y, U, V))
    assert (want['status'] == _hip.FRAME_OK).sum() > 40
    for fmt in ('nv12', 'i420', 'yv12'):
        arr = conventional420(Y, U, V, fmt)
        assert np.array_equal(arr, conventional(Y, U, V, fmt))
        old = reader.read_yuv_frames(arr, fmt)
        assert old.tobytes() == want.tobytes()
        v = _hip.yuv_planar_frames_view(arr, fmt)
        (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == old.tobytes() and dev.tobytes() == old.tobytes(), fmt
    nv12_swapped = conventional420(Y, V, U, 'nv12')
    assert reader.read_yuv_planar_frames(nv12_swapped, 'nv21').tobytes() == want.tobytes()
    assert reader.read_yuv_frames(nv12_swapped, 'nv12').tobytes() == reader.read_yuv_planar_frames(nv12_swapped, 'nv12').tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')])
def test_each_match_kernel(env, monkeypatch, kind, kernel):  # noqa: F811
    groups = []
    for fmt in ('i422', 'nv42'):
        fam = fc.yuv_planar(*FORMATS[fmt][:2])
        groups.append((fam, (fmt,), fc.as_conventional(fam, lambda fmt: 0)))
    fc.each_match_kernel(env['sample-images1'], monkeypatch, kind, kernel, groups, n=256, seed=5, rng_seed=7, min_not_found=28,
                         min_ok=128)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SUBSAMPLINGS))
def test_odd_geometry(env, tmp_path, name):
    """meter_rect (50, 160)-(300, 410) at all four parities of origin and of size; the frames are shifted by as much."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    src = fc.synth(e['frames'], 24, 3)
    rng = np.random.default_rng(13)
    formats = [f for f in NAMES if FORMATS[f][:2] == SUBSAMPLINGS[name] and f not in ('nv12', 'i420', 'yv12')]
    for (k, (dx, dy, dw, dh)) in enumerate(((1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1), (1, 1, -1, -1))):
        params = fc.params_with_rect(tmp_path, 'sample-images1', (50 + dx, 160 + dy, 300 + dx + dw, 410 + dy + dh), 'odd%d' % k)
        r = MeterReader(params)
        try:
            wants = _check_formats(r, np.roll(src, (dy, dx), axis=(1, 2)), (dx, dy, dw, dh), rng, formats=formats, pitch=(k % 2 == 0))
            assert all((w['status'] == _hip.FRAME_OK).sum() > 12 for w in wants.values()), (dx, dy, dw, dh)
        finally:
            r.close()


@pytest.mark.gpu
def test_frame_edges_and_batch_sizes(env):
    """meter_rect reaching the right and bottom frame edges, and past them (numpy clamp); device copies of exactly the
    descriptor's extent at the start of their allocation (what lies behind them is mapped: test_buffer_ends places them at its
    end); batch sizes around the 32-frame group and 131."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(11)
    src = fc.synth(e['frames'], 131, 3)
    one_each = ('i422', 'nv61', 'yv24', 'nv24', 'i440', 'nv21')
    for (H, W) in ((410, 300), (400, 290)):
        wants = _check_formats(reader, np.ascontiguousarray(src[:12, :H, :W]), (H, W), rng, formats=one_each)
        assert all((w['status'] == _hip.FRAME_OK).sum() >= 6 for w in wants.values()), (H, W)
    for n in (1, 31, 32, 33, 131):
        _check_formats(reader, src[:n], n, rng, formats=('yv16', 'nv16', 'i444', 'nv42') if n != 131 else ('i422', 'nv24'), pitch=n < 131)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SUBSAMPLINGS))
def test_buffer_ends(env, monkeypatch, tmp_path, name):
    """tests/frame_cases.py: buffer_ends -- pitched buffers of exactly the descriptor's extent that end where their allocation ends,
    at every base phase the descriptor check accepts, the match at the crop's bottom-right corner, 1 and 33 frames, every match
    kernel; every format of one chroma subsampling per case."""
    fam = fc.yuv_planar(*SUBSAMPLINGS[name])
    assert sorted(f for s in SUBSAMPLINGS.values() for f in fc.yuv_planar(*s).formats) == sorted(NAMES)
    fc.buffer_ends(monkeypatch, tmp_path, **fc.family_ends(fam), phases_of=lambda fmt: (0, 1, 2, 3))


@pytest.mark.gpu
def test_first_byte_and_byte_phases(env):
    """The base at each of the four byte phases (1, 2 and 3 bytes into an allocation) and the chroma planes at each of the four
    byte phases relative to Y (gap 0 .. 3), with the fixtures' meter_rect: every window's v_alignbit phase.  (The crop is far from
    the base here; test_crop_at_the_buffers_first_byte puts it there.)"""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(17)
    bgr = fc.synth(e['frames'], 33, 8)
    for fmt in ('i422', 'nv16', 'i444', 'nv24'):
        (sx, sy, _step, _vf) = FORMATS[fmt]
        (Y, U, V) = bgr_to_yuv(bgr, sx, sy)
        wb = reader.read_frames(yuv_planar_to_bgr(Y, U, V, sx, sy)).tobytes()
        for gap in range(4):
            lead = (gap + 1) % 4
            (raw, desc, lead) = pitched(Y, U, V, fmt, y_pad=gap, c_pad=1, gap=gap, stride_pad=gap, rng=rng, lead=lead)
            extent = raw.nbytes - lead
            assert extent == _desc_extent(desc)
            assert reader.ctx.process_yuv_planar(raw.ctypes.data + lead, desc).tobytes() == wb, (fmt, gap, 'host')
            buf = DevBuf(raw.ctypes.data, raw.nbytes)   # the frames' base is `lead` bytes into the allocation
            try:
                assert reader.ctx.process_yuv_planar_dev(buf.d.value + lead, desc).tobytes() == wb, (fmt, gap, 'device')
            finally:
                buf.free()


@pytest.mark.gpu
def test_crop_at_the_buffers_first_byte(env, tmp_path):
    """meter_rect (0, 0)-(250, 250) on frames cut so that the meter lies in their top left corner (as
    tests/test_planar_frames.py::test_frame_edges_and_batch_sizes does), once with the frame larger than the crop and once with
    the crop filling it: the Y samples of the crop's first row are the buffer's first bytes.  With the base 1, 2 and 3 bytes into
    an allocation the prep kernel's aligned window of those samples would start before the base: rows_safe fails for the first
    row of the first frame group because of the base, lane 0 of row 0 of frame 0 fails the per-lane test and takes the byte
    loads, and the chroma windows' lower bounds are evaluated beside it.  One planar and one semi-planar layout at 4:2:2 and at
    4:4:4, the base at each of the four phases, host and device (a device buffer of exactly lead + extent bytes), byte-identical
    to read_frames."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    rng = np.random.default_rng(23)
    src = fc.synth(e['frames'], 40, 3)
    for (k, (y1, x1)) in enumerate(((480, 640), (410, 300))):
        bgr = np.ascontiguousarray(src[:, 160:y1, 50:x1])
        r = MeterReader(fc.params_with_rect(tmp_path, 'sample-images1', (0, 0, 250, 250), 'corner%d' % k))
        try:
            for fmt in ('i422', 'nv16', 'i444', 'nv24'):
                (sx, sy, _step, _vf) = FORMATS[fmt]
                (Y, U, V) = bgr_to_yuv(bgr, sx, sy)
                want = r.read_frames(yuv_planar_to_bgr(Y, U, V, sx, sy))
                assert (want['status'] == _hip.FRAME_OK).sum() >= 20, (y1, x1, fmt)
                wb = want.tobytes()
                # the raw-video array: an aligned base
                assert r.read_yuv_planar_frames(conventional(Y, U, V, fmt, 0, rng), fmt).tobytes() == wb, (y1, x1, fmt)
                for phase in range(4):
                    (raw, desc, lead) = pitched(Y, U, V, fmt, y_pad=phase, c_pad=1, gap=phase, stride_pad=phase, rng=rng, lead=phase)
                    assert lead == phase and raw.nbytes - lead == _desc_extent(desc)
                    assert r.ctx.process_yuv_planar(raw.ctypes.data + lead, desc).tobytes() == wb, (y1, x1, fmt, phase, 'host')
                    buf = DevBuf(raw.ctypes.data, raw.nbytes)   # the frames' base is `phase` bytes into the allocation
                    try:
                        assert (buf.d.value + lead) % 4 == phase
                        assert r.ctx.process_yuv_planar_dev(buf.d.value + lead, desc).tobytes() == wb, (y1, x1, fmt, phase, 'device')
                    finally:
                        buf.free()
        finally:
            r.close()


@pytest.mark.gpu
def test_host_staging_three_chunks(env, tmp_path):
    """257 host frames of 410 x 300: three staging chunks (as tests/test_host_staging.py for the other families)."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(257)
    bgr = np.ascontiguousarray(fc.synth(e['frames'], 257, 4)[:, :410, :300])
    for fmt in ('i422', 'nv61', 'i444', 'nv24', 'i440', 'nv21'):
        (sx, sy, _step, _vf) = FORMATS[fmt]
        (Y, U, V) = bgr_to_yuv(bgr, sx, sy)
        want = reader.read_frames(yuv_planar_to_bgr(Y, U, V, sx, sy))
        assert (want['status'] == _hip.FRAME_OK).sum() > 128
        assert reader.read_yuv_planar_frames(conventional(Y, U, V, fmt, 0, rng), fmt).tobytes() == want.tobytes(), fmt


@pytest.mark.gpu
def test_random_frames(env):
    """Uniform random Y, U, V bytes: every clamp of the conversion is hit, in every kernel that converts."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(99)
    (H, W) = e['frames'][2].shape[:2]
    n = 40
    for fmt in ('yv16', 'nv16', 'i444', 'nv42', 'i440', 'nv21'):
        (sx, sy, _step, _vf) = FORMATS[fmt]
        (Y, U, V) = (rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H >> sy, W >> sx), dtype=np.uint8),
                     rng.integers(0, 256, (n, H >> sy, W >> sx), dtype=np.uint8))
        # half of the frames carry a fixture's meter, so that the dial reader runs on them (random chroma under it)
        Y[::2] = bgr_to_yuv(np.stack(e['frames'][2:2 + n // 2]), 0, 0)[0]
        U[::2] = 128 + (U[::2].astype(np.int16) - 128) // 16
        V[::2] = 128 + (V[::2].astype(np.int16) - 128) // 16
        bgr = yuv_planar_to_bgr(Y, U, V, sx, sy, 2)
        assert (bgr == 0).any() and (bgr == 255).any()
        want = reader.read_frames(bgr)
        assert (want['status'] != _hip.FRAME_DIALS_NOT_FOUND).sum() >= n // 4
        (raw, desc, _lead) = pitched(Y, U, V, fmt, y_pad=3, c_pad=1, gap=1, stride_pad=5, rng=rng, matrix=2)
        (host, dev) = _read_both(reader, raw.ctypes.data, desc, raw.nbytes)
        assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes(), fmt


@pytest.mark.gpu
def test_1080p_six_dials_nv16_padded(env, tmp_path):
    """The configuration of tests/test_yuv_frames.py::test_1080p_six_dials_nv12_padded as NV16 with padded rows, 8 frames."""
    import shutil

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
    good = env['sample-images1']['frames'][2:10]
    frames = rng.integers(0, 256, size=(len(good), 1080, 1920, 3), dtype=np.uint8)
    for (i, f) in enumerate(good):
        frames[i, 420:670, 1210:1460] = f[160:410, 50:300]
    (Y, U, V) = bgr_to_yuv(frames, 1, 0)
    reader = MeterReader(params)
    try:
        want = reader.read_frames(yuv_planar_to_bgr(Y, U, V, 1, 0))
        assert (want['status'] == _hip.FRAME_OK).any()
        arr = conventional(Y, U, V, 'nv16', 64, rng)
        v = _hip.yuv_planar_frames_view(arr, 'nv16')
        assert not v.copied and v.y_pitch == 1920 + 64 and v.c_pitch == 1920 + 64 and v.n == 8
        (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()
    finally:
        reader.close()


@pytest.mark.gpu
def test_resident_lanes_two_streams(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1) and two caller streams, the layout and the entry-point family changing from call to call:
    every call's records equal a synchronous call's."""
    from meterelf_amd import MeterReader
    e = env['sample-images2']
    bgr = fc.synth(e['frames'], 96, 21)
    nf = len(bgr)
    r = MeterReader(e['params'])
    bufs = []
    keep = []
    try:
        calls = []   # (entry point bound to its device buffer and descriptor, wanted bytes)
        for (k, fmt) in enumerate(('i422', 'nv24', 'nv12-old', 'nv61', 'i440', 'yv24', 'nv21', 'bgr')):
            if fmt == 'bgr':
                want = r.read_frames(bgr)
                bufs.append(DevBuf(bgr.ctypes.data, bgr.nbytes))
                calls.append((functools.partial(r.ctx.process_batch_dev, bufs[-1].d.value, nf, bgr.shape[1], bgr.shape[2]), want.tobytes()))
                continue
            if fmt == 'nv12-old':
                (Y, U, V) = bgr_to_yuv(bgr, 1, 1)
                want = r.read_frames(yuv420_to_bgr(Y, U, V))
                (buf, desc) = pitched420(Y, U, V, 'nv12', y_pad=4, c_pad=2, gap=2, stride_pad=2, rng=np.random.default_rng(k))
                keep.append(buf)
                bufs.append(DevBuf(buf.ctypes.data, buf.nbytes))
                calls.append((functools.partial(r.ctx.process_yuv_dev, bufs[-1].d.value, desc), want.tobytes()))
                continue
            (sx, sy, _step, _vf) = FORMATS[fmt]
            (Y, U, V) = bgr_to_yuv(bgr, sx, sy)
            want = r.read_frames(yuv_planar_to_bgr(Y, U, V, sx, sy))
            assert (want['status'] == _hip.FRAME_OK).sum() > 48
            (raw, desc, _lead) = pitched(Y, U, V, fmt, y_pad=k, c_pad=2 * k + 1, gap=k, stride_pad=k, rng=np.random.default_rng(k))
            keep.append(raw)
            bufs.append(DevBuf(raw.ctypes.data, raw.nbytes))
            calls.append((functools.partial(r.ctx.process_yuv_planar_dev, bufs[-1].d.value, desc), want.tobytes()))
        fc.resident_calls(r, nf, calls, 2 * len(calls), lambda i: (3 * i) % len(calls))
    finally:
        r.close()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_argument_errors_launch_nothing(env):
    e = env['sample-images1']
    ctx = e['reader'].ctx
    L = _hip.lib()
    (Y, U, V) = bgr_to_yuv(np.stack(e['frames'][2:6]), 1, 0)
    (n, H, W) = Y.shape
    arr = conventional(Y, U, V, 'i422')
    buf = DevBuf(arr.ctypes.data, arr.nbytes)
    try:
        ctx.set_profiling(1)
        before = fc.launch_counts(ctx)
        out = np.zeros(n, _hip.RESULT_DTYPE)
        bgr_out = np.zeros((n, H, W, 3), np.uint8)
        F = _hip.MelfYuvPlanarFrames
        (fs, q, uo) = (2 * H * W, H * W // 2, H * W)

        def D(matrix=0, n=n, H=H, W=W, sub_x=1, sub_y=0, c_step=1, reserved=0, y_pitch=W, c_pitch=W // 2, u=uo, v=uo + q, fs=fs):
            return F(matrix, n, H, W, sub_x, sub_y, c_step, reserved, y_pitch, c_pitch, u, v, fs)
        # (what melf_last_error must name, the descriptor)
        bad = [
            ('reserved', D(reserved=1)),
            ('sub_x and sub_y', D(sub_x=2)), ('sub_x and sub_y', D(sub_x=-1)), ('sub_x and sub_y', D(sub_y=2)), ('sub_x and sub_y', D(sub_y=-1)),
            ('c_step must be', D(c_step=0)), ('c_step must be', D(c_step=3)),
            ('adjacent', D(c_step=2, c_pitch=W, u=uo, v=uo + 2)),                # semi-planar: offsets not adjacent
            ('adjacent', D(c_step=2, c_pitch=W, u=uo, v=uo)),
            ('even width', D(W=W - 1, y_pitch=W)),                               # odd W with sub_x
            ('even height', D(sub_y=1, H=H - 1)),                                # odd H with sub_y
            ('batch shape', D(H=0)), ('batch shape', D(W=0)), ('batch shape', D(n=-1)),
            ('negative', D(u=-1)), ('negative', D(v=-2)),
            ('matrix', D(matrix=1)), ('matrix', D(matrix=5)), ('matrix', D(matrix=-1)),
            ('y_pitch', D(y_pitch=W - 1)),
            ('c_pitch', D(c_pitch=W // 2 - 1)),
            ('c_pitch', D(c_step=2, c_pitch=W - 1, u=uo, v=uo + 1)),
            ('c_pitch', D(sub_x=0, c_pitch=W - 1, u=uo, v=uo + H * W, fs=3 * H * W)),
            ('two chroma planes', D(u=uo, v=uo + q - 1)),                        # the chroma planes' spans overlap each other
            ('two chroma planes', D(u=uo + q - 1, v=uo)),
            ("Y plane's span", D(u=uo - 1)),                                     # a chroma plane starts inside the Y plane's span
            ("Y plane's span", D(u=uo + q, v=uo - 1)),
            ("Y plane's span", D(c_step=2, c_pitch=W, u=uo - 1, v=uo)),
            ('frame_stride', D(fs=fs - 1)),                                      # stride smaller than one frame's span
            ('frame_stride', D(c_step=2, c_pitch=W, u=uo + 1, v=uo, fs=fs - 1)),
            ('y_pitch', D(y_pitch=2 ** 31)), ('c_pitch', D(c_pitch=2 ** 31)),
        ]
        fields = [f[0] for f in F._fields_]
        for (word, f) in bad:
            key = (word,) + tuple(getattr(f, k) for k in fields)
            assert L.melf_process_yuv_planar_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(f), None, _hip._ptr(out), None) == -1, key
            assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
            assert L.melf_process_yuv_planar(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(out)) == -1, key
            assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
            assert L.melf_yuv_planar_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(bgr_out)) == -1, key
            assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
        assert L.melf_process_yuv_planar_dev(ctx._h, C.c_void_p(buf.d.value), None, None, _hip._ptr(out), None) == -1
        assert L.melf_process_yuv_planar(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(out)) == -1
        assert 'descriptor is NULL' in L.melf_last_error().decode()
        assert L.melf_yuv_planar_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(bgr_out)) == -1
        good = D()
        assert L.melf_process_yuv_planar_dev(ctx._h, None, C.byref(good), None, _hip._ptr(out), None) == -1   # NULL frames
        assert 'frames pointer is NULL' in L.melf_last_error().decode()
        assert L.melf_process_yuv_planar(ctx._h, None, C.byref(good), _hip._ptr(out)) == -1
        assert 'frames pointer is NULL' in L.melf_last_error().decode()
        assert L.melf_yuv_planar_to_bgr(ctx._h, None, C.byref(good), _hip._ptr(bgr_out)) == -1
        assert 'frames pointer is NULL' in L.melf_last_error().decode()
        empty = D(n=0)
        assert L.melf_process_yuv_planar_dev(ctx._h, None, C.byref(empty), None, None, None) == 0             # n == 0 passes
        assert L.melf_process_yuv_planar(ctx._h, None, C.byref(empty), None) == 0
        assert fc.launch_counts(ctx) == before
        # a good descriptor runs
        assert L.melf_process_yuv_planar_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
        assert fc.launch_counts(ctx) != before
        assert out.tobytes() == e['reader'].read_frames(yuv_planar_to_bgr(Y, U, V, 1, 0)).tobytes()
    finally:
        ctx.set_profiling(0)
        buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_yuv_planar_frames with torch tensors, in a child process that imports torch first."""
    fc.run_torch_child('yuv_planar')
