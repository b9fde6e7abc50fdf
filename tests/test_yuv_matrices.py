"""The colour conversion of YUV frames as a choice: BT.601 / BT.709, limited / full range, for 4:2:0 (melf_process_yuv*,
melf_yuv_to_bgr) and packed 4:2:2 (melf_process_yuv422*, melf_yuv422_to_bgr) frames alike -- the `matrix` field of both
descriptors, the `matrix` argument of _hip.yuv_frames_view / yuv422_frames_view and MeterReader.read_yuv_frames /
read_yuv422_frames.

The contract: the records of a YUV frame are byte-identical to read_frames() of the packed BGR frame that the integer conversion
below makes of it under the descriptor's matrix (include/meterelf_hip.h), >> arithmetic:

    yy = max(Y - YOFF, 0) * CY        u = U - 128        v = V - 128
    R = clamp((yy + (1 << 19) + CRV * v)           >> 20, 0, 255)
    G = clamp((yy + (1 << 19) + CGV * v + CGU * u) >> 20, 0, 255)
    B = clamp((yy + (1 << 19) + CBU * u)           >> 20, 0, 255)

MATRIX of tests/frame_cases.py restates the table of offsets and coefficients, its yuv_to_bgr the arithmetic: the expected side of
every comparison.  Its bgr_to_yuv (float64 RGB -> YUV per matrix and range from Kr and Kb, chroma means, round half up, clip) only
makes test input from the BGR fixtures; nothing is compared against it.  test_yuv_frames.py and test_yuv422_frames.py keep pinning code 0 bit for bit, and code
1 as a rejected descriptor.
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
from tests.frame_cases import F420, F422, MATRIX, STANDARD, DevBuf, env, packed422  # noqa: E402,F401

NAMES = {'bt601': 0, 'bt601-full': 2, 'bt709': 3, 'bt709-full': 4}
NEW = (2, 3, 4)


def exact_coefficients(code):
    """(YOFF, cy, crv, cgv, cgu, cbu) of the standard in float64: the derivation rule of include/meterelf_hip.h."""
    (kr, kb, limited) = STANDARD[code]
    kg = 1.0 - kr - kb
    (crv, cbu) = (2.0 * (1.0 - kr), 2.0 * (1.0 - kb))
    (cgu, cgv) = (-kb * cbu / kg, -kr * crv / kg)
    (sc, sy) = (255.0 / 224.0, 255.0 / 219.0) if limited else (1.0, 1.0)
    return (16 if limited else 0, sy, crv * sc, cgv * sc, cgu * sc, cbu * sc)


# ------------------------------------------------------------------------------------------------- the conversion, restated ---
def yuv420_to_bgr(Y, U, V, code):
    """Y (..., H, W), U and V (..., H / 2, W / 2): the nearest chroma sample."""
    return fc.yuv_to_bgr(Y, U, V, 1, 1, code)


def yuv422_to_bgr(Y, U, V, code):
    """Y (..., H, W), U and V (..., H, W / 2): the two pixels of a macropixel share its chroma."""
    return fc.yuv_to_bgr(Y, U, V, 1, 0, code)


def forward_both(bgr, code):
    """Test input only: the 4:2:0 planes (2 x 2 chroma mean) and the 4:2:2 planes (pair mean) of the BGR frames."""
    return fc.bgr_to_yuv(bgr, 1, 1, code), fc.bgr_to_yuv(bgr, 1, 0, code)


@functools.lru_cache(maxsize=None)
def table(code):
    """The conversion of all 2^24 triples: (2^24, 3) uint8 BGR at index Y << 16 | V << 8 | U."""
    i = np.arange(1 << 24, dtype=np.uint32)
    return fc.yuv_to_bgr((i >> 16).astype(np.uint8), (i & 255).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), 0, 0, code)


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_matrix_codes_match_header(tmp_path):
    src = tmp_path / 'm.c'
    src.write_text('#include <stdio.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%d %d %d %d\\n", MELF_YUV_BT601_LIMITED, MELF_YUV_BT601_FULL, MELF_YUV_BT709_LIMITED, '
                   'MELF_YUV_BT709_FULL);return 0;}\n')
    exe = tmp_path / 'm'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [0, 2, 3, 4]
    assert got == [_hip.YUV_BT601_LIMITED, _hip.YUV_BT601_FULL, _hip.YUV_BT709_LIMITED, _hip.YUV_BT709_FULL]
    assert _hip.YUV_MATRIX_CODES == NAMES
    assert sorted(MATRIX) == sorted(NAMES.values()) and 1 not in MATRIX


def test_coefficients_are_the_standards_rounded():
    """Rows 2 - 4: round(2^20 c) of the coefficients derived from Kr and Kb here; row 0: cv2's three-decimal constants, literally."""
    for code in NEW:
        (yoff, cy, crv, cgv, cgu, cbu) = exact_coefficients(code)
        want = (yoff,) + tuple(int(np.floor(c * (1 << 20) + 0.5)) for c in (cy, crv, cgv, cgu, cbu))
        assert MATRIX[code] == want, (code, want)
    # cv2 (color_yuv.simd.hpp): ITUR_BT_601_CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527, Y - 16
    assert MATRIX[0] == (16, 1220542, 1673527, -852492, -409993, 2116026)
    # which is round(2^20 c) of the three-decimal 1.164, 1.596, -0.813, -0.391, 2.018, not of the exact BT.601 coefficients
    assert MATRIX[0][1:] == tuple(int(np.floor(c * (1 << 20) + 0.5)) for c in (1.164, 1.596, -0.813, -0.391, 2.018))


@pytest.mark.parametrize('code,differing', [(2, 8924), (3, 1315), (4, 0)])
def test_conversion_bounds_all_triples(code, differing):
    """Over all 2^24 (Y, U, V): every operand fits the 24-bit multiply, every sum stays below 2^30, every channel is within 1 of
    the float64 conversion (exact coefficients, rounded half up, clipped); the number of triples that differ from it at all."""
    (yoff, cy, crv, cgv, cgu, cbu) = MATRIX[code]
    assert all(abs(c) < (1 << 23) for c in (cy, crv, cgv, cgu, cbu))   # and the samples are within -128 .. 255
    i = np.arange(1 << 24, dtype=np.uint32)
    (Y, u, v) = ((i >> 16).astype(np.int64), (i & 255).astype(np.int64) - 128, ((i >> 8) & 255).astype(np.int64) - 128)
    yy = np.maximum(Y - yoff, 0) * cy
    sums = (yy + (1 << 19) + cbu * u, yy + (1 << 19) + cgv * v + cgu * u, yy + (1 << 19) + crv * v)
    worst = 0
    for parts in ((yy,), (cbu * u,), (cgv * v,), (cgu * u,), (crv * v,), (cgv * v + cgu * u + (1 << 19),), sums):
        for p in parts:
            worst = max(worst, int(np.abs(p).max()))
    assert worst < (1 << 30), worst
    (_, fy, frv, fgv, fgu, fbu) = exact_coefficients(code)
    (Yf, uf, vf) = (np.maximum(Y - yoff, 0).astype(np.float64) * fy, u.astype(np.float64), v.astype(np.float64))
    got = table(code)
    diff = np.zeros(1 << 24, bool)
    for (ch, ref) in ((0, Yf + fbu * uf), (1, Yf + fgv * vf + fgu * uf), (2, Yf + frv * vf)):
        want = np.clip(np.floor(ref + 0.5), 0, 255).astype(np.int16)
        d = np.abs(got[:, ch].astype(np.int16) - want)
        assert int(d.max()) <= 1, (code, ch)
        diff |= d != 0
    assert int(diff.sum()) == differing


def _one(code, y, u, v):
    px = yuv420_to_bgr(np.full((2, 2), y, np.uint8), np.full((1, 1), u, np.uint8), np.full((1, 1), v, np.uint8), code)
    p2 = yuv422_to_bgr(np.full((1, 2), y, np.uint8), np.full((1, 1), u, np.uint8), np.full((1, 1), v, np.uint8), code)
    assert (px == px[0, 0]).all() and (p2 == px[0, 0]).all()
    return tuple(int(c) for c in px[0, 0])   # (B, G, R)


def test_restatement_hand_derived_bt601_full():
    """Code 2: yy = Y * 1048576 = Y << 20, so that a grey pixel is its Y."""
    assert _one(2, 0, 128, 128) == (0, 0, 0)
    assert _one(2, 255, 128, 128) == (255, 255, 255)
    # Y below 16 is kept (limited range would clamp it to black): (7 << 20) + 524288 >> 20 = 7
    assert _one(2, 7, 128, 128) == (7, 7, 7)
    # clamped red: Y = 128, v = 127: 134217728 + 524288 + 1470104 * 127 = 321445224 >> 20 = 306 -> 255;
    #   G: 134742016 - 748826 * 127 = 39641114 >> 20 = 37;  B: u = 0: 134742016 >> 20 = 128
    assert _one(2, 128, 128, 255) == (128, 37, 255)
    # clamped blue: u = 127: 134742016 + 1858077 * 127 = 370717795 >> 20 = 353 -> 255;  G: 134742016 - 360853 * 127 = 88913685 >> 20 = 84
    assert _one(2, 128, 255, 128) == (255, 84, 128)
    # a negative sum floors: Y = 0, v = -1: R: 524288 - 1470104 = -945816 >> 20 = -1 -> 0;  G: 524288 + 748826 = 1273114 >> 20 = 1;  B: 0
    assert _one(2, 0, 128, 127) == (0, 1, 0)


def test_restatement_hand_derived_bt709_limited():
    """Code 3: yy = max(Y - 16, 0) * 1220945."""
    assert _one(3, 16, 128, 128) == (0, 0, 0)
    # white: 219 * 1220945 = 267386955; + 524288 = 267911243 >> 20 = 255 (255 << 20 = 267386880)
    assert _one(3, 235, 128, 128) == (255, 255, 255)
    assert _one(3, 7, 128, 128) == (0, 0, 0)       # Y below 16 is 16
    # clamped red: Y = 126: 110 * 1220945 + 524288 = 134828238;  R: + 1879825 * 127 = 373566013 >> 20 = 356 -> 255;
    #   G: 134828238 - 558796 * 127 = 63861146 >> 20 = 60;  B: 134828238 >> 20 = 128
    assert _one(3, 126, 128, 255) == (128, 60, 255)
    # clamped blue: B: 134828238 + 2215014 * 127 = 416135016 >> 20 = 396 -> 255;  G: 134828238 - 223607 * 127 = 106430149 >> 20 = 101
    assert _one(3, 126, 255, 128) == (255, 101, 128)
    # a negative sum floors: Y = 16, v = -1: R: 524288 - 1879825 = -1355537 >> 20 = -2 -> 0;  G: 524288 + 558796 = 1083084 >> 20 = 1;  B: 0
    assert _one(3, 16, 128, 127) == (0, 1, 0)


def test_restatement_hand_derived_bt709_full():
    """Code 4: yy = Y << 20."""
    assert _one(4, 0, 128, 128) == (0, 0, 0)
    assert _one(4, 255, 128, 128) == (255, 255, 255)
    assert _one(4, 7, 128, 128) == (7, 7, 7)       # Y below 16 is kept
    # clamped red: Y = 128, v = 127: 134742016 + 1651297 * 127 = 344456735 >> 20 = 328 -> 255;  G: 134742016 - 490864 * 127 = 72402288 >> 20 = 69
    assert _one(4, 128, 128, 255) == (128, 69, 255)
    # clamped blue: 134742016 + 1945738 * 127 = 381850742 >> 20 = 364 -> 255;  G: 134742016 - 196424 * 127 = 109796168 >> 20 = 104
    assert _one(4, 128, 255, 128) == (255, 104, 128)
    # a negative sum floors: Y = 0, u = -1: B: 524288 - 1945738 = -1421450 >> 20 = -2 -> 0;  G: 524288 + 196424 = 720712 >> 20 = 0;  R: 0
    assert _one(4, 0, 127, 128) == (0, 0, 0)
    # and v = -2 on Y = 1: R: 1048576 + 524288 - 3302594 = -1729730 >> 20 = -2 -> 0;  G: 1572864 + 981728 = 2554592 >> 20 = 2;  B: 1
    assert _one(4, 1, 128, 126) == (1, 2, 0)


def test_views_carry_the_matrix():
    a = np.zeros((3, 12, 8), np.uint8)
    b = np.zeros((3, 8, 8, 2), np.uint8)
    assert _hip.yuv_frames_view(a, 'nv12').descriptor().matrix == 0 and _hip.yuv422_frames_view(b, 'yuyv').descriptor().matrix == 0
    for (name, code) in NAMES.items():
        for m in (name, name.upper(), code):
            v = _hip.yuv_frames_view(a, 'i420', m)
            assert (v.matrix, v.descriptor().matrix, v.descriptor().format) == (code, code, _hip.YUV_I420)
            v = _hip.yuv422_frames_view(b, 'uyvy', matrix=m)
            assert (v.matrix, v.descriptor().matrix, v.descriptor().format) == (code, code, _hip.YUV422_UYVY)
    for bad in ('bt2020', 'rec709', '', 'bt601-limited', 1, 5, -1, 256, None, 2.5):
        with pytest.raises(ValueError):
            _hip.yuv_frames_view(a, 'nv12', bad)
        with pytest.raises(ValueError):
            _hip.yuv422_frames_view(b, 'yuyv', bad)


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _check_layouts(reader, p420, p422, code, tag, rng, pitched=True):
    """NV12, I420 and YUYV under matrix `code`, conventional (and pitched), host and device, against read_frames of the restated
    conversion.  Returns (records of the 4:2:0 frames, records of the 4:2:2 frames)."""
    name = [k for (k, c) in NAMES.items() if c == code][0]
    (f0, f2) = (fc.with_matrix(F420, code), fc.with_matrix(F422, code))
    want0 = reader.read_frames(f0.bgr_of(*p420))
    want2 = reader.read_frames(f2.bgr_of(*p422))
    for fmt in ('nv12', 'i420', 'yuyv'):
        (fam, planes, wb) = (f2, p422, want2.tobytes()) if fmt == 'yuyv' else (f0, p420, want0.tobytes())
        arr = packed422(*planes, fmt) if fmt == 'yuyv' else fc.conventional420(*planes, fmt, 10 if fmt == 'nv12' else 0, rng)
        assert getattr(reader, fam.read)(arr, fmt, matrix=name).tobytes() == wb, (tag, fmt, 'reader')
        v = fam.view(arr, fmt)
        assert not v.copied and v.descriptor().matrix == code
        (host, dev) = fc.read_both(fam, reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == wb, (tag, fmt, 'host')
        assert dev.tobytes() == wb, (tag, fmt, 'device')
        if pitched:
            (buf, desc) = fam.pitched(*planes, fmt, rng=rng, **fam.check_pitch(0))
            assert desc.matrix == code
            (host, dev) = fc.read_both(fam, reader, buf.ctypes.data, desc, buf.nbytes)
            assert host.tobytes() == wb, (tag, fmt, 'pitched host')
            assert dev.tobytes() == wb, (tag, fmt, 'pitched device')
    return want0, want2


@functools.lru_cache(maxsize=None)
def _triples420():
    """One 4096 x 4096 frame whose 2 x 2 blocks share chroma: block b has (U, V) = (b & 255, (b >> 8) & 255) and the four Y
    values 4 (b >> 16) .. + 3: all 2^24 triples.  (Y, U, V, index of every pixel into table())."""
    b = np.arange(2048 * 2048, dtype=np.uint32).reshape(2048, 2048)
    U = (b & 255).astype(np.uint8)[None]
    V = ((b >> 8) & 255).astype(np.uint8)[None]
    k = (b >> 16).astype(np.uint8) * 4
    Y = np.empty((1, 4096, 4096), np.uint8)
    for (j, (r, c)) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        Y[0, r::2, c::2] = k + j
    idx = (Y[0].astype(np.uint32) << 16) | np.repeat(np.repeat(b & 0xffff, 2, axis=0), 2, axis=1)
    seen = np.zeros(1 << 24, bool)
    seen[idx.ravel()] = True
    assert seen.all()
    return Y, U, V, idx


@functools.lru_cache(maxsize=None)
def _triples422():
    """One 4096 x 8192 frame: macropixel b has (U, V) = (b & 255, (b >> 8) & 255), Y0 = b >> 16 and Y1 = 255 - Y0: all 2^24
    triples at the even and at the odd pixel of a macropixel."""
    b = np.arange(4096 * 4096, dtype=np.uint32).reshape(4096, 4096)
    U = (b & 255).astype(np.uint8)[None]
    V = ((b >> 8) & 255).astype(np.uint8)[None]
    Y = np.empty((1, 4096, 8192), np.uint8)
    Y[0, :, 0::2] = (b >> 16).astype(np.uint8)
    Y[0, :, 1::2] = 255 - (b >> 16).astype(np.uint8)
    idx = (Y[0].astype(np.uint32) << 16) | np.repeat(b & 0xffff, 2, axis=1)
    for par in (0, 1):
        seen = np.zeros(1 << 24, bool)
        seen[idx[:, par::2].ravel()] = True
        assert seen.all()
    return Y, U, V, idx


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', ('nv12', 'i420'))
@pytest.mark.parametrize('code', NEW)
def test_yuv_to_bgr_all_triples(env, code, fmt):
    """melf_yuv_to_bgr == the restatement for all 2^24 (Y, U, V) under each new matrix."""
    ctx = env['sample-images1']['reader'].ctx
    (Y, U, V, idx) = _triples420()
    v = _hip.yuv_frames_view(fc.conventional420(Y, U, V, fmt), fmt, code)
    got = ctx.yuv_to_bgr(v.ptr, v.descriptor())
    want = table(code)[idx]
    if code == NEW[0] and fmt == 'nv12':   # the table is the restatement of the frame (once: the gather is the cheaper form)
        assert np.array_equal(want[:64], yuv420_to_bgr(Y[0, :64], U[0, :32], V[0, :32], code))
    bad = np.flatnonzero((got[0] != want).any(axis=-1).ravel())
    assert bad.size == 0, (code, fmt, bad.size, bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', ('yuyv', 'uyvy', 'yvyu'))
@pytest.mark.parametrize('code', NEW)
def test_yuv422_to_bgr_all_triples(env, code, fmt):
    """melf_yuv422_to_bgr == the restatement for all 2^24 (Y, U, V) under each new matrix, at the even and at the odd pixel of a
    macropixel, in each byte order."""
    ctx = env['sample-images1']['reader'].ctx
    (Y, U, V, idx) = _triples422()
    v = _hip.yuv422_frames_view(packed422(Y, U, V, fmt), fmt, code)
    assert not v.copied
    got = ctx.yuv422_to_bgr(v.ptr, v.descriptor())
    want = table(code)[idx]
    if code == NEW[0] and fmt == 'yuyv':
        assert np.array_equal(want[:64], yuv422_to_bgr(Y[0, :64], U[0, :64], V[0, :64], code))
    bad = np.flatnonzero((got[0] != want).any(axis=-1).ravel())
    assert bad.size == 0, (code, fmt, bad.size, bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize('sd,count', [('sample-images1', 81), ('sample-images2', 223)])
@pytest.mark.parametrize('code', NEW)
def test_fixture_frames(env, code, sd, count):
    """The fixture frames, forward-converted with the matrix, read under it: records byte-identical to read_frames of the restated
    conversion, and at least three quarters of the set read OK on that BGR side (BT.601 limited: 79 of 81, 222 / 223 of 223)."""
    e = env[sd]
    assert len(e['frames']) == count
    rng = np.random.default_rng(count + code)
    shapes = {}
    for fr in e['frames']:
        shapes.setdefault(fr.shape, []).append(fr)
    (ok0, ok2) = (0, 0)
    for (shape, group) in shapes.items():
        (p420, p422) = forward_both(np.stack(group), code)
        (w0, w2) = _check_layouts(e['reader'], p420, p422, code, '%s %s' % (sd, shape), rng)
        ok0 += int((w0['status'] == _hip.FRAME_OK).sum())
        ok2 += int((w2['status'] == _hip.FRAME_OK).sum())
    print('matrix %d %s: %d (4:2:0) and %d (4:2:2) of %d frames read OK on the BGR side' % (code, sd, ok0, ok2, count))
    assert 4 * ok0 >= 3 * count and 4 * ok2 >= 3 * count, (ok0, ok2, count)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')])
@pytest.mark.parametrize('code', NEW)
def test_each_match_kernel(env, monkeypatch, code, kind, kernel):  # noqa: F811
    """256 frames (the tuned matrix-core kernel's batch) with each match kernel forced: the prep kernels and the dot4 matcher
    convert under the matrix."""
    (f0, f2) = (fc.with_matrix(F420, code), fc.with_matrix(F422, code))
    groups = [(f0, ('nv12', 'i420'), fc.as_conventional(f0, lambda fmt: 0)), (f2, ('yuyv',), fc.as_conventional(f2, lambda fmt: 0))]
    fc.each_match_kernel(env['sample-images1'], monkeypatch, kind, kernel, groups, n=256, seed=5, rng_seed=0, min_not_found=28,
                         min_ok=128)


@pytest.mark.gpu
def test_the_matrix_reaches_the_kernels(env):
    """The same NV12 and YUYV bytes read under the four matrices: each equals the BGR path of its own conversion, and any two
    matrices give different records on at least one fixture frame."""
    e = env['sample-images1']
    reader = e['reader']
    shapes = [f.shape for f in e['frames']]
    group = np.stack([f for f in e['frames'] if f.shape == max(set(shapes), key=shapes.count)])
    (p420, p422) = forward_both(group, 0)
    nv12 = fc.conventional420(*p420, 'nv12')
    yuyv = packed422(*p422, 'yuyv')
    for (arr, planes, conv, read) in ((nv12, p420, yuv420_to_bgr, reader.read_yuv_frames), (yuyv, p422, yuv422_to_bgr, reader.read_yuv422_frames)):
        recs = {}
        for (name, code) in NAMES.items():
            recs[code] = read(arr, matrix=name).tobytes()
            assert recs[code] == reader.read_frames(conv(*planes, code)).tobytes(), name
        assert len(set(recs.values())) == len(recs)


@pytest.mark.gpu
def test_odd_origin_and_frame_edges(env, tmp_path):
    """Under BT.709 limited: meter_rect (50, 160)-(300, 410) moved to an odd x0 and y0 (the frames shifted by as much), and
    reaching the right and bottom edge of 300 x 410 frames (the host staging path rounds the crop to whole chroma samples)."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    src = fc.synth(e['frames'], 40, 3)
    rng = np.random.default_rng(13)
    r = MeterReader(fc.params_with_rect(tmp_path, 'sample-images1', (53, 165, 304, 416), 'odd'))
    try:
        (p420, p422) = forward_both(np.roll(src, (5, 3), axis=(1, 2)), 3)
        (w0, w2) = _check_layouts(r, p420, p422, 3, 'odd origin', rng)
        assert (w0['status'] == _hip.FRAME_OK).sum() > 20 and (w2['status'] == _hip.FRAME_OK).sum() > 20
    finally:
        r.close()
    (p420, p422) = forward_both(np.ascontiguousarray(src[:12, :410, :300]), 3)
    (w0, w2) = _check_layouts(e['reader'], p420, p422, 3, 'edges', rng)
    assert (w0['status'] == _hip.FRAME_OK).sum() >= 6 and (w2['status'] == _hip.FRAME_OK).sum() >= 6


@pytest.mark.gpu
def test_resident_lanes_two_streams_changing_matrix(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1), two caller streams, a different matrix (and family) on consecutive calls of one context:
    every call's records equal a synchronous read of its own conversion."""
    from meterelf_amd import MeterReader
    e = env['sample-images2']
    src = fc.synth(e['frames'], 96, 21)
    planes = {code: forward_both(src, code) for code in (0, 2, 3, 4)}   # every call's frames are encoded with its own matrix
    r = MeterReader(e['params'])
    (bufs, keep, calls) = ([], [], [])
    try:
        for (k, (fmt, code)) in enumerate((('nv12', 2), ('yuyv', 3), ('i420', 4), ('nv12', 0), ('uyvy', 2), ('nv12', 3))):
            (p420, p422) = planes[code]
            if fmt in ('nv12', 'i420'):
                (buf, desc) = fc.pitched420(*p420, fmt, y_pad=4 * k, c_pad=2 * k, gap=k, stride_pad=k, rng=np.random.default_rng(k), matrix=code)
                want = r.read_frames(yuv420_to_bgr(*p420, code))
                fn = r.ctx.process_yuv_dev
            else:
                (buf, desc) = fc.pitched422(*p422, fmt, row_pad=4 * k, stride_pad=8 * k, rng=np.random.default_rng(k), matrix=code)
                want = r.read_frames(yuv422_to_bgr(*p422, code))
                fn = r.ctx.process_yuv422_dev
            assert (want['status'] == _hip.FRAME_OK).sum() > 48
            keep.append(buf)
            bufs.append(DevBuf(buf.ctypes.data, buf.nbytes))
            calls.append((functools.partial(fn, bufs[-1].d.value, desc), want.tobytes()))
        fc.resident_calls(r, len(src), calls, 2 * len(calls), lambda i: i % len(calls))
    finally:
        r.close()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_rejected_matrix_codes_launch_nothing(env):
    """Codes 1, 5, -1 and 256 on either descriptor, through every entry point: MELF_ERR_INVALID and no kernel launched."""
    e = env['sample-images1']
    ctx = e['reader'].ctx
    L = _hip.lib()
    (p420, p422) = forward_both(np.stack(e['frames'][2:6]), 3)
    (n, H, W) = p420[0].shape
    a0 = fc.conventional420(*p420, 'nv12')
    a2 = packed422(*p422, 'yuyv')
    (b0, b2) = (DevBuf(a0.ctypes.data, a0.nbytes), DevBuf(a2.ctypes.data, a2.nbytes))
    try:
        ctx.set_profiling(1)
        before = fc.launch_counts(ctx)
        out = np.zeros(n, _hip.RESULT_DTYPE)
        bgr_out = np.zeros((n, H, W, 3), np.uint8)
        for code in (1, 5, -1, 256):
            f = _hip.MelfYuvFrames(_hip.YUV_NV12, code, n, H, W, 0, W, W, H * W, H * W + 1, H * W * 3 // 2)
            g = _hip.MelfYuv422Frames(_hip.YUV422_YUYV, code, n, H, W, 0, 2 * W, 2 * H * W)
            for rc in (L.melf_process_yuv_dev(ctx._h, C.c_void_p(b0.d.value), C.byref(f), None, _hip._ptr(out), None),
                       L.melf_process_yuv(ctx._h, C.c_void_p(a0.ctypes.data), C.byref(f), _hip._ptr(out)),
                       L.melf_yuv_to_bgr(ctx._h, C.c_void_p(a0.ctypes.data), C.byref(f), _hip._ptr(bgr_out)),
                       L.melf_process_yuv422_dev(ctx._h, C.c_void_p(b2.d.value), C.byref(g), None, _hip._ptr(out), None),
                       L.melf_process_yuv422(ctx._h, C.c_void_p(a2.ctypes.data), C.byref(g), _hip._ptr(out)),
                       L.melf_yuv422_to_bgr(ctx._h, C.c_void_p(a2.ctypes.data), C.byref(g), _hip._ptr(bgr_out))):
                assert rc == -1, code
                msg = L.melf_last_error().decode()
                assert 'matrix' in msg and all(s in msg for s in ('0', '2', '3', '4')), msg
        assert fc.launch_counts(ctx) == before
        assert not out.tobytes().strip(b'\0') and not bgr_out.any()
        # every accepted code runs
        for code in (0, 2, 3, 4):
            f = _hip.MelfYuvFrames(_hip.YUV_NV12, code, n, H, W, 0, W, W, H * W, H * W + 1, H * W * 3 // 2)
            assert L.melf_process_yuv_dev(ctx._h, C.c_void_p(b0.d.value), C.byref(f), None, _hip._ptr(out), None) == 0
            assert out.tobytes() == e['reader'].read_frames(yuv420_to_bgr(*p420, code)).tobytes()
        assert fc.launch_counts(ctx) != before
    finally:
        ctx.set_profiling(0)
        b0.free()
        b2.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_yuv_frames / read_yuv422_frames with matrix= on torch device tensors and out=, in a child process that imports torch
    first (tests/frame_cases.py says why)."""
    fc.run_torch_child('yuv_matrix')
