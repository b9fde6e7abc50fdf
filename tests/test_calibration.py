"""Calibration path (reference meterelf/_calibration.py).

CPU: the oracle restatement against the reference's own golden (tests/test_meterelf.py:118-144,
EXPECTED_CENTER_DATA) and the product's host geometry (contours, ellipse fit) against the oracle.
GPU: the product's find_dial_centers against the same golden and the oracle."""
import glob
import os

import numpy as np
import pytest

from oracle import calibration as ocal
from oracle import pyoracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EXPECTED_CENTER_DATA = [(37.4, 63.5, 14), (94.5, 86.3, 15), (135.6, 71.5, 13), (161.0, 36.5, 13)]
BAD = ('20180814021309-01-e01.jpg', '20180814021310-00-e02.jpg')


def _files():
    return [f for f in sorted(glob.glob(os.path.join(GOLDEN, 'sample-images1', '*.jpg')))
            if os.path.basename(f) not in BAD]


def _check_against_golden(result):
    assert len(result) == 4
    for ((center, diameter), (ex, ey, ed)) in zip(result, EXPECTED_CENTER_DATA):
        assert diameter == ed
        assert abs(center[0] - ex) < 0.05 and abs(center[1] - ey) < 0.05
    assert list(result) == sorted(result, key=lambda r: r[0][0])


def test_oracle_calibration_matches_reference_golden():
    params = po.Params(os.path.join(GOLDEN, 'sample-images1', 'params.yml'))
    _check_against_golden(ocal.find_dial_centers(params, _files()))


def test_host_contours_and_ellipse_match_oracle():
    from meterelf_amd import _calibration as cal
    rng = np.random.default_rng(12)
    checked = 0
    for k in range(60):
        img = np.zeros((30, 40), np.uint8)
        for _ in range(int(rng.integers(1, 5))):  # blobs, rings, thin lines
            (cx, cy, r) = (rng.integers(5, 35), rng.integers(5, 25), rng.integers(1, 7))
            (yy, xx) = np.ogrid[:30, :40]
            d2 = (xx - cx) ** 2 + (yy - cy) ** 2
            img[(d2 <= r * r) & ((k % 3 != 0) | (d2 >= (r - 2) ** 2))] = 255
        if k % 4 == 0:
            img[int(rng.integers(2, 28)), 3:30] = 255
        img[rng.random(img.shape) < 0.03] = 0
        got = cal.find_external_contours(img)
        exp = ocal.external_contours(img)
        assert len(got) == len(exp)
        for (g, e) in zip(got, exp):
            assert np.array_equal(g, e)
            if len(e) >= 12:
                (gc, gs, _ga) = cal.fit_ellipse(g)
                (ec, es, _ea) = ocal.fit_ellipse(e)
                if np.all(np.isfinite(es)) and min(es) > 1:
                    assert np.allclose(gc, ec, atol=1e-4) and np.allclose(gs, es, atol=1e-4)
                    checked += 1
    assert checked > 20


@pytest.mark.gpu
def test_gpu_find_dial_centers():
    from meterelf_amd import _calibration as cal
    from meterelf_amd import _params
    pfile = os.path.join(GOLDEN, 'sample-images1', 'params.yml')
    params = _params.load(pfile)
    files = _files()
    avg = cal.get_average_meter_image(params, files)
    oparams = po.Params(pfile)
    crops = (ocal.aligned_crop(po.crop_meter(po.decode_bgr(f), oparams), oparams) for f in files)
    assert np.array_equal(avg, ocal.average_image(crops))  # float64 running mean, bit-exact
    result = cal.find_dial_centers(params, files)
    _check_against_golden([(c.center, c.diameter) for c in result])
    oracle = ocal.find_dial_centers(oparams, files)
    for (c, o) in zip(result, oracle):
        assert c.diameter == o[1] and np.allclose(c.center, o[0], atol=1e-4)
    # get_image_filenames: the glob minus the two unreadable frames (meterelf/_calibration.py:72-79)
    assert sorted(cal.get_image_filenames(params)) == files


# ------------------------------------------------ the two calibration kernels, directed ----

@pytest.fixture(scope='module')
def gpu_ctx():
    from meterelf_amd import MeterReader, _hip, _params
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    reader = MeterReader(_params.load(os.path.join(GOLDEN, 'sample-images1', 'params.yml')))
    yield reader.ctx
    reader.close()


def _expected_average(frames, mx, my, ax, ay, oparams):
    crops = [ocal.translate(po.crop_meter(f, oparams), ax - int(x), ay - int(y)) for (f, x, y) in zip(frames, mx, my)]
    return ocal.average_image(iter(crops))


# meter_rect of sample-images1 is (50, 160) .. (300, 410): a 250 x 250 crop
@pytest.mark.gpu
@pytest.mark.parametrize('n,kind', [(1, 'still'), (1, 'out'), (2, 'half'), (2, 'half-shifted'), (3, 'shifts'), (7, 'shifts'),
                                    (7, 'some-out'), (64, 'shifts'), (64, 'all-out')])
def test_aligned_average_directed(gpu_ctx, n, kind):
    """k_aligned_average against oracle.calibration.translate + average_image, bit-exact: the float64 running mean in the
    reference's operation order, (p * 255 + 0.5) truncated.  'half': two frames whose pixel sums are all odd, so every mean
    sits exactly on .5, where the last bit of the float64 operations decides (a fused multiply-add or a reordered mean would show);
    'shifts': match positions that move the crop left, right, up and down; 'out': moved out of the crop entirely (the
    zero border is all that is left)."""
    oparams = po.Params(os.path.join(GOLDEN, 'sample-images1', 'params.yml'))
    rng = np.random.default_rng(n * 31 + len(kind))
    (H, W) = (413, 304)
    (ax, ay) = (ocal.ALIGN_X, ocal.ALIGN_Y)
    frames = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    (mx, my) = (np.full(n, ax, np.int32), np.full(n, ay, np.int32))
    if kind.startswith('half'):
        frames[1] = frames[0] ^ 1                      # a + (a ^ 1) is odd for every byte
        if kind == 'half-shifted':
            (mx[:], my[:]) = (ax - 9, ay + 4)           # both by the same amount: the overlap still pairs a with a ^ 1
    elif kind in ('shifts', 'some-out'):
        moves = [(-17, 0), (23, 0), (0, -30), (0, 41), (-5, 7), (249, -249), (0, 0)]
        for i in range(n):
            (mx[i], my[i]) = (ax + moves[i % 7][0], ay + moves[i % 7][1])
        if kind == 'some-out':
            (mx[1], my[1]) = (ax + 250, ay)             # exactly one crop width: nothing left
            (mx[4], my[4]) = (ax, ay - 1000)
    elif kind in ('out', 'all-out'):
        for i in range(n):
            (mx[i], my[i]) = [(ax + 250, ay), (ax - 250, ay), (ax, ay + 250), (ax - 3000, ay + 3000)][i % 4]
    got = gpu_ctx.aligned_average(frames, mx, my, ax, ay)
    exp = _expected_average(frames, mx, my, ax, ay, oparams)
    assert got.shape == (250, 250, 3)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:5]
    if kind in ('out', 'all-out'):
        assert not got.any()
    else:
        assert got.any()
    if kind == 'half':
        s = frames[0, 160:410, 50:300].astype(np.int64) + frames[1, 160:410, 50:300]
        # every exact mean is k + .5; the float64 operations land just below or just above it, so both roundings occur and
        # only the reference's operation order gives the reference's bytes
        assert (s % 2 == 1).all()
        (up, down) = (int((exp == (s + 1) // 2).sum()), int((exp == s // 2).sum()))
        assert up + down == s.size and up > 1000 and down > 1000, (up, down)


@pytest.mark.gpu
def test_aligned_average_padded_frame_stride(gpu_ctx):
    """frame_stride larger than a frame (through the C entry; the Python wrapper passes packed frames)."""
    from meterelf_amd import _hip
    oparams = po.Params(os.path.join(GOLDEN, 'sample-images1', 'params.yml'))
    rng = np.random.default_rng(77)
    (n, H, W, pad) = (5, 413, 304, 1000 + 7)
    (ax, ay) = (ocal.ALIGN_X, ocal.ALIGN_Y)
    buf = rng.integers(0, 256, size=(n, H * W * 3 + pad), dtype=np.uint8)
    frames = np.ascontiguousarray(buf[:, :H * W * 3]).reshape(n, H, W, 3)
    mx = (ax + np.array([0, -12, 30, 3, -250])).astype(np.int32)
    my = (ay + np.array([0, 8, -2, 120, 0])).astype(np.int32)
    got = np.empty((250, 250, 3), np.uint8)
    _hip.check(gpu_ctx._L.melf_aligned_average(gpu_ctx._h, _hip._ptr(buf), n, H, W, H * W * 3 + pad, _hip._ptr(mx), _hip._ptr(my),
                                               ax, ay, _hip._ptr(got)))
    assert np.array_equal(got, _expected_average(frames, mx, my, ax, ay, oparams))
    assert np.array_equal(got, gpu_ctx.aligned_average(frames, mx, my, ax, ay))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(1, 1), (250, 250), (7, 37), (3, 257), (1, 255)])
def test_inrange_directed(gpu_ctx, shape):
    """k_inrange3 against numpy's statement of cv2.inRange, bit-exact: lo == hi, lo > hi (empty), 0 .. 255 (full), mixed
    bounds; a 1 x 1 image and sizes that are not a multiple of the 256-thread block."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    img[0, 0] = (7, 200, 31)
    img[-1, -1] = (7, 200, 31)
    cases = [((7, 200, 31), (7, 200, 31)), ((8, 0, 0), (7, 255, 255)), ((0, 0, 0), (255, 255, 255)), ((0, 100, 30), (127, 100, 255)),
             ((0, 0, 255), (255, 255, 255)), ((40, 60, 80), (200, 180, 160)), ((0, 0, 0), (0, 0, 0)), ((255, 255, 255), (255, 255, 255))]
    for (lo, hi) in cases:
        got = gpu_ctx.inrange(img, lo, hi)
        exp = (np.all((img >= np.array(lo)) & (img <= np.array(hi)), axis=-1) * 255).astype(np.uint8)
        assert got.dtype == np.uint8 and np.array_equal(got, exp), (lo, hi)
    assert gpu_ctx.inrange(img, (7, 200, 31), (7, 200, 31))[0, 0] == 255 and not gpu_ctx.inrange(img, (8, 0, 0), (7, 255, 255)).any()
    assert (gpu_ctx.inrange(img, (0, 0, 0), (255, 255, 255)) == 255).all()
