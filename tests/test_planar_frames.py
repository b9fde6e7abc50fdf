"""Planar, channels-first frames -- (N, 3, H, W) / (N, 4, H, W) uint8: torch's decoders and pre-processing pipelines, ffmpeg's
gbrp, rgb24 split into planes -- read in place (melf_process_planes, melf_process_planes_dev, _hip.planar_frames_view,
MeterReader.read_planar_frames).

The contract: the records of a planar frame are byte-identical to read_frames() of the packed BGR frame whose pixel (x, y) is
(B[y][x], G[y][x], R[y][x]).  No colour conversion is involved, so the same records are also held against the CPU oracle on that
BGR frame, under the rules of tests/test_gpu_parity.py (_compare_records: status, match position, float32 match value bit-exact,
positions and angles to 1e-9, the digits).

CPU tests: the descriptor against the header, planar_frames_view's mapping of numpy arrays and torch CPU tensors, the exported
symbols, the new kernels' code-object notes.  GPU tests: the fixtures as RGB, BGR and GBR planes, every match kernel, plane
offsets and pitches that put the three planes at every byte phase relative to each other and to the base, meter_rect at every
parity and at the frame's edges, 4-plane tensors, batch sizes, random bytes, 1080p with six dials, resident lanes on two caller
streams, rejected descriptors, torch tensors (in a child process that imports torch first: tests/test_pixel_formats.py says why).
Every device buffer has exactly the descriptor's extent and ends where its allocation ends.
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

ORDERS3 = ('rgb', 'bgr', 'gbr')
POS_TOL = 1e-9   # tests/test_gpu_parity.py


def to_planes(bgr, order, rng=None):
    """(n, H, W, 3) BGR -> the (n, C, H, W) array whose planes are in `order`; a 4th plane ('a' / 'x') is random."""
    rng = rng if rng is not None else np.random.default_rng(0)
    (n, H, W, _c) = bgr.shape
    out = rng.integers(0, 256, size=(n, len(order), H, W), dtype=np.uint8)
    for (k, ch) in enumerate(order):
        if ch in 'bgr':
            out[:, k] = bgr[..., 'bgr'.index(ch)]
    return out


def pitched(bgr, order='rgb', row_pad=0, gaps=(0, 0, 0), stride_pad=0, rng=None):
    """A byte buffer of exactly the descriptor's extent: the three planes in `order`, rows row_pad bytes longer than W, gaps[k]
    bytes in front of plane k (gaps[0]: from the frame's first byte), stride_pad bytes behind a frame's last sample; random
    filling.  Returns (buffer, MelfPlanarFrames)."""
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


def _desc_extent(d):
    return (d.n - 1) * d.frame_stride + max(d.b_offset, d.g_offset, d.r_offset) + (d.H - 1) * d.row_pitch + d.W


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_planar_struct_matches_header(tmp_path):
    fields = ('n', 'H', 'W', 'reserved', 'b_offset', 'g_offset', 'r_offset', 'row_pitch', 'frame_stride')
    src = tmp_path / 'planar.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(melf_planar_frames));\n'
                   + ''.join('printf(" %%zu", offsetof(melf_planar_frames, %s));\n' % f for f in fields)
                   + 'printf(" %d\\n", MELF_ABI_VERSION);return 0;}\n')
    exe = tmp_path / 'planar'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfPlanarFrames
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in fields] + [3]   # the ABI version stays
    assert C.sizeof(F) == 56
    assert _hip.ABI_VERSION == 3


def test_planar_symbols_exported():
    for name in ('melf_process_planes', 'melf_process_planes_dev'):
        assert name in _hip.EXPORTS
        assert hasattr(_hip.lib(), name), name
    with open(os.path.join(ROOT, 'include', 'meterelf_hip.h')) as fp:
        header = fp.read()
    assert 'int melf_process_planes(' in header and 'int melf_process_planes_dev(' in header


def test_pitched_helper_places_the_samples():
    """The test's own buffer builder: offsets, pitch, stride and extent worked out by hand."""
    bgr = np.arange(2 * 3 * 5 * 3, dtype=np.uint8).reshape(2, 3, 5, 3)
    (buf, d) = pitched(bgr, 'gbr', row_pad=2, gaps=(1, 3, 0), stride_pad=4)
    # pitch 7, span 2 * 7 + 5 = 19; g at 1, b at 1 + 19 + 3 = 23, r at 23 + 19 = 42; stride 42 + 19 + 4 = 65
    assert (d.row_pitch, d.g_offset, d.b_offset, d.r_offset, d.frame_stride) == (7, 1, 23, 42, 65)
    assert buf.size == 65 + 42 + 19 == _desc_extent(d)
    assert buf[65 + 23 + 7 * 2 + 4] == bgr[1, 2, 4, 0] and buf[1 + 7 + 3] == bgr[0, 1, 3, 1] and buf[42] == bgr[0, 0, 0, 2]
    t = to_planes(bgr, 'bgrx')
    assert t.shape == (2, 4, 3, 5) and np.array_equal(t[:, 0], bgr[..., 0]) and np.array_equal(t[:, 2], bgr[..., 2])


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_planar_frames_view_layouts(kind):
    if kind == 'torch':
        torch = pytest.importorskip('torch')

        def z(shape, dtype=np.uint8):
            return torch.zeros(shape, dtype=torch.uint8 if dtype == np.uint8 else torch.int16)
    else:
        def z(shape, dtype=np.uint8):
            return np.zeros(shape, dtype)

    def addr(a):
        return a.ctypes.data if kind == 'numpy' else a.data_ptr()

    def fields(v):
        return (v.n, v.H, v.W, v.b_offset, v.g_offset, v.r_offset, v.row_pitch, v.frame_stride, v.extent, v.copied, v.ptr)
    (n, H, W) = (5, 7, 13)
    P = H * W
    a = z((n, 3, H, W))
    # contiguous NCHW, every 3-plane order: the offsets say which plane is which
    for (order, (b, g, r)) in (('rgb', (2, 1, 0)), ('bgr', (0, 1, 2)), ('gbr', (1, 0, 2)), ('RGB', (2, 1, 0))):
        v = _hip.planar_frames_view(a, order)
        assert fields(v) == (n, H, W, b * P, g * P, r * P, W, 3 * P, n * 3 * P, False, addr(a)), order
        assert (v.on_device, v.device) == (False, None)
    assert _hip.planar_frames_view(a).r_offset == 0   # the default is 'rgb'
    d = _hip.planar_frames_view(a, 'gbr').descriptor()
    assert (d.n, d.H, d.W, d.reserved, d.b_offset, d.g_offset, d.r_offset, d.row_pitch, d.frame_stride) == (n, H, W, 0, P, 0, 2 * P, W, 3 * P)
    # 4-plane tensors: three planes named, the extent stops at the last named sample
    a4 = z((n, 4, H, W))
    for (order, (b, g, r)) in (('rgba', (2, 1, 0)), ('rgbx', (2, 1, 0)), ('bgra', (0, 1, 2)), ('bgrx', (0, 1, 2))):
        v = _hip.planar_frames_view(a4, order)
        assert fields(v) == (n, H, W, b * P, g * P, r * P, W, 4 * P, (n - 1) * 4 * P + 3 * P, False, addr(a4)), order
    # x[:, :3] of a 4-plane tensor, and its last three planes
    v = _hip.planar_frames_view(a4[:, :3], 'rgb')
    assert fields(v) == (n, H, W, 2 * P, P, 0, W, 4 * P, (n - 1) * 4 * P + 3 * P, False, addr(a4))
    v = _hip.planar_frames_view(a4[:, 1:], 'bgr')
    assert fields(v) == (n, H, W, 0, P, 2 * P, W, 4 * P, (n - 1) * 4 * P + 3 * P, False, addr(a4) + P)
    # crops: the row stride and the plane stride stay, the extent stops at the last sample of the last row
    v = _hip.planar_frames_view(a[..., :4, :9], 'rgb')
    assert fields(v) == (n, 4, 9, 2 * P, P, 0, W, 3 * P, (n - 1) * 3 * P + 2 * P + 3 * W + 9, False, addr(a))
    v = _hip.planar_frames_view(a[..., 2:, 3:], 'bgr')   # any origin: planes are bytes
    assert fields(v) == (n, H - 2, W - 3, 0, P, 2 * P, W, 3 * P, (n - 1) * 3 * P + 2 * P + (H - 3) * W + W - 3, False, addr(a) + 2 * W + 3)
    # every other frame, a frame range, one frame, no frame
    v = _hip.planar_frames_view(a[::2], 'rgb')
    assert fields(v) == (3, H, W, 2 * P, P, 0, W, 6 * P, 2 * 6 * P + 3 * P, False, addr(a))
    v = _hip.planar_frames_view(a[1:4], 'rgb')
    assert fields(v) == (3, H, W, 2 * P, P, 0, W, 3 * P, 9 * P, False, addr(a) + 3 * P)
    v = _hip.planar_frames_view(a[2:3, :, :, :9], 'rgb')   # n == 1: the frame stride is a packed array's
    assert fields(v) == (1, H, 9, 2 * P, P, 0, W, 2 * P + (H - 1) * W + 9, 2 * P + (H - 1) * W + 9, False, addr(a) + 6 * P)
    v = _hip.planar_frames_view(a[:0], 'rgb')
    assert (v.n, v.extent, v.copied) == (0, 0, False)
    # size-1 dimensions: H == 1 and W == 1 get a packed array's strides
    v = _hip.planar_frames_view(a[:, :, 3:4, :], 'bgr')
    assert fields(v) == (n, 1, W, 0, P, 2 * P, W, 3 * P, (n - 1) * 3 * P + 2 * P + W, False, addr(a) + 3 * W)
    v = _hip.planar_frames_view(a[:, :, :, 5:6], 'bgr')
    assert fields(v) == (n, H, 1, 0, P, 2 * P, W, 3 * P, (n - 1) * 3 * P + 2 * P + (H - 1) * W + 1, False, addr(a) + 5)

    def copied(view, order='rgb'):
        v = _hip.planar_frames_view(view, order)
        (n_, H_, W_) = (v.n, v.H, v.W)
        (b, g, r) = (order.index('b'), order.index('g'), order.index('r'))
        assert v.copied and v.ptr == addr(v.array) and tuple(v.array.shape) == (n_, 3, H_, W_), (tuple(view.shape), order)
        assert (v.b_offset, v.g_offset, v.r_offset, v.row_pitch, v.frame_stride, v.extent) == \
               (b * H_ * W_, g * H_ * W_, r * H_ * W_, W_, 3 * H_ * W_, n_ * 3 * H_ * W_)
        return v
    # copied once: a W stride other than 1 (a permuted NHWC tensor; every other column)
    nhwc = z((n, H, W, 3))
    chw = nhwc.permute(0, 3, 1, 2) if kind == 'torch' else nhwc.transpose(0, 3, 1, 2)
    v = copied(chw)
    assert v.ptr != addr(nhwc)
    copied(a[..., ::2], 'bgr')
    # copied: overlapping planes (a plane stride of zero, or smaller than a plane)
    one = z((n, 1, H, W))
    copied(one.expand(n, 3, H, W) if kind == 'torch' else np.broadcast_to(one, (n, 3, H, W)))
    # copied: a 4-plane tensor goes to three planes
    nhwc4 = z((n, H, W, 4))
    v = copied(nhwc4.permute(0, 3, 1, 2) if kind == 'torch' else nhwc4.transpose(0, 3, 1, 2), 'bgra')
    if kind == 'numpy':
        # negative strides: frames, planes, rows, columns
        copied(a[::-1])
        copied(a[:, ::-1])
        copied(a[:, :, ::-1])
        copied(a[..., ::-1])
        # frames that overlap (a frame stride smaller than a frame's planes)
        flat = np.zeros(8 * P, np.uint8)
        copied(np.lib.stride_tricks.as_strided(flat, shape=(3, 3, H, W), strides=(2 * P, P, W, 1)))
        # the copy holds the caller's samples, plane by plane in the caller's order
        src = np.arange(n * H * W * 4, dtype=np.uint32).astype(np.uint8).reshape(n, H, W, 4)
        v = _hip.planar_frames_view(src.transpose(0, 3, 1, 2), 'rgbx')
        assert v.copied and np.array_equal(np.asarray(v.array), src.transpose(0, 3, 1, 2)[:, :3])
    # rejected: dtype, rank, plane count, empty planes, names that do not fit
    with pytest.raises(ValueError):
        _hip.planar_frames_view(z((n, 3, H, W), np.int16), 'rgb')
    with pytest.raises(ValueError):
        _hip.planar_frames_view(z((3, H, W)), 'rgb')
    with pytest.raises(ValueError):
        _hip.planar_frames_view(z((1, n, 3, H, W)), 'rgb')
    for c in (1, 2, 5):
        with pytest.raises(ValueError):
            _hip.planar_frames_view(z((n, c, H, W)), 'rgb')
    with pytest.raises(ValueError):
        _hip.planar_frames_view(z((n, 3, 0, W)), 'rgb')
    with pytest.raises(ValueError):
        _hip.planar_frames_view(z((n, 3, H, 0)), 'rgb')
    for bad in ('rgba', 'bgrx', 'grb', 'yuv', 'nv12', ''):
        with pytest.raises(ValueError):
            _hip.planar_frames_view(a, bad)
    for bad in ('rgb', 'bgr', 'gbr', 'argb'):
        with pytest.raises(ValueError):
            _hip.planar_frames_view(a4, bad)
    # frames_view keeps copying channel-strided views (its contract is unchanged)
    assert _hip.frames_view(a.permute(0, 2, 3, 1) if kind == 'torch' else a.transpose(0, 2, 3, 1), 'rgb').copied


def test_planar_kernels_metadata():
    """The kernels that read planar frames are in the library (one prep kernel, one dot4 matcher, a dial reader per NR), without a
    private segment or spilled VGPRs; the dial readers within k_dials' register count."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    names = ('k_planar_lplane', 'k_planar_match', 'k_planar_needle')
    new = {k: d for (k, d) in meta.items() if any(s in k for s in names)}
    assert [sum(s in k for k in new) for s in names] == [1, 1, 6]
    dials_vgpr = max(d['vgpr_count'] for (k, d) in meta.items() if 'k_dials' in k)
    for (k, d) in new.items():
        assert d.get('private_segment_fixed_size', 0) == 0 and d.get('vgpr_spill_count', 0) == 0, (k, d)
        if 'k_planar_needle' in k:
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
        pfile = os.path.join(GOLDEN, sd, 'params.yml')
        params = _params.load(pfile)
        frames = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(GOLDEN, sd, '*.jpg')))]
        out[sd] = dict(pfile=pfile, params=params, frames=frames, reader=MeterReader(params))
    yield out
    for e in out.values():
        e['reader'].close()


def _hip_rt():
    from tests.helpers import hip_runtime
    return hip_runtime()


class DevBuf:
    """Device copy of `nbytes` bytes at host address `ptr`: exactly that many bytes, ending where the allocation (a whole number
    of 4 KiB pages) ends.  phase 0..3: the copy's address has that residue modulo 4 instead, as close to the allocation's end as
    that allows (at most 3 bytes of it left behind the copy)."""

    def __init__(self, ptr, nbytes, phase=None):
        self.hip = _hip_rt()
        self.base = C.c_void_p()
        alloc = (nbytes + 3 + 4095) // 4096 * 4096
        assert self.hip.hipMalloc(C.byref(self.base), C.c_size_t(alloc)) == 0
        at = alloc - nbytes
        if phase is not None:
            at -= (self.base.value + at - phase) % 4
        assert at >= 0
        self.d = C.c_void_p(self.base.value + at)
        assert self.hip.hipMemcpy(self.d, C.c_void_p(ptr), C.c_size_t(nbytes), 1) == 0

    def free(self):
        self.hip.hipFree(self.base)


def _read_both(reader, ptr, desc, extent, phase=None):
    """Records of the host path and of the device path (a device buffer of exactly `extent` bytes)."""
    assert extent == _desc_extent(desc)
    host = reader.ctx.process_planes(ptr, desc)
    buf = DevBuf(ptr, extent, phase)
    try:
        dev = reader.ctx.process_planes_dev(buf.d.value, desc)
    finally:
        buf.free()
    return host, dev


def _check_orders(reader, bgr, tag, rng, orders=ORDERS3, want=None):
    """Every order, as an (N, C, H, W) array and as a pitched buffer with odd gaps, host and device, against read_frames."""
    if want is None:
        want = reader.read_frames(bgr)
    wb = want.tobytes()
    for (k, order) in enumerate(orders):
        arr = to_planes(bgr, order, rng)
        assert reader.read_planar_frames(arr, order).tobytes() == wb, (tag, order, 'reader')
        v = _hip.planar_frames_view(arr, order)
        assert not v.copied
        (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == wb, (tag, order, 'host')
        assert dev.tobytes() == wb, (tag, order, 'device')
        (buf, desc) = pitched(bgr, order[:3], row_pad=5 + k, gaps=(k, 1 + k, 6 - k), stride_pad=7 + k, rng=rng)
        (host, dev) = _read_both(reader, buf.ctypes.data, desc, buf.nbytes)
        assert host.tobytes() == wb, (tag, order, 'pitched host')
        assert dev.tobytes() == wb, (tag, order, 'pitched device')
    return want


def _compare_records(recs, ores, ndials=4, tag=''):
    """tests/test_gpu_parity.py's rules for the whole path."""
    for i in range(len(recs)):
        (r, o) = (recs[i], ores[i])
        assert int(r['status']) == o.status, (tag, i, int(r['status']), o.status)
        assert (int(r['match_x']), int(r['match_y'])) == (o.match_x, o.match_y), (tag, i)
        assert float(r['match_val']) == o.match_val, (tag, i)  # float32, bit-exact
        if o.status == 0:
            assert np.allclose(r['pos'][:ndials], list(o.pos)[:ndials], rtol=0, atol=POS_TOL), (tag, i)
            assert np.allclose(r['angle'][:ndials], list(o.angle)[:ndials], rtol=0, atol=POS_TOL), (tag, i)
            assert abs(float(r['value']) - o.value) < 1e-8, (tag, i)
            assert int(float(r['value'])) == int(o.value), (tag, i)  # the three dial digits
        elif o.status == 2:
            assert int(r['failed_dial']) == o.failed_dial, (tag, i)
        elif o.status == 3:
            assert int(r['unreadable_mask']) == o.unreadable_mask, (tag, i)


@pytest.mark.gpu
@pytest.mark.parametrize('sd,count', [('sample-images1', 81), ('sample-images2', 223)])
def test_fixture_frames(env, sd, count):
    """The fixture frames as RGB, BGR and GBR planes: byte-identical to read_frames of the BGR frames, and equal to the oracle."""
    from oracle import pyoracle as po
    e = env[sd]
    assert len(e['frames']) == count
    oparams = po.Params(e['pfile'])
    rng = np.random.default_rng(count)
    shapes = {}
    for fr in e['frames']:
        shapes.setdefault(fr.shape, []).append(fr)
    (ok, ok_bgr) = (0, 0)
    for (shape, group) in shapes.items():
        bgr = np.stack(group)
        want = e['reader'].read_frames(bgr)
        ok_bgr += int((want['status'] == _hip.FRAME_OK).sum())
        _check_orders(e['reader'], bgr, '%s %s' % (sd, shape), rng, want=want)
        got = e['reader'].read_planar_frames(to_planes(bgr, 'rgb', rng), 'rgb')
        ok += int((got['status'] == _hip.FRAME_OK).sum())
        for (i, fr) in enumerate(group):
            _compare_records([got[i]], [po.process_frames(fr[None], oparams)[0]], tag='%s %s %d' % (sd, shape, i))
    print('%s: %d of %d planar frames read OK (BGR: %d)' % (sd, ok, count, ok_bgr))
    assert ok == ok_bgr and ok > 0   # the equality is one of readings, not of failures


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
    bgr = _synth(e['frames'], 256, 5)
    monkeypatch.setenv('MELF_MATCH', kind)
    r = MeterReader(e['params'])
    try:
        want = r.read_frames(bgr)
        assert r.ctx.last_match()['kernel'] == kernel
        assert (want['status'] == _hip.FRAME_DIALS_NOT_FOUND).sum() >= 28 and (want['status'] == _hip.FRAME_OK).sum() >= 128
        rng = np.random.default_rng(7)
        for (k, order) in enumerate(ORDERS3):
            (buf, desc) = pitched(bgr, order, row_pad=3, gaps=(1, 2, 1), stride_pad=9 + k, rng=rng)
            assert r.ctx.process_planes(buf.ctypes.data, desc).tobytes() == want.tobytes(), (kind, order, 'host')
            assert r.ctx.last_match()['kernel'] == kernel
            dbuf = DevBuf(buf.ctypes.data, buf.nbytes)
            try:
                assert r.ctx.process_planes_dev(dbuf.d.value, desc).tobytes() == want.tobytes(), (kind, order, 'device')
            finally:
                dbuf.free()
            assert r.ctx.last_match()['kernel'] == kernel
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['fast', 'dot4'])
def test_plane_phases(env, monkeypatch, kind):
    """The G and the R plane at each of the four byte phases relative to the B plane (16 pairs), the pitch at the four phases too
    (the phases then move from row to row), the base at each of its four: every combination of alignbit shifts of the prep
    kernel and every phase of the dial reader's unaligned dwords."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    bgr = _synth(e['frames'], 12, 17)
    monkeypatch.setenv('MELF_MATCH', kind)
    r = MeterReader(e['params'])
    try:
        want = r.read_frames(bgr)
        assert (want['status'] == _hip.FRAME_OK).sum() >= 8
        (n, H, W, _c) = bgr.shape
        rng = np.random.default_rng(23)
        seen = set()
        for pg in range(4):
            for pr in range(4):
                row_pad = (pg + pr) % 4
                span = (H - 1) * (W + row_pad) + W
                # plane order b, g, r: g starts span + gap_g behind b, r span + gap_r behind g
                gap_g = (pg - span) % 4
                gap_r = (pr - pg - span) % 4
                (buf, desc) = pitched(bgr, 'bgr', row_pad=row_pad, gaps=((pg + 2 * pr) % 5, gap_g, gap_r), stride_pad=(pr + 1) % 4, rng=rng)
                assert ((desc.g_offset - desc.b_offset) % 4, (desc.r_offset - desc.b_offset) % 4) == (pg, pr)
                seen.add(((desc.g_offset - desc.b_offset) % 4, (desc.r_offset - desc.b_offset) % 4))
                phase = (pg + pr) % 4
                (host, dev) = _read_both(r, buf.ctypes.data, desc, buf.nbytes, phase=phase)
                assert host.tobytes() == want.tobytes(), (pg, pr, 'host')
                assert dev.tobytes() == want.tobytes(), (pg, pr, 'device')
        assert len(seen) == 16
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
    """meter_rect (50, 160)-(300, 410) moved to all four parities of (x0, y0), and given sizes of all four parities; the frames
    are shifted by as much, so that the meter stays inside."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    src = _synth(e['frames'], 40, 3)
    rng = np.random.default_rng(13)
    cases = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0),       # origins at the four parities of (x, y), even sizes
             (0, 0, -1, 0), (0, 0, 0, -1), (0, 0, -1, -1),                  # sizes at the other three parities
             (1, 1, -1, -1), (1, 0, 1, 1), (3, 5, 1, 1), (2, 3, 2, 1))
    for (k, (dx, dy, dw, dh)) in enumerate(cases):
        params = _params_with_rect(tmp_path, 'sample-images1', (50 + dx, 160 + dy, 300 + dx + dw, 410 + dy + dh), 'odd%d' % k)
        bgr = np.roll(src, (dy, dx), axis=(1, 2))
        r = MeterReader(params)
        try:
            want = _check_orders(r, bgr, (dx, dy, dw, dh), rng, orders=(ORDERS3[k % 3], ORDERS3[(k + 1) % 3]))
            assert (want['status'] == _hip.FRAME_OK).sum() > 20, (dx, dy, dw, dh)
        finally:
            r.close()


@pytest.mark.gpu
def test_frame_edges_and_batch_sizes(env, tmp_path):
    """meter_rect reaching the right and bottom frame edges, and past them (numpy clamp); meter_rect at the frame's first row and
    column, where a plane at offset 0 starts at the buffer's first byte (at every phase of the base: the aligned window of the
    very first samples must not start before it); device buffers of exactly the descriptor's extent; batch sizes around the
    32-frame group and above the 128 frames of a host-path chunk."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(11)
    src = _synth(e['frames'], 131, 3)
    for (H, W) in ((410, 300), (399, 290), (405, 297)):
        bgr = np.ascontiguousarray(src[:12, :H, :W])
        want = _check_orders(reader, bgr, (H, W), rng)
        assert (want['status'] == _hip.FRAME_OK).sum() >= 6, (H, W)
    # the crop in the frame's top left corner, and filling the frame
    for (k, (y1, x1)) in enumerate(((480, 640), (410, 300))):
        bgr = np.ascontiguousarray(src[:12, 160:y1, 50:x1])
        r = MeterReader(_params_with_rect(tmp_path, 'sample-images1', (0, 0, 250, 250), 'corner%d' % k))
        try:
            want = _check_orders(r, bgr, ('corner', y1, x1), rng)
            assert (want['status'] == _hip.FRAME_OK).sum() >= 6
            for phase in range(4):
                for order in ORDERS3:
                    (buf, desc) = pitched(bgr, order, row_pad=phase, gaps=(0, phase, 1), stride_pad=phase, rng=rng)
                    assert min(desc.b_offset, desc.g_offset, desc.r_offset) == 0
                    (host, dev) = _read_both(r, buf.ctypes.data, desc, buf.nbytes, phase=phase)
                    assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes(), (y1, x1, phase, order)
        finally:
            r.close()
    want = reader.read_frames(src)
    assert (want['status'] == _hip.FRAME_OK).sum() > 80
    for (k, n) in enumerate((1, 31, 32, 33, 131)):
        _check_orders(reader, src[:n], n, rng, orders=(ORDERS3[k % 3],), want=want[:n])


@pytest.mark.gpu
def test_four_plane_tensors(env):
    """(N, 4, H, W) arrays with three named planes: the 4th (random here) is never looked at; x[:, :3] and x[:, 1:] views, crops
    and every other frame in place."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(41)
    bgr = _synth(e['frames'], 24, 8)
    want = reader.read_frames(bgr)
    assert (want['status'] == _hip.FRAME_OK).sum() >= 12
    for order in ('rgba', 'rgbx', 'bgra', 'bgrx'):
        arr = to_planes(bgr, order, rng)
        v = _hip.planar_frames_view(arr, order)
        assert not v.copied and v.frame_stride == 4 * arr.shape[2] * arr.shape[3]
        (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
        assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes(), order
        assert reader.read_planar_frames(arr, order).tobytes() == want.tobytes(), order
        v3 = _hip.planar_frames_view(arr[:, :3], order[:3])
        assert not v3.copied and v3.ptr == v.ptr
        assert reader.read_planar_frames(arr[:, :3], order[:3]).tobytes() == want.tobytes(), order
        assert reader.read_planar_frames(arr[::2], order).tobytes() == want[::2].tobytes(), order
    xrgb = to_planes(bgr, 'xrgb', rng)   # the helper writes the named planes wherever they are
    v = _hip.planar_frames_view(xrgb[:, 1:], 'rgb')
    assert not v.copied
    (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
    assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()
    # a wider and higher array, the frames a crop of it
    (n, H, W, _c) = bgr.shape
    big = rng.integers(0, 256, size=(n, 3, H + 3, W + 5), dtype=np.uint8)
    big[:, :, 2:2 + H, 1:1 + W] = to_planes(bgr, 'gbr')
    view = big[:, :, 2:2 + H, 1:1 + W]
    v = _hip.planar_frames_view(view, 'gbr')
    assert not v.copied and v.row_pitch == W + 5
    (host, dev) = _read_both(reader, v.ptr, v.descriptor(), v.extent)
    assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()
    # what cannot be described goes through one packed copy and gives the same records
    nhwc = np.ascontiguousarray(bgr[..., ::-1])
    v = _hip.planar_frames_view(nhwc.transpose(0, 3, 1, 2), 'rgb')
    assert v.copied
    assert reader.read_planar_frames(nhwc.transpose(0, 3, 1, 2), 'rgb').tobytes() == want.tobytes()


@pytest.mark.gpu
def test_random_frames(env):
    """Uniform random bytes in the three planes; half of the frames carry a fixture's meter, so that the dial reader runs."""
    e = env['sample-images1']
    rng = np.random.default_rng(99)
    n = 40
    bgr = rng.integers(0, 256, size=(n,) + e['frames'][2].shape, dtype=np.uint8)
    bgr[::2] = np.stack(e['frames'][2:2 + n // 2])
    want = _check_orders(e['reader'], bgr, 'random', rng)
    assert (want['status'] != _hip.FRAME_DIALS_NOT_FOUND).sum() >= n // 4


@pytest.mark.gpu
def test_1080p_six_dials_padded(env, tmp_path):
    """The configuration of tests/test_pixel_formats.py::test_1080p_six_dials_bgra_padded as GBR planes with a padded pitch."""
    import yaml
    from meterelf_amd import MeterReader, _params
    src = os.path.join(GOLDEN, 'sample-images1')
    with open(os.path.join(src, 'params.yml')) as fp:
        data = yaml.safe_load(fp)
    data['meter_rect'] = {'top_left': [1211, 421], 'bottom_right': [1461, 671]}
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
        frames[i, 421:671, 1211:1461] = f[160:410, 50:300]
    reader = MeterReader(params)
    try:
        want = reader.read_frames(frames)
        assert (want['status'] == _hip.FRAME_OK).any()
        (buf, desc) = pitched(frames, 'gbr', row_pad=33, gaps=(3, 2, 1), stride_pad=5, rng=rng)
        (host, dev) = _read_both(reader, buf.ctypes.data, desc, buf.nbytes)
        assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()
        arr = to_planes(frames, 'rgb', rng)
        assert reader.read_planar_frames(arr, 'rgb').tobytes() == want.tobytes()
    finally:
        reader.close()


@pytest.mark.gpu
def test_resident_lanes_two_streams(env):
    """melf_ctx_set_frames_resident(1) and two caller streams, layouts alternating: every call's records equal a synchronous call's."""
    from meterelf_amd import MeterReader
    e = env['sample-images2']
    hip = _hip_rt()
    bgr = _synth(e['frames'], 96, 21)
    rsz = _hip.RESULT_DTYPE.itemsize
    r = MeterReader(e['params'])
    bufs = []
    streams = [C.c_void_p(), C.c_void_p()]
    d_res = C.c_void_p()
    try:
        want = r.read_frames(bgr)
        assert (want['status'] == _hip.FRAME_OK).sum() > 48
        descs = []
        for (k, order) in enumerate(('rgb', 'bgr', 'gbr', 'rgb')):
            (buf, desc) = pitched(bgr, order, row_pad=k, gaps=(k, 1, 2), stride_pad=3 * k, rng=np.random.default_rng(k))
            bufs.append(DevBuf(buf.ctypes.data, buf.nbytes))
            descs.append(desc)
            assert r.ctx.process_planes_dev(bufs[-1].d.value, desc).tobytes() == want.tobytes(), order   # the synchronous call
        for s in streams:
            assert hip.hipStreamCreate(C.byref(s)) == 0
        assert hip.hipMalloc(C.byref(d_res), C.c_size_t(8 * len(bgr) * rsz)) == 0
        r.ctx.set_frames_resident(True)
        for i in range(8):
            r.ctx.process_planes_dev(bufs[i % 4].d.value, descs[i % 4], d_results_ptr=d_res.value + i * len(bgr) * rsz, want_host=False,
                                     stream=streams[i % 2].value)
        r.ctx.sync()
        got = np.zeros(8 * len(bgr), _hip.RESULT_DTYPE)
        assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), d_res, C.c_size_t(got.nbytes), 2) == 0
        for i in range(8):
            assert got[i * len(bgr):(i + 1) * len(bgr)].tobytes() == want.tobytes(), i
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
    bgr = np.stack(e['frames'][2:6])
    (n, H, W, _c) = bgr.shape
    host = np.ascontiguousarray(to_planes(bgr, 'bgr'))
    P = H * W
    buf = DevBuf(host.ctypes.data, host.nbytes)
    try:
        ctx.set_profiling(1)
        before = {k: cnt for (k, (_ms, cnt)) in ctx.timings().items()}
        out = np.zeros(n, _hip.RESULT_DTYPE)
        F = _hip.MelfPlanarFrames
        bad = [
            F(n, 0, W, 0, 0, P, 2 * P, W, 3 * P),             # H, W <= 0, n < 0
            F(n, H, 0, 0, 0, P, 2 * P, W, 3 * P),
            F(n, -1, W, 0, 0, P, 2 * P, W, 3 * P),
            F(n, H, -3, 0, 0, P, 2 * P, W, 3 * P),
            F(-1, H, W, 0, 0, P, 2 * P, W, 3 * P),
            F(n, H, W, 1, 0, P, 2 * P, W, 3 * P),             # reserved != 0
            F(n, H, W, -1, 0, P, 2 * P, W, 3 * P),
            F(n, H, W, 0, -1, P, 2 * P, W, 3 * P),            # a negative offset
            F(n, H, W, 0, 0, -P, 2 * P, W, 3 * P),
            F(n, H, W, 0, 0, P, -2 * P, W, 3 * P),
            F(n, H, W, 0, 0, P, 2 * P, W - 1, 3 * P),         # row_pitch < W
            F(n, H, W, 0, 0, P, 2 * P, 0, 3 * P),
            F(n, H, W, 0, 0, 2 ** 40, 2 ** 41, 2 ** 31, 2 ** 42),   # row_pitch > 2^31 - 1
            F(n, H, W, 0, 0, P - 1, 2 * P, W, 3 * P),         # two planes closer together than a plane: overlapping
            F(n, H, W, 0, 0, P, 2 * P - 1, W, 3 * P),
            F(n, H, W, 0, 0, P, 0, W, 3 * P),                 # the same plane named twice
            F(n, H, W, 0, P, P, P, W, 3 * P),
            F(n, H - 1, W, 0, 0, P - W, 2 * P, W + 1, 3 * P), # overlapping through the pitch: (H - 2) (W + 1) + W > P - W
            F(n, H, W, 0, 0, P, 2 * P, W, 3 * P - 1),         # frame_stride smaller than the span of a frame's planes
            F(n, H, W, 0, 2 * P, P, 0, W, 2 * P),
            F(n, H, W, 0, 0, P, 2 * P, W, 0),
        ]

        def all_fail(dptr, hptr, fref, key):
            assert L.melf_process_planes_dev(ctx._h, dptr, fref, None, _hip._ptr(out), None) == -1, key
            assert L.melf_last_error().decode()
            assert L.melf_process_planes(ctx._h, hptr, fref, _hip._ptr(out)) == -1, key
            assert L.melf_last_error().decode()
        for f in bad:
            all_fail(C.c_void_p(buf.d.value), C.c_void_p(host.ctypes.data), C.byref(f),
                     (f.n, f.H, f.W, f.reserved, f.b_offset, f.g_offset, f.r_offset, f.row_pitch, f.frame_stride))
        good = F(n, H, W, 0, 0, P, 2 * P, W, 3 * P)
        all_fail(C.c_void_p(buf.d.value), C.c_void_p(host.ctypes.data), None, 'NULL descriptor')
        all_fail(None, None, C.byref(good), 'NULL frames')
        # n == 0 passes, whatever the pointers
        empty = F(0, H, W, 0, 0, P, 2 * P, W, 3 * P)
        assert L.melf_process_planes_dev(ctx._h, None, C.byref(empty), None, None, None) == 0
        assert L.melf_process_planes(ctx._h, None, C.byref(empty), None) == 0
        assert {k: cnt for (k, (_ms, cnt)) in ctx.timings().items()} == before
        # a good descriptor runs; planes that touch without overlapping are good
        assert L.melf_process_planes_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
        assert {k: cnt for (k, (_ms, cnt)) in ctx.timings().items()} != before
        assert out.tobytes() == e['reader'].read_frames(bgr).tobytes()
    finally:
        ctx.set_profiling(0)
        buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_planar_frames with torch tensors, in a child process that imports torch first."""
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.abspath(__file__), 'torch'], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch planar path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


def _torch_main():
    import torch  # before the package loads the library: one HIP runtime in the process
    from meterelf_amd import MeterReader, _params
    from meterelf_amd._image import imread_bgr
    params = _params.load(os.path.join(GOLDEN, 'sample-images1', 'params.yml'))
    files = sorted(glob.glob(os.path.join(GOLDEN, 'sample-images1', '*.jpg')))
    frames = [imread_bgr(f) for f in files]
    bgr = _synth(frames, 128, 9)
    reader = MeterReader(params, device=0)
    dev = torch.device('cuda', 0)
    want = reader.read_frames(bgr)
    assert (want['status'] == _hip.FRAME_OK).sum() > 64
    rsz = _hip.RESULT_DTYPE.itemsize
    rng = np.random.default_rng(1)
    (n, H, W, _c) = bgr.shape
    for order in ('rgb', 'bgr', 'gbr', 'rgba', 'bgrx'):
        t = torch.from_numpy(to_planes(bgr, order, rng)).to(dev)
        assert t.is_contiguous() and not _hip.planar_frames_view(t, order).copied
        assert reader.read_planar_frames(t, order).tobytes() == want.tobytes(), order
        # host tensors take the host path
        assert reader.read_planar_frames(t.cpu(), order).tobytes() == want.tobytes(), order
        # out=: records into a device tensor on the current stream, nothing synchronised
        out = torch.empty((n, rsz), dtype=torch.uint8, device=dev)
        assert reader.read_planar_frames(t, order, out=out) is out
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), (order, 'out')
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
    out = torch.empty((n, rsz), dtype=torch.uint8, device=dev)
    reader.read_planar_frames(nhwc.permute(0, 3, 1, 2), 'rgb', out=out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        reader.read_planar_frames(t.cpu(), 'rgb', out=out)   # out= takes device frames only
    with pytest.raises(ValueError):
        reader.read_planar_frames(t, 'rgba')
    # resident frames, two caller streams, out= on each
    reader.ctx.set_frames_resident(True)
    (sa, sb) = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    outs = []
    torch.cuda.synchronize()
    for i in range(6):
        with torch.cuda.stream(sa if i % 2 == 0 else sb):
            o = torch.empty((n, rsz), dtype=torch.uint8, device=dev)
            reader.read_planar_frames(view if i % 3 else t4, 'rgb' if i % 3 else 'rgba', out=o)
            outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
        assert o.cpu().numpy().tobytes() == want.tobytes()
    reader.ctx.set_frames_resident(False)
    reader.ctx.sync()
    reader.close()
    print('torch planar path ok')


if __name__ == '__main__' and sys.argv[1:] == ['torch']:
    _torch_main()
