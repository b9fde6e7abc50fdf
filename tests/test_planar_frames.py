"""Planar, channels-first frames -- (N, 3, H, W) / (N, 4, H, W) uint8: torch's decoders and pre-processing pipelines, ffmpeg's
gbrp, rgb24 split into planes -- read in place (melf_process_planes, melf_process_planes_dev, _hip.planar_frames_view,
MeterReader.read_planar_frames).

The contract: the records of a planar frame are byte-identical to read_frames() of the packed BGR frame whose pixel (x, y) is
(B[y][x], G[y][x], R[y][x]).  No colour conversion is involved, so the same records are also held against the CPU oracle on that
BGR frame, under the rules of tests/test_gpu_parity.py (its _compare_records: status, match position, float32 match value
bit-exact, positions and angles to 1e-9, the digits).

CPU tests: the descriptor against the header, planar_frames_view's mapping of numpy arrays and torch CPU tensors, the exported
symbols, the new kernels' code-object notes.  GPU tests: the fixtures as RGB, BGR and GBR planes, every match kernel, plane
offsets and pitches that put the three planes at every byte phase relative to each other and to the base, meter_rect at every
parity and at the frame's edges, 4-plane tensors, batch sizes, random bytes, 1080p with six dials, resident lanes on two caller
streams, rejected descriptors, torch tensors (in a child process that imports torch first: tests/frame_cases.py says why).
Every device buffer has exactly the descriptor's extent and ends where its allocation ends.
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
from tests.frame_cases import PLANAR, env, extent_planes as _desc_extent, pitched_planes as pitched, to_planes  # noqa: E402,F401

ORDERS3 = PLANAR.formats
DevBuf = fc.DevBuf.at_end   # every device buffer of this file ends where its allocation ends


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
_read_both = functools.partial(fc.read_both, PLANAR)


def _check_orders(reader, bgr, tag, rng, orders=ORDERS3, want=None):
    """Every order, as an (N, C, H, W) array and as a pitched buffer with odd gaps, host and device, against read_frames."""
    return fc.check_formats(PLANAR, reader, (bgr,), tag, rng, orders, want)


def _check_source(reader, src, tag, rng, **kw):
    return _check_orders(reader, *src, tag, rng, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('sd,count', [('sample-images1', 81), ('sample-images2', 223)])
def test_fixture_frames(env, sd, count):
    """The fixture frames as RGB, BGR and GBR planes: byte-identical to read_frames of the BGR frames, and equal to the oracle."""
    from oracle import pyoracle as po
    from tests.test_gpu_parity import _compare_records
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


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')])
def test_each_match_kernel(env, monkeypatch, kind, kernel):  # noqa: F811
    layout = fc.as_pitched(PLANAR, lambda k: dict(row_pad=3, gaps=(1, 2, 1), stride_pad=9 + k))
    fc.each_match_kernel(env['sample-images1'], monkeypatch, kind, kernel, [(PLANAR, ORDERS3, layout)], n=256, seed=5, rng_seed=7,
                         min_not_found=28, min_ok=128)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['fast', 'dot4'])
def test_plane_phases(env, monkeypatch, kind):
    """The G and the R plane at each of the four byte phases relative to the B plane (16 pairs), the pitch at the four phases too
    (the phases then move from row to row), the base at each of its four: every combination of alignbit shifts of the prep
    kernel and every phase of the dial reader's unaligned dwords."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    bgr = fc.synth(e['frames'], 12, 17)
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


@pytest.mark.gpu
def test_odd_geometry(env, tmp_path):  # noqa: F811
    """meter_rect (50, 160)-(300, 410) moved to all four parities of (x0, y0), and given sizes of all four parities; the frames
    are shifted by as much, so that the meter stays inside."""
    cases = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0),       # origins at the four parities of (x, y), even sizes
             (0, 0, -1, 0), (0, 0, 0, -1), (0, 0, -1, -1),                  # sizes at the other three parities
             (1, 1, -1, -1), (1, 0, 1, 1), (3, 5, 1, 1), (2, 3, 2, 1))
    fc.odd_geometry(PLANAR, env['sample-images1'], tmp_path, cases,
                    lambda r, src, tag, rng, k: _check_source(r, src, tag, rng, orders=(ORDERS3[k % 3], ORDERS3[(k + 1) % 3])),
                    n=40, seed=3, rng_seed=13, min_ok=20)


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
    src = fc.synth(e['frames'], 131, 3)
    fc.frame_edges(PLANAR, reader, src, rng, 12, ((410, 300), (399, 290), (405, 297)), _check_source, min_ok=6)
    # the crop in the frame's top left corner, and filling the frame
    for (k, (y1, x1)) in enumerate(((480, 640), (410, 300))):
        bgr = np.ascontiguousarray(src[:12, 160:y1, 50:x1])
        r = MeterReader(fc.params_with_rect(tmp_path, 'sample-images1', (0, 0, 250, 250), 'corner%d' % k))
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
    fc.batch_sizes(PLANAR, reader, src, rng, (1, 31, 32, 33, 131), lambda k: (ORDERS3[k % 3],),
                   lambda r, src_, tag, rng_, formats, want: _check_source(r, src_, tag, rng_, orders=formats, want=want), min_ok=80)


@pytest.mark.gpu
def test_four_plane_tensors(env):
    """(N, 4, H, W) arrays with three named planes: the 4th (random here) is never looked at; x[:, :3] and x[:, 1:] views, crops
    and every other frame in place."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(41)
    bgr = fc.synth(e['frames'], 24, 8)
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
def test_resident_lanes_two_streams(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1) and two caller streams, layouts alternating: every call's records equal a synchronous call's."""
    fc.resident_lanes_two_streams(PLANAR, env['sample-images2'], ('rgb', 'bgr', 'gbr', 'rgb'),
                                  lambda k: dict(row_pad=k, gaps=(k, 1, 2), stride_pad=3 * k), n=96, seed=21, min_ok=48,
                                  keep_host=False)


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
        before = fc.launch_counts(ctx)
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
        assert fc.launch_counts(ctx) == before
        # a good descriptor runs; planes that touch without overlapping are good
        assert L.melf_process_planes_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
        assert fc.launch_counts(ctx) != before
        assert out.tobytes() == e['reader'].read_frames(bgr).tobytes()
    finally:
        ctx.set_profiling(0)
        buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_planar_frames with torch tensors, in a child process that imports torch first."""
    fc.run_torch_child('planar')
