"""Frames in the layouts callers have -- RGB, BGRA / BGRx, RGBA / RGBx, padded rows and frames -- read in place
(melf_process_frames, melf_process_frames_dev, _hip.frames_view, MeterReader.read_frame_views).

The contract: the records of a frame in any layout are byte-identical to read_frames() of the packed BGR frame made from it
(what get_bgr_image + _crop_meter would have read, meterelf/_image.py:46-55).  CPU tests: the descriptor's layout against the
header, frames_view's mapping of numpy arrays and torch CPU tensors, the new kernels' code-object notes.  GPU tests: records
against the BGR path on the fixtures, with every match kernel, at 1080p, at the frame edges, over lanes and streams.

The helpers these tests share with the other frame formats' -- the readers, device buffers, frame synthesis, the torch child
process -- are in tests/frame_cases.py.  The bodies here stay the file's own: packed pixels go through frames_view and
process_frames' argument list, not through a descriptor as the other families do.
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
from tests.frame_cases import env, read_packed_dev as _read_dev, to_layout  # noqa: E402,F401

FORMATS = ('bgr', 'rgb', 'bgra', 'rgba')


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_frames_struct_matches_header(tmp_path):
    src = tmp_path / 'frames.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(melf_frames),'
                   'offsetof(melf_frames, pixel_format), offsetof(melf_frames, n), offsetof(melf_frames, H), offsetof(melf_frames, W),'
                   'offsetof(melf_frames, row_pitch), offsetof(melf_frames, frame_stride),'
                   'MELF_PIX_BGR, MELF_PIX_RGB, MELF_PIX_BGRA, MELF_PIX_RGBA);return 0;}\n')
    exe = tmp_path / 'frames'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfFrames
    assert got == [C.sizeof(F), F.pixel_format.offset, F.n.offset, F.H.offset, F.W.offset, F.row_pitch.offset, F.frame_stride.offset,
                   _hip.PIX_BGR, _hip.PIX_RGB, _hip.PIX_BGRA, _hip.PIX_RGBA]
    for name in ('melf_process_frames', 'melf_process_frames_dev'):
        assert name in _hip.EXPORTS


def _arrays():
    """numpy and (when importable) torch CPU flavours of the same test array."""
    yield np.zeros
    try:
        import torch
    except ImportError:
        return
    yield lambda shape, dtype: torch.zeros(shape, dtype=torch.uint8 if dtype == np.uint8 else torch.int16)


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_frames_view_layouts(kind):
    makers = list(_arrays())
    if kind == 'torch' and len(makers) < 2:
        pytest.skip('torch is not installed')
    z = makers[0 if kind == 'numpy' else 1]
    (n, H, W) = (4, 10, 12)
    for (fmt, ch, code) in (('bgr', 3, _hip.PIX_BGR), ('rgb', 3, _hip.PIX_RGB), ('bgra', 4, _hip.PIX_BGRA), ('rgba', 4, _hip.PIX_RGBA)):
        a = z((n, H, W, ch), np.uint8)
        v = _hip.frames_view(a, fmt)
        assert (v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride, v.extent, v.copied, v.on_device) == \
               (code, n, H, W, W * ch, H * W * ch, n * H * W * ch, False, False)
        # padded rows, every other frame: described by the strides, no copy
        v = _hip.frames_view(a[:, :, :7], fmt)
        assert (v.W, v.row_pitch, v.frame_stride, v.extent, v.copied) == (7, W * ch, H * W * ch, 3 * H * W * ch + 9 * W * ch + 7 * ch, False)
        v = _hip.frames_view(a[::2], fmt)
        assert (v.n, v.frame_stride, v.extent, v.copied) == (2, 2 * H * W * ch, 2 * H * W * ch + H * W * ch, False)
        # the last frame's last row unpadded: the extent stops at its last pixel
        v = _hip.frames_view(a[1:3, 2:9, 1:6], fmt)
        assert v.extent == H * W * ch + 6 * W * ch + 5 * ch and not v.copied
        assert v.ptr == (a.ctypes.data if kind == 'numpy' else a.data_ptr()) + H * W * ch + 2 * W * ch + ch
    # a 3-channel view of 4-byte pixels: the 4-byte format of the same order, read in place
    a = z((n, H, W, 4), np.uint8)
    for (fmt, code) in (('bgr', _hip.PIX_BGRA), ('rgb', _hip.PIX_RGBA)):
        v = _hip.frames_view(a[..., :3], fmt)
        assert (v.pixel_format, v.row_pitch, v.frame_stride, v.copied) == (code, W * 4, H * W * 4, False)
    # ... but not when its channels start one byte in (misaligned, and the last pixel's 4th byte lies behind the array): copied
    v = _hip.frames_view(a[..., 1:], 'rgb')
    assert (v.pixel_format, v.row_pitch, v.frame_stride, v.copied) == (_hip.PIX_RGB, W * 3, H * W * 3, True)
    # a misaligned 4-byte layout: copied once to a packed (aligned) array
    if kind == 'numpy':
        b = np.zeros(n * H * W * 4 + 1, np.uint8)[1:].reshape(n, H, W, 4)
        v = _hip.frames_view(b, 'bgra')
        assert v.copied and v.pixel_format == _hip.PIX_BGRA and v.ptr % 4 == 0 and v.row_pitch == W * 4
        # reversed channels (negative stride): copied, the format names the view's channels
        c = np.arange(n * H * W * 3, dtype=np.uint8).reshape(n, H, W, 3)
        v = _hip.frames_view(c[..., ::-1], 'rgb')
        assert v.copied and v.pixel_format == _hip.PIX_RGB and np.array_equal(v.array, c[..., ::-1])
        # every other pixel: a pixel stride of 6, copied
        v = _hip.frames_view(c[:, :, ::2], 'bgr')
        assert v.copied and (v.W, v.row_pitch) == (6, 18)
    # rejected: not uint8, C = 2, a format that does not name the channels
    with pytest.raises(ValueError):
        _hip.frames_view(z((n, H, W, 3), np.int16), 'bgr')
    with pytest.raises(ValueError):
        _hip.frames_view(z((n, H, W, 2), np.uint8), 'bgr')
    with pytest.raises(ValueError):
        _hip.frames_view(z((n, H, W, 3), np.uint8), 'bgra')
    with pytest.raises(ValueError):
        _hip.frames_view(z((n, H, W, 4), np.uint8), 'yuv')


def test_new_kernels_metadata():
    """The kernels that read the new layouts are in the library, without scratch, within the dial reader's register budget."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    new = {k: d for (k, d) in meta.items() if any(s in k for s in ('k_lplane_px4', 'k_match_px4', 'k_needles'))}
    assert sum('k_lplane_px4' in k for k in new) == 1 and sum('k_match_px4' in k for k in new) == 1
    assert sum('k_needles' in k for k in new) == 12
    dials_vgpr = max(d['vgpr_count'] for (k, d) in meta.items() if 'k_dials' in k)
    for (k, d) in new.items():
        assert d.get('private_segment_fixed_size', 0) == 0 and d.get('vgpr_spill_count', 0) == 0, (k, d)
        if 'k_needles' in k:
            assert d['vgpr_count'] <= dials_vgpr, (k, d)


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _check_all_layouts(reader, bgr, tag, rng):
    want = reader.read_frames(bgr).tobytes()
    for fmt in FORMATS:
        for pad in (0, 13):
            (arr, f) = to_layout(bgr, fmt, pad, rng)
            assert reader.read_frame_views(arr, f).tobytes() == want, (tag, fmt, pad, 'host')
            v = _hip.frames_view(arr, f)
            assert not v.copied
            assert _read_dev(reader.ctx, v).tobytes() == want, (tag, fmt, pad, 'device')


@pytest.mark.gpu
@pytest.mark.parametrize('sd,count', [('sample-images1', 81), ('sample-images2', 223)])
def test_fixture_frames_every_layout(env, sd, count):
    e = env[sd]
    assert len(e['frames']) == count
    rng = np.random.default_rng(count)
    shapes = {}
    for fr in e['frames']:
        shapes.setdefault(fr.shape, []).append(fr)
    for (shape, group) in shapes.items():
        _check_all_layouts(e['reader'], np.stack(group), '%s %s' % (sd, shape), rng)
    # the 3-channel view of 4-byte pixels goes the 4-byte way, in place
    bgr = np.stack(shapes[e['frames'][0].shape][:40])
    (arr, f) = to_layout(bgr, 'rgba', 5, rng, view3=True)
    v = _hip.frames_view(arr, f)
    assert v.pixel_format == _hip.PIX_RGBA and not v.copied
    assert e['reader'].read_frame_views(arr, f).tobytes() == e['reader'].read_frames(bgr).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')])
def test_each_match_kernel(env, monkeypatch, kind, kernel):
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    bgr = fc.synth(e['frames'], 256, 5)
    monkeypatch.setenv('MELF_MATCH', kind)
    r = MeterReader(e['params'])
    try:
        want = r.read_frames(bgr)
        assert (want['status'] == _hip.FRAME_DIALS_NOT_FOUND).sum() >= 28 and (want['status'] == _hip.FRAME_OK).any()
        rng = np.random.default_rng(7)
        for fmt in FORMATS:
            (arr, f) = to_layout(bgr, fmt, 7, rng)
            assert r.read_frame_views(arr, f).tobytes() == want.tobytes(), (kind, fmt, 'host')
            assert r.ctx.last_match()['kernel'] == kernel
            assert _read_dev(r.ctx, _hip.frames_view(arr, f)).tobytes() == want.tobytes(), (kind, fmt, 'device')
            assert r.ctx.last_match()['kernel'] == kernel
    finally:
        r.close()


@pytest.mark.gpu
def test_1080p_six_dials_bgra_padded(env, tmp_path):
    """BASELINE config 5 shape (tests/test_gpu_parity.py::test_1080p_six_dials): BGRA with padded rows reads like BGR."""
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
    good = env['sample-images1']['frames'][2:7]   # the frames test_1080p_six_dials places (the two rejected ones are 0 and 1)
    frames = rng.integers(0, 256, size=(len(good), 1080, 1920, 3), dtype=np.uint8)
    for (i, f) in enumerate(good):
        frames[i, 420:670, 1210:1460] = f[160:410, 50:300]
    reader = MeterReader(params)
    try:
        want = reader.read_frames(frames)
        assert (want['status'] == _hip.FRAME_OK).any()
        (arr, f) = to_layout(frames, 'bgra', 64, rng)
        assert reader.read_frame_views(arr, f).tobytes() == want.tobytes()
        assert _read_dev(reader.ctx, _hip.frames_view(arr, f)).tobytes() == want.tobytes()
    finally:
        reader.close()


@pytest.mark.gpu
def test_frame_edges_and_batch_sizes(env):
    """meter_rect (50, 160)-(300, 410) reaching the right and bottom frame edges, and past them (numpy clamp), device copies of
    exactly the descriptor's extent at the start of their allocation (what lies behind them is mapped: test_buffer_ends places
    them at its end); batch sizes around the 32-frame group."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(11)
    src = fc.synth(e['frames'], 70, 3)
    assert (reader.read_frames(src)['status'] == _hip.FRAME_OK).sum() > 40
    for (H, W) in ((410, 300), (400, 290)):
        bgr = np.ascontiguousarray(src[:12, :H, :W])
        want = reader.read_frames(bgr).tobytes()
        for fmt in FORMATS:
            (arr, f) = to_layout(bgr, fmt, 3, rng)
            assert reader.read_frame_views(arr, f).tobytes() == want, (H, W, fmt)
            assert _read_dev(reader.ctx, _hip.frames_view(arr, f)).tobytes() == want, (H, W, fmt)
    for n in (1, 31, 33, 70):
        want = reader.read_frames(src[:n]).tobytes()
        for fmt in ('rgb', 'bgra'):
            (arr, f) = to_layout(src[:n], fmt, 9, rng)
            assert reader.read_frame_views(arr, f).tobytes() == want, (n, fmt)
            assert _read_dev(reader.ctx, _hip.frames_view(arr, f)).tobytes() == want, (n, fmt)


@pytest.mark.gpu
def test_buffer_ends(env, monkeypatch, tmp_path):  # noqa: F811
    """tests/frame_cases.py: buffer_ends -- pitched buffers of exactly the descriptor's extent that end where their allocation ends,
    at every base phase the descriptor check accepts, the match at the crop's bottom-right corner, 1 and 33 frames, every match
    kernel."""
    def layouts(src, k, fmt, rng):
        return [fc.pitched_packed(src[0], fmt, pad, rng) for pad in ((0, 12) if fmt in ('bgra', 'rgba') else (0, 7))]
    fc.buffer_ends(monkeypatch, tmp_path, FORMATS, from_bgr=lambda bgr: (bgr,), bgr_of=lambda bgr: bgr,
                   layouts=layouts, read_dev=lambda ctx, d, a: ctx.process_frames_dev(d, *a), nframes_stride=lambda a: (a[1], a[5]),
                   phases_of=lambda fmt: (0,) if fmt in ('bgra', 'rgba') else (0, 1, 2, 3))


@pytest.mark.gpu
def test_first_bytes_unaligned_base(env, monkeypatch, tmp_path):  # noqa: F811
    """tests/frame_cases.py: first_bytes -- a base at byte phases 1 .. 3 and the meter crop at the frame's first row and first
    columns, where the launcher sends the prep kernel down its sample-by-sample path: the records are the BGR path's.  (Where the
    loads start is swept on the CPU, tests/prep_bounds_main.cpp.)"""
    fc.first_bytes(monkeypatch, tmp_path, ('bgr', 'rgb'), from_bgr=lambda bgr: (bgr,), bgr_of=lambda bgr: bgr,
                   layouts=lambda src, k, fmt, rng: [fc.pitched_packed(src[0], fmt, 0, rng)],
                   read_dev=lambda ctx, d, a: ctx.process_frames_dev(d, *a), x0s=(0, 1))


@pytest.mark.gpu
def test_resident_lanes_two_streams(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1) and two caller streams: every call's records equal a single synchronous call's."""
    from meterelf_amd import MeterReader
    e = env['sample-images2']
    src = fc.synth(e['frames'], 96, 21)
    r = MeterReader(e['params'])
    bufs = []
    try:
        want = r.read_frames(src)
        assert (want['status'] == _hip.FRAME_OK).sum() > 48
        calls = []
        for (k, fmt) in enumerate(FORMATS):
            (arr, f) = to_layout(src, fmt, 4 * k, np.random.default_rng(k))
            v = _hip.frames_view(arr, f)
            bufs.append(fc.DevBuf(v.ptr, v.extent))
            calls.append((functools.partial(r.ctx.process_frames_dev, bufs[-1].d.value, v.pixel_format, v.n, v.H, v.W, v.row_pitch,
                                            v.frame_stride), want.tobytes()))
        fc.resident_calls(r, len(src), calls, 8, lambda i: i % 4)   # formats in turn, streams alternating, each call its own records
    finally:
        r.close()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_argument_errors_launch_nothing(env):
    e = env['sample-images1']
    ctx = e['reader'].ctx
    L = _hip.lib()
    bgr = np.stack(e['frames'][2:6])
    (n, H, W, _) = bgr.shape
    bgra = np.zeros((n, H, W, 4), np.uint8)
    view = _hip.frames_view(bgra, 'bgra')
    buf = fc.DevBuf(view.ptr, view.extent)
    try:
        ctx.set_profiling(1)
        before = fc.launch_counts(ctx)
        out = np.zeros(n, _hip.RESULT_DTYPE)
        F = _hip.MelfFrames
        bad = [
            (F(7, n, H, W, W * 3, H * W * 3), 0),                        # unknown format
            (F(-1, n, H, W, W * 3, H * W * 3), 0),
            (F(_hip.PIX_BGR, n, H, W, W * 3 - 1, H * W * 3), 0),         # pitch too small
            (F(_hip.PIX_BGRA, n, H, W, W * 4, (H - 1) * W * 4 + W * 4 - 1), 0),   # stride too small
            (F(_hip.PIX_BGRA, n, H, W, W * 4 + 2, H * (W * 4 + 2)), 0),  # misaligned pitch
            (F(_hip.PIX_RGBA, n, H, W, W * 4, H * W * 4 + 1), 0),        # misaligned stride
            (F(_hip.PIX_RGBA, n, H, W, W * 4, H * W * 4), 1),            # misaligned base
            (F(_hip.PIX_BGR, n, 0, W, W * 3, H * W * 3), 0),             # bad shape
        ]
        for (f, off) in bad:
            for dev in (True, False):
                if dev:
                    rc = L.melf_process_frames_dev(ctx._h, C.c_void_p(buf.d.value + off), C.byref(f), None, _hip._ptr(out), None)
                else:
                    rc = L.melf_process_frames(ctx._h, C.c_void_p(bgra.ctypes.data + off), C.byref(f), _hip._ptr(out))
                assert rc == -1, (f.pixel_format, f.row_pitch, f.frame_stride, off, dev)
                assert L.melf_last_error().decode()
        assert L.melf_process_frames_dev(ctx._h, C.c_void_p(buf.d.value), None, None, _hip._ptr(out), None) == -1
        assert L.melf_process_frames(ctx._h, C.c_void_p(bgra.ctypes.data), None, _hip._ptr(out)) == -1
        assert fc.launch_counts(ctx) == before
        # a good descriptor runs
        good = F(_hip.PIX_BGRA, n, H, W, W * 4, H * W * 4)
        assert L.melf_process_frames_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
        assert fc.launch_counts(ctx) != before
    finally:
        ctx.set_profiling(0)
        buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_frame_views with torch tensors, in a child process that imports torch first (tests/frame_cases.py says why)."""
    fc.run_torch_child('packed')
