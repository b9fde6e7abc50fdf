"""RGB frames of wide samples -- 16-bit words, float16, bfloat16, float32 -- read in place (melf_process_wide, melf_process_wide_dev,
melf_wide_to_bgr, _hip.wide_frames_view, MeterReader.read_wide_frames).

The contract (include/meterelf_hip.h): a sample becomes one byte by the narrowing rule -- tests/wide_cases.py restates it in numpy,
the reference of every comparison here --, and the records are byte-identical to melf_process_frames (packed) / melf_process_planes
(planar) on the 8-bit frames of those bytes.

CPU tests: the descriptor against the header, wide_frames_view's mapping of arrays and its ValueErrors.  GPU tests: the narrowing
kernel alone over every 16-bit pattern and the directed float32 set (melf_wide_to_bgr, byte for byte numpy's), eight fixture frames
in every sample type through both entry points, the timings, torch tensors (in a child process that imports torch first:
tests/frame_cases.py says why)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402

from tests import frame_cases as fc  # noqa: E402
from tests import wide_cases as wc  # noqa: E402
from tests.frame_cases import env  # noqa: E402,F401

NP_DTYPE = {wc.U16: np.uint16, wc.F16: np.float16, wc.BF16: np.uint16, wc.F32: np.float32}   # bf16 travels as its bits
PACKED_PIX = {'bgr': _hip.PIX_BGR, 'rgb': _hip.PIX_RGB, 'bgra': _hip.PIX_BGRA, 'rgba': _hip.PIX_RGBA}
ROUNDINGS = {'nearest': 0, 'floor': 1}


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_wide_struct_matches_header(tmp_path):
    fields = ('sample_type', 'layout', 'pixel_format', 'shift', 'rounding', 'reserved', 'scale', 'offset', 'n', 'H', 'W', 'reserved2',
              'b_offset', 'g_offset', 'r_offset', 'row_pitch', 'frame_stride')
    src = tmp_path / 'wide.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(melf_wide_frames));\n'
                   + ''.join('printf(" %%zu", offsetof(melf_wide_frames, %s));\n' % f for f in fields)
                   + 'printf(" %d %d %d %d %d %d %d %d %d\\n", MELF_WIDE_U16, MELF_WIDE_F16, MELF_WIDE_BF16, MELF_WIDE_F32, MELF_WIDE_PACKED,'
                   ' MELF_WIDE_PLANAR, MELF_ROUND_NEAREST, MELF_ROUND_FLOOR, MELF_ABI_VERSION);return 0;}\n')
    exe = tmp_path / 'wide'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfWideFrames
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in fields] + [
        _hip.WIDE_U16, _hip.WIDE_F16, _hip.WIDE_BF16, _hip.WIDE_F32, _hip.WIDE_PACKED, _hip.WIDE_PLANAR, _hip.ROUND_NEAREST, _hip.ROUND_FLOOR, 3]
    assert C.sizeof(F) == 104 and _hip.ABI_VERSION == 3   # the ABI version stays
    for name in ('melf_process_wide', 'melf_process_wide_dev', 'melf_wide_to_bgr'):
        assert name in _hip.EXPORTS and hasattr(_hip.lib(), name), name


def test_wide_frames_view_layouts():
    """numpy arrays: the descriptor of contiguous arrays, of a channel slice of 4 channels, of a spatial crop and of a base with
    the sample's own alignment only; the coefficient order; every ValueError."""
    (n, H, W) = (3, 6, 10)
    for (dt, code, ss) in ((np.uint16, _hip.WIDE_U16, 2), (np.float16, _hip.WIDE_F16, 2), (np.float32, _hip.WIDE_F32, 4)):
        kw = dict(shift=4) if dt == np.uint16 else {}
        a = np.zeros((n, 3, H, W), dt)
        v = _hip.wide_frames_view(a, 'chw', 'gbr', **kw)
        P = H * W * ss
        assert (v.sample_type, v.layout, v.n, v.H, v.W, v.g_offset, v.b_offset, v.r_offset, v.row_pitch, v.frame_stride, v.extent, v.ptr) == (
            code, _hip.WIDE_PLANAR, n, H, W, 0, P, 2 * P, W * ss, 3 * P, n * 3 * P, a.ctypes.data)
        assert v.shift == (4 if dt == np.uint16 else 0) and not v.copied and not v.on_device
        # a channel slice of 4 planes, a spatial crop (its base has the sample's alignment only)
        a4 = np.zeros((n, 4, H, W), dt)
        v = _hip.wide_frames_view(a4[:, :3], 'chw', 'rgb', **kw)
        assert (v.r_offset, v.g_offset, v.b_offset, v.frame_stride, v.extent) == (0, P, 2 * P, 4 * P, 2 * 4 * P + 3 * P)
        v = _hip.wide_frames_view(a4[:, :, 1:, 3:], 'chw', 'rgbx', **kw)
        assert (v.H, v.W, v.row_pitch, v.ptr, v.g_offset) == (H - 1, W - 3, W * ss, a4.ctypes.data + (W + 3) * ss, P)
        assert v.ptr % (2 * ss) == ss % (2 * ss)
        # channels last: 3 samples a pixel, 4, and a 3-channel view of 4
        h = np.zeros((n, H, W, 3), dt)
        v = _hip.wide_frames_view(h, 'hwc', 'rgb', **kw)
        assert (v.layout, v.pixel_format, v.row_pitch, v.frame_stride, v.extent) == (_hip.WIDE_PACKED, _hip.PIX_RGB, 3 * W * ss, 3 * P, n * 3 * P)
        h4 = np.zeros((n, H, W, 4), dt)
        assert _hip.wide_frames_view(h4, 'hwc', 'bgrx', **kw).pixel_format == _hip.PIX_BGRA
        v = _hip.wide_frames_view(h4[..., :3], 'hwc', 'rgb', **kw)
        assert (v.pixel_format, v.row_pitch, v.extent) == (_hip.PIX_RGBA, 4 * W * ss, n * 4 * P)
        v = _hip.wide_frames_view(h[:, 2:, 1:], 'hwc', 'bgr', **kw)
        assert (v.H, v.W, v.row_pitch, v.ptr) == (H - 2, W - 1, 3 * W * ss, h.ctypes.data + (2 * W + 1) * 3 * ss)
        d = v.descriptor()
        assert (d.sample_type, d.layout, d.pixel_format, d.n, d.H, d.W, d.reserved, d.reserved2, d.row_pitch) == (
            code, _hip.WIDE_PACKED, _hip.PIX_BGR, n, H - 2, W - 1, 0, 0, 3 * W * ss)
        # strides that do not fit: nothing is copied
        for bad in (a[:, :, :, ::2], a[:, :, ::-1], np.zeros((n, H, W, 3), dt).transpose(0, 3, 1, 2), a[:, [0, 0, 1]][:, :, :, :0:-1]):
            with pytest.raises(ValueError, match='do not fit melf_wide_frames'):
                _hip.wide_frames_view(bad, 'chw', 'rgb', **kw)
        with pytest.raises(ValueError, match='do not fit melf_wide_frames'):
            _hip.wide_frames_view(h[..., ::-1], 'hwc', 'rgb', **kw)
        with pytest.raises(ValueError, match='do not fit melf_wide_frames'):
            _hip.wide_frames_view(a.transpose(0, 2, 3, 1), 'hwc', 'rgb', **kw)
    f = np.zeros((2, 3, 4, 5), np.float32)
    # scale and offset: a scalar or three values in the order of channel_order -> B, G, R
    v = _hip.wide_frames_view(f, 'chw', 'rgb', scale=(1.0, 2.0, 3.0), offset=(4.0, 5.0, 6.0), rounding='floor')
    assert (v.scale, v.offset, v.rounding) == ((3.0, 2.0, 1.0), (6.0, 5.0, 4.0), _hip.ROUND_FLOOR)
    v = _hip.wide_frames_view(f, 'chw', 'gbr', scale=(1.0, 2.0, 3.0))
    assert (v.scale, v.offset, v.rounding) == ((2.0, 1.0, 3.0), (0.0, 0.0, 0.0), _hip.ROUND_NEAREST)
    assert _hip.wide_frames_view(f, 'chw').scale == (255.0, 255.0, 255.0)
    assert _hip.wide_frames_view(f, 'chw', scale=2).scale == (2.0, 2.0, 2.0)
    d = _hip.wide_frames_view(f, 'chw', 'bgr', scale=(1.0, 2.0, 3.0), offset=0.5).descriptor()
    assert (list(d.scale), list(d.offset)) == ([1.0, 2.0, 3.0], [0.5, 0.5, 0.5])
    u = np.zeros((2, 3, 4, 5), np.uint16)
    for (args, kw, msg) in (((f, 'nchw'), {}, 'layout'), ((f.astype(np.float64), 'chw'), {}, 'must be uint16, float16'),
                            ((f.view(np.int32), 'chw'), {}, 'must be uint16, float16'), ((u.view(np.int16), 'chw'), dict(shift=8), 'must be uint16, float16'),
                            ((f, 'chw', 'rgba'), {}, 'does not name the 3 channels'), ((f, 'hwc', 'gbr'), {}, 'is not one of'),
                            ((f[0], 'chw'), {}, r'must be \(N, C, H, W\)'), ((np.zeros((2, 4, 5, 2), np.float32), 'hwc'), {}, r'must be \(N, H, W, C\)'),
                            ((u, 'chw'), {}, 'integer frames need shift'), ((u, 'chw'), dict(shift=9), 'integer frames need shift'),
                            ((u, 'chw'), dict(shift=8, scale=2.0), 'take no scale'), ((u, 'chw'), dict(shift=8, rounding='floor'), 'take no scale'),
                            ((f, 'chw'), dict(shift=8), 'float frames take no shift'), ((f, 'chw'), dict(rounding='up'), 'rounding'),
                            ((f, 'chw'), dict(scale=(1.0, 2.0)), 'scalar or three'), ((f, 'chw'), dict(scale=np.inf), 'finite'),
                            ((f, 'chw'), dict(scale=2.0 ** 25), 'finite'), ((f, 'chw'), dict(offset=np.nan), 'finite')):
        with pytest.raises(ValueError, match=msg):
            _hip.wide_frames_view(*args, **kw)
    # the numpy statement of the rule the package carries equals the tests' reference
    x = np.linspace(-0.2, 1.2, 1001, dtype=np.float32)
    for (s, o, r) in wc.TRIPLES:
        assert np.array_equal(_hip.narrow_wide(x, s, o, r), wc.narrow_float(x, s, o, r))
    assert np.array_equal(_hip.narrow_wide(np.arange(65536, dtype=np.uint32).astype(np.uint16), shift=2), wc.narrow_u16(np.arange(65536), 2))


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def wide_buffer(samples, planar, order, type_, row_pad=0, stride_pad=0, gap=0, lead=0, rng=None):
    """samples: (n, H, W, C) (packed, order names the C samples of a pixel) or (n, 3, H, W) (planar, order names the planes) of the
    type's numpy dtype -> (buf, fields): a byte buffer of exactly the descriptor's extent -- rows row_pad, frames stride_pad and
    planes gap SAMPLES apart beyond their own, random filling; lead: the base is `lead` samples behind a 64-byte boundary -- and the
    geometry fields of a MelfWideFrames."""
    rng = rng if rng is not None else np.random.default_rng(0)
    ss = samples.dtype.itemsize
    assert samples.dtype == NP_DTYPE[type_]
    if planar:
        (n, _c, H, W) = samples.shape
        row = W * ss
    else:
        (n, H, W, ch) = samples.shape
        row = W * ch * ss
    rp = row + row_pad * ss
    span = (H - 1) * rp + row
    ps = span + gap * ss
    frame = 2 * ps + span if planar else span
    fs = frame + stride_pad * ss
    total = (n - 1) * fs + frame
    raw = rng.integers(0, 256, size=total + 128, dtype=np.uint8)
    start = -raw.ctypes.data % 64 + lead * ss
    buf = raw[start:start + total]
    assert buf.ctypes.data % 64 == lead * ss
    rows = np.ascontiguousarray(samples).view(np.uint8)
    off = {}
    for f in range(n):
        if planar:
            for (k, chn) in enumerate(order):
                np.lib.stride_tricks.as_strided(buf[f * fs + k * ps:], shape=(H, row), strides=(rp, 1))[...] = rows[f, k].reshape(H, row)
                off[chn] = k * ps
        else:
            np.lib.stride_tricks.as_strided(buf[f * fs:], shape=(H, row), strides=(rp, 1))[...] = rows[f].reshape(H, row)
    return buf, dict(layout=int(planar), pixel_format=0 if planar else PACKED_PIX[order], n=n, H=H, W=W, b_offset=off.get('b', 0),
                     g_offset=off.get('g', 0), r_offset=off.get('r', 0), row_pitch=rp, frame_stride=fs)


def descriptor(type_, geom, shift=0, scale=(255.0,) * 3, offset=(0.0,) * 3, rounding='nearest'):
    """scale / offset: B, G, R"""
    g = geom
    return _hip.MelfWideFrames(type_, g['layout'], g['pixel_format'], shift, ROUNDINGS[rounding], 0, (C.c_float * 3)(*scale), (C.c_float * 3)(*offset),
                               g['n'], g['H'], g['W'], 0, g['b_offset'], g['g_offset'], g['r_offset'], g['row_pitch'], g['frame_stride'])


def spread(values, npix):
    """values resized (repeated) to npix pixels"""
    return np.resize(np.asarray(values), npix)


PATTERN_SHAPE = (4, 32, 513)   # 65 664 pixels hold the 65 536 patterns; a packed row is 1539 or 2052 samples, a plane's 513: tails of 3, 4 and 1


def to_bgr_of(ctx, px, type_, planar, order, **rule):
    """px: (n, H, W) samples, the same in every channel of a pixel -> melf_wide_to_bgr of the frames in the layout"""
    (n, H, W) = px.shape
    ch = len(order)
    if planar:
        samples = np.ascontiguousarray(np.broadcast_to(px[:, None], (n, 3, H, W)))
    else:
        samples = np.ascontiguousarray(np.broadcast_to(px[..., None], (n, H, W, ch)))
        if ch == 4:   # the 4th sample: random bits, never converted
            ss = samples.dtype.itemsize
            alpha = np.random.default_rng(5).integers(0, 1 << (8 * ss), size=(n, H, W), dtype=np.uint64)
            samples[..., 3] = alpha.astype(np.uint16 if ss == 2 else np.uint32).view(samples.dtype)
    (buf, geom) = wide_buffer(samples, planar, order, type_, row_pad=1, stride_pad=3, gap=2, lead=1)
    return ctx.wide_to_bgr(buf.ctypes.data, descriptor(type_, geom, **rule))


@pytest.mark.gpu
@pytest.mark.parametrize('rounding', ['nearest', 'floor'])
@pytest.mark.parametrize('type_', [wc.F16, wc.BF16])
def test_device_narrowing_of_every_16_bit_float(env, type_, rounding):  # noqa: F811
    """melf_wide_to_bgr over all 65 536 patterns of the type, every pattern in every channel, the three (scale, offset) pairs of
    wide_cases.TRIPLES on B, G, R: byte for byte numpy's, packed (RGB, and BGRA with a random 4th sample) and planar.  A contracted
    multiply-add or a flushed denormal would show here."""
    ctx = env['sample-images1']['reader'].ctx
    bits = spread(np.arange(65536, dtype=np.uint32).astype(np.uint16), int(np.prod(PATTERN_SHAPE))).reshape(PATTERN_SHAPE)
    x32 = wc.widen(bits, type_)
    px = bits.view(np.float16) if type_ == wc.F16 else bits
    (scale, offset) = (tuple(t[0] for t in wc.TRIPLES), tuple(t[1] for t in wc.TRIPLES))
    want = np.stack([wc.narrow_float(x32, scale[k], offset[k], rounding) for k in range(3)], axis=-1)
    for (planar, order) in ((False, 'rgb'), (False, 'bgra'), (True, 'gbr')):
        got = to_bgr_of(ctx, px, type_, planar, order, scale=scale, offset=offset, rounding=rounding)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (planar, order, len(bad), bad[:5], [(hex(int(bits[tuple(b[:3])])), got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


@pytest.mark.gpu
def test_device_narrowing_of_every_16_bit_word(env):  # noqa: F811
    """melf_wide_to_bgr over all u16 values at shifts 0, 2, 4, 6 and 8: min(s >> shift, 255), packed and planar."""
    ctx = env['sample-images1']['reader'].ctx
    px = spread(np.arange(65536, dtype=np.uint32).astype(np.uint16), int(np.prod(PATTERN_SHAPE))).reshape(PATTERN_SHAPE)
    for shift in wc.SHIFTS:
        want = np.repeat(wc.narrow_u16(px, shift)[..., None], 3, axis=-1)
        for (planar, order) in ((False, 'bgr'), (False, 'rgba'), (True, 'rgb')):
            got = to_bgr_of(ctx, px, wc.U16, planar, order, shift=shift)
            assert np.array_equal(got, want), (shift, planar, order, int((got != want).sum()))


@pytest.mark.gpu
def test_device_narrowing_of_the_directed_float32_set(env):  # noqa: F811
    """melf_wide_to_bgr over wide_cases.f32_sets -- exact ties, the special values, and the values for which a fused multiply-add
    gives another byte -- laid out as small frames, packed and planar: byte for byte numpy's."""
    ctx = env['sample-images1']['reader'].ctx
    for (s, o, r, v) in wc.f32_sets():
        W = 37
        H = -(-len(v) // W)
        px = spread(v, H * W).reshape(1, H, W)
        want = np.repeat(wc.narrow_float(px, s, o, r)[..., None], 3, axis=-1)
        for (planar, order) in ((False, 'rgb'), (False, 'bgra'), (True, 'gbr')):
            got = to_bgr_of(ctx, px, wc.F32, planar, order, scale=(s,) * 3, offset=(o,) * 3, rounding=r)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (s, o, r, planar, order, len(bad), [(float(px[tuple(b[:3])]), got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


@pytest.fixture(scope='module')
def eight(env):  # noqa: F811
    frames = np.stack(env['sample-images1']['frames'][2:10])
    assert frames.shape == (8, 640, 480, 3)
    return frames


# (sample type, shift, the narrowed frame is the fixture's own)
TYPES = [(wc.U16, 0, True), (wc.U16, 8, True), (wc.F16, 0, True), (wc.F32, 0, True), (wc.BF16, 0, False)]
# Normalize(mean, std) of ImageNet, R G B: the frames hold (v / 255 - mean) / std, and scale = std * 255, offset = mean * 255 undo it
(MEAN, STD) = (np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225]))


def both_entry_points(reader, bgr8, type_, shift, exact, planar, order, row_pad=0, stride_pad=0, gap=0, lead=0, normalize=False, rounding='nearest'):
    """bgr8 expressed in the sample type and the layout, read with melf_process_wide and melf_process_wide_dev: both equal
    melf_process_frames / melf_process_planes on the numpy-narrowed frames, record for record; exact: and all frames read OK."""
    rng = np.random.default_rng(11)
    idx = ['bgr'.index(c) for c in order[:3]]
    chans = bgr8[..., idx]                                        # (n, H, W, 3) in the layout's channel order
    (scale, offset) = (np.full(3, 255.0), np.zeros(3))
    if normalize:
        rgb = ['rgb'.index(c) for c in order[:3]]
        (scale, offset) = (STD[rgb] * 255.0, MEAN[rgb] * 255.0)
    wide = wc.as_type(chans, type_, shift, scale, offset, rng)
    (scale32, offset32) = (scale.astype(np.float32), offset.astype(np.float32))
    narrowed = wc.narrowed(wide, type_, shift, scale32, offset32, rounding)
    if exact and not normalize:
        assert np.array_equal(narrowed, chans)
    if planar:
        samples = np.ascontiguousarray(wide.transpose(0, 3, 1, 2))
        want = reader.read_planar_frames(np.ascontiguousarray(narrowed.transpose(0, 3, 1, 2)), order)
    else:
        samples = wide
        narrowed8 = narrowed
        if len(order) == 4:
            alpha = rng.integers(0, 65536, size=wide.shape[:3] + (1,)).astype(np.uint16)
            samples = np.concatenate([wide, alpha.view(wide.dtype) if wide.dtype.itemsize == 2 else alpha.astype(np.float32)], axis=-1)
            narrowed8 = np.concatenate([narrowed, rng.integers(0, 256, size=alpha.shape, dtype=np.uint8)], axis=-1)
        want = reader.read_frame_views(np.ascontiguousarray(narrowed8), order)
    if exact:
        assert (want['status'] == _hip.FRAME_OK).all(), want['status']
    (buf, geom) = wide_buffer(np.ascontiguousarray(samples), planar, order, type_, row_pad, stride_pad, gap, lead, rng)
    by_bgr = [order.index(c) for c in 'bgr']
    desc = descriptor(type_, geom, shift, tuple(scale32[by_bgr]), tuple(offset32[by_bgr]), rounding)
    got = reader.ctx.process_wide(buf.ctypes.data, desc)
    assert got.tobytes() == want.tobytes(), ('host', type_, shift, order)
    dev = fc.DevBuf.at_end(buf.ctypes.data, buf.nbytes, phase=2 if lead and samples.dtype.itemsize == 2 else 0)
    try:
        got = reader.ctx.process_wide_dev(dev.d.value, desc)
    finally:
        dev.free()
    assert got.tobytes() == want.tobytes(), ('dev', type_, shift, order)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('type_,shift,exact', TYPES, ids=['u16>>0', 'u16>>8', 'f16', 'f32', 'bf16'])
def test_records_through_both_entry_points(env, eight, type_, shift, exact):  # noqa: F811
    """Eight fixture frames in the sample type: packed RGB, BGR and RGBA, planar in G B R order, a padded pitch and stride at a base
    with the sample's own alignment only, and a Normalize-style scale / offset (the float types)."""
    reader = env['sample-images1']['reader']
    both_entry_points(reader, eight, type_, shift, exact, False, 'rgb')
    both_entry_points(reader, eight, type_, shift, exact, False, 'bgr', row_pad=3, stride_pad=5, lead=1)
    both_entry_points(reader, eight, type_, shift, exact, False, 'rgba', row_pad=1, lead=1)
    both_entry_points(reader, eight, type_, shift, exact, True, 'gbr')
    both_entry_points(reader, eight, type_, shift, exact, True, 'gbr', row_pad=7, stride_pad=1, gap=3, lead=1)
    if type_ != wc.U16:
        both_entry_points(reader, eight, type_, shift, exact, False, 'rgb', normalize=True)
        both_entry_points(reader, eight, type_, shift, exact, True, 'rgb', normalize=True, lead=1)
        both_entry_points(reader, eight, type_, shift, False, False, 'bgr', rounding='floor')


@pytest.mark.gpu
def test_meter_rect_clamped_at_the_frame_edge(env, eight, tmp_path):  # noqa: F811
    """meter_rect (50, 160)-(1000, 1000) on 480 x 640 frames: the crop is clamped to the frame's right and bottom edges, its last
    row and column the frame's own."""
    from meterelf_amd import MeterReader
    r = MeterReader(fc.params_with_rect(tmp_path, 'sample-images1', (50, 160, 1000, 1000), 'edge'))
    try:
        for (type_, shift, exact) in TYPES:
            both_entry_points(r, eight, type_, shift, exact, False, 'rgb', lead=1)
            both_entry_points(r, eight, type_, shift, exact, True, 'gbr', row_pad=1, lead=1)
    finally:
        r.close()


@pytest.mark.gpu
def test_the_narrowing_is_timed_as_the_gather(env, eight):  # noqa: F811
    """melf_ctx_timings: a wide call launches exactly one MELF_K_GATHER kernel per chunk of 1024 frames -- one for eight frames, two
    for 1025 --, and melf_ctx_last_dials reports the family of the 8-bit frames the staged batch is: packed3 / packed4 / bgr for
    'views', planar."""
    ctx = env['sample-images1']['reader'].ctx
    cut = np.ascontiguousarray(eight[:, :412, :302])   # the frames' top-left part that holds meter_rect (50, 160)-(300, 410)
    try:
        ctx.set_profiling(1)
        for (planar, order, family) in ((False, 'rgb', 'packed3'), (False, 'bgr', 'bgr'), (False, 'rgba', 'packed4'), (True, 'gbr', 'planar')):
            idx = ['bgr'.index(c) for c in order[:3]]
            chans = cut[..., idx]
            if len(order) == 4:
                chans = np.concatenate([chans, chans[..., :1]], axis=-1)
            samples = np.ascontiguousarray((chans.transpose(0, 3, 1, 2) if planar else chans).astype(np.float32) / np.float32(255))
            (buf, geom) = wide_buffer(samples, planar, order, wc.F32)
            dev = fc.DevBuf(buf.ctypes.data, buf.nbytes)
            try:
                ctx.timings()
                got = ctx.process_wide_dev(dev.d.value, descriptor(wc.F32, geom))
                t = ctx.timings()
            finally:
                dev.free()
            assert t['k_gather'][1] == 1 and t['k_gather'][0] > 0 and t['k_dials'][1] == 1, (order, t)
            assert ctx.last_dials()['family'] == family, (order, ctx.last_dials())
            assert (got['status'] == _hip.FRAME_OK).all()
        want8 = got
        n = 1025
        many = np.tile(cut.transpose(0, 3, 1, 2)[:, [1, 0, 2]].astype(np.uint16) << np.uint16(4), (-(-n // 8), 1, 1, 1))[:n]   # G, B, R planes
        P = 412 * 302 * 2
        geom = dict(layout=1, pixel_format=0, n=n, H=412, W=302, g_offset=0, b_offset=P, r_offset=2 * P, row_pitch=302 * 2, frame_stride=3 * P)
        assert many.flags.c_contiguous and many.nbytes == n * 3 * P
        dev = fc.DevBuf(many.ctypes.data, many.nbytes)
        try:
            ctx.timings()
            got = ctx.process_wide_dev(dev.d.value, descriptor(wc.U16, geom, shift=4))
            t = ctx.timings()
        finally:
            dev.free()
        assert t['k_gather'][1] == 2 and t['k_dials'][1] == 2, t
        assert got.tobytes() == np.tile(want8, -(-n // 8))[:n].tobytes()
    finally:
        ctx.set_profiling(0)


@pytest.mark.gpu
def test_rejected_descriptors_launch_nothing(env, eight):  # noqa: F811
    """MELF_ERR_INVALID with the check's message from all three entry points, before anything is launched; n == 0 passes."""
    ctx = env['sample-images1']['reader'].ctx
    samples = eight[:2].astype(np.float32)
    (buf, geom) = wide_buffer(samples, False, 'bgr', wc.F32)
    ctx.set_profiling(1)
    try:
        before = fc.launch_counts(ctx)
        for (change, msg) in ((dict(row_pitch=geom['row_pitch'] + 2), 'multiples of the sample size'), (dict(frame_stride=4), 'smaller than a frame'),
                              (dict(pixel_format=7), 'unknown pixel_format'), (dict(H=0), 'bad batch shape')):
            d = descriptor(wc.F32, dict(geom, **change))
            for call in (lambda: ctx.process_wide(buf.ctypes.data, d), lambda: ctx.process_wide_dev(buf.ctypes.data, d),
                         lambda: ctx.wide_to_bgr(buf.ctypes.data, d)):
                with pytest.raises(_hip.HipError, match=msg):
                    call()
        for call in (lambda d: ctx.process_wide(buf.ctypes.data + 2, d), lambda d: ctx.process_wide_dev(buf.ctypes.data + 2, d)):
            with pytest.raises(_hip.HipError, match='multiple of the sample size'):
                call(descriptor(wc.F32, geom))
        with pytest.raises(_hip.HipError, match='finite'):
            ctx.process_wide(buf.ctypes.data, descriptor(wc.F32, geom, scale=(1.0, float('inf'), 1.0)))
        assert len(ctx.process_wide(0, descriptor(wc.F32, dict(geom, n=0)))) == 0
        assert fc.launch_counts(ctx) == before
    finally:
        ctx.set_profiling(0)


@pytest.mark.gpu
def test_read_wide_frames_in_a_torch_process():
    """MeterReader.read_wide_frames with torch tensors on the reader's GPU -- float16, bfloat16, float32, (N, 3, H, W) and (N, H, W, 3),
    a channel slice of 4 channels, a spatial-crop view, a non-default current stream with out= -- in a child process that imports
    torch first (tests/frame_cases.py says why)."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'wide_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch wide path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
