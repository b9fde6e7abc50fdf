"""Support for tests/test_wide_list.py, tests/wide_list_torch_child.py and tools' tests (melf_process_wide_list*,
melf_process_wide_plane_list*, melf_wide_list_to_bgr): the shape sweep of the list kernels, samples with the values a conversion can
get wrong at the places an address can get wrong, frames and planes as separate arrays of exactly their readable extent, and the
fixture frames as a wide batch, a list of frames and a list of planes holding the same samples.  tests/wide_cases.py restates the
narrowing rule: the reference of every comparison."""
import ctypes as C
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import wide_cases as wc  # noqa: E402

NP_DTYPE = {wc.U16: np.uint16, wc.F16: np.float16, wc.BF16: np.uint16, wc.F32: np.float32}   # bf16 travels as its bits
PACKED_PIX = {'bgr': _hip.PIX_BGR, 'rgb': _hip.PIX_RGB, 'bgra': _hip.PIX_BGRA, 'rgba': _hip.PIX_RGBA}
ROUNDINGS = {'nearest': 0, 'floor': 1}

# (planar, channel order, H, W, row padding in samples).  H: one row, exactly one wave's rows (gather::ROWS_PER_WAVE = 8), one more,
# three blocks.  W: a tail-only row; 15 samples (packed-3 W = 5, planar W = 15); whole pieces with no tail (packed-3 and packed-4
# W = 16, planar 16 and 32); whole pieces and a 15-sample tail (packed-3 W = 37); more than 64 pieces in a wave's block (W = 400).
FORMS = ((False, 'bgr'), (False, 'rgb'), (False, 'bgra'), (False, 'rgba'), (True, 'gbr'))
SHAPES = [(planar, order, H, W, pad) for (planar, order) in FORMS for H in (1, 8, 9, 17) for W in (1, 5, 15, 16, 32, 37, 400) for pad in (0, 3)]


def rules(type_):
    """the narrowing rules of the stage-parity sweep; scale / offset: B, G, R"""
    if type_ == wc.U16:
        return [dict(shift=0), dict(shift=8)]
    out = [dict(scale=(s,) * 3, offset=(o,) * 3, rounding=r) for (s, o, r) in wc.TRIPLES]
    out.append(dict(scale=tuple(t[0] for t in wc.TRIPLES), offset=tuple(t[1] for t in wc.TRIPLES), rounding='nearest'))   # one triple per channel
    return out


def _bits(type_, values):
    """float values -> samples of the type (bf16: its bits)"""
    v = np.asarray(values, np.float32)
    if type_ == wc.F32:
        return v
    if type_ == wc.F16:
        with np.errstate(over='ignore'):
            return v.astype(np.float16)
    return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)   # (the specials below are exact in bfloat16)


def random_samples(type_, planar, ch, n, H, W, rng):
    """(n, H, W, ch) or (n, 3, H, W) samples of the type: u16: any word.  Floats: finite values around [0, 1] -- and NaN, +inf,
    -inf and a negative number in the first and last sample of a row and in the row's tail piece (its last 1 .. 15 samples)."""
    shape = (n, 3, H, W) if planar else (n, H, W, ch)
    if type_ == wc.U16:
        return rng.integers(0, 65536, size=shape, dtype=np.uint16)
    x = wc.as_type(rng.uniform(-0.25, 1.25, size=shape) * 255.0, type_)
    rows = x.reshape(n, 3 * H, W) if planar else x.reshape(n, H, W * ch)   # rows of samples as a row run has them
    L = rows.shape[2]
    special = _bits(type_, [np.nan, np.inf, -np.inf, -3.0])
    tail0 = L - (L % 16 or 16)   # the first sample of the row's last piece
    for (k, at) in enumerate((0, L - 1, tail0, max(tail0, L - 2))):
        rows[:, k % rows.shape[1]::3, at] = special[k]
    rows[:, -1, L - 1] = special[0]
    rows[:, 0, 0] = special[2]
    return x


def _lay_rows(dst, rows, rp):
    """rows (H, row bytes) into the byte array dst at a pitch of rp bytes"""
    (H, row) = rows.shape
    np.lib.stride_tricks.as_strided(dst, shape=(H, row), strides=(rp, 1))[...] = rows


def separate(samples, planar, order, type_, pad, gap=2, rng=None):
    """samples of random_samples' shapes -> (frames, planes, geom): per frame a uint8 array of exactly one frame's extent (rows pad
    samples longer than their own; planar: the planes in the order `order`, gap samples between them), per frame its [B, G, R]
    planes as uint8 arrays of exactly (H - 1) * row_pitch + W * sample size bytes (planar only), and the geometry fields of a
    MelfWideFrames of the frames (frame_stride 0: not looked at by the lists)."""
    rng = rng if rng is not None else np.random.default_rng(0)
    ss = samples.dtype.itemsize
    assert samples.dtype == NP_DTYPE[type_]
    raw = np.ascontiguousarray(samples).view(np.uint8)
    if planar:
        (n, _c, H, W) = samples.shape
        row = W * ss
    else:
        (n, H, W, ch) = samples.shape
        row = W * ch * ss
    rp = row + pad * ss
    span = (H - 1) * rp + row
    ps = span + gap * ss
    extent = 2 * ps + span if planar else span
    (frames, planes, off) = ([], [], {})
    for f in range(n):
        buf = rng.integers(0, 256, size=extent, dtype=np.uint8)
        if planar:
            own = {}
            for (k, chn) in enumerate(order):
                _lay_rows(buf[k * ps:], raw[f, k].reshape(H, row), rp)
                off[chn] = k * ps
                own[chn] = buf[k * ps:k * ps + span].copy()
            planes.append([own[c] for c in 'bgr'])
        else:
            _lay_rows(buf, raw[f].reshape(H, row), rp)
        frames.append(buf)
    geom = dict(layout=int(planar), pixel_format=0 if planar else PACKED_PIX[order], n=n, H=H, W=W, b_offset=off.get('b', 0),
                g_offset=off.get('g', 0), r_offset=off.get('r', 0), row_pitch=rp, frame_stride=0)
    return frames, planes, geom


def descriptor(type_, geom, rule):
    g = geom
    return _hip.MelfWideFrames(type_, g['layout'], g['pixel_format'], rule.get('shift', 0), ROUNDINGS[rule.get('rounding', 'nearest')], 0,
                               (C.c_float * 3)(*rule.get('scale', (255.0,) * 3)), (C.c_float * 3)(*rule.get('offset', (0.0,) * 3)),
                               g['n'], g['H'], g['W'], 0, g['b_offset'], g['g_offset'], g['r_offset'], g['row_pitch'], g['frame_stride'])


def narrowed_bgr(samples, planar, order, type_, rule):
    """(n, H, W, 3) BGR bytes: numpy's narrowing of the samples under the rule (scale / offset of B, G, R)"""
    out = []
    for (k, c) in enumerate('bgr'):
        x = samples[:, order.index(c)] if planar else samples[..., order.index(c)]
        out.append(wc.narrowed(x, type_, rule.get('shift', 0), np.float32(rule.get('scale', (255.0,) * 3)[k]),
                               np.float32(rule.get('offset', (0.0,) * 3)[k]), rule.get('rounding', 'nearest')))
    return np.stack(out, axis=-1)


def with_n(desc, n):
    return changed(desc, n=n)


def changed(desc, **fields):
    d = _hip.MelfWideFrames.from_buffer_copy(desc)
    for (k, v) in fields.items():
        setattr(d, k, v)
    return d


def fixture_case(bgr8, type_, shift, planar, row_pad=1, stride_pad=3):
    """BGR uint8 frames (n, H, W, 3) as wide frames of the type that narrow back to them (wide_cases.as_type), packed in R G B
    order or planar in G B R order -> a namespace: buf / desc: one contiguous batch (rows row_pad, frames stride_pad samples
    apart beyond their own) and its descriptor; view: what frame_list_cases.DevFrames needs of it; list_desc, host_frames: the
    same frames one array each, of exactly a frame's extent; plane_desc, host_planes: per frame its [B, G, R] planes, one array
    each of exactly a plane's extent (planar)."""
    order = 'gbr' if planar else 'rgb'
    idx = ['bgr'.index(c) for c in order]
    wide = wc.as_type(bgr8[..., idx], type_, shift, rng=np.random.default_rng(17))
    rule = dict(shift=shift) if type_ == wc.U16 else {}
    samples = np.ascontiguousarray(wide.transpose(0, 3, 1, 2)) if planar else wide
    (frames, planes, geom) = separate(samples, planar, order, type_, row_pad)
    ss = samples.dtype.itemsize
    n = len(frames)
    extent = frames[0].nbytes
    fs = extent + stride_pad * ss
    raw = np.zeros((n - 1) * fs + extent + 128, np.uint8)
    start = -raw.ctypes.data % 64 + ss   # the base: one sample behind a 64-byte boundary
    buf = raw[start:start + (n - 1) * fs + extent]
    for (i, f) in enumerate(frames):
        buf[i * fs:i * fs + extent] = f
    desc = descriptor(type_, dict(geom, frame_stride=fs), rule)
    return types.SimpleNamespace(
        buf=buf, desc=desc, ss=ss, n=n, view=types.SimpleNamespace(ptr=buf.ctypes.data, n=n, frame_stride=fs, extent=buf.nbytes),
        list_desc=descriptor(type_, geom, rule), host_frames=frames,
        plane_desc=descriptor(type_, dict(geom, b_offset=0, g_offset=0, r_offset=0), rule) if planar else None, host_planes=planes)
