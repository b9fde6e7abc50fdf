"""What the tests of the wide RGB frames (test_wide_narrow, test_wide_frames, wide_torch_child) share: the narrowing rule restated
in numpy -- the reference of every comparison --, the pattern sets (every 16-bit pattern of f16, bf16 and u16, and a directed float32
set), the builder of the stand-alone host programs, and the fixture frames expressed in each sample type.

The rule (include/meterelf_hip.h): u16: min(s >> shift, 255).  f16 / bf16 / f32: x widened to float32 (exact), t = x * scale
rounded to float32, q = t + offset rounded to float32 -- two roundings, never a fused multiply-add --, r = rint(q) (ties to even)
or floor(q); NaN or r < 0 -> 0, r > 255 -> 255."""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

(U16, F16, BF16, F32) = (0, 1, 2, 3)
TYPE_NAMES = {U16: 'u16', F16: 'f16', BF16: 'bf16', F32: 'f32'}
SHIFTS = (0, 2, 4, 6, 8)
# (scale, offset, rounding): the default; torchvision's convert_image_dtype; an ImageNet Normalize undone (std * 255, mean * 255)
TRIPLES = ((255.0, 0.0, 'nearest'), (255.999, 0.0, 'floor'), (58.395, 123.675, 'nearest'))
FUSE = (58.395, 123.675)   # the scale and offset of the non-fusion search


def widen(bits, type_):
    """uint16 patterns of f16 / bf16 -> the float32 values they stand for (exact)"""
    bits = np.asarray(bits, np.uint16)
    if type_ == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow_float(x32, scale, offset, rounding):
    """THE reference: float32 x * s, then + o, np.rint / np.floor, NaN to 0, clip.  scale / offset broadcast."""
    x32 = np.asarray(x32)
    assert x32.dtype == np.float32
    with np.errstate(all='ignore'):
        t = x32 * np.asarray(scale, np.float32)
        assert t.dtype == np.float32
        q = t + np.asarray(offset, np.float32)
        assert q.dtype == np.float32
        r = np.floor(q) if rounding == 'floor' else np.rint(q)
        return np.clip(np.where(np.isnan(r), np.float32(0), r), 0, 255).astype(np.uint8)


def narrow_u16(s, shift):
    return np.minimum(np.asarray(s, np.uint16) >> np.uint16(shift), np.uint16(255)).astype(np.uint8)


def fused_byte(x32, scale, offset, rounding):
    """What a fused multiply-add would give: the product exact (float64 holds it), one rounding to float32 after the sum."""
    with np.errstate(all='ignore'):
        q = (x32.astype(np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(offset))).astype(np.float32)
        r = np.floor(q) if rounding == 'floor' else np.rint(q)
        return np.clip(np.where(np.isnan(r), np.float32(0), r), 0, 255).astype(np.uint8)


def ulp_neighbours(x32, k=64):
    """the float32 values within k ulps of each x (x finite, away from 0)"""
    bits = np.asarray(x32, np.float32).view(np.int32)[:, None] + np.arange(-k, k + 1, dtype=np.int32)[None, :]
    return np.unique(bits.reshape(-1)).view(np.float32)


def non_fusion_values(rounding):
    """float32 x around every rounding boundary of x * 58.395 + 123.675 -- q = k + 0.5 under 'nearest', q = k under 'floor' -- for
    which fused arithmetic gives another byte than the two-rounding rule."""
    (s, o) = FUSE
    k = np.arange(0, 256, dtype=np.float64)
    bound = k + 0.5 if rounding == 'nearest' else k
    x0 = ((bound - o) / s).astype(np.float32)
    x0 = x0[np.abs(x0) > 1e-3]
    cand = ulp_neighbours(x0)
    return cand[narrow_float(cand, s, o, rounding) != fused_byte(cand, s, o, rounding)]


def f32_sets():
    """[(scale, offset, rounding, float32 values)]: exact ties at scale 1, the special values, and the non-fusion sets (at least 64
    values each, asserted: the condition is a property of the reference alone)."""
    ties = (np.arange(-3, 259, dtype=np.float32) + np.float32(0.5))
    specials = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, 0.9999999,
                         1.0000001, 3.4028235e38, -3.4028235e38, 0.5, 254.5 / 255.0, 255.5 / 255.0, 0.00196078431, 2.0 ** -25],
                        dtype=np.float32)
    sets = [(1.0, 0.0, 'nearest', ties), (1.0, 0.0, 'floor', ties), (1.0, 0.5, 'nearest', ties), (-1.0, 255.0, 'nearest', ties)]
    for (s, o, r) in TRIPLES:
        sets.append((s, o, r, specials))
    sets.append((16777216.0, 0.0, 'nearest', specials))
    sets.append((-16777216.0, 3.0e38, 'floor', specials))
    for rounding in ('nearest', 'floor'):
        v = non_fusion_values(rounding)
        assert len(v) >= 64, (rounding, len(v))
        sets.append(FUSE + (rounding, v))
    return sets


def build(tmp_path, name, san=('-fsanitize=address,undefined',)):
    """tests/<name>.cpp as a stand-alone program under the host sanitizers -> its path"""
    exe = str(tmp_path / name)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-std=c++17', '-Wall', '-Werror', '-O1', '-g', '-fno-sanitize-recover=all'] + list(san)
                          + ['-o', exe, os.path.join(ROOT, 'tests', name + '.cpp')])
    return exe


def run(cmd):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, (cmd, p.stdout[-2000:], p.stderr[-4000:])
    out = p.stdout.decode()
    assert out.splitlines()[-1] == 'failures 0', out[-2000:]
    return out


def pattern_record(type_, arg, scale, offset, rounding, count):
    return struct.pack('<iiffii', type_, arg, scale, offset, int(rounding == 'floor'), count)


# ---------------------------------------------------------------------------------------------- frames of the fixture ---
def as_type(frames8, type_, shift=0, scale=255.0, offset=0.0, rng=None):
    """uint8 frames -> an array of the sample type that narrows back to them: u16: v << shift plus random low bits; float: the
    float64 (v - offset) / scale rounded to the type (the caller asserts the round trip where it claims one).  bf16: uint16 bits."""
    v = frames8.astype(np.float64)
    if type_ == U16:
        low = rng.integers(0, 1 << shift, size=frames8.shape, dtype=np.uint16) if (rng is not None and shift) else np.uint16(0)
        return (frames8.astype(np.uint16) << np.uint16(shift)) | low
    x = (v - np.asarray(offset, np.float64)) / np.asarray(scale, np.float64)
    if type_ == F16:
        return x.astype(np.float16)
    x32 = x.astype(np.float32)
    if type_ == F32:
        return x32
    b = x32.view(np.uint32)
    return ((b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)   # round to nearest even


def narrowed(arr, type_, shift=0, scale=255.0, offset=0.0, rounding='nearest'):
    """the bytes the library reads an array of as_type's kind as"""
    if type_ == U16:
        return narrow_u16(arr, shift)
    x32 = widen(arr, BF16) if type_ == BF16 else np.asarray(arr).astype(np.float32)
    return narrow_float(x32, scale, offset, rounding)
