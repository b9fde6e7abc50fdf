"""Support for tests/test_oriented.py (melf_process_oriented*, melf_orient_frames, MeterReader.read_oriented_frames): the orientation
table as a numpy function, and -- generic over the six families that can be oriented -- the planes of a batch from its descriptor,
a descriptor of the same format for other dimensions and pitches, and the stored batch whose oriented frames are a given upright
batch.  New support lives here; tests/frame_cases.py and tests/frame_list_cases.py are used as they are."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402

CODES = tuple(range(1, 9))
INVERSE = {6: 8, 8: 6}   # every other code is its own inverse
FAMILIES = ('views', 'yuv', 'yuv_planar', 'yuv16', 'packed32', 'planar')   # read_frame_list's names of the six families


def orient(a, code, axes=(0, 1)):
    """The oriented frame O of the stored frame a (rows and columns on `axes`): the table of include/meterelf_hip.h.
    1 O[y][x] = S[y][x]; 2 S[y][W-1-x]; 3 S[H-1-y][W-1-x]; 4 S[H-1-y][x]; 5 S[x][y]; 6 S[H-1-x][y]; 7 S[H-1-x][W-1-y]; 8 S[x][W-1-y]."""
    (r, c) = axes
    a = np.asarray(a)
    if code in (3, 4, 6, 7):   # the stored row index runs backwards
        a = np.flip(a, r)
    if code in (2, 3, 7, 8):   # the stored column index runs backwards
        a = np.flip(a, c)
    return np.swapaxes(a, r, c) if code >= 5 else a


def inverse(code):
    return INVERSE.get(code, code)


# ------------------------------------------------------------------------------------------- planes of a described batch ---
def plane_table(family, d):
    """The planes of one frame of descriptor d, in slot order (the one packed plane; B, G, R; Y, U, V; Y, the interleaved pairs):
    (offset, rows, elements per row, bytes per element, pitch, the descriptor's offset fields that lie in the plane)."""
    if family in ('views', 'packed32'):
        eb = 4 if family == 'packed32' else _hip.PIX_BYTES[d.pixel_format]
        return [(0, d.H, d.W, eb, d.row_pitch, ())]
    if family == 'planar':
        return [(getattr(d, f), d.H, d.W, 1, d.row_pitch, (f,)) for f in ('b_offset', 'g_offset', 'r_offset')]
    bps = 2 if family == 'yuv16' else 1
    if family == 'yuv':
        (sx, sy, semi) = (1, 1, d.format == _hip.YUV_NV12)
    elif family == 'yuv_planar':
        (sx, sy, semi) = (d.sub_x, d.sub_y, d.c_step == 2)
    else:
        (sx, sy, semi) = (1, d.sub_y, d.c_step == 2)
    (ch, cw) = (d.H >> sy, d.W >> sx)
    planes = [(0, d.H, d.W, bps, d.y_pitch, ())]
    if semi:
        return planes + [(min(d.u_offset, d.v_offset), ch, cw, 2 * bps, d.c_pitch, ('u_offset', 'v_offset'))]
    return planes + [(d.u_offset, ch, cw, bps, d.c_pitch, ('u_offset',)), (d.v_offset, ch, cw, bps, d.c_pitch, ('v_offset',))]


def align_of(family, d):
    """what the family's check wants the base, the pitches and the stride to be multiples of"""
    return 4 if family == 'packed32' or (family == 'views' and _hip.PIX_BYTES[d.pixel_format] == 4) else (2 if family == 'yuv16' else 1)


def frame_extent(family, d):
    return max(off + (rows - 1) * pitch + cols * eb for (off, rows, cols, eb, pitch, _f) in plane_table(family, d))


def batch_extent(family, d):
    return (d.n - 1) * d.frame_stride + frame_extent(family, d)


def copy_desc(d):
    return type(d).from_buffer_copy(d)


def relayout(family, d, H, W, pad=0):
    """A descriptor of the same format, plane order and n as d for frames of H x W: pad 0: every plane tight, the planes back to
    back in d's memory order; pad k > 0: rows, planes and frames k * (5, 7, 9 ..) * the family's alignment apart from tight."""
    a = align_of(family, d)
    new = copy_desc(d)
    (new.H, new.W) = (H, W)
    old = plane_table(family, d)
    planes = plane_table(family, new)   # the new geometry (offsets and pitches still the old ones)
    pitch_field = 'row_pitch' if family in ('views', 'packed32', 'planar') else None
    pitches = []
    for (k, (_off, _rows, cols, eb, _pitch, _f)) in enumerate(planes):
        extra = pad * (5 + 2 * min(k, 1)) * a   # U and V share one pitch field
        pitches.append(cols * eb + extra)
    if pitch_field:
        pitches = [max(pitches)] * len(planes)   # B, G and R share theirs
        setattr(new, pitch_field, pitches[0])
    else:
        (new.y_pitch, new.c_pitch) = (pitches[0], pitches[1])
    at = pad * a   # planar RGB may start behind the frame's first byte; Y and the packed plane are at 0
    for k in sorted(range(len(planes)), key=lambda k: old[k][0]):
        (off, rows, cols, eb, _pitch, fields) = planes[k]
        if not fields:
            at = 0
        for f in fields:
            setattr(new, f, at + (getattr(d, f) - old[k][0]))   # an interleaved pair keeps which sample comes first
        at += (rows - 1) * pitches[k] + cols * eb + pad * 3 * a
        at += -at % max(a, 2)                                   # NV12's pairs start on an even offset
    new.frame_stride = at + pad * 7 * a
    new.frame_stride += -new.frame_stride % max(a, 1)
    return new


def plane_views(buf, family, d):
    """The planes of every frame of the batch in buf (a uint8 array of batch_extent bytes), slot order: views (n, rows, cols, eb)."""
    out = []
    for (off, rows, cols, eb, pitch, _f) in plane_table(family, d):
        out.append(np.lib.stride_tricks.as_strided(buf[off:], shape=(d.n, rows, cols, eb), strides=(d.frame_stride, pitch, eb, 1)))
    return out


def pack(family, d, planes, rng=None):
    """A uint8 buffer of exactly batch_extent(d) bytes holding `planes` (slot order, (n, rows, cols, eb)) as d describes them; what
    lies between rows, planes and frames is random (rng) or zero."""
    n = batch_extent(family, d)
    buf = rng.integers(0, 256, n, dtype=np.uint8) if rng is not None else np.zeros(n, np.uint8)
    for (dst, src) in zip(plane_views(buf, family, d), planes):
        dst[...] = src
    return buf


def as_buffer(v):
    """the bytes of a *FramesView's batch"""
    return np.frombuffer((C.c_uint8 * v.extent).from_address(v.ptr), np.uint8)


def stored_batch(family, d_up, up_buf, code, pad=0, rng=None):
    """(descriptor, buffer) of the STORED batch whose frames, oriented by `code`, are the upright batch (d_up, up_buf): every plane
    of the upright batch under the inverse orientation, in the same format."""
    (H, W) = (d_up.W, d_up.H) if code >= 5 else (d_up.H, d_up.W)
    d = relayout(family, d_up, H, W, pad)
    planes = [orient(p, inverse(code), axes=(1, 2)) for p in plane_views(up_buf, family, d_up)]
    return d, pack(family, d, planes, rng)


def tight_oriented(family, d, buf, code):
    """What melf_orient_frames returns for the stored batch (d, buf): per frame the oriented planes, tight, in slot order."""
    planes = [orient(p, code, axes=(1, 2)).reshape(d.n, -1) for p in plane_views(buf, family, d)]
    return np.ascontiguousarray(np.concatenate(planes, axis=1)).reshape(-1)
