"""The dial reader's two kernel families of the 32-bit packed 4:4:4 frames (k_p32_needle<YUV, NR>, melf_process_packed32*): every
instantiation production can pick, launched, ASSERTED to be the one that ran (melf_ctx_last_dials) and compared, the way
tests/test_yuv422_10_dials.py does it for the packed 10-bit 4:2:2 frames -- with the contexts, frames and edge scenes of
tests/test_dials_instantiations.py (imported, not copied).

Two families times six row counts NR: 12 kernels.  The sweep runs both at the eleven contexts whose largest dial has R = 13 .. 29,
both ends of every NR class: 'y410' and 'vuya' for the YUV family, 'x2rgb10' for the RGB family.  The phase cases move the crop's x
origin through four consecutive columns, so that a lane's quad -- four words, one 16-byte load from a 4-byte aligned address -- starts
at every word phase modulo 16 bytes, with the frame cut to w0, w0 + 1, w0 + 2 and w0 + 3 columns (W need not be even here, which is
new for a YUV family: the crop's right edge lies on the frame's last column, then one, two and three short of it); the edge scenes put
dial windows at the dials crop's first and last columns ('leave': outside, the exact path; 'flush': the last quad ends on the
template's last column) and the match on crop columns 0 and 1.  Expected records: the existing paths' (read_yuv_planar_frames of the
8-bit i444 frames, read_frames of the BGR frames), byte for byte.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import p32_cases as pc  # noqa: E402
from tests import test_dials_instantiations as di  # noqa: E402

FAMILIES32 = ('p32yuv', 'p32rgb')
CASES = (('y410', 'p32yuv'), ('vuya', 'p32yuv'), ('x2rgb10', 'p32rgb'))   # the formats compared, and the family each runs
ALL_PAIRS32 = frozenset((f, nr) for f in FAMILIES32 for nr in (32, 40, 48, 52, 56, 64))
SEEN32 = set()     # (family, NR) pairs this module launched and asserted
_SWEPT32 = {}
PHASE_X0S = tuple(range(di.RECT_X0, di.RECT_X0 + 4))


def quad_phase(data, dial, match_x):
    """Restated from DialWord32::window and DialFrame::pieces_inside: (the quads lie inside the crop's columns, the word phase
    modulo 4 words = 16 bytes of every lane's first pixel in its row -- the lanes are four pixels apart, so they share it)."""
    nd = data['needle_data'][dial]
    tw = data['dials_template_size'][0]
    x0 = data['meter_rect']['top_left'][0]
    R = di.dial_radius(nd)
    (wx0, ws) = (di.py_round(nd['center'][0]) - R - 2, 2 * R + 5)
    n = (ws + 3) >> 2
    inside = wx0 >= 0 and wx0 + 4 * n <= tw
    return inside, (x0 + match_x + wx0) % 4, wx0 + 4 * n == tw


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_family_names_and_codes():
    assert _hip.DIALS32_FAMILIES == FAMILIES32
    assert tuple(_hip.DIALS_FAMILIES) == di.FAMILIES            # the twelve stay the twelve
    import re
    with open(os.path.join(ROOT, 'include', 'meterelf_hip.h')) as fp:
        text = fp.read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r'\bMELF_DIALS32_([A-Z0-9_]+) = (\d+)', text)}
    assert values == {'YUV': 16, 'RGB': 17}
    assert {(f, nr) for f in FAMILIES32 for nr in di.NR_CLASSES} == ALL_PAIRS32 and len(ALL_PAIRS32) == 12
    assert (_hip.DIALS_FAMILIES + _hip.DIALS16_FAMILIES + _hip.DIALS10_FAMILIES + _hip.DIALS32_FAMILIES).index('p32yuv') == 16


def test_phase_cases_meet_quads_on_and_off_and_every_phase():
    """Over the four crop origins of the phase cases and the two match columns, the windows whose quads are used start at every
    word phase modulo 16 bytes -- for every dial that has such windows at all --, 'flush' has a window whose last quad ends on the
    template's last column, and 'leave' has windows outside the crop's columns (quads off: the exact path) at every origin."""
    phases = set()
    for x0 in PHASE_X0S:
        flush = False
        for dial in range(4):
            for mx in di.edge_match_x(1):
                (inside, ph, ends) = quad_phase(di.edge_data('flush', 1, x0), dial, mx)
                if inside:
                    phases.add((dial, ph))
                    flush = flush or ends
        assert flush, x0
        off = [not quad_phase(di.edge_data('leave', 1, x0), dial, mx)[0] for dial in (0, 3) for mx in di.edge_match_x(1)]
        on = [quad_phase(di.edge_data('leave', 1, x0), dial, mx)[0] for dial in (1, 2) for mx in di.edge_match_x(1)]
        assert all(off) and all(on), (x0, off, on)
    dials = {d for (d, _p) in phases}
    assert dials and all({p for (d, p) in phases if d == dial} == {0, 1, 2, 3} for dial in dials), sorted(phases)
    assert {x % 4 for x in PHASE_X0S} == {0, 1, 2, 3} and set(di.edge_match_x(1)) == {0, 1}


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _ran(c, family):
    got = c.ctx.last_dials()
    assert got == dict(family=family, nr=c.nr, ws_max=c.ws_max), (c.tag, family, got)
    SEEN32.add((got['family'], got['nr']))


def _run32(c, bgr, rng, want_match_x=None, pads=(4, 8)):
    """The three formats, host and device path (a device buffer of exactly the extent), byte for byte against the 8-bit planar 4:4:4
    path and the BGR path; melf_ctx_last_dials after every call."""
    src8 = fc.bgr_to_yuv(bgr, 0, 0, pc.MATRIX)
    want = {'yuv': c.read_bgr(fc.yuv_to_bgr(*src8, 0, 0, pc.MATRIX)), 'rgb': c.read_bgr(bgr)}
    for w in want.values():
        assert (w['status'] == _hip.FRAME_OK).all(), c.tag
        if want_match_x is not None:
            assert [int(x) for x in w['match_x']] == want_match_x, c.tag
    i444 = c.reader.read_yuv_planar_frames(fc.conventional_yuv_planar(*src8, 'i444', 0, rng), 'i444', pc.MATRIX)
    assert i444.tobytes() == want['yuv'].tobytes(), c.tag
    for (fmt, family) in CASES:
        kind = pc.kind_of(fmt)
        (buf, desc) = pc.pitched32(*(src8 if kind == 'yuv' else (bgr,)), fmt, row_pad=pads[0], stride_pad=pads[1], rng=rng)
        assert c.ctx.process_packed32(buf.ctypes.data, desc).tobytes() == want[kind].tobytes(), (c.tag, fmt, 'host')
        _ran(c, family)
        dbuf = fc.DevBuf(buf.ctypes.data, buf.nbytes)
        try:
            assert c.ctx.process_packed32_dev(dbuf.d.value, desc).tobytes() == want[kind].tobytes(), (c.tag, fmt, 'device')
        finally:
            dbuf.free()
        _ran(c, family)


def _sweep32(r_max):
    if r_max in _SWEPT32:
        if _SWEPT32[r_max] is not None:
            raise _SWEPT32[r_max]
        return
    try:
        c = di._Ctx(di.sweep_data(r_max), 'r%d' % r_max)
        try:
            assert c.ctx.last_dials()['ws_max'] == 2 * r_max + 5
            _run32(c, di.sweep_frames(), np.random.default_rng(r_max))
        finally:
            c.close()
        _SWEPT32[r_max] = None
    except BaseException as e:
        _SWEPT32[r_max] = e
        raise


@pytest.mark.gpu
@pytest.mark.parametrize('r_max', di.R_MAXES)
def test_both_families_at_every_window_class(r_max):
    _sweep32(r_max)
    assert {(f, di.expected_nr(2 * r_max + 5)) for f in FAMILIES32} <= SEEN32


@pytest.mark.gpu
@pytest.mark.parametrize('x0', PHASE_X0S)
@pytest.mark.parametrize('kind', ('leave', 'flush'))
def test_every_phase(kind, x0):
    """The crop's x origin at four consecutive columns, frames cut to w0 .. w0 + 3 columns (odd widths among them; at w0 the crop's
    right edge is the frame's), dial windows at the dials crop's first and last columns, the match on crop columns 0 and 1."""
    data = di.edge_data(kind, 1, x0)
    bgr = di.edge_frames(1, x0)
    w0 = data['meter_rect']['bottom_right'][0]
    c = di._Ctx(data, 'p32_%s_x%d' % (kind, x0))
    try:
        assert c.nr == 48
        for k in range(4):
            _run32(c, np.ascontiguousarray(bgr[:, :, :w0 + k]), np.random.default_rng(x0 + k), want_match_x=di.edge_match_x(1), pads=(4 * (k % 2), 0))
        assert {(w0 + k) % 2 for k in range(4)} == {0, 1}
    finally:
        c.close()


@pytest.mark.gpu
def test_all_12_instantiations_were_launched_and_asserted():
    for r_max in di.R_MAXES:
        _sweep32(r_max)
    assert SEEN32 == ALL_PAIRS32, sorted(ALL_PAIRS32 - SEEN32)
