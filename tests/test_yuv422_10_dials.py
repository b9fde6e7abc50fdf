"""The dial reader's two kernel families of the packed 10-bit YUV 4:2:2 frames (k_v210_needle<NR>, k_y210_needle<NR>,
melf_process_yuv422_10*): every instantiation production can pick, launched, ASSERTED to be the one that ran (melf_ctx_last_dials)
and compared, the way tests/test_yuv16_dials.py does it for the 16-bit planes -- with the contexts, frames and edge scenes of
tests/test_dials_instantiations.py (imported, not copied).

Two families times six row counts NR: 12 kernels.  The sweep runs both at the eleven contexts whose largest dial has R = 13 .. 29,
both ends of every NR class.  The phase cases move the crop's x origin through all six residues modulo 6 -- a v210 lane's quad starts
at pair slot 0, 1 or 2 of its group, and for slot 2 reaches into the next group -- with the frame cut to W0, W0 + 2 and W0 + 4
columns, so that the row's last group is whole, one third and two thirds full; the edge scenes put dial windows at the dials crop's
first and last columns ('leave': outside, the exact path; 'flush': the last quad ends on the template's last column) and the match
on crop columns 0 and 1, both parities.  Expected records: read_yuv422_frames of the unpacked 8-bit YUYV frames, which equal
read_frames of the BGR frames the conversion makes (p10_cases.want_8bit).
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
from tests import p10_cases as pc  # noqa: E402
from tests import test_dials_instantiations as di  # noqa: E402

FAMILIES10 = ('v210', 'y210')
ALL_PAIRS10 = frozenset([
    ('v210', 32), ('v210', 40), ('v210', 48), ('v210', 52), ('v210', 56), ('v210', 64),
    ('y210', 32), ('y210', 40), ('y210', 48), ('y210', 52), ('y210', 56), ('y210', 64),
])
SEEN10 = set()     # (family, NR) pairs this module launched and asserted
_SWEPT10 = {}


def quad_phases(data, dial, match_x):
    """Restated from melf_p10_addr.h: (the quads lie inside the crop's columns, the residues modulo 6 of the lanes' first pixels)."""
    nd = data['needle_data'][dial]
    tw = data['dials_template_size'][0]
    x0 = data['meter_rect']['top_left'][0]
    R = di.dial_radius(nd)
    (wx0, ws) = (di.py_round(nd['center'][0]) - R - 2, 2 * R + 5)
    shift = (x0 + match_x + wx0) & 1
    (qx0, n) = (wx0 - shift, (ws + shift + 3) >> 2)
    inside = qx0 >= 0 and qx0 + 4 * n <= tw and n <= 16
    return inside, {(x0 + match_x + qx0 + 4 * min(p, n - 1)) % 6 for p in range(16)}


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_family_names_and_codes():
    assert _hip.DIALS10_FAMILIES == FAMILIES10
    assert tuple(_hip.DIALS_FAMILIES) == di.FAMILIES            # the twelve stay the twelve
    import re
    with open(os.path.join(ROOT, 'include', 'meterelf_hip.h')) as fp:
        text = fp.read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r'\bMELF_DIALS10_([A-Z0-9_]+) = (\d+)', text)}
    assert values == {'V210': 14, 'Y210': 15}
    assert {(f, nr) for f in FAMILIES10 for nr in di.NR_CLASSES} == ALL_PAIRS10


def test_phase_cases_meet_every_pair_slot():
    """Over the six crop origins of the phase cases every dial's quads start at residues 0, 2 and 4 of a group (a window of 4 or
    more quads steps through all three anyway: 4 mod 6 generates them), at both parities of the match; 'leave' has windows outside
    the crop's columns (the exact path) at every origin."""
    for x0 in PHASE_X0S:
        for dial in range(4):
            seen = set()
            for mx in di.edge_match_x(1):
                (inside, ph) = quad_phases(di.edge_data('flush', 1, x0), dial, mx)
                if inside:
                    seen |= ph
            assert seen == {0, 2, 4}, (x0, dial, seen)
        assert any(not quad_phases(di.edge_data('leave', 1, x0), dial, mx)[0] for dial in (0, 3) for mx in di.edge_match_x(1)), x0
    assert {x % 6 for x in PHASE_X0S} == {0, 1, 2, 3, 4, 5}
    assert set(di.edge_match_x(1)) == {0, 1}


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _ran(c, family):
    got = c.ctx.last_dials()
    assert got == dict(family=family, nr=c.nr, ws_max=c.ws_max), (c.tag, family, got)
    SEEN10.add((got['family'], got['nr']))


def _run10(c, bgr, rng, want_match_x=None, pads=(16, 16)):
    """Both formats, host and device path (a device buffer of exactly the extent), byte for byte against the 8-bit 4:2:2 path and
    the BGR path; melf_ctx_last_dials after every call."""
    src8 = fc.bgr_to_yuv(bgr, 1, 0, pc.MATRIX)
    want = c.read_bgr(fc.yuv_to_bgr(*src8, 1, 0, pc.MATRIX))
    assert (want['status'] == _hip.FRAME_OK).all(), c.tag
    if want_match_x is not None:
        assert [int(x) for x in want['match_x']] == want_match_x, c.tag
    assert c.reader.read_yuv422_frames(fc.packed422(*src8, 'yuyv'), 'yuyv', pc.MATRIX).tobytes() == want.tobytes(), c.tag
    for fmt in FAMILIES10:
        (buf, desc) = pc.pitched10(*src8, fmt, row_pad=pads[0], stride_pad=pads[1], rng=rng)
        assert c.ctx.process_yuv422_10(buf.ctypes.data, desc).tobytes() == want.tobytes(), (c.tag, fmt, 'host')
        _ran(c, fmt)
        dbuf = fc.DevBuf(buf.ctypes.data, buf.nbytes)
        try:
            assert c.ctx.process_yuv422_10_dev(dbuf.d.value, desc).tobytes() == want.tobytes(), (c.tag, fmt, 'device')
        finally:
            dbuf.free()
        _ran(c, fmt)


def _sweep10(r_max):
    if r_max in _SWEPT10:
        if _SWEPT10[r_max] is not None:
            raise _SWEPT10[r_max]
        return
    try:
        c = di._Ctx(di.sweep_data(r_max), 'r%d' % r_max)
        try:
            assert c.ctx.last_dials()['ws_max'] == 2 * r_max + 5
            _run10(c, di.sweep_frames(), np.random.default_rng(r_max))
        finally:
            c.close()
        _SWEPT10[r_max] = None
    except BaseException as e:
        _SWEPT10[r_max] = e
        raise


@pytest.mark.gpu
@pytest.mark.parametrize('r_max', di.R_MAXES)
def test_both_families_at_every_window_class(r_max):
    _sweep10(r_max)
    assert {(f, di.expected_nr(2 * r_max + 5)) for f in FAMILIES10} <= SEEN10


PHASE_X0S = tuple(range(di.RECT_X0, di.RECT_X0 + 6))   # 50 .. 55: residues 2, 3, 4, 5, 0, 1 modulo 6


@pytest.mark.gpu
@pytest.mark.parametrize('x0', PHASE_X0S)
@pytest.mark.parametrize('kind', ('leave', 'flush'))
def test_every_phase(kind, x0):
    """The crop's x origin at every residue modulo 6, frames cut to W0, W0 + 2 and W0 + 4 columns (the last group whole, one third
    and two thirds full: W modulo 6 takes its three values), dial windows at the dials crop's first and last columns, the match on
    crop columns 0 and 1."""
    data = di.edge_data(kind, 1, x0)
    bgr = di.edge_frames(1, x0)
    w0 = (data['meter_rect']['bottom_right'][0] + 1) & ~1
    c = di._Ctx(data, 'p10_%s_x%d' % (kind, x0))
    try:
        assert c.nr == 48
        for (k, W) in enumerate((w0, w0 + 2, w0 + 4)):
            _run10(c, np.ascontiguousarray(bgr[:, :, :W]), np.random.default_rng(x0 + k), want_match_x=di.edge_match_x(1), pads=(16 * (k % 2), 0))
        assert {W % 6 for W in (w0, w0 + 2, w0 + 4)} == {0, 2, 4}
    finally:
        c.close()


@pytest.mark.gpu
def test_all_12_instantiations_were_launched_and_asserted():
    for r_max in di.R_MAXES:
        _sweep10(r_max)
    assert SEEN10 == ALL_PAIRS10, sorted(ALL_PAIRS10 - SEEN10)
