"""The dial reader's two kernel families of the 16-bit YUV frames (k_y16_needle<CSTEP, NR>, melf_process_yuv16*): every
instantiation production can pick, launched, ASSERTED to be the one that ran (melf_ctx_last_dials) and compared, the way
tests/test_dials_instantiations.py does it for the twelve families of the 8-bit layouts -- with that module's contexts, frames and
edge cases (imported, not copied).

Two families (planar, interleaved pairs) times six row counts NR: 12 kernels.  The sweep runs both at the eleven contexts whose
largest dial has R = 13 .. 29, both ends of every NR class.  The edge cases put the match on neighbouring crop columns, at both
parities of the crop's origin: the lanes' quads of these kernels start at an even pixel of the frame, one column left of the window
where its first column is odd (DialYuv16, melf_frame_src.h), so both forms of every window run, and the windows that leave the
crop's columns take the exact path.  Expected records: read_frames of the packed BGR frame the conversion makes of the reduced
samples (the contract of include/meterelf_hip.h), which the sweep of the other module holds against the oracle.
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
from tests import test_dials_instantiations as di  # noqa: E402
from tests import yuv16_cases as yc  # noqa: E402

FAMILIES16 = ('yuv16_step1', 'yuv16_step2')
ALL_PAIRS16 = frozenset([
    ('yuv16_step1', 32), ('yuv16_step1', 40), ('yuv16_step1', 48), ('yuv16_step1', 52), ('yuv16_step1', 56), ('yuv16_step1', 64),
    ('yuv16_step2', 32), ('yuv16_step2', 40), ('yuv16_step2', 48), ('yuv16_step2', 52), ('yuv16_step2', 56), ('yuv16_step2', 64),
])
MATRIX = 3
SEEN16 = set()     # (family, NR) pairs this module launched and asserted
_SWEPT16 = {}


def quads_of(data, dial, match_x):
    """The quads of one dial's window, restated from melf_y16_addr.h: (shift, first crop column, count, inside the crop's columns)."""
    nd = data['needle_data'][dial]
    tw = data['dials_template_size'][0]
    x0 = data['meter_rect']['top_left'][0]
    R = di.dial_radius(nd)
    (wx0, ws) = (di.py_round(nd['center'][0]) - R - 2, 2 * R + 5)
    shift = (x0 + match_x + wx0) & 1
    (qx0, n) = (wx0 - shift, (ws + shift + 3) >> 2)
    return shift, qx0, n, qx0 >= 0 and qx0 + 4 * n <= tw and n <= 16


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_family_names_and_codes():
    assert _hip.DIALS16_FAMILIES == FAMILIES16
    assert tuple(_hip.DIALS_FAMILIES) == di.FAMILIES            # the twelve stay the twelve
    import re
    with open(os.path.join(ROOT, 'include', 'meterelf_hip.h')) as fp:
        text = fp.read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r'\bMELF_DIALS16_([A-Z0-9_]+) = (\d+)', text)}
    assert values == {'STEP1': 12, 'STEP2': 13}
    assert {(f, nr) for f in FAMILIES16 for nr in di.NR_CLASSES} == ALL_PAIRS16


def test_edge_cases_force_both_quad_shifts():
    """The edge cases of the other module put the matches on crop columns 0 .. k: for every dial, windows at both parities of the
    first column -- quads that start at the window (shift 0) and one column left of it (shift 1) -- inside the crop's columns, at
    both parities of the crop's origin; 'leave' has windows outside (the exact path).  A shifted window never takes a quad more
    than the plain one: ws = 2 R + 5 is odd, so ws + 1 columns fit the quads that hold ws."""
    for x0 in (di.RECT_X0, di.RECT_X0 + 1):
        for k in (1, 3):
            for dial in range(4):
                inside = {quads_of(di.edge_data('near', k, x0), dial, mx)[0] for mx in di.edge_match_x(k)
                          if quads_of(di.edge_data('near', k, x0), dial, mx)[3]}
                assert inside == {0, 1}, (x0, k, dial, inside)
            leave = [quads_of(di.edge_data('leave', k, x0), dial, mx) for dial in (0, 3) for mx in di.edge_match_x(k)]
            assert any(not q[3] for q in leave), (x0, k)
    more = set()
    for r_max in di.R_MAXES:
        data = di.sweep_data(r_max)
        for dial in range(4):
            R = di.dial_radius(data['needle_data'][dial])
            ws = 2 * R + 5
            more.add(((ws + 1 + 3) >> 2) - ((ws + 3) >> 2))
            assert (ws + 1 + 3) >> 2 <= 16
    assert more == {0}


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _ran(c, family):
    got = c.ctx.last_dials()
    assert got == dict(family=family, nr=c.nr, ws_max=c.ws_max), (c.tag, family, got)
    SEEN16.add((got['family'], got['nr']))


def _run16(c, bgr, rng, formats, want_match_x=None):
    """Every format named, host and device path (a device buffer of exactly the extent), byte for byte against read_frames of the
    BGR frames the conversion makes of the reduced samples; melf_ctx_last_dials after every call."""
    wants = {}
    for fmt in formats:
        (sy, step, _vf, _shift) = yc.FORMATS[fmt]
        if sy not in wants:
            src8 = fc.bgr_to_yuv(bgr, 1, sy, MATRIX)
            wants[sy] = (src8, c.read_bgr(fc.yuv_to_bgr(*src8, 1, sy, MATRIX)))
            assert (wants[sy][1]['status'] == _hip.FRAME_OK).all(), (c.tag, fmt)
            if want_match_x is not None:
                assert [int(x) for x in wants[sy][1]['match_x']] == want_match_x, (c.tag, fmt)
        (src8, want) = wants[sy]
        family = 'yuv16_step%d' % step
        (raw, desc, _lead) = yc.pitched16(*yc.widen_planes(src8, fmt, rng), fmt, y_pad=2, c_pad=6, gap=2, stride_pad=2, rng=rng, matrix=MATRIX)
        assert c.ctx.process_yuv16(raw.ctypes.data, desc).tobytes() == want.tobytes(), (c.tag, fmt, 'host')
        _ran(c, family)
        buf = fc.DevBuf(raw.ctypes.data, raw.nbytes)
        try:
            assert c.ctx.process_yuv16_dev(buf.d.value, desc).tobytes() == want.tobytes(), (c.tag, fmt, 'device')
        finally:
            buf.free()
        _ran(c, family)


def _sweep16(r_max):
    if r_max in _SWEPT16:
        if _SWEPT16[r_max] is not None:
            raise _SWEPT16[r_max]
        return
    try:
        c = di._Ctx(di.sweep_data(r_max), 'r%d' % r_max)
        try:
            assert c.ctx.last_dials()['ws_max'] == 2 * r_max + 5
            # 4:2:2 and 4:2:0 in turn from context to context, a planar and a semi-planar format each, three shifts
            formats = ('i210', 'p210') if r_max % 2 else ('i012', 'p010')
            _run16(c, di.sweep_frames(), np.random.default_rng(r_max), formats)
        finally:
            c.close()
        _SWEPT16[r_max] = None
    except BaseException as e:
        _SWEPT16[r_max] = e
        raise


@pytest.mark.gpu
@pytest.mark.parametrize('r_max', di.R_MAXES)
def test_both_families_at_every_window_class(r_max):
    _sweep16(r_max)
    assert {(f, di.expected_nr(2 * r_max + 5)) for f in FAMILIES16} <= SEEN16


@pytest.mark.gpu
@pytest.mark.parametrize('x0', (di.RECT_X0, di.RECT_X0 + 1))
@pytest.mark.parametrize('k', (1, 3))
@pytest.mark.parametrize('kind', di.EDGE_KINDS)
def test_both_quad_shifts_and_the_crop_edges(kind, k, x0):
    """Matches on crop columns 0 .. k (neighbouring columns: both parities of every lane's first pixel), at both parities of the
    crop's origin; 'leave': windows that leave the crop's columns; 'flush': the last quad ends on the template's last column."""
    data = di.edge_data(kind, k, x0)
    bgr = di.edge_frames(k, x0)
    c = di._Ctx(data, '%s_k%d_x%d' % (kind, k, x0))
    try:
        assert c.nr == 48
        _run16(c, bgr, np.random.default_rng(7 + k), ('i010', 'p010', 'i210', 'p216'), want_match_x=di.edge_match_x(k))
    finally:
        c.close()


@pytest.mark.gpu
def test_all_12_instantiations_were_launched_and_asserted():
    for r_max in di.R_MAXES:
        _sweep16(r_max)
    assert SEEN16 == ALL_PAIRS16, sorted(ALL_PAIRS16 - SEEN16)
