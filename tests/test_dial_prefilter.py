"""A census of the packed 16-bit integer prefilter in the dial reader's pixel phase (k_dials_body.inc, "Two steps").

The prefilter tests L and S of four pixels per lane with integers -- sum = max + min against 2 lol - 1 and 2 hil + 1, 255 diff
against (los - 1) den and (his + 1) den, all in 16-bit halves -- and may only err towards "maybe": a pixel it drops never reaches
the exact float test.  A prefilter that dropped a pixel sitting exactly on a bound would change a reading only when that pixel
carries weight, which fixture frames and random bytes almost never arrange.  Here every (max, min) pair whose exact L or S lies
within one step of a bound is painted as a single pixel of the needle's ring, where it is a ring point of its own.

The observable: one dial of positive momentum whose core is a flat colour C, so that its bounds are HLS(C) +- color_range.  Test
pixels are single pixels in the annulus, four apart (the 3 x 3 closing bridges less), all within 0.115 turn of east, so the
momentum keeps every one that is in range; no contour exceeds area 100, so the needle is the whole mask.  Dropping any one
in-range test pixel moves the oracle's angle by more than 1e-6 (asserted; a frame where it does not is rebuilt with the pixels
in other places).

Four bounds settings: the fixture dial's ranges; ranges 0 (lo == hi); ranges 255, every L and S bound clamped, on a dial small
enough for its whole window to fit the candidate list (27 x 27 = 729 <= DIAL_LIST_CAP: every pixel passes a prefilter whose
bounds are open, and a longer list sends the window down the exact path, past the prefilter); a grey core with los = 0, which
admits diff = 0.  The test triples are (min, mid, max) as B, G, R or B and G swapped, mid at or just above min: hue 0, H = the
hue shift, inside every setting's hue range, for grey, black and white too.

CPU: a numpy restatement of the integer test, over all 32 896 pairs: with the kernel's margins it accepts whatever the exact
path accepts; with margins 0 it rejects pairs the exact path accepts (counted).  GPU: the frames as BGR, RGB, BGRA and RGBA -- both
byte widths, both selector sets -- against the oracle, and against melf_read_dials on the oracle-converted HLS crop, which takes
the exact path for every pixel.  The crop is 188 wide (no scalar-tail conversion), the frames 4-byte aligned and the windows
inside the crop: the conditions under which the window is fetched as quads and the prefilter runs (tests/test_gpu_parity.py:1100,
test_dial_window_fetch_edge_paths).
"""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pyoracle as po  # noqa: E402
from tests import dial_records as dr  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests.dial_scenes import TH, TW  # noqa: E402
from tests.test_dials_instantiations import _Ctx, _fixture_data, dial_radius, py_round  # noqa: E402
from tests.test_gpu_parity import _compare_records  # noqa: E402

DIAL_LIST_CAP = 768      # k_dials.hip
CENTRE = (94.0, 59.0)
EAST = 0.25
SECTOR = 0.115           # any two test pixels lie within 0.23 turn: the momentum of some keeps all
DROP_TOL = 1e-6
GREY = (235, 235, 235)
FIXTURE_RANGE = _fixture_data()['needle_data'][0]['color_range']

# name: core colour (B, G, R), color_range, (diameter, dist_from_center, circle_thickness), background
SETTINGS = {
    'fixture': dict(core=(40, 40, 200), ranges=dict(FIXTURE_RANGE), ring=(10, 5, 11), background=GREY),
    'point': dict(core=(40, 40, 200), ranges=dict(h=10, l=0, s=0), ring=(10, 5, 11), background=GREY),
    # every window pixel is a candidate: R = 11, a window of 27 x 27.  The background differs in hue, not in L or S
    'clamped': dict(core=(40, 40, 200), ranges=dict(h=10, l=255, s=255), ring=(6, 2, 7), background=(235, 120, 40)),
    'grey': dict(core=(100, 100, 100), ranges=dict(h=10, l=60, s=40), ring=(10, 5, 11), background=GREY),
}
HAS_INTERIOR = ('fixture', 'grey')   # ... and a bound that something lies beyond: 'point' is lo == hi, 'clamped' has no outside


def setting_data(name):
    s = SETTINGS[name]
    data = dr.whole_frame(_fixture_data())
    (diameter, dist, thick) = s['ring']
    data['needle_data'] = [{'name': 'p', 'color_range': dict(s['ranges']), 'dist_from_center': dist, 'circle_thickness': thick,
                            'angle_of_zero': 0.0, 'center': list(CENTRE), 'diameter': diameter, 'negative_momentum': False}]
    return data


@functools.lru_cache(maxsize=None)
def oparams(name):
    return po.Params(dr.params_file(setting_data(name), 'prefilter_' + name))


def hls_of(triples):
    """The oracle's conversion of (N, 3) BGR triples, every one in the four-pixel form (as in a crop 188 wide)."""
    t = np.asarray(triples, np.uint8).reshape(-1, 1, 3)
    img = np.ascontiguousarray(np.repeat(t, 4, axis=1))
    return po.bgr2hls(img, _fixture_data()['hue_shift'])[:, 0].astype(np.int64)


@functools.lru_cache(maxsize=None)
def ls_table():
    """Exact L and S (oracle) of every pair: [vmax][vmin], entries with vmin > vmax unused."""
    (vmax, vmin) = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    hls = hls_of(np.stack([vmin, vmin, vmax], axis=-1).reshape(-1, 3)).reshape(256, 256, 3)
    return (hls[..., 1], hls[..., 2])


@functools.lru_cache(maxsize=None)
def bounds(name):
    """((loh, lol, los), (hih, hil, his)): HlsColor.get_range around the oracle's conversion of the flat core."""
    s = SETTINGS[name]
    c = hls_of([s['core']])[0]
    r = (s['ranges']['h'], s['ranges']['l'], s['ranges']['s'])
    return (tuple(int(max(c[k] - r[k], 0)) for k in range(3)), tuple(int(min(c[k] + r[k], 255)) for k in range(3)))


def integer_test(vmax, vmin, lo, hi, margin):
    """The prefilter, restated: true where the pixel stays a candidate.  16-bit arithmetic throughout, as v_pk_*_u16."""
    u16 = lambda a: np.asarray(a, np.int64) & 0xffff   # noqa: E731
    (_loh, lol, los) = lo
    (_hih, hil, his) = hi
    (LO2, HI2) = (max(2 * lol - margin, 0), 2 * hil + margin)
    (SLO, SHI) = (max(los - margin, 0), his + margin)
    (vmax, vmin) = (np.asarray(vmax, np.int64), np.asarray(vmin, np.int64))
    total = u16(vmax + vmin)
    diff = u16(vmax - vmin)
    den = np.minimum(total, u16(0x01fe - total))
    lbad = np.minimum(np.maximum(total, LO2), HI2) != total
    a = u16(diff * 0x00ff)
    sbad = np.minimum(np.maximum(a, u16(den * SLO)), u16(den * SHI)) != a
    return ~(lbad | sbad)


def all_pairs():
    (vmax, vmin) = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    keep = vmin <= vmax
    return (vmax[keep], vmin[keep])


def exact_accepts(vmax, vmin, lo, hi):
    (L, S) = ls_table()
    (l, s) = (L[vmax, vmin], S[vmax, vmin])
    return (l >= lo[1]) & (l <= hi[1]) & (s >= lo[2]) & (s <= hi[2])


BOUND_NAMES = ('lol', 'hil', 'los', 'his')


@functools.lru_cache(maxsize=None)
def census(name):
    """Every pair whose exact L or S lies within one step of a bound, inside or outside: (vmax, vmin, tags), tags a bit per bound
    of BOUND_NAMES the pair lies near."""
    (lo, hi) = bounds(name)
    (vmax, vmin) = all_pairs()
    (L, S) = ls_table()
    (l, s) = (L[vmax, vmin], S[vmax, vmin])
    tags = np.zeros(len(vmax), np.int64)
    for (k, (plane, b)) in enumerate(((l, lo[1]), (l, hi[1]), (s, lo[2]), (s, hi[2]))):
        tags |= (np.abs(plane - b) <= 1).astype(np.int64) << k
    keep = tags != 0
    return (vmax[keep], vmin[keep], tags[keep])


@functools.lru_cache(maxsize=None)
def triples(name):
    """One BGR triple per census pair: R the maximum, B and G the minimum, or one of them one or two above it where the hue stays
    inside the range (so that the three bytes differ and a selector that took the wrong one would show)."""
    (lo, hi) = bounds(name)
    (vmax, vmin, _tags) = census(name)
    n = len(vmax)
    out = np.stack([vmin, vmin, vmax], axis=-1)
    variant = np.arange(n) % 5            # 0: none; 1, 3: G + 1, + 2; 2, 4: B + 1, + 2
    delta = (variant + 1) // 2
    cand = out.copy()
    cand[np.arange(n), np.where(variant % 2 == 1, 1, 0)] += np.where(variant > 0, delta, 0)
    ok = cand[:, :2].max(axis=1) < vmax       # the middle value stays below the maximum: the pair is unchanged
    h = hls_of(cand)[:, 0]
    ok &= (h >= lo[0]) & (h <= hi[0])
    out[ok] = cand[ok]
    hls = hls_of(out)
    (L, S) = ls_table()
    assert np.array_equal(hls[:, 1], L[vmax, vmin]) and np.array_equal(hls[:, 2], S[vmax, vmin])
    assert ((hls[:, 0] >= lo[0]) & (hls[:, 0] <= hi[0])).all()      # H inside the range for every pair, grey included
    in_range = np.all((hls >= np.array(lo)) & (hls <= np.array(hi)), axis=1)
    return (out.astype(np.uint8), in_range)


def window_of(name):
    nd = setting_data(name)['needle_data'][0]
    R = dial_radius(nd)
    return (py_round(CENTRE[0]) - R - 2, py_round(CENTRE[1]) - R - 2, 2 * R + 5)


@functools.lru_cache(maxsize=None)
def slots(name, phase):
    """Places for test pixels: a lattice of the annulus four apart in both directions, each row of it one column further right
    than the row above and the whole lattice `phase` columns further right (frame by frame, so that all four positions of a
    lane's quad occur on the small dial too), within SECTOR of east."""
    op = oparams(name)
    annulus = op.masks()[0, 1] > 0
    (cx, cy) = (int(CENTRE[0]), int(CENTRE[1]))
    out = []
    for r in range(-6, 7):
        y = cy + 4 * r
        for x in range(cx + ((r + phase) % 4), TW, 4):
            if max(x - cx, abs(y - cy)) < 6:     # three pixels clear of the 5 x 5 core as well
                continue
            if annulus[y, x] and abs(po.angle_by_vector(x - CENTRE[0], y - CENTRE[1]) - EAST) < SECTOR:
                out.append((x, y))
    assert len(out) <= 40
    return tuple(out)


def _paint(name, chunk, phase, shift):
    """One frame: the core, and census triple chunk[i] at slot (i + shift) mod the slots' count.  -> (frame, [(x, y)])"""
    s = SETTINGS[name]
    sl = slots(name, phase)
    frame = np.empty((TH, TW, 3), np.uint8)
    frame[:] = s['background']
    (cx, cy) = (int(CENTRE[0]), int(CENTRE[1]))
    frame[cy - 2:cy + 3, cx - 2:cx + 3] = s['core']
    where = []
    for (i, t) in enumerate(chunk):
        (x, y) = sl[(i + shift) % len(sl)]
        frame[y, x] = t
        where.append((x, y))
    return (frame, where)


def _every_pixel_bears(name, frame, where, in_range):
    """Dropping any one in-range test pixel changes the oracle's status or moves its angle by more than DROP_TOL."""
    op = oparams(name)
    hls = po.bgr2hls(frame, op.hue_shift)
    base = po.read_dials(hls, op)
    back = hls_of([SETTINGS[name]['background']])[0]
    for ((x, y), inr) in zip(where, in_range):
        if not inr:
            continue
        cut = hls.copy()
        cut[y, x] = back
        o = po.read_dials(cut, op)
        if o.status == base.status and not abs(o.angle[0] - base.angle[0]) > DROP_TOL:
            return False
    return True


def lane_positions(name, idx, where, seen=None):
    """{bound: lane positions (column in the window mod 4) at which an ACCEPTED pixel near that bound sits}, added to `seen`."""
    (_tri, in_range) = triples(name)
    tags = census(name)[2]
    wx0 = window_of(name)[0]
    seen = {k: set() for k in range(4)} if seen is None else seen
    for (i, (x, _y)) in zip(idx, where):
        for k in range(4):
            if tags[i] >> k & 1 and in_range[i]:
                seen[k].add((x - wx0) % 4)
    return seen


FEW = 8


def pair_positions(name, pairs, idxs, wheres):
    """{census index: the lane positions that pair has sat in} for the pairs named."""
    wx0 = window_of(name)[0]
    out = {i: set() for i in pairs}
    for (idx, where) in zip(idxs, wheres):
        for (i, (x, _y)) in zip(idx, where):
            if i in out:
                out[i].add((x - wx0) % 4)
    return out


@functools.lru_cache(maxsize=None)
def census_frames(name):
    """(frames, [census indices per frame], [[(x, y)] per frame], placements rebuilt, frames repeated).  Every census pair is
    painted once, chunk by chunk, the lattice's phase turning with the frame.  A bound whose accepted pairs are too few to have
    come by all four lane positions that way (lo == hi has two accepted pairs in all; L = 0 .. 1 is black and three more) then
    has them painted again, under other phases and placements, until EACH of them has sat in every position (a bound with more
    than FEW accepted pairs: up to FEW of them, until the bound has)."""
    (tri, in_range) = triples(name)
    tags = census(name)[2]
    (frames, idxs, wheres, rebuilt) = ([], [], [], 0)
    at = 0
    while at < len(tri):
        phase = len(frames) % 4
        per = len(slots(name, phase))
        idx = list(range(at, min(at + per, len(tri))))
        for shift in range(per):
            (frame, where) = _paint(name, tri[idx], phase, shift)
            if _every_pixel_bears(name, frame, where, in_range[idx]):
                break
            rebuilt += 1
        else:
            raise AssertionError('%s: no placement of pairs %d.. makes every in-range pixel bear on the angle' % (name, at))
        frames.append(frame)
        idxs.append(idx)
        wheres.append(where)
        at += per
    once = len(frames)
    seen = {k: set() for k in range(4)}
    for (idx, where) in zip(idxs, wheres):
        lane_positions(name, idx, where, seen)
    for k in range(4):
        accepted = [int(i) for i in np.flatnonzero((tags >> k & 1 == 1) & in_range)]
        few = accepted[:FEW]
        each = pair_positions(name, few, idxs, wheres) if len(accepted) <= FEW else None
        wx0 = window_of(name)[0]
        for phase in (0, 1, 2, 3, 0, 1, 2, 3):
            per = len(slots(name, phase))
            for shift in range(per):
                # the pairs that still lack a position go first: a small dial's lattice holds fewer than FEW
                group = few if each is None else sorted(few, key=lambda i: (len(each[i]) == 4, i))
                group = group[:per]
                (frame, where) = _paint(name, tri[group], phase, shift)
                if each is None:
                    new = bool(lane_positions(name, group, where)[k] - seen[k])
                else:
                    new = any((x - wx0) % 4 not in each[i] for (i, (x, _y)) in zip(group, where))
                if new and _every_pixel_bears(name, frame, where, in_range[group]):
                    frames.append(frame)
                    idxs.append(group)
                    wheres.append(where)
                    lane_positions(name, group, where, seen)
                    if each is not None:
                        for (i, (x, _y)) in zip(group, where):
                            each[i].add((x - wx0) % 4)
    return (np.stack(frames), idxs, wheres, rebuilt, len(frames) - once)


@functools.lru_cache(maxsize=None)
def oracle_records(name):
    return po.process_frames(census_frames(name)[0], oparams(name))


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_settings_are_what_they_claim():
    want = {'fixture': ((118, 85, 105), (138, 155, 235)), 'point': ((118, 120, 170), (138, 120, 170)),
            'clamped': ((118, 0, 0), (138, 255, 255)), 'grey': ((118, 40, 0), (138, 160, 40))}
    for name in SETTINGS:
        assert bounds(name) == want[name], (name, bounds(name))
        (wx0, wy0, ws) = window_of(name)
        assert wx0 >= 0 and wx0 + 4 * ((ws + 3) >> 2) <= TW and wy0 >= 0 and wy0 + ws <= TH    # the window is fetched as quads
        assert TW % 4 == 0                                                                       # no scalar-tail conversion
        back = hls_of([SETTINGS[name]['background']])[0]
        (lo, hi) = bounds(name)
        assert not np.all((back >= np.array(lo)) & (back <= np.array(hi)))
        # the background stays off the candidate list, or the whole window fits it: the prefilter's verdict is what is used
        (bmax, bmin) = (max(SETTINGS[name]['background']), min(SETTINGS[name]['background']))
        assert not integer_test(bmax, bmin, lo, hi, 1) or ws * ws <= DIAL_LIST_CAP, name
    assert window_of('clamped')[2] ** 2 == 729
    (lo, hi) = bounds('grey')
    assert lo[2] == 0 and exact_accepts(np.array([77]), np.array([77]), lo, hi).all()    # diff = 0 is admitted


@pytest.mark.parametrize('name', list(SETTINGS))
def test_products_stay_below_2_16(name):
    (lo, hi) = bounds(name)
    assert 255 * 255 < 1 << 16 and 255 * (hi[2] + 1) < 1 << 16 and 2 * hi[1] + 1 < 1 << 16
    (vmax, vmin) = all_pairs()
    den = np.minimum(vmax + vmin, 510 - (vmax + vmin))
    assert den.max() == 255 and den.min() == 0 and (den * (hi[2] + 1)).max() < 1 << 16


@pytest.mark.parametrize('name', list(SETTINGS))
def test_census_sits_on_every_bound(name):
    """Every bound from both sides -- where a side exists: nothing lies outside a bound clamped at 0 or 255 -- and, for L, odd
    sums rounded up and rounded down; grey, black and white are among the pairs where the bounds reach them."""
    (lo, hi) = bounds(name)
    (vmax, vmin, tags) = census(name)
    (L, S) = ls_table()
    (l, s) = (L[vmax, vmin], S[vmax, vmin])
    for (k, (plane, b, inside)) in enumerate(((l, lo[1], 1), (l, hi[1], -1), (s, lo[2], 1), (s, hi[2], -1))):
        near = (tags >> k & 1) == 1
        assert (plane[near] == b).any(), (name, BOUND_NAMES[k], 'on')
        if 0 <= b - inside <= 255:
            assert (plane[near] == b - inside).any(), (name, BOUND_NAMES[k], 'outside')
        if lo[1 + k // 2] != hi[1 + k // 2] and 0 <= b + inside <= 255:
            # (one value no pair takes: S = 254 -- diff and den have the same parity, and (den - 2) / den < 253.5 / 255)
            occurs = ((L, S)[k // 2][all_pairs()] == b + inside).any()
            assert occurs == (not (k >= 2 and b + inside == 254)), (name, BOUND_NAMES[k])
            assert (plane[near] == b + inside).any() == occurs, (name, BOUND_NAMES[k], 'inside')
    for (k, b) in ((0, lo[1]), (1, hi[1])):
        near = ((tags >> k & 1) == 1) & ((vmax + vmin) % 2 == 1)
        up = l[near] == (vmax[near] + vmin[near] + 1) // 2
        if 0 < b < 255:     # (beside a clamped bound lie two odd sums at most, 1 and 3 or 507 and 509)
            assert up.any() and (~up).any(), (name, BOUND_NAMES[k])
        else:
            assert near.any(), (name, BOUND_NAMES[k])
    pairs = set(zip(vmax.tolist(), vmin.tolist()))
    if name == 'clamped':
        assert {(0, 0), (255, 255), (255, 0)} <= pairs and sum(a == b for (a, b) in pairs) == 256
    if name == 'grey':
        assert sum(a == b for (a, b) in pairs) >= 6      # greys of L 39 .. 41 and 159 .. 161, S = 0 on the lower bound


# pairs the exact path accepts and margins 0 reject, over all 32 896 (the figures DESIGN.md quotes)
MARGIN0_REJECTS = {'fixture': 54, 'point': 1, 'clamped': 0, 'grey': 49}


@pytest.mark.parametrize('name', list(SETTINGS))
def test_margins_accept_what_the_exact_path_accepts(name):
    """Over ALL pairs.  The margin-0 variant (LO2 = 2 lol, HI2 = 2 hil, SLO = los, SHI = his) is wrong: the count of pairs the exact
    path accepts and it rejects is in the assertion's message (and in DESIGN.md)."""
    (lo, hi) = bounds(name)
    (vmax, vmin) = all_pairs()
    exact = exact_accepts(vmax, vmin, lo, hi)
    kept = integer_test(vmax, vmin, lo, hi, 1)
    assert not (exact & ~kept).any(), (name, list(zip(vmax[exact & ~kept].tolist(), vmin[exact & ~kept].tolist()))[:8])
    lost = exact & ~integer_test(vmax, vmin, lo, hi, 0)
    (cmax, cmin, _tags) = census(name)
    census_pairs = set(zip(cmax.tolist(), cmin.tolist()))
    assert all(p in census_pairs for p in zip(vmax[lost].tolist(), vmin[lost].tolist())), name   # they all sit on a bound
    print('%s: margins 0 reject %d of the %d pairs the exact path accepts; the kernel\'s margins keep %d candidates of %d pairs'
          % (name, lost.sum(), exact.sum(), kept.sum(), len(vmax)))
    assert int(lost.sum()) == MARGIN0_REJECTS[name], '%s: margins 0 reject %d accepted pairs' % (name, lost.sum())
    assert all(MARGIN0_REJECTS[k] > 0 for k in HAS_INTERIOR) and MARGIN0_REJECTS['point'] > 0
    if name == 'clamped':
        # Bounds clamped at 0 and 255 have nothing beyond them for a margin to let in: LO2 = 0 <= sum <= 510 = HI2, SLO = 0, and
        # diff <= den gives 255 diff <= 255 den = SHI den.  Margins 0 are right here; what this setting is for is the other end of the
        # claim, products that stay below 2^16 at SHI = 256 (test_products_stay_below_2_16) and den = 0.
        assert lost.sum() == 0 and integer_test(vmax, vmin, lo, hi, 0).all() and kept.all()


@pytest.mark.parametrize('name', list(SETTINGS))
def test_census_frames_show_every_pixel(name):
    (frames, idxs, wheres, rebuilt, repeated) = census_frames(name)
    (tri, in_range) = triples(name)
    (_vmax, _vmin, tags) = census(name)
    once = len(frames) - repeated
    assert [i for idx in idxs[:once] for i in idx] == list(range(len(tri))) and max(len(w) for w in wheres) <= 40
    print('%s: %d pairs (%d in range) on %d frames, %d placements rebuilt, %d frames of repeated pairs'
          % (name, len(tri), in_range.sum(), once, rebuilt, repeated))
    (wx0, wy0, ws) = window_of(name)
    op = oparams(name)
    disk = op.masks()[0, 0] > 0
    back = np.array(SETTINGS[name]['background'], np.uint8)
    seen = {k: set() for k in range(4)}
    for (f, (idx, where)) in enumerate(zip(idxs, wheres)):
        inr = in_range[idx]
        assert len(idx) == len(where) == len(set(where))
        for (x, y) in where:
            assert wx0 <= x < wx0 + ws and wy0 <= y < wy0 + ws
        lane_positions(name, idx, where, seen)
        # every two test pixels four apart or more, and all of them four from the core
        xy = np.array(where)
        apart = np.abs(xy[:, None, :] - xy[None, :, :]).max(axis=-1)
        assert (apart[~np.eye(len(xy), dtype=bool)] >= 4).all(), (name, f)
        assert (np.abs(xy - np.array([int(CENTRE[0]), int(CENTRE[1])])).max(axis=-1) >= 6).all(), (name, f)
        assert np.array_equal(frames[f][xy[:, 1], xy[:, 0]], tri[idx])
        o = oracle_records(name)[f]
        assert (o.match_x, o.match_y) == (0, 0) and o.contour_area[0] <= 100
        if o.status == 0:   # every in-range test pixel is a ring point, and the momentum keeps it
            assert o.n_outer[0] == o.n_kept[0] == int(np.sum(inr)), (name, f)
            assert o.n_needle[0] == 25 + int(np.sum(inr))
        else:
            assert o.status == po.ANGLE_UNDETERMINED and not np.any(inr), (name, f)
        # candidates: what the restated prefilter keeps of the window
        win = frames[f, wy0:wy0 + ws, wx0:wx0 + ws].astype(np.int64)
        ncand = int(integer_test(win.max(axis=-1), win.min(axis=-1), *bounds(name), 1).sum())
        assert ncand <= DIAL_LIST_CAP, (name, f, ncand)
        assert not (frames[f][~disk] != back).any()
    # each position of a lane's four pixels (both halves h, both pixels of a half) carries an accepted pixel for every bound
    for k in range(4):
        accepted = int(np.sum((tags >> k & 1 == 1) & in_range))
        print('%s %s: %d accepted pairs at lane positions %s' % (name, BOUND_NAMES[k], accepted, sorted(seen[k])))
        assert accepted > 0 and seen[k] == {0, 1, 2, 3}, (name, BOUND_NAMES[k], accepted, seen[k])
        if accepted <= FEW:   # ... and where a bound has only a handful, each of them does
            each = pair_positions(name, [int(i) for i in np.flatnonzero((tags >> k & 1 == 1) & in_range)], idxs, wheres)
            assert all(v == {0, 1, 2, 3} for v in each.values()), (name, BOUND_NAMES[k], each)
    assert (oracle_status_counts(name)[0] > 0)


def oracle_status_counts(name):
    st = [int(o.status) for o in oracle_records(name)]
    return {s: st.count(s) for s in (0, 2, 3)}


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _against_oracle(recs, ores, tag):
    _compare_records(recs, ores, ndials=1, tag=tag)
    for (i, (r, o)) in enumerate(zip(recs, ores)):
        assert (int(r['status']), int(r['failed_dial']), int(r['unreadable_mask'])) == (o.status, o.failed_dial, o.unreadable_mask), (tag, i)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(SETTINGS))
def test_prefilter_census(name):
    """Every format is compared with the oracle on its own and the failures are collected, so that a wrong prefilter shows in
    each kernel family it runs in: last_dials names family and NR, not the path a window took, and what shows that the quads and
    the prefilter ran for a format is that the margin-0 build fails for it."""
    frames = census_frames(name)[0]
    ores = oracle_records(name)
    op = oparams(name)
    failures = []

    def collect(tag, check):
        try:
            check()
        except AssertionError as e:
            failures.append((tag, str(e)[:300]))

    c = _Ctx(setting_data(name), 'records_prefilter_' + name)
    try:
        assert c.ctx.params.ndials == 1
        recs = c.read_bgr(frames)
        collect('bgr', lambda: _against_oracle(recs, ores, name + ' bgr'))
        # the other byte width and the swapped selectors
        rng = np.random.default_rng(5)
        for (fmt, family) in (('rgb', 'packed3'), ('bgra', 'packed4'), ('rgba', 'packed4')):
            (arr, f) = fc.to_layout(frames, fmt, 0, rng)
            got = c.reader.read_frame_views(arr, f)
            c.ran(family)
            collect(fmt, lambda: _against_oracle(got, ores, name + ' ' + fmt))
        # the exact path: the oracle-converted HLS crops through melf_read_dials
        exact = c.ctx.read_dials(np.stack([po.bgr2hls(f, op.hue_shift) for f in frames]))
        c.ran('hls')

        def equals_exact():
            for key in ('status', 'failed_dial', 'unreadable_mask', 'pos', 'angle', 'value'):
                assert np.array_equal(recs[key], exact[key]), (name, key, np.flatnonzero(np.any(np.atleast_2d(recs[key].T != exact[key].T), axis=0))[:8])
        collect('bgr against the exact path', equals_exact)
        for (tag, text) in failures:
            print('%s, %s: %s' % (name, tag, text))
        assert not failures, 'differing: ' + ', '.join(tag for (tag, _text) in failures)
    finally:
        c.close()
