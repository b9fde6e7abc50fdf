"""The record stage of the dial reader (k_dials_body.inc's error aggregation and digit combine, launch_dials, write_record) and
the parameters that feed it: dial sets of one to eight dials, frames whose dials fail in a chosen way, and a plain-Python
restatement of the rule that turns per-dial outcomes into a record.

The other dial tests launch four dials (three to six in one random test) whose names sort in file order, and reach the failure
rule through random crops only.  Here:

* dial_set(n) gives needle_data for n = 1 .. 8 dials on the fixture's 188 x 119 template, on a 4 x 2 grid, every dial different
  from every other in each of its parameters, its window inside the crop; the default names do NOT sort in file order;
* paint(data, kinds, angles) paints every dial as one of three kinds -- 'ok' (core, needle, and the heavy opposite arm a
  negative-momentum dial needs: Scene.finish's needle), 'unread' (the core alone: a needle mask without a ring point) and 'none'
  (a checker core of two colours whose mean has neither in range: no mask pixel in the disk) -- as a label map, which two
  palettes turn into the input of either entry point, as tests/dial_scenes.py does;
* reference_record(names, per_dial) restates meterelf/_reading.py:98-111 and :163-182 with sorted, % and int: nothing of
  oracle/ and nothing of the package.

Nothing here needs a GPU.
"""
import copy
import functools
import itertools

import numpy as np

from tests.dial_scenes import BGR_BACKGROUND, BGR_NEEDLE, HLS_BACKGROUND, HLS_NEEDLE, LOW_THRESHOLD, TH, TW
from tests.test_dials_instantiations import _fixture_data, _params_dir, dial_radius, py_round

MAX_DIALS = 8
KINDS = ('ok', 'unread', 'none')

# ---- the dial set.  Grid: four columns 46 apart, two rows 62 apart; R <= 20, so a window (2 R + 5 = 45 rows, 12 pieces of four
# columns) stays inside the crop and neighbouring disks, grown by the closing's two pixels, stay apart.  Some centres integral,
# some fractional (the core is cut around int(), the masks are drawn around round()). ----
CENTRES = ((23.0, 28.0), (69.4, 27.4), (115.5, 28.5), (161.0, 29.0), (23.7, 89.0), (69.0, 90.3), (115.0, 88.6), (160.3, 90.0))
DIAMETERS = (10, 12, 8, 14, 9, 16, 6, 11)
DISTS = (3, 2, 4, 1, 5, 6, 7, 8)
THICKNESSES = (13, 12, 10, 11, 9, 7, 8, 6)
ANGLES_OF_ZERO = (-4.5, 3.0, -12.5, 8.25, 0.0, -7.75, 15.5, -1.25)
RANGES = tuple((10 + 4 * k, 45 + 5 * k, 50 + 6 * k) for k in range(MAX_DIALS))
NEGATIVE = (False, True, False, True, True, False, False, True)
DEFAULT_NAMES = ('m3', 'm1', 'm7', 'm0', 'm5', 'm2', 'm6', 'm4')   # in no prefix's sorted order, except the first alone
FIXTURE_NAMES = ('0.0001', '0.001', '0.01', '0.1')

# labels of the painter: background, the needle colour, the two colours of a 'none' dial's checker core
(BACKGROUND, NEEDLE, CHECK_A, CHECK_B) = range(4)
HLS_PALETTE = {BACKGROUND: HLS_BACKGROUND, NEEDLE: HLS_NEEDLE, CHECK_A: (125, 0, 130), CHECK_B: (125, 255, 130)}
BGR_PALETTE = {BACKGROUND: BGR_BACKGROUND, NEEDLE: BGR_NEEDLE, CHECK_A: (0, 0, 0), CHECK_B: (255, 255, 255)}


def dial_set(n, names=None):
    """needle_data of n dials."""
    assert 1 <= n <= MAX_DIALS
    names = list(DEFAULT_NAMES[:n] if names is None else names)
    assert len(names) == n and len(set(names)) == n
    out = []
    for k in range(n):
        (h, l, s) = RANGES[k]
        out.append({'name': names[k], 'color_range': {'h': h, 'l': l, 's': s}, 'dist_from_center': DISTS[k],
                    'circle_thickness': THICKNESSES[k], 'angle_of_zero': ANGLES_OF_ZERO[k], 'center': list(CENTRES[k]),
                    'diameter': DIAMETERS[k], 'negative_momentum': NEGATIVE[k]})
    return out


def whole_frame(data):
    """data with the template-sized frame as its meter_rect and a threshold every match passes: the match is (0, 0), 1 x 1."""
    data = copy.deepcopy(data)
    data['meter_rect'] = {'top_left': [0, 0], 'bottom_right': [TW, TH]}
    data['dials_template_match_threshold'] = LOW_THRESHOLD
    return data


def set_data(n, names=None):
    """The fixture's params.yml with dial_set(n, names) as its dials."""
    data = whole_frame(_fixture_data())
    data['needle_data'] = dial_set(n, names)
    return data


def renamed_fixture(names):
    """The fixture's own four dials under other names (the geometry the carry scenes of tests/dial_scenes.py are painted for)."""
    data = whole_frame(_fixture_data())
    assert [nd['name'] for nd in data['needle_data']] == list(FIXTURE_NAMES)
    for (nd, name) in zip(data['needle_data'], names):
        nd['name'] = name
    return data


def params_file(data, tag):
    return _params_dir(data, 'records_' + tag)


def windows_inside(data):
    """Every dial's window, as the kernel cuts it (2 R + 5 rows, whole pieces of four columns), lies inside the crop."""
    for nd in data['needle_data']:
        R = dial_radius(nd)
        (wx0, wy0, ws) = (py_round(nd['center'][0]) - R - 2, py_round(nd['center'][1]) - R - 2, 2 * R + 5)
        if not (R <= 20 and wx0 >= 0 and wx0 + 4 * ((ws + 3) >> 2) <= TW and wy0 >= 0 and wy0 + ws <= TH):
            return False
    return True


# ---- the painter ----
def _ray(labels, centre, angle, r0, r1, half_width):
    """Scene.ray of tests/dial_scenes.py: a bar of 2 half_width + 1 pixels along the ray at `angle` (turns, clockwise from north)."""
    (cx, cy) = centre
    a = 2 * np.pi * angle
    (dx, dy) = (np.sin(a), -np.cos(a))
    (t, w) = np.meshgrid(np.linspace(r0, r1, 8 * int(r1 - r0) + 1), np.linspace(-half_width, half_width, 4 * half_width + 1))
    (x, y) = (np.floor(cx + t * dx + w * dy + 0.5).astype(int), np.floor(cy + t * dy - w * dx + 0.5).astype(int))
    assert x.min() >= 0 and x.max() < TW and y.min() >= 0 and y.max() < TH
    labels[y, x] = NEEDLE


def paint(data, kinds, angles):
    """The label map of one frame: dial d painted as kinds[d], its needle (kind 'ok') at angles[d]."""
    nds = data['needle_data']
    assert len(kinds) == len(nds) == len(angles) and set(kinds) <= set(KINDS)
    labels = np.zeros((TH, TW), np.uint8)
    for (nd, kind, angle) in zip(nds, kinds, angles):
        (cx, cy) = nd['center']
        (x, y) = (int(cx), int(cy))
        if kind == 'none':
            for j in range(-2, 3):
                for i in range(-2, 3):
                    labels[y + j, x + i] = CHECK_A if (i + j) % 2 == 0 else CHECK_B   # thirteen of A, twelve of B
            continue
        labels[y - 2:y + 3, x - 2:x + 3] = NEEDLE
        if kind == 'ok':
            R = dial_radius(nd)
            _ray(labels, (cx, cy), angle, 0, R - 1, 1)
            if nd['negative_momentum']:   # the heavy arm points away from the needle
                _ray(labels, (cx, cy), angle + 0.5, 0, R - 1, 3)
    return labels


def colour(labels, palette):
    out = np.empty(labels.shape + (3,), np.uint8)
    for (label, c) in palette.items():
        out[labels == label] = c
    return out


def hls_crops(label_maps):
    return np.stack([colour(m, HLS_PALETTE) for m in label_maps])


def bgr_frames(label_maps):
    return np.stack([colour(m, BGR_PALETTE) for m in label_maps])


def angle_for(nd, position):
    """The needle angle at which dial nd reads `position`."""
    return (position / 10.0 + nd['angle_of_zero'] / 360.0) % 1.0


# ---- the frame sets ----
def count_frames(n, nframes=16):
    """All dials readable, needle angles that differ from dial to dial and from frame to frame."""
    data = set_data(n)
    return [paint(data, ['ok'] * n, [(0.03 + 0.0625 * f + 0.137 * d) % 1.0 for d in range(n)]) for f in range(nframes)]


def failure_mixes(n):
    """[(kinds, why)]: one readable frame, every single 'none', every ordered pair ('none' at i, 'unread' at j != i), every
    pair of 'none', every one of the 2^n - 1 'unread' subsets."""
    out = [(['ok'] * n, 'ok')]

    def frame(**at):
        kinds = ['ok'] * n
        for (kind, where) in at.items():
            for d in where:
                kinds[d] = kind
        return kinds
    for i in range(n):
        out.append((frame(none=[i]), 'none %d' % i))
    for i in range(n):
        for j in range(n):
            if i != j:
                out.append((frame(none=[i], unread=[j]), 'none %d unread %d' % (i, j)))
    for (i, j) in itertools.combinations(range(n), 2):
        out.append((frame(none=[i, j]), 'none %d %d' % (i, j)))
    for mask in range(1, 1 << n):
        out.append((frame(unread=[d for d in range(n) if mask >> d & 1]), 'unread %#x' % mask))
    return out


@functools.lru_cache(maxsize=None)
def mix_frames(n):
    """(label maps, [kinds]) of failure_mixes(n); the readable dials' needles turn with the frame."""
    data = set_data(n)
    mixes = failure_mixes(n)
    maps = [paint(data, kinds, [(0.11 + 0.019 * f + 0.21 * d) % 1.0 for d in range(n)]) for (f, (kinds, _why)) in enumerate(mixes)]
    return (maps, [kinds for (kinds, _why) in mixes])


def expected_of_kinds(kinds):
    """(status, failed dial, mask) the kinds of a frame's dials must give, by the rule in words: the first 'none' in file order
    wins, the 'unread' before it are remembered, later ones never looked at; without a 'none', every 'unread' is in the mask."""
    if 'none' in kinds:
        i = list(kinds).index('none')
        return (2, i, sum(1 << d for d in range(i) if kinds[d] == 'unread'))
    mask = sum(1 << d for (d, k) in enumerate(kinds) if k == 'unread')
    return (3 if mask else 0, -1, mask)


# three plain frames of the fixture's dials: four distinct integer parts each, fractions near one half (no carry)
PLAIN_POSITIONS = ((1.5, 4.5, 7.5, 9.5), (8.5, 2.5, 0.5, 5.5), (3.5, 6.5, 9.5, 0.5))
NAME_ASSIGNMENTS = tuple(itertools.permutations(range(4)))   # p: dial i is named FIXTURE_NAMES[p[i]]; the first is the identity


def assignment_names(p):
    return [FIXTURE_NAMES[k] for k in p]


@functools.lru_cache(maxsize=None)
def name_order_scenes():
    """The carry_* scenes of tests/dial_scenes.py and three plain frames, all on the fixture's geometry: (names, label maps)."""
    from tests import dial_scenes as ds
    carry = [s for s in ds.scenes() if s.name.startswith('carry')]
    assert len(carry) == len(ds.CARRY_POSITIONS) and all(s.geometry == 'fixture' and not s.overrides for s in carry)
    nds = _fixture_data()['needle_data']
    plain = [ds.Scene('plain_%d' % k, 'fixture', 0, [], angles=[angle_for(nd, p) for (nd, p) in zip(nds, pos)]).finish()
             for (k, pos) in enumerate(PLAIN_POSITIONS)]
    scenes = carry + plain
    assert all(set(np.unique(s.labels)) <= {BACKGROUND, NEEDLE} for s in scenes)
    return ([s.name for s in scenes], [s.labels for s in scenes])


# ---- the rule, restated ----
def value_by_positions(names, positions):
    """determine_value_by_dial_positions (meterelf/_reading.py:163-182) of {name: position}."""
    assert len(names) == len(positions) == 4
    (r4, r3, r2, r1) = [x for (_, x) in sorted(zip(names, positions))]
    d3 = (int(r3) + (1 if r3 % 1.0 > 0.55 and r4 <= 2 else 0) - (1 if r3 % 1.0 < 0.45 and r4 >= 8 else 0)) % 10
    d2 = (int(r2) + (1 if r2 % 1.0 > 0.55 and d3 <= 2 else 0) - (1 if r2 % 1.0 < 0.45 and d3 >= 8 else 0)) % 10
    d1 = (int(r1) + (1 if r1 % 1.0 > 0.55 and d2 <= 2 else 0) - (1 if r1 % 1.0 < 0.45 and d2 >= 8 else 0)) % 10
    return (d1 * 100.0) + (d2 * 10.0) + (d3 * 1.0) + r4 / 10.0


def reference_record(names, per_dial):
    """per_dial[d], in file order: a float (the dial's position), 'none' (no contours) or 'unread' (no kept ring point).
    Returns dict(status, failed_dial, mask, value, result): `result` is what the Python layer must produce -- the dict of
    get_meter_value, or the message of the exception it raises.  The loop of meterelf/_reading.py:28-96 raises at the first dial
    without contours (the unreadable ones before it stay in the record's mask, the reference never reports them); :98-106 raise
    for the unreadable dials, named in file order; :108-111 add 'value' -- the digit combine asserts four dials, and a record of
    another count carries none."""
    assert len(names) == len(per_dial)
    positions = {}
    unreadable = []
    for (d, (name, outcome)) in enumerate(zip(names, per_dial)):
        if isinstance(outcome, str) and outcome == 'none':
            return dict(status=2, failed_dial=d, mask=sum(1 << names.index(u) for u in unreadable), value=0.0,
                        result='Cannot find needle contours of a dial (dial = %s)' % name)
        if isinstance(outcome, str):
            assert outcome == 'unread'
            unreadable.append(name)
            continue
        positions[name] = float(outcome)
    if unreadable:
        return dict(status=3, failed_dial=-1, mask=sum(1 << names.index(u) for u in unreadable), value=0.0,
                    result='Cannot determine angle of a dial (unreadable dials = %s)' % ', '.join(unreadable))
    result = dict(positions)
    value = 0.0
    if len(names) == 4:
        value = value_by_positions(list(names), [positions[k] for k in names])
        result['value'] = value
    return dict(status=0, failed_dial=-1, mask=0, value=value, result=result)


def outcomes_of(status, failed_dial, mask, positions, n):
    """The per-dial outcomes a record states (what reference_record is fed with to check a record against itself)."""
    out = []
    for d in range(n):
        if status == 2 and d == failed_dial:
            out.append('none')
        elif mask >> d & 1:
            out.append('unread')
        else:
            out.append(float(positions[d]))
    return out


# ---- wrong rules (test_wrong_rules_separate: each must answer differently from reference_record somewhere) ----
def order_of(names):
    return sorted(range(len(names)), key=names.__getitem__)


def value_in_order(order, positions):
    """The digit combine as the kernel runs it with a name_order array: (r4, r3, r2, r1) = positions[order[k]].  Giving dial
    order[k] the k-th of four sorted names makes sorted() visit the dials in that order."""
    names = [None] * 4
    for (k, d) in enumerate(order):
        names[d] = 'abcd'[k]
    return value_by_positions(names, list(positions))


def inverse(order):
    inv = [0] * len(order)
    for (k, d) in enumerate(order):
        inv[d] = k
    return inv


NAME_ORDER_RULES = {
    'identity': lambda order: [0, 1, 2, 3],
    'inverse': inverse,
    'reversed': lambda order: list(reversed(order)),
}


def precedence_rule(rule, kinds):
    """(status, failed dial, mask) of a wrong failure rule."""
    n = len(kinds)
    nones = [d for d in range(n) if kinds[d] == 'none']
    unread = sum(1 << d for d in range(n) if kinds[d] == 'unread')
    if rule == 'last_failing':
        if nones:
            return (2, nones[-1], unread & ((1 << nones[-1]) - 1))
    elif rule == 'unreadable_first':
        if unread:
            return (3, -1, unread)
        if nones:
            return (2, nones[0], 0)
    elif rule == 'mask_uncut':
        if nones:
            return (2, nones[0], unread)
    elif rule == 'mask_first_bit':
        keep = unread & -unread
        if nones:
            return (2, nones[0], keep & ((1 << nones[0]) - 1))
        return (3 if keep else 0, -1, keep)
    else:
        raise KeyError(rule)
    return (3 if unread else 0, -1, unread)


PRECEDENCE_RULES = ('last_failing', 'unreadable_first', 'mask_uncut', 'mask_first_bit')
