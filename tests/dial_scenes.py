"""Directed scenes for the dial reader: one painted crop for every semantic the oracle restates (oracle/melf_oracle.c, ORC_OPT_*).

The parity tests feed the dial reader fixtures and random crops, and those reach few of the restated semantics (the polygon-area
rule, the first-of-equal-contours rule, erode's border, the trim's second sort key ...).  Each scene here is built so that one of
them decides the reading: flipping that switch in the oracle changes the scene's record (asserted on the CPU by
tests/test_dial_scenes.py), so a kernel that followed the flipped rule cannot equal the unflipped oracle on it.

A scene is a label map of template size (sample-images1: 188 x 119).  Label 0 is the background, label 1 the needle colour; the
range scenes define further labels.  Two palettes turn one label map into the input of either entry point: HLS crops for the
`hls` family (melf_read_dials) and BGR frames for the production path.  Every dial of every scene is painted readably (a 5 x 5
core, a plain needle on the side the dial's negative_momentum expects), and the dial under test then gets its structure; blobs
that must stay apart keep a gap of three pixels, since the 3 x 3 closing bridges two.

Nothing here needs a GPU.
"""
import copy
import functools

import numpy as np

from tests.test_dials_instantiations import _fixture_data, _params_dir, dial_radius, sweep_data

(TW, TH) = (188, 119)
LOW_THRESHOLD = -(1 << 40)   # below every TM_CCOEFF value of a 188 x 119 u8 template (|value| < 2^31): the match is always taken

# ---- palettes: label -> colour.  HLS: the crop's bytes as they are.  BGR: frames whose BGR2HLS_FULL (+ hue_shift 128) lies on
# the same side of every dial's range as the HLS colour of the label -- test_palettes_agree, through the oracle's conversion. ----
HLS_BACKGROUND = (20, 220, 10)
HLS_NEEDLE = (125, 80, 130)          # sample-images1's needle_color
BGR_BACKGROUND = (235, 235, 235)
BGR_NEEDLE = (40, 30, 200)

# angle (turns, clockwise from north) of the plain needle every dial gets unless the scene says otherwise
PLAIN_ANGLE = (0.30, 0.62, 0.85, 0.45)


class Scene:
    def __init__(self, name, geometry, dial, kills, status=0, unreadable=0, overrides=None, angles=None, n_kept=None):
        self.name = name
        self.geometry = geometry          # 'fixture' or 'r29'
        self.dial = dial                  # the dial under test
        self.kills = tuple(kills)         # the switches of pyoracle.OPTIONS whose flip changes this scene's record
        self.status = status              # what the unflipped oracle answers
        self.unreadable = unreadable
        self.overrides = overrides or {}  # dial index -> needle_data fields
        self.angles = list(angles or PLAIN_ANGLE)
        self.n_kept = n_kept              # the ring points the dial under test keeps (trim scenes)
        self.labels = np.zeros((TH, TW), np.uint8)
        self.hls = {0: HLS_BACKGROUND, 1: HLS_NEEDLE}
        self.bgr = {0: BGR_BACKGROUND, 1: BGR_NEEDLE}
        self.plain = [True] * 4           # dials still to get their plain needle

    # -- parameters --
    def context_key(self):
        return (self.geometry, repr(sorted((k, sorted(v.items())) for (k, v) in self.overrides.items())))

    def data(self):
        """The scene's params.yml: its geometry, the frame as meter_rect, a threshold every match passes, its overrides."""
        data = copy.deepcopy(_fixture_data() if self.geometry == 'fixture' else sweep_data(29))
        data['meter_rect'] = {'top_left': [0, 0], 'bottom_right': [TW, TH]}
        data['dials_template_match_threshold'] = LOW_THRESHOLD
        if self.geometry == 'r29':
            # dial 1 is the one of R = 29; a lone blob reads only on a dial of positive momentum
            data['needle_data'][1]['negative_momentum'] = False
        for (k, fields) in self.overrides.items():
            data['needle_data'][k].update(copy.deepcopy(fields))
        return data

    def centre(self, d):
        return tuple(self.data()['needle_data'][d]['center'])

    def radius(self, d):
        return dial_radius(self.data()['needle_data'][d])

    # -- painting --
    def rect(self, x0, y0, w, h, label=1):
        assert 0 <= x0 and x0 + w <= TW and 0 <= y0 and y0 + h <= TH, (self.name, x0, y0, w, h)
        self.labels[y0:y0 + h, x0:x0 + w] = label

    def core(self, d):
        (cx, cy) = self.centre(d)
        self.rect(int(cx) - 2, int(cy) - 2, 5, 5)

    def ray(self, d, angle, r0, r1, half_width, label=1):
        """A bar of 2 half_width + 1 pixels along the ray at `angle` from dial d's centre, radius r0 to r1."""
        (cx, cy) = self.centre(d)
        a = 2 * np.pi * angle
        (dx, dy) = (np.sin(a), -np.cos(a))
        for t in np.linspace(r0, r1, 8 * int(r1 - r0) + 1):
            for w in np.linspace(-half_width, half_width, 4 * half_width + 1):
                (x, y) = (int(np.floor(cx + t * dx + w * dy + 0.5)), int(np.floor(cy + t * dy - w * dx + 0.5)))
                if 0 <= x < TW and 0 <= y < TH:
                    self.labels[y, x] = label

    def finish(self):
        """The plain needle of every dial the scene has not painted itself."""
        negative = [bool(nd['negative_momentum']) for nd in self.data()['needle_data']]
        for d in range(4):
            if not self.plain[d]:
                continue
            R = self.radius(d)
            self.core(d)
            self.ray(d, self.angles[d], 0, R - 1, 1)
            if negative[d]:   # the heavy arm points away from the needle
                self.ray(d, self.angles[d] + 0.5, 0, R - 1, 3)
        self.labels.setflags(write=False)
        return self

    # -- the two inputs --
    def _paint(self, palette):
        out = np.empty((TH, TW, 3), np.uint8)
        for (label, colour) in palette.items():
            out[self.labels == label] = colour
        assert set(np.unique(self.labels)) <= set(palette), self.name
        return out

    def hls_crop(self):
        return self._paint(self.hls)

    def bgr_frame(self):
        return self._paint(self.bgr)


def params_file(scene):
    import zlib
    (geometry, overrides) = scene.context_key()
    return _params_dir(scene.data(), 'scene_%s_%08x' % (geometry, zlib.crc32(overrides.encode())))


# ------------------------------------------------------------------------------------------------------- the scenes -------
def _own(s, d):
    """Dial d gets no plain needle: only its core."""
    s.plain[d] = False
    s.core(d)
    (cx, cy) = s.centre(d)
    return (int(cx), int(cy))


def _tie2(geometry):
    """Two blobs of equal polygon area (> 100) above and below the core: the first in raster order is the needle."""
    if geometry == 'fixture':   # 9 x 14 pixels: polygon area 8 * 13 = 104, inside the disk
        s = Scene('tie2', geometry, 0, ['contour_tie'])
        (x, y) = _own(s, 0)
        s.rect(x - 4, y - 19, 9, 14)
        s.rect(x - 4, y + 6, 9, 14)
    else:   # dial 1, R = 29, window rows 55 .. 117, columns 63 .. 125: the bars run to the window's first and last rows, the
        # disk cuts both alike (one is the other turned by half a turn about the integral centre)
        s = Scene('tie2', geometry, 1, ['contour_tie'])
        (x, y) = _own(s, 1)
        s.rect(x - 8, y - 31, 12, 26)
        s.rect(x - 3, y + 6, 12, 26)
    return s.finish()


def _tie3(geometry):
    """Three equal blobs whose raster order (right, left, bottom) is not their order from left to right (left, bottom, right)."""
    if geometry == 'fixture':
        s = Scene('tie3', geometry, 0, ['contour_tie'])
        (x, y) = _own(s, 0)
        s.rect(x + 6, y - 7, 14, 9)
        s.rect(x - 19, y - 6, 14, 9)
        s.rect(x - 4, y + 6, 9, 14)
    else:   # to the window's last column, first column and last row; quarter and half turns of one bar about the integral centre
        s = Scene('tie3', geometry, 1, ['contour_tie'])
        (x, y) = _own(s, 1)
        s.rect(x + 6, y - 9, 26, 12)
        s.rect(x - 31, y - 2, 26, 12)
        s.rect(x - 2, y + 6, 12, 26)
    return s.finish()


def _area(geometry, half):
    """An 11 x 11 square above the core -- polygon area exactly 100 through the pixel centres, 121 pixels -- and a 5 x 6 blob to
    its upper right.  At 100 the contour is NOT taken and the needle is the whole mask; `half` adds one pixel above the square's
    corner (area 100.5), and the square alone is the needle."""
    d = 0 if geometry == 'fixture' else 1
    s = Scene('area100_5' if half else 'area100', geometry, d, [] if half else ['area_rule', 'area_ge'])
    (x, y) = _own(s, d)
    s.rect(x - 5, y - 17, 11, 11)
    s.rect(x + 10, y - 19, 5, 6)
    if half:
        s.rect(x - 5, y - 18, 1, 1)    # above the corner pixel: a triangle of half a pixel
    return s.finish()


def _erode_top():
    """Dial 0 moved up so that its disk reaches crop row 0, with a three-pixel needle running to row 0: a zero border would
    erode the needle's end rows away."""
    s = Scene('erode_top', 'fixture', 0, ['erode_border'], overrides={0: {'center': [37.3, 15.4]}})
    (x, y) = _own(s, 0)
    s.rect(x - 1, 0, 3, y)
    return s.finish()


def _erode_right():
    """The same on the crop's last column, dial 3."""
    s = Scene('erode_right', 'fixture', 3, ['erode_border'], overrides={3: {'center': [172.4, 36.5]}})
    (x, y) = _own(s, 3)
    s.rect(x, y - 1, TW - x, 3)
    return s.finish()


def _ring_island(geometry):
    """A closed ring with an island in its hole, over the annulus: the island is no external contour, and the fill paints hole and
    island alike."""
    d = 0 if geometry == 'fixture' else 1
    s = Scene('ring_island', geometry, d, ['no_hole_fill'])
    (x, y) = _own(s, d)
    s.rect(x - 6, y - 21, 15, 15)
    s.rect(x - 3, y - 18, 9, 9, label=0)
    s.rect(x, y - 15, 3, 3)
    return s.finish()


def _unwrap(north):
    """A needle due north on dial 0's fractional centre: ring angles on both sides of 0 / 1.  North-east: nothing to unwrap."""
    s = Scene('unwrap_north' if north else 'unwrap_north_east', 'fixture', 0, ['no_unwrap'] if north else [])
    _own(s, 0)
    s.ray(0, 0.0 if north else 0.125, 0, 20, 1)
    return s.finish()


def _trim(n):
    """A one-pixel needle on dial 0 whose tip leaves exactly n ring points (the annulus starts at radius 12): the cut is
    min(2, (n - 3) // 2) from each end, and none below five."""
    s = Scene('trim_%d' % n, 'fixture', 0, ['trim_cut'] if n in (5, 6) else [], n_kept=n)
    (x, y) = _own(s, 0)
    s.rect(x, y - 11 - n, 1, 11 + n)
    return s.finish()


def _trim_key():
    """A one-pixel vertical needle below dial 1's integral centre: its ring points share one exact angle and differ in distance
    only; three more pixels beside its tip have smaller angles, so the cut of two falls inside the group of equal angles."""
    s = Scene('trim_key', 'fixture', 1, ['trim_key'])
    (x, y) = _own(s, 1)
    s.rect(x, y, 1, 21)
    s.rect(x + 1, y + 18, 1, 3)
    s.rect(x - 4, y - 20, 9, 20)    # the heavy arm of a negative-momentum dial
    return s.finish()


# needle angles whose positions land in every branch of determine_value_by_dial_positions (test_carry_branches asserts which);
# the last three sit between the reference's thresholds and one half: the carry_half mutant reads another digit there
CARRY_POSITIONS = {
    'carry_up_wrap': (1.0, 9.7, 4.7, 2.8),        # d3: 9 + 1 -> 0, d2: + 1, d1: none
    'carry_down_wrap': (9.0, 0.2, 3.3, 0.3),      # d3: 0 - 1 -> 9, d2: - 1, d1: none
    'carry_up_high': (5.0, 1.5, 9.8, 9.9),        # d3: none, d2: 9 + 1 -> 0, d1: 9 + 1 -> 0
    'carry_down_high': (5.0, 8.5, 0.1, 0.2),      # d3: none, d2: 0 - 1 -> 9, d1: 0 - 1 -> 9
    'carry_half_d3_up': (1.0, 3.525, 6.0, 6.0),
    'carry_half_d3_down': (9.0, 3.475, 6.0, 6.0),
    'carry_half_d2_up': (5.0, 1.2, 6.525, 6.0),
    'carry_half_d2_down': (5.0, 9.2, 6.475, 6.0),
    'carry_half_d1_up': (5.0, 1.2, 1.7, 4.525),
    'carry_half_d1_down': (5.0, 9.2, 8.7, 4.475),
}


def _carry(name):
    angles = [(p / 10.0 - 4.5 / 360.0) % 1.0 for p in CARRY_POSITIONS[name]]   # angle_of_zero is -4.5 degrees on every dial
    return Scene(name, 'fixture', 1, ['carry_half'] if 'half' in name else [], angles=angles).finish()


def _zero(geometry, central):
    """On dial 1's integral centre.  central: a point-symmetric cross, momentum exactly (0, 0), the dial unreadable.  Otherwise a
    scene symmetric about the horizontal axis only: momentum_y is exactly 0, the momentum angle exactly 0.25 or 0.75, and the one
    pixel row on the needle's side gives ring points of that exact angle."""
    s = Scene(('zero_central' if central else 'zero_horizontal'), geometry, 1, [], status=3 if central else 0,
              unreadable=2 if central else 0)
    (x, y) = _own(s, 1)
    R = s.radius(1) + 2    # to the window's first and last columns (rows)
    if central:
        s.rect(x - R, y - 1, 2 * R + 1, 3)
        s.rect(x - 1, y - R, 3, 2 * R + 1)
    else:
        s.rect(x - R, y, R, 1)
        s.rect(x, y - 3, R + 1, 7)
    return s.finish()


# ---- the range scenes.  Labels 2 + 2 c + k lie ON bound k (0 lower, 1 upper) of channel c (H, L, S) of dial 2's range around
# the scene's own core colour (color_range h 10, l 45, s 50), the other channels inside; labels 8 + 2 c + k lie ONE STEP OUTSIDE
# that bound.  Where a bound is clamped at 0 / 255 nothing lies outside it, and the label takes the colour outside the channel's
# other bound.  The BGR triples were found by searching all 2^24 conversions; test_range_labels_sit_on_the_bounds holds both
# palettes to the above through the oracle's conversion. ----
RANGE_OF_DIAL_2 = (10, 45, 50)
RANGE_COLOURS = {
    # every bound free
    'range_edges': dict(hls_core=(125, 80, 130), bgr={
        1: (40, 30, 200), 2: (95, 47, 209), 3: (44, 72, 209), 4: (29, 15, 124), 5: (87, 103, 232), 6: (69, 56, 188), 7: (27, 8, 233),
        8: (100, 45, 209), 9: (56, 86, 209), 10: (28, 16, 122), 11: (102, 88, 233), 12: (86, 57, 189), 13: (17, 8, 242)}),
    # HLS: the lower bounds of H and L clamped at 0, the upper bound of S at 255.  BGR (core converts to (137, 27, 24)): the lower
    # bounds of L and S clamped at 0 -- black is the only colour of L = 0, and lies on both
    'range_clamped': dict(hls_core=(5, 30, 230), bgr={
        1: (24, 25, 29), 2: (51, 50, 81), 3: (45, 55, 67), 4: (0, 0, 0), 5: (56, 58, 87), 6: (36, 36, 36), 7: (39, 49, 71),
        8: (45, 44, 69), 9: (39, 53, 69), 10: (58, 65, 88), 11: (58, 65, 88), 12: (42, 44, 77), 13: (42, 44, 77)}),
}


def range_bounds(core):
    return ([max(core[c] - RANGE_OF_DIAL_2[c], 0) for c in range(3)], [min(core[c] + RANGE_OF_DIAL_2[c], 255) for c in range(3)])


def _range(name):
    """Dial 2.  The needle is six segments of two rows, each on one bound of one channel: a closed range keeps them all, an open
    one none.  Beside every segment lies a patch one step outside that bound, which no range takes -- taken, it would be one blob
    with the needle."""
    s = Scene(name, 'fixture', 2, ['inrange_open'])
    core = RANGE_COLOURS[name]['hls_core']
    (lo, hi) = range_bounds(core)
    s.hls[1] = core
    for c in range(3):
        for k in range(2):
            (on, out) = (list(core), list(core))
            on[c] = (lo, hi)[k][c]
            out[c] = on[c] + (-1, 1)[k]
            if not 0 <= out[c] <= 255:
                out[c] = (hi[c] + 1, lo[c] - 1)[k]
            s.hls[2 + 2 * c + k] = tuple(on)
            s.hls[8 + 2 * c + k] = tuple(out)
    s.bgr.update(RANGE_COLOURS[name]['bgr'])
    (x, y) = _own(s, 2)
    for seg in range(6):
        s.rect(x - 1, y - 4 - 2 * seg, 3, 2, label=2 + seg)    # radius 3 to 14: the annulus of dial 2 starts at 10
        s.rect(x + 2, y - 4 - 2 * seg, 3, 2, label=8 + seg)
    return s.finish()


# ---- the template mean (cv::mean as sum * (1. / N)): a 9 x 11 template and constant images, for which the exact value is 0 and
# the two forms of the mean leave different rounding residues (test_mean_form_template_case) ----
MEAN_FORM_TEMPLATE = dict(seed=2, th=9, tw=11, rows=64, cols=70)


def mean_form_case():
    """(template, images): constant images 1 .. 32 for the seeded random template."""
    m = MEAN_FORM_TEMPLATE
    tpl = np.random.default_rng(m['seed']).integers(0, 256, size=(m['th'], m['tw']), dtype=np.uint8)
    imgs = np.stack([np.full((m['rows'], m['cols']), c, np.uint8) for c in range(1, 33)])
    return (tpl, imgs)


@functools.lru_cache(maxsize=None)
def scenes():
    out = []
    for g in ('fixture', 'r29'):
        out += [_tie2(g), _tie3(g), _area(g, False), _area(g, True), _ring_island(g), _zero(g, True), _zero(g, False)]
    out += [_erode_top(), _erode_right(), _unwrap(True), _unwrap(False)]
    out += [_trim(n) for n in (4, 5, 6, 7, 8)]
    out += [_trim_key()]
    out += [_carry(name) for name in CARRY_POSITIONS]
    out += [_range('range_edges'), _range('range_clamped')]
    assert len({(s.name, s.geometry) for s in out}) == len(out)
    return tuple(out)


def contexts():
    """The scenes grouped by the parameters they read with: {key: [scene, ...]}."""
    by = {}
    for s in scenes():
        by.setdefault(s.context_key(), []).append(s)
    return by
