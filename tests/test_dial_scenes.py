"""The directed scenes of tests/dial_scenes.py: that each one reaches the semantic it is there for (CPU), and that the dial reader
equals the oracle on all of them (GPU).

CPU: the unflipped oracle reads every scene as the scene declares; for every (scene, switch) pair the table names, flipping the
switch changes the scene's record -- in status, failed_dial or unreadable_mask, in a position by more than 1e-6 (a thousand times
the parity tests' POS_TOL, so a kernel that followed the flipped rule cannot pass within tolerance), or, for the digit carry, which
moves no position, in a digit of the value; every switch of pyoracle.OPTIONS has a killing scene, a separating input of the stage
it belongs to, or a proof that no input can reach it; the two palettes of a scene fall on the same side of every range.

GPU: one batch of all scenes per context.  The HLS crops through melf_read_dials, the BGR frames -- whole frames of template size,
meter_rect the frame, so the match map is 1 x 1 -- through read_frames, both against the oracle with the bars of
tests/test_gpu_parity.py, the kernel that ran asserted after every call.
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
from tests import dial_scenes as ds  # noqa: E402
from tests.test_dials_instantiations import _Ctx, expected_nr, ws_max_of  # noqa: E402
from tests.test_gpu_parity import POS_TOL, _compare_records, _reader_with_template  # noqa: E402

KILL_TOL = 1e-6
assert KILL_TOL >= 999 * POS_TOL   # a thousand times the parity bar (999: 1000 * 1e-9 rounds above 1e-6)

SCENES = ds.scenes()
IDS = ['%s-%s' % (s.name, s.geometry) for s in SCENES]
KILLS = [(s, k) for s in SCENES for k in s.kills]

# Switches no dial scene can kill, and the test that stands for each.
# The HLS conversion and minMaxLoc come before the dial stage; a separating input of their own stage is asserted instead.
OTHER_STAGE = {
    'hls_variant': 'test_hls_switches_have_separating_triples',
    'hls_round': 'test_hls_switches_have_separating_triples',
    'l_integer': 'test_hls_switches_have_separating_triples',
    'minmax_last': 'test_minmax_last_has_a_separating_map',
    'mean_form': 'test_mean_form_template_case',         # the template-mean half; the dial-colour half is unreachable, below
}
# Semantics no input reaches: both forms give the same bytes, by exhaustion.
UNREACHABLE = {
    'mean_form (dial colour)': 'test_mean_form_cannot_change_a_dial_colour',
    'hue_g_first': 'test_hue_g_first_cannot_change_a_pixel',
}


@functools.lru_cache(maxsize=None)
def oparams(key):
    (scene,) = [s for s in SCENES if s.context_key() == key][:1]
    return po.Params(ds.params_file(scene))


def record(o):
    return dict(status=o.status, failed_dial=o.failed_dial, unreadable_mask=o.unreadable_mask, pos=list(o.pos)[:4], value=o.value)


def differs(a, b):
    if (a['status'], a['failed_dial'], a['unreadable_mask']) != (b['status'], b['failed_dial'], b['unreadable_mask']):
        return True
    if a['status'] != 0:
        return False
    if max(abs(x - y) for (x, y) in zip(a['pos'], b['pos'])) > KILL_TOL:
        return True
    return int(a['value']) != int(b['value'])   # the three digits


@functools.lru_cache(maxsize=None)
def base(i):
    """The unflipped oracle's reading of scene i's HLS crop: computed once, shared."""
    s = SCENES[i]
    return po.read_dials(s.hls_crop(), oparams(s.context_key()))


def flipped(i, switch):
    s = SCENES[i]
    po.set_option(switch, 1)
    try:
        return po.read_dials(s.hls_crop(), oparams(s.context_key()))
    finally:
        po.set_option(switch, 0)


# ------------------------------------------------------------------------------------------------------------- CPU ---------
@pytest.mark.parametrize('i', range(len(SCENES)), ids=IDS)
def test_scene_reads_as_declared(i):
    s = SCENES[i]
    o = base(i)
    assert (o.status, o.unreadable_mask) == (s.status, s.unreadable), (s.name, o.status, o.unreadable_mask)
    if s.n_kept is not None:
        assert o.n_kept[s.dial] == s.n_kept
    area = o.contour_area[s.dial]
    if s.name.startswith('tie'):
        assert area > 100
    if s.name == 'area100':
        assert area == 100.0 and o.n_needle[s.dial] > 121      # not taken: the needle is the whole mask
    if s.name == 'area100_5':
        assert area == 100.5 and o.n_needle[s.dial] == 122     # taken: the square and its extra pixel alone
    if s.name == 'zero_horizontal':
        # momentum_y is exactly zero: the momentum angle is exactly a quarter; on the fixture's dial the kept ring points lie
        # on the one row through the integral centre, and their mean is exact as well
        assert o.status == 0
        want = 0.75 if s.geometry == 'fixture' else 0.25
        assert abs(o.angle[1] - want) < 1e-12 and (s.geometry != 'fixture' or o.angle[1] == want)
    if s.name == 'unwrap_north_east':
        assert not differs(record(o), record(flipped(i, 'no_unwrap')))   # the correct path unwraps nothing here


@pytest.mark.parametrize('i,switch', [(SCENES.index(s), k) for (s, k) in KILLS], ids=['%s-%s-%s' % (s.name, s.geometry, k) for (s, k) in KILLS])
def test_flipping_the_switch_changes_the_scene(i, switch):
    (a, b) = (record(base(i)), record(flipped(i, switch)))
    assert differs(a, b), (SCENES[i].name, switch, a, b)


def test_every_switch_has_a_killing_scene_or_a_proof():
    killed = {k for (_s, k) in KILLS}
    here = globals()
    for name in po.OPTIONS:
        assert name in killed or name in OTHER_STAGE or name in UNREACHABLE, name
    for fn in list(OTHER_STAGE.values()) + list(UNREACHABLE.values()):
        assert callable(here[fn]), fn
    # every dial-stage switch is killed by a scene, at both geometries where the issue asks for both
    for name in ('contour_tie', 'area_rule', 'area_ge', 'no_hole_fill', 'erode_border', 'no_unwrap', 'trim_cut', 'trim_key', 'carry_half',
                 'inrange_open'):
        assert name in killed, name
    for name in ('contour_tie', 'area_rule', 'area_ge', 'no_hole_fill'):
        assert {s.geometry for (s, k) in KILLS if k == name} == {'fixture', 'r29'}, name
    assert {s.n_kept for s in SCENES if s.n_kept is not None} == {4, 5, 6, 7, 8}


def test_scenes_reach_the_edges_they_name():
    by = {(s.name, s.geometry): s for s in SCENES}
    # R = 29: dial 1's window is rows 55 .. 117, columns 63 .. 125, and the kernels hold 64 rows
    data = by[('tie2', 'r29')].data()
    assert ws_max_of(data) == 63 and expected_nr(63) == 64 and expected_nr(ws_max_of(by[('tie2', 'fixture')].data())) == 48
    (t2, t3, zc) = (by[('tie2', 'r29')].labels, by[('tie3', 'r29')].labels, by[('zero_central', 'r29')].labels)
    assert t2[55].any() and t2[117].any()
    assert t3[:, 63].any() and t3[:, 125].any() and t3[117].any()
    assert zc[55].any() and zc[117].any() and zc[:, 63].any() and zc[:, 125].any()
    # the erode scenes: needle pixels of the disk on the crop's first row / last column
    for (name, d, where) in (('erode_top', 0, np.s_[0, :]), ('erode_right', 3, np.s_[:, ds.TW - 1])):
        s = by[(name, 'fixture')]
        disk = oparams(s.context_key()).masks()[d, 0]
        assert ((s.labels == 1) & (disk > 0))[where].sum() == 3, name
    # the threshold of the area rule lies between the two area scenes
    for g in ('fixture', 'r29'):
        (a, b) = (base(SCENES.index(by[('area100', g)])), base(SCENES.index(by[('area100_5', g)])))
        assert differs(record(a), record(b)), g
    # the ring's island is inside the hole, and apart from the ring
    ring = by[('ring_island', 'fixture')]
    (n, _area, _filled) = po.largest_contour(((ring.labels == 1) & (oparams(ring.context_key()).masks()[0, 0] > 0)).astype(np.uint8) * 255)
    assert n == 2    # the core and the ring: the island is no external contour


def test_carry_branches():
    """The carry scenes' positions, as the oracle reads them, take every branch of determine_value_by_dial_positions
    (meterelf/_reading.py:163-182) at each digit, the 9 -> 0 and 0 -> 9 wraps included; the carry_half scenes sit between the
    reference's thresholds and one half."""
    seen = set()
    for (i, s) in enumerate(SCENES):
        if not s.name.startswith('carry'):
            continue
        o = base(i)
        (r4, r3, r2, r1) = list(o.pos)[:4]     # the dials' names sort in the file's order
        lower = r4
        digits = []
        for (k, r) in ((3, r3), (2, r2), (1, r1)):
            step = (1 if r % 1.0 > 0.55 and lower <= 2 else 0) - (1 if r % 1.0 < 0.45 and lower >= 8 else 0)
            seen.add((k, step))
            if int(r) + step in (-1, 10):
                seen.add((k, 'wrap', step))
            if s.name == 'carry_half_d%d_up' % k:
                assert 0.5 < r % 1.0 < 0.55 and lower <= 2, s.name
            if s.name == 'carry_half_d%d_down' % k:
                assert 0.45 < r % 1.0 < 0.5 and lower >= 8, s.name
            lower = (int(r) + step) % 10
            digits.append(lower)
        want = digits[2] * 100.0 + digits[1] * 10.0 + digits[0] + r4 / 10.0
        assert o.value == want, (s.name, o.value, want)
    assert seen >= {(k, step) for k in (1, 2, 3) for step in (-1, 0, 1)} | {(k, 'wrap', step) for k in (1, 2, 3) for step in (-1, 1)}, seen


def _inrange(hls, lo, hi):
    return np.all((hls >= np.array(lo)) & (hls <= np.array(hi)), axis=-1)


@pytest.mark.parametrize('i', range(len(SCENES)), ids=IDS)
def test_palettes_agree(i):
    """The BGR frame, converted by the oracle, lies inside and outside every dial's range exactly where the HLS crop does --
    over the dial's disk grown by two pixels, beyond which no pixel reaches the dial's reading (the closing looks one pixel
    further twice, and everything after it is cut to the disk) -- and the production path's reading of the one has the status of the dial stage's reading of the other -- and its positions too,
    since equal masks give equal points: to 1e-12."""
    s = SCENES[i]
    op = oparams(s.context_key())
    (hls, frame) = (s.hls_crop(), s.bgr_frame())
    conv = po.bgr2hls(frame, op.hue_shift)
    (a, b) = (base(i), po.process_crop(frame, op))
    assert (b.match_x, b.match_y) == (0, 0)
    for (d, nd) in enumerate(op.dials):
        cr = nd['color_range']
        for (img, o) in ((hls, a), (conv, b)):
            col = list(o.dial_color[d])
            assert tuple(col) == tuple(int(v) for v in img[int(nd['center'][1]), int(nd['center'][0])]), (s.name, d)   # the core is flat
        rng = (cr['h'], cr['l'], cr['s'])
        masks = []
        for (img, o) in ((hls, a), (conv, b)):
            col = list(o.dial_color[d])
            masks.append(_inrange(img, [max(c - r, 0) for (c, r) in zip(col, rng)], [min(c + r, 255) for (c, r) in zip(col, rng)]))
        near = np.pad(op.masks()[d, 0] > 0, 2)
        near = np.any([near[dy:dy + ds.TH, dx:dx + ds.TW] for dy in range(5) for dx in range(5)], axis=0)
        assert np.array_equal(masks[0] & near, masks[1] & near), (s.name, d)
        assert (masks[0] & near).any()
    assert (a.status, a.failed_dial, a.unreadable_mask) == (b.status, b.failed_dial, b.unreadable_mask)
    if a.status == 0:
        assert max(abs(x - y) for (x, y) in zip(list(a.pos)[:4], list(b.pos)[:4])) <= 1e-12
        assert a.value == b.value


@pytest.mark.parametrize('name', sorted(ds.RANGE_COLOURS))
def test_range_labels_sit_on_the_bounds(name):
    """Both palettes of the range scenes: label 2 + 2 c + k lies on bound k of channel c with the other channels inside the
    range, label 8 + 2 c + k one step outside a bound of channel c (that very bound unless it is clamped) with the other channels
    inside; one dial's bounds are clamped at 0 and at 255."""
    (s,) = [s for s in SCENES if s.name == name]
    clamped = set()
    for palette in ('hls', 'bgr'):
        if palette == 'hls':
            colour = {k: tuple(v) for (k, v) in s.hls.items()}
        else:
            keys = sorted(s.bgr)
            conv = po.bgr2hls(np.array([[s.bgr[k] for k in keys]], np.uint8), 128)[0]
            colour = {k: tuple(int(v) for v in conv[j]) for (j, k) in enumerate(keys)}
        (lo, hi) = ds.range_bounds(colour[1])
        for c in range(3):
            for k in range(2):
                (on, out) = (colour[2 + 2 * c + k], colour[8 + 2 * c + k])
                bound = (lo, hi)[k][c]
                assert on[c] == bound and _inrange(np.array(on), lo, hi), (palette, c, k, on)
                others = [j for j in range(3) if j != c]
                assert all(lo[j] <= out[j] <= hi[j] for j in others) and not _inrange(np.array(out), lo, hi), (palette, c, k, out)
                if 0 <= bound + (-1, 1)[k] <= 255:
                    assert out[c] == bound + (-1, 1)[k], (palette, c, k, out)
                else:
                    clamped.add((palette, bound))
                    assert out[c] in (lo[c] - 1, hi[c] + 1)
        assert not _inrange(np.array(colour[0]), lo, hi)
    if name == 'range_clamped':
        assert {b for (_p, b) in clamped} == {0, 255}
    else:
        assert not clamped


def test_mean_form_cannot_change_a_dial_colour():
    """cv::mean of the 5 x 5 core as sum * (1. / N) or as sum / N, then Python's round(): the same integer for every count of
    pixels from 1 to 25 (the core is clipped at the crop's edges) and every sum of that many bytes.  The dial-colour half of the
    mean_form switch can therefore change no record: unreachable."""
    for n in range(1, 26):
        s = np.arange(0, 255 * n + 1, dtype=np.float64)
        assert np.array_equal(np.rint(s * (1.0 / n)), np.rint(s / n)), n


def test_mean_form_template_case():
    """The template-mean half CAN be reached: for constant images the exact TM_CCOEFF value is 0 and what is left is the
    rounding residue of window_sum * mean, which differs between the two forms.  (The fixtures' template gives equal residues for
    all 256 constant images.)  The GPU compares this case in test_match_stage_mean_form_case."""
    (tpl, imgs) = ds.mean_form_case()
    differing = 0
    for img in imgs:
        a = po.match_ccoeff(img, tpl, want_map=True)[3]
        po.set_option('mean_form', 1)
        try:
            b = po.match_ccoeff(img, tpl, want_map=True)[3]
        finally:
            po.set_option('mean_form', 0)
        differing += int(not np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    assert differing >= 8, differing


def test_hue_g_first_cannot_change_a_pixel():
    """The hue sector test differs only where r == g is the maximum: both orders give the same three bytes for all 32 896 such
    triples, in the SIMD form and in the scalar-tail form (an image one pixel wide)."""
    v = np.arange(256)
    (m, b) = np.meshgrid(v, v, indexing='ij')
    keep = b <= m
    tri = np.stack([b[keep], m[keep], m[keep]], axis=-1).astype(np.uint8)     # B, G, R with G == R >= B
    assert len(tri) == 32896
    for img in (np.ascontiguousarray(tri.reshape(257, 128, 3)), np.ascontiguousarray(tri.reshape(-1, 1, 3))):
        a = po.bgr2hls(img, 0)
        po.set_option('hue_g_first', 1)
        try:
            assert np.array_equal(a, po.bgr2hls(img, 0))
        finally:
            po.set_option('hue_g_first', 0)


def test_hls_switches_have_separating_triples():
    """The HLS-stage switches belong to the conversion, which tests/test_gpu_parity.py compares for all 2^24 triples; here only
    that each has a triple that separates it.  (190, 116, 116) gives S = 92 in the SIMD form and 93 in the scalar tail."""
    wide = np.array([[(190, 116, 116)] * 4, [(1, 0, 0)] * 4], np.uint8)         # four columns: every pixel in the SIMD form
    narrow = np.ascontiguousarray(wide[:, :1])                                   # one column: every pixel in the scalar tail
    for (switch, value, img) in (('hls_variant', 1, wide), ('hls_variant', 2, narrow), ('hls_round', 1, wide), ('l_integer', 1, wide)):
        a = po.bgr2hls(img, 0)
        po.set_option(switch, value)
        try:
            assert not np.array_equal(a, po.bgr2hls(img, 0)), (switch, value)
        finally:
            po.set_option(switch, 0)


def test_minmax_last_has_a_separating_map():
    """An all-equal map: the first maximum is (0, 0), the last the map's far corner (tests/test_gpu_parity.py's match tests run
    this case on the GPU: 'all-equal map: first position wins')."""
    tpl = ds.mean_form_case()[0]
    img = np.zeros((12, 14), np.uint8)
    assert po.match_ccoeff(img, tpl)[1:3] == (0, 0)
    po.set_option('minmax_last', 1)
    try:
        assert po.match_ccoeff(img, tpl)[1:3] == (3, 3)
    finally:
        po.set_option('minmax_last', 0)


# ------------------------------------------------------------------------------------------------------------- GPU ---------
CONTEXTS = sorted(ds.contexts())


@functools.lru_cache(maxsize=None)
def production_oracle(key):
    group = ds.contexts()[key]
    return po.process_frames(np.stack([s.bgr_frame() for s in group]), oparams(key))


def test_contexts_cover_every_scene_once():
    assert sum(len(g) for g in ds.contexts().values()) == len(SCENES)
    assert {k[0] for k in CONTEXTS} == {'fixture', 'r29'} and len(CONTEXTS) == 4


@pytest.mark.gpu
@pytest.mark.parametrize('key', CONTEXTS, ids=['%s-%d' % (k[0], j) for (j, k) in enumerate(CONTEXTS)])
def test_dial_reader_equals_the_oracle_on_every_scene(key):
    group = ds.contexts()[key]
    tag = '%s: %s' % (key[0], ' '.join(s.name for s in group))
    c = _Ctx(group[0].data(), os.path.basename(os.path.dirname(ds.params_file(group[0]))))
    try:
        assert c.nr == (48 if key[0] == 'fixture' else 64)
        # the `hls` family: the crops as they are.  This entry point runs no match, so the records' match fields say nothing:
        # the oracle's are set to the record's own before the comparison
        got = c.ctx.read_dials(np.stack([s.hls_crop() for s in group]))
        c.ran('hls')
        want = [po.OrcResult.from_buffer_copy(base(SCENES.index(s))) for s in group]   # copies: the shared ones stay as they are
        for (r, o) in zip(got, want):
            (o.match_x, o.match_y, o.match_val) = (int(r['match_x']), int(r['match_y']), float(r['match_val']))
        _compare_records(got, want, tag='hls ' + tag)
        # the production path: whole BGR frames of template size, a 1 x 1 match map
        frames = np.stack([s.bgr_frame() for s in group])
        recs = c.read_bgr(frames)
        ores = production_oracle(key)
        assert all((o.match_x, o.match_y) == (0, 0) for o in ores)
        _compare_records(recs, ores, tag='bgr ' + tag)
    finally:
        c.close()


@pytest.mark.gpu
def test_match_stage_mean_form_case(tmp_path):
    """The match kernel on the case that separates the two forms of the template mean: whole float32 maps, bit for bit."""
    (tpl, imgs) = ds.mean_form_case()
    reader = _reader_with_template(tmp_path / 'mean_form', tpl)
    try:
        (mv, mx, my, rmap) = reader.ctx.match_ccoeff(imgs, want_map=True)
    finally:
        reader.close()
    for i in range(len(imgs)):
        (ev, ex, ey, emap) = po.match_ccoeff(imgs[i], tpl, want_map=True)
        assert np.array_equal(rmap[i].view(np.uint32), emap.view(np.uint32)), i
        assert (float(mv[i]), int(mx[i]), int(my[i])) == (ev, ex, ey), i
