"""The dial reader's record stage (k_dials_body.inc: error aggregation and digit combine; launch_dials; write_record) and the
parameters that feed it, on the frames of tests/dial_records.py: every dial count 1 .. 8, names that do not sort in file order,
and directed mixes of failing dials.

CPU: the plain-Python rule (dial_records.reference_record) equals the reference's own recorded values bit for bit; the oracle
reads every frame for the cause the frame was painted for, and its record is the rule applied to its own positions; every wrong
rule -- a name order applied inverted, not at all or reversed; a failure rule that picks the last failing dial, lets unreadable
dials win, keeps the whole mask or one bit of it -- answers differently from the rule on a frame the GPU tests run, or is listed
as inseparable with the reason; name_order through the loader, the blob and back; the Python layer's three converters on
synthetic records of every status.

GPU: the records of melf_read_dials (HLS crops) and of the production path (BGR frames; RGBA and NV12 at both ends of the dial
count) against the oracle under tests/test_gpu_parity.py's bars, the fields that bar leaves out compared too, and each record
against the rule applied to its own positions.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import dial_records as dr  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests.test_dials_instantiations import _Ctx  # noqa: E402
from tests.test_gpu_parity import _compare_records  # noqa: E402   (its POS_TOL = 1e-9 on positions and angles, 1e-8 on the value)

COUNTS = tuple(range(1, dr.MAX_DIALS + 1))
MIX_COUNTS = (1, 4, 8)


# ---- shared inputs and the oracle's readings of them: computed once ----
def set_tag(n):
    return 'set%d' % n


@functools.lru_cache(maxsize=None)
def oparams_of_set(n):
    return po.Params(dr.params_file(dr.set_data(n), set_tag(n)))


def names_of_set(n):
    return list(dr.DEFAULT_NAMES[:n])


def _oracle(hls, bgr, op):
    """(the oracle's reading of every HLS crop, its reading of every BGR frame through the production path)"""
    return (po.read_dials_batch(hls, op), po.process_frames(bgr, op))


@functools.lru_cache(maxsize=None)
def count_case(n):
    maps = dr.count_frames(n)
    (hls, bgr) = (dr.hls_crops(maps), dr.bgr_frames(maps))
    return (hls, bgr) + _oracle(hls, bgr, oparams_of_set(n))


@functools.lru_cache(maxsize=None)
def mix_case(n):
    (maps, kinds) = dr.mix_frames(n)
    (hls, bgr) = (dr.hls_crops(maps), dr.bgr_frames(maps))
    return (hls, bgr) + _oracle(hls, bgr, oparams_of_set(n)) + (kinds,)


@functools.lru_cache(maxsize=None)
def nv12_case(n):
    """The count frames of n dials through NV12: (Y, U, V, the packed BGR frames the conversion defines, the oracle's reading of
    those).  NV12 needs an even number of rows: one more row of background below the meter_rect, which stays (0, 0)-(188, 119)."""
    bgr = count_case(n)[1]
    tall = np.concatenate([bgr, np.broadcast_to(np.array(dr.BGR_PALETTE[dr.BACKGROUND], np.uint8), (len(bgr), 1, dr.TW, 3))], axis=1)
    (Y, U, V) = fc.F420.from_bgr(tall)
    back = fc.F420.bgr_of(Y, U, V)
    return (Y, U, V, back, po.process_frames(back, oparams_of_set(n)))


def assignment_tag(p):
    return 'names' + ''.join(str(k) for k in p)


@functools.lru_cache(maxsize=None)
def name_case(p):
    """The name-order frames read with the fixture's dials named by assignment p."""
    from tests import dial_scenes as ds
    (_scene_names, maps) = dr.name_order_scenes()
    hls = np.stack([dr.colour(m, {0: ds.HLS_BACKGROUND, 1: ds.HLS_NEEDLE}) for m in maps])
    bgr = np.stack([dr.colour(m, {0: ds.BGR_BACKGROUND, 1: ds.BGR_NEEDLE}) for m in maps])
    op = po.Params(dr.params_file(dr.renamed_fixture(dr.assignment_names(p)), assignment_tag(p)))
    return (hls, bgr) + _oracle(hls, bgr, op)


def fields(o):
    return (int(o.status), int(o.failed_dial), int(o.unreadable_mask))


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_the_dial_sets_are_what_they_claim():
    for n in COUNTS:
        data = dr.set_data(n)
        nds = data['needle_data']
        assert len(nds) == n and dr.windows_inside(data)
        for key in ('angle_of_zero', 'diameter', 'dist_from_center', 'circle_thickness'):
            assert len({nd[key] for nd in nds}) == n, key
        assert len({tuple(sorted(nd['color_range'].items())) for nd in nds}) == n
        assert len({tuple(nd['center']) for nd in nds}) == n
    nds = dr.dial_set(8)
    assert {nd['negative_momentum'] for nd in nds} == {False, True}
    assert any(float(c).is_integer() for nd in nds for c in nd['center']) and any(not float(c).is_integer() for nd in nds for c in nd['center'])
    # the default names sort in file order for no count but one
    assert [dr.order_of(names_of_set(n)) == list(range(n)) for n in COUNTS] == [True] + [False] * 7
    assert len(dr.failure_mixes(8)) == 1 + 8 + 56 + 28 + 255 and len(dr.failure_mixes(4)) == 1 + 4 + 12 + 6 + 15


def test_reference_value_equals_the_recorded_vectors():
    """The digit combine of reference_record against every value_by_positions vector the reference itself recorded, bit for bit --
    each under another assignment of the four names to the dials, so that the sort by name is part of what is compared."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'pure_fn_vectors.json')) as fp:
        vectors = json.load(fp)['value_by_positions']
    assert len(vectors) >= 100
    for (i, (r4321, want)) in enumerate(vectors):
        p = dr.NAME_ASSIGNMENTS[i % 24]
        names = dr.assignment_names(p)
        per_dial = [r4321[k] for k in p]      # dial d carries the p[d]-th name in sorted order
        got = dr.reference_record(names, per_dial)
        assert got['value'] == want and got['result']['value'] == want, (i, p, got['value'], want)
        assert got['value'] == dr.value_in_order(dr.order_of(names), per_dial)


def _check_mechanism(o, kinds, n, tag):
    """The diagnostics of one oracle reading show the cause each dial was painted for (the oracle stops at the first dial
    without contours: what follows it was never read)."""
    for d in range(n):
        if kinds[d] == 'none':
            # no contour at all in closed mask & disk: this is where the oracle returns
            assert (o.status, o.failed_dial) == (po.NEEDLE_CONTOURS_NOT_FOUND, d) and o.contour_area[d] == 0.0, (tag, d)
            break
        if kinds[d] == 'unread':
            assert o.n_needle[d] > 0 and o.n_outer[d] == 0, (tag, d, o.n_needle[d], o.n_outer[d])
        else:
            assert o.n_kept[d] >= 5, (tag, d, o.n_kept[d])


def _check_against_rule(o, names, kinds, tag):
    """The oracle's record is reference_record of the kinds painted and the oracle's own positions."""
    n = len(names)
    want = dr.reference_record(names, [kinds[d] if kinds[d] != 'ok' else float(o.pos[d]) for d in range(n)])
    assert fields(o) == (want['status'], want['failed_dial'], want['mask']) == dr.expected_of_kinds(kinds), (tag, fields(o), want)
    assert float(o.value) == want['value'], (tag, o.value, want['value'])
    assert (po.error_message(o, type('P', (), {'names': names})) or None) == (want['result'] if want['status'] else None), tag


@pytest.mark.parametrize('n', COUNTS)
def test_count_frames_read_for_the_intended_cause(n):
    (_hls, _bgr, oh, ob) = count_case(n)
    for (entry, res) in (('hls', oh), ('bgr', ob)):
        for (f, o) in enumerate(res):
            _check_mechanism(o, ['ok'] * n, n, (n, entry, f))
            _check_against_rule(o, names_of_set(n), ['ok'] * n, (n, entry, f))
            assert (o.match_x, o.match_y) == (0, 0)
    # the needles do turn: every dial reads at least eight different digits over the sixteen frames
    for d in range(n):
        assert len({int(o.pos[d]) for o in oh}) >= 8, d


@pytest.mark.parametrize('n', (1, 8))
def test_nv12_frames_read_for_the_intended_cause(n):
    """The frames as they come back from 4:2:0: the chroma of needle edges is blurred, every dial still reads from five ring points
    or more, and the record is the rule's."""
    (_Y, _U, _V, back, ores) = nv12_case(n)
    assert back.shape == (16, dr.TH + 1, dr.TW, 3)
    for (f, o) in enumerate(ores):
        _check_mechanism(o, ['ok'] * n, n, (n, 'nv12', f))
        _check_against_rule(o, names_of_set(n), ['ok'] * n, (n, 'nv12', f))
        assert (o.match_x, o.match_y) == (0, 0)


@pytest.mark.parametrize('n', MIX_COUNTS)
def test_mix_frames_fail_for_the_intended_cause(n):
    (_hls, _bgr, oh, ob, kinds) = mix_case(n)
    assert len(kinds) == len(dr.failure_mixes(n))
    for (entry, res) in (('hls', oh), ('bgr', ob)):
        for (f, o) in enumerate(res):
            _check_mechanism(o, kinds[f], n, (n, entry, f))
            _check_against_rule(o, names_of_set(n), kinds[f], (n, entry, f))
        assert {int(o.status) for o in res} == {0, 2, 3}
    # a 'none' dial's two colours and the background lie outside the range around its core's mean, in both palettes
    op = oparams_of_set(n)
    (maps, _k) = dr.mix_frames(n)
    f = 1   # the frame whose dial 0 is 'none'
    assert kinds[f][0] == 'none'
    nd = op.dials[0]
    (x, y) = (int(nd['center'][0]), int(nd['center'][1]))
    for img in (dr.hls_crops(maps[f:f + 1])[0], po.bgr2hls(dr.bgr_frames(maps[f:f + 1])[0], op.hue_shift)):
        core = img[y - 2:y + 3, x - 2:x + 3].reshape(-1, 3).astype(np.float64)
        assert set(core[:, 1]) == {0.0, 255.0}
        mean = [int(round(v)) for v in core.sum(axis=0) * (1.0 / 25)]
        cr = nd['color_range']
        (lo, hi) = ([max(m - r, 0) for (m, r) in zip(mean, (cr['h'], cr['l'], cr['s']))], [min(m + r, 255) for (m, r) in zip(mean, (cr['h'], cr['l'], cr['s']))])
        disk = op.masks()[0, 0] > 0
        inr = np.all((img >= lo) & (img <= hi), axis=-1)
        assert not (inr & disk).any()


def test_name_frames_read_and_separate_the_assignments():
    """All 24 assignments of the fixture's four names read every frame; on the three plain frames alone they give 24 distinct
    triples of values."""
    (scene_names, _maps) = dr.name_order_scenes()
    plain = [i for (i, s) in enumerate(scene_names) if s.startswith('plain')]
    assert len(plain) == 3
    triples = set()
    for p in dr.NAME_ASSIGNMENTS:
        names = dr.assignment_names(p)
        (_hls, _bgr, oh, ob) = name_case(p)
        for (entry, res) in (('hls', oh), ('bgr', ob)):
            for (f, o) in enumerate(res):
                _check_mechanism(o, ['ok'] * 4, 4, (p, entry, f))
                _check_against_rule(o, names, ['ok'] * 4, (p, entry, f))
        triples.add(tuple(int(oh[i].value) for i in plain))
    assert len(triples) == 24
    for i in plain:   # four distinct integer parts
        assert len({int(v) for v in list(name_case(dr.NAME_ASSIGNMENTS[0])[2][i].pos)[:4]}) == 4


# Wrong rules that CANNOT answer differently, by name, with the reason.
INSEPARABLE_NAME_ORDERS = {
    # the inverse of an involution is the involution: the nine non-identity assignments that are their own inverse
    'inverse': sorted(p for p in dr.NAME_ASSIGNMENTS[1:] if dr.inverse(list(p)) == list(p)),
    'identity': [],
    'reversed': [],
}
# one dial: a frame has at most one failing dial, and no rule has anything to choose between
INSEPARABLE_PRECEDENCE = {1: dr.PRECEDENCE_RULES, 4: (), 8: ()}


def test_wrong_name_orders_separate():
    """Host logic.  For every non-identity assignment: the digit combine run with name_order as it is, against the same with the
    identity, the inverse permutation and the reversed order in its place, on the positions the oracle reads from the name-order
    frames.  They differ in floor(value) on at least one frame, unless the wrong order IS the right one."""
    assert len(INSEPARABLE_NAME_ORDERS['inverse']) == 9
    (_hls, _bgr, oh, _ob) = name_case(dr.NAME_ASSIGNMENTS[0])
    positions = [list(o.pos)[:4] for o in oh]
    for p in dr.NAME_ASSIGNMENTS[1:]:
        names = dr.assignment_names(p)
        order = dr.order_of(names)
        right = [dr.reference_record(names, pos)['value'] for pos in positions]
        assert right == [dr.value_in_order(order, pos) for pos in positions]
        for (rule, wrong_of) in dr.NAME_ORDER_RULES.items():
            wrong = wrong_of(order)
            if wrong == order:
                assert p in INSEPARABLE_NAME_ORDERS[rule], (rule, p)
                continue
            assert p not in INSEPARABLE_NAME_ORDERS[rule], (rule, p)
            differing = sum(int(dr.value_in_order(wrong, pos)) != int(v) for (pos, v) in zip(positions, right))
            assert differing > 0, (rule, p)


@pytest.mark.parametrize('n', MIX_COUNTS)
def test_wrong_precedence_rules_separate(n):
    (_maps, kinds) = dr.mix_frames(n)
    for rule in dr.PRECEDENCE_RULES:
        differing = sum(dr.precedence_rule(rule, k) != dr.expected_of_kinds(k) for k in kinds)
        if rule in INSEPARABLE_PRECEDENCE[n]:
            assert differing == 0, (n, rule)
        else:
            assert differing > 0, (n, rule)


SORT_NAMES = ('9', '10', 'b', 'B', 'dial', 'dial2', 'dial10', 'Dial')   # digits as strings, mixed case, a shared prefix


def test_name_order_through_the_loader_and_the_blob():
    from meterelf_amd import _engine, _params
    assert sorted(SORT_NAMES) == ['10', '9', 'B', 'Dial', 'b', 'dial', 'dial10', 'dial2']
    for n in COUNTS:
        for (tag, names) in (('sort', list(SORT_NAMES[:n])), ('default', names_of_set(n))):
            params = _params.load(dr.params_file(dr.set_data(n, names), 'order_%s%d' % (tag, n)))
            assert params.dial_names == names
            want = sorted(range(n), key=names.__getitem__)
            cp = params.to_c()
            assert cp.ndials == n and list(cp.name_order)[:n] == want, (n, names)
            back = _hip.blob_params(_engine.make_blob(params))
            assert back.ndials == n and list(back.name_order) == list(cp.name_order), (n, names)
            assert list(po.Params(dr.params_file(dr.set_data(n, names), 'order_%s%d' % (tag, n))).name_order()) == want
    assert dr.order_of(list(SORT_NAMES)) == [1, 0, 3, 7, 2, 4, 6, 5]


def _synthetic(n, names):
    """(records, what reference_record says of each): every status, every failed dial, masks of one, several and all dials."""
    cases = [[0.25 + 1.1 * d for d in range(n)], [9.75 - 1.2 * d for d in range(n)]]
    for i in range(n):
        cases.append([('none' if d == i else ('unread' if d % 3 == 1 else 0.5 + d)) for d in range(n)])
    for mask in sorted({1, 1 << (n - 1), (1 << n) - 1, 0x55 & ((1 << n) - 1), 0xa6 & ((1 << n) - 1)} - {0}):
        cases.append([('unread' if mask >> d & 1 else 1.5 + d) for d in range(n)])
    recs = np.zeros(len(cases) + 1, _hip.RESULT_DTYPE)
    wants = []
    for (rec, per_dial) in zip(recs, cases):
        want = dr.reference_record(names, per_dial)
        (rec['status'], rec['failed_dial'], rec['unreadable_mask'], rec['value']) = (want['status'], want['failed_dial'], want['mask'], want['value'])
        for (d, v) in enumerate(per_dial):
            if not isinstance(v, str):
                rec['pos'][d] = v
        wants.append(want['result'])
    (recs[-1]['status'], recs[-1]['failed_dial'], recs[-1]['match_val']) = (_hip.FRAME_DIALS_NOT_FOUND, -1, 12345.5)
    wants.append('Dials not found (match val = 12345.5)')
    return (recs, wants)


@pytest.mark.parametrize('n', MIX_COUNTS)
def test_python_layer_agrees_with_the_rule(n):
    from meterelf_amd import _engine
    from meterelf_amd.exceptions import DialAngleDeterminingError, DialsNotFoundError, NeedleContoursNotFoundError
    kind_of = {1: DialsNotFoundError, 2: NeedleContoursNotFoundError, 3: DialAngleDeterminingError}
    base = list(dr.FIXTURE_NAMES) if n == 4 else names_of_set(n)
    for names in (base, list(reversed(base)), sorted(base), list(SORT_NAMES[:n])):
        (recs, wants) = _synthetic(n, names)
        assert {int(s) for s in recs['status']} == ({0, 1, 2, 3})
        files = ['f%d.jpg' % i for i in range(len(recs))]
        ok = [True] * len(recs)
        many = _engine.records_to_python(recs, ok, names, files)
        items = _engine.records_to_items(recs, ok, names, files, lambda f, v, e, mv: (f, v, e, mv))
        for (i, want) in enumerate(wants):
            one = _engine.result_to_python(recs[i], names, files[i])
            for (values, err) in (one, many[i], items[i][3:1:-1]):
                if isinstance(want, dict):
                    assert err is None and values == want and list(values) == list(want), (n, names, i)
                    assert ('value' in values) == (n == 4)
                else:
                    assert values == {} and type(err) is kind_of[int(recs[i]['status'])], (n, names, i)
                    assert err.get_message() == want, (n, names, i, err.get_message(), want)
            assert items[i][0] == files[i] and items[i][1] == (want.get('value') if isinstance(want, dict) else None)
        # the dial named is names[failed_dial]; unreadable dials come in file order
        for (i, want) in enumerate(wants):
            if int(recs[i]['status']) == 2:
                assert want.endswith('(dial = %s)' % names[int(recs[i]['failed_dial'])])
            if int(recs[i]['status']) == 3:
                bad = [names[d] for d in range(n) if int(recs[i]['unreadable_mask']) >> d & 1]
                assert want.endswith('(unreadable dials = %s)' % ', '.join(bad))


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _check_records(recs, ores, names, tag):
    """tests/test_gpu_parity.py's bars, then what they leave out: failed dial and mask whatever the status; nothing beyond the
    context's dials; no value unless there are four; and the record against the rule applied to its own positions."""
    n = len(names)
    assert len(recs) == len(ores)
    _compare_records(recs, ores, ndials=n, tag=tag)
    for (i, (r, o)) in enumerate(zip(recs, ores)):
        got = (int(r['status']), int(r['failed_dial']), int(r['unreadable_mask']))
        assert got == fields(o), (tag, i, got, fields(o))
        assert not r['pos'][n:].any() and not r['angle'][n:].any(), (tag, i)
        assert r['pos'][n:].tobytes() == bytes(8 * (dr.MAX_DIALS - n)) and r['angle'][n:].tobytes() == bytes(8 * (dr.MAX_DIALS - n)), (tag, i)
        if n != 4 or got[0] != 0:
            assert float(r['value']) == 0.0 and r['value'].tobytes() == bytes(8), (tag, i)
        want = dr.reference_record(names, dr.outcomes_of(got[0], got[1], got[2], r['pos'], n))
        assert got == (want['status'], want['failed_dial'], want['mask']), (tag, i)
        assert np.floor(float(r['value'])) == np.floor(want['value']), (tag, i, float(r['value']), want['value'])


def _hls_wants(got, ores):
    """melf_read_dials runs no match: the oracle's match fields are set to the record's own before the comparison."""
    out = [po.OrcResult.from_buffer_copy(o) for o in ores]
    for (r, o) in zip(got, out):
        (o.match_x, o.match_y, o.match_val) = (int(r['match_x']), int(r['match_y']), float(r['match_val']))
    return out


def _prefilled_results(n):
    """Device memory for n records, every byte 0xFF: write_record promises to write them all."""
    host = np.full(n * _hip.RESULT_DTYPE.itemsize, 0xFF, np.uint8)
    return fc.DevBuf(host.ctypes.data, host.nbytes)


def _dev_into_prefilled(n, frames_ptr, frames_bytes, call):
    (src, dst) = (fc.DevBuf(frames_ptr, frames_bytes), _prefilled_results(n))
    try:
        return call(src.d.value, dst.d.value)
    finally:
        src.free()
        dst.free()


def _both_entry_points(c, hls, bgr, oh, ob, names, tag):
    n = len(names)
    got = c.ctx.read_dials(hls)
    c.ran('hls')
    _check_records(got, _hls_wants(got, oh), names, 'hls ' + tag)
    recs = c.read_bgr(bgr)
    _check_records(recs, ob, names, 'bgr ' + tag)
    assert all((int(r['match_x']), int(r['match_y'])) == (0, 0) for r in recs)
    dev = _dev_into_prefilled(len(bgr), bgr.ctypes.data, bgr.nbytes,
                              lambda d, out: c.ctx.process_batch_dev(d, len(bgr), *bgr.shape[1:3], d_results_ptr=out))
    c.ran('bgr')
    assert dev.tobytes() == recs.tobytes(), tag
    return recs


def _context(data, tag, n):
    c = _Ctx(data, 'records_' + tag)
    names = [nd['name'] for nd in data['needle_data']]
    assert c.ctx.params.ndials == n and c.nr == 48
    assert list(c.ctx.params.name_order)[:n] == sorted(range(n), key=names.__getitem__), tag
    return c


@pytest.mark.gpu
@pytest.mark.parametrize('n', COUNTS)
def test_every_dial_count(n):
    """n dials, sixteen readable frames: block 64 n, n dials' LDS, the momentum tables behind 3 n row-mask planes.  At n = 1 and
    n = 8 also a kernel whose own argument follows the common ones (RGBA: k_needles) and one with lead arguments (NV12), against
    read_frames of the packed BGR frames their conversions define, and those against the oracle."""
    (hls, bgr, oh, ob) = count_case(n)
    names = names_of_set(n)
    c = _context(dr.set_data(n), set_tag(n), n)
    try:
        recs = _both_entry_points(c, hls, bgr, oh, ob, names, 'n=%d' % n)
        assert (recs['status'] == _hip.FRAME_OK).all()
        if n in (1, 8):
            rng = np.random.default_rng(n)
            (arr, f) = fc.to_layout(bgr, 'rgba', 5, rng)
            v = _hip.frames_view(arr, f)
            got = c.reader.read_frame_views(arr, f)
            c.ran('packed4')
            assert got.tobytes() == recs.tobytes()
            dev = _dev_into_prefilled(len(bgr), v.ptr, v.extent, lambda d, out: c.ctx.process_frames_dev(
                d, v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride, d_results_ptr=out))
            c.ran('packed4')
            assert dev.tobytes() == recs.tobytes()
            (Y, U, V, back, oback) = nv12_case(n)
            want = c.read_bgr(back)
            _check_records(want, oback, names, 'nv12 frames as bgr n=%d' % n)
            yv = _hip.yuv_frames_view(fc.conventional420(Y, U, V, 'nv12', 10, rng), 'nv12')
            got = c.ctx.process_yuv(yv.ptr, yv.descriptor())
            c.ran('nv12')
            assert got.tobytes() == want.tobytes()
            dev = _dev_into_prefilled(len(bgr), yv.ptr, yv.extent, lambda d, out: c.ctx.process_yuv_dev(d, yv.descriptor(), d_results_ptr=out))
            c.ran('nv12')
            assert dev.tobytes() == want.tobytes()
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize('n', MIX_COUNTS)
def test_failure_mixes(n):
    """One batch per dial count: every single dial without contours, every ordered pair (without contours, unreadable), every pair
    without contours, every subset of unreadable dials."""
    (hls, bgr, oh, ob, kinds) = mix_case(n)
    c = _context(dr.set_data(n), set_tag(n), n)
    try:
        recs = _both_entry_points(c, hls, bgr, oh, ob, names_of_set(n), 'mixes n=%d' % n)
        assert {int(s) for s in recs['status']} == {0, 2, 3}
        for (r, k) in zip(recs, kinds):
            assert (int(r['status']), int(r['failed_dial']), int(r['unreadable_mask'])) == dr.expected_of_kinds(k), k
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize('p', dr.NAME_ASSIGNMENTS, ids=[assignment_tag(p) for p in dr.NAME_ASSIGNMENTS])
def test_every_name_order(p):
    """The fixture's four dials under each of the 24 assignments of its four names, one context each."""
    (hls, bgr, oh, ob) = name_case(p)
    names = dr.assignment_names(p)
    c = _context(dr.renamed_fixture(names), assignment_tag(p), 4)
    try:
        recs = _both_entry_points(c, hls, bgr, oh, ob, names, assignment_tag(p))
        assert (recs['status'] == _hip.FRAME_OK).all()
        # (value to the digit, against the rule on the ORACLE's positions too: the record's own cannot hide a common shift)
        for (r, o) in zip(recs, ob):
            assert int(float(r['value'])) == int(dr.reference_record(names, list(o.pos)[:4])['value'])
    finally:
        c.close()
