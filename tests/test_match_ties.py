"""The first-maximum rule of the match stage under PLANNED ties: every kernel, layout and fold on images whose map has a known,
small set of exactly equal maxima at chosen positions (tests/match_ties.py).

cv2.minMaxLoc returns the first maximum in raster order.  The all-equal maps of the other tests have it at (0, 0) -- the first
element of the first lane of the first partial of every kernel -- where "keep your own on equal", "the lower partial slot wins"
and "the first element visited wins" all give the right answer.  Here the equal maxima lie in different halves of a wave, in
different column blocks of a lane, on both sides of every boundary between map rows, in H-form blocks and V-form columns, and in
partial slots whose order is not the raster order.

CPU part: by the exact reference alone, every scene's maxima are exactly the planned set; every wrong rule (match_ties.WRONG_RULES)
answers differently from the right one on at least one scene of every (kernel, layout) the GPU part runs -- or provably cannot,
which is asserted as such; the restated partial slots cover every map.
GPU part: (max value, x, y) of every scene, bit for bit, through melf_match_ccoeff with and without a result map (the host fold)
and through read_frames (the dial kernels' device fold), with the kernel and layout that ran asserted.
"""
import numpy as np
import pytest

from tests import match_exact as mx
from tests import match_ties as mt
from tests.helpers import hip_runtime
from tests.test_match_layouts import ALL_LAYOUTS, EXPECTED_GEN_LAYOUT, EXPECTED_LAYOUT, _DevBuf, _check_gen_plan

SID2 = 't119x188_i250x250'     # the tuned kernel's two column blocks
SID1 = 't119x188_i250x215'     # its one-block forms
SID_C4 = 't119x188_i135x220'
SID_V4 = 't119x188_i300x223'
SID_33 = 't33x33_i96x97'
SID_33W = 't33x33_i96x161'


def _nscenes(sid):
    return len(mt.scene_anchors(*mt.SHAPES[sid]))


def _runs():
    """Every (kernel, layout) of the GPU part: (id, kernel, shape id, batch size, forced tuned layout or None, expected layout string
    or None where the forced fields are asserted instead)."""
    runs = []
    for (rb, pairs, cols, ks) in ALL_LAYOUTS:
        sid = SID2 if cols == 250 else SID1
        runs.append(('A-rb%d-p%d-c%d-k%d' % (rb, pairs, cols, ks), 'mfma', sid, _nscenes(sid), (rb, pairs, ks), None))
    for n in (256, 1024):
        runs.append(('B-n%d' % n, 'mfma', SID2, n, None, EXPECTED_LAYOUT[n]))
    for n in sorted(EXPECTED_GEN_LAYOUT):
        runs.append(('C-c4-n%d' % n, 'gen', SID_C4, n, None, EXPECTED_GEN_LAYOUT[n]))
    runs.append(('C-v4', 'gen', SID_V4, _nscenes(SID_V4), None, 'r4x1/4+v4'))       # four V columns, six V row blocks
    runs.append(('C-33', 'gen', SID_33, _nscenes(SID_33), None, 'r2x1/2+v1'))       # two column blocks and a V column
    runs.append(('C-n3', 'gen', SID2, 3, None, None))                               # sliced tiles (asserted: slices > 1)
    runs.append(('D-250', 'dot4', SID2, _nscenes(SID2), None, 'dot4'))
    runs.append(('D-33w', 'dot4', SID_33W, _nscenes(SID_33W), None, 'dot4'))       # three column blocks, two row blocks
    return runs


RUNS = _runs()
RUN_IDS = [r[0] for r in RUNS]


def _geometry(run, monkeypatch):
    (_id, kernel, sid, n, force, want) = run
    monkeypatch.delenv('MELF_MATCH_LAYOUT', raising=False)
    if force is not None:
        monkeypatch.setenv('MELF_MATCH_LAYOUT', '%d,%d,%d' % force)
    g = mt.geometry(kernel, mt.SHAPES[sid], n)
    if force is not None:
        (rb, pairs, ks) = force
        assert (g['rb'], g['ks']) == (rb, ks) and (g['np'] > 0) == (pairs > 0 and g['rw'] > 32), g
    elif want is not None:
        assert g['layout'] == want, (run, g['layout'])
    return g


def separation(g, planned):
    """rule -> number of scenes on which the wrong rule's answer differs from the first maximum, or None where it provably cannot."""
    slots = mt.slot_table(g)
    out = {}
    for rule in mt.rules_of(g['kernel']):
        differ = sum(1 for ties in planned if mt.WRONG_RULES[rule](ties, g) != ties[0])
        if mt.inseparable(rule, g, slots):
            assert differ == 0, (rule, g['layout'])
            out[rule] = None
        else:
            out[rule] = differ
    return out


# ------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize('sid', list(mt.SHAPES))
def test_scenes_hold_planned_ties(sid):
    """By the exact reference alone: in EVERY scene the positions that attain the map's maximum are exactly the planned set, at
    least two, and the reference's first maximum is the raster-first of them.  No scene is left out."""
    s = mt.scene_set(sid)
    (th, tw, rows, cols) = mt.SHAPES[sid]
    assert s['imgs'].shape == (len(mt.scene_anchors(th, tw, rows, cols)), rows, cols) and len(s['planned']) == len(s['imgs'])
    for (k, ties) in enumerate(s['planned']):
        m = s['map'][k]
        at_max = [(int(y), int(x)) for (y, x) in zip(*np.nonzero(m == m.max()))]
        assert at_max == ties and len(ties) >= 2, (sid, k, s['families'][k], s['anchors'][k], at_max[:6], ties[:6])
        assert set(s['anchors'][k]) <= set(ties)
        (v, x, y) = s['firsts'][k]
        assert (y, x) == ties[0] == min(ties) and v == float(m.max()) and v > 0, (sid, k)
    print('%s: %d scenes, reference %.1f s (%.3f s a frame)' % (sid, len(s['imgs']), s['seconds'], s['seconds'] / len(s['imgs'])))


def test_scene_families_present():
    """What the scene sets must contain, per shape."""
    fam = {sid: [f for (f, _a) in mt.scene_anchors(*shape)] for (sid, shape) in mt.SHAPES.items()}
    for (sid, (th, tw, rows, cols)) in mt.SHAPES.items():
        (rh, rw) = (rows - th + 1, cols - tw + 1)
        anchors = mt.scene_anchors(th, tw, rows, cols)
        assert {'row_half', 'column', 'triple'} <= set(fam[sid]), sid
        firsts_half = {(a[0][1] >> 2) & 1 for (f, a) in anchors if f == 'row_half'}
        assert firsts_half == {0, 1}, sid                                  # the first maximum in half 0 and in half 1
        ys = sorted(a[0][0] for (f, a) in anchors if f in ('up_right_4', 'up_right_32'))
        assert ys == list(range(rh - 1)), sid                              # a pair across EVERY boundary between map rows
        if rw > 36:
            assert 'row_block' in fam[sid] and 'up_right_32' in fam[sid], sid
        if mt.gen_vform(rw)[1]:
            assert 'v_same_row' in fam[sid] and 'v_first' in fam[sid], sid
        if rw > mt.VALU_CBLK:
            assert 'valu_block' in fam[sid], sid
    assert fam[SID_33W].count('valu_block') >= 3       # both block boundaries of the 129-column map


def test_negative_scene():
    """The 1 x 2 map: two equal values below zero, so no fold's initial value (0, -inf) may win; the first is (0, 0)."""
    (tpl, img) = mt.negative_scene()
    (_cc, _ws, rmap, firsts) = mx.exact_match(img[None], tpl)
    assert rmap.shape == (1, 1, 2) and rmap[0, 0, 0] == rmap[0, 0, 1] and rmap[0, 0, 0] < -1e6
    assert firsts[0] == (float(rmap[0, 0, 0]), 0, 0)
    g = dict(kernel='dot4', rh=1, rw=2, nrb=1, nparts=1)
    assert mt.rule_last([(0, 0), (0, 1)], g) == (0, 1)      # the one wrong rule that two positions in one row can tell


@pytest.mark.parametrize('run', RUNS, ids=RUN_IDS)
def test_wrong_rules_separate(run, monkeypatch):
    """Host logic (the layout queries need no GPU): every wrong rule that applies to the kernel answers differently from the right
    one on at least one scene of the batch the GPU test runs -- or cannot in this layout, which is asserted (slot_low where the
    partial slots never decrease along the raster order: the tuned kernel in every layout, the VALU kernel on one column block)."""
    g = _geometry(run, monkeypatch)
    sep = separation(g, mt.planned_sets(run[2]))
    print('%-22s %-14s %s' % (run[0], g['layout'], ' '.join('%s=%s' % (r, 'inseparable' if c is None else c) for (r, c) in sep.items())))
    for (rule, count) in sep.items():
        assert count is None or count > 0, (run[0], g['layout'], rule)
    if g['kernel'] == 'mfma':
        assert sep['slot_low'] is None, 'the tuned kernel numbers its partials in raster order'
        assert sep['slot_high'] is not None
    if run[0] in ('D-33w', 'C-v4', 'C-33') or run[0].startswith('C-c4'):
        assert sep['slot_low'] is not None and sep['slot_low'] > 0       # column-block-major slots / V-form tiles numbered last


@pytest.mark.parametrize('run', RUNS, ids=RUN_IDS)
def test_partial_slots_cover_the_map(run, monkeypatch):
    """partial_slot gives every map position one slot below the kernel's nparts, and it agrees with the
    forward statement of the same layout: the general kernel's tasks painted as _check_gen_plan paints its cover, the tuned
    kernel's tiles row by row (match_block), the VALU kernel's grid."""
    g = _geometry(run, monkeypatch)
    (_id, kernel, sid, n, _force, _want) = run
    (th, tw, rows, cols) = mt.SHAPES[sid]
    slots = mt.slot_table(g)
    assert slots.min() == 0 and slots.max() < g['nparts']
    # (the tuned kernel's last tile, or its last slices, may lie below the map: their partials say "no position")
    assert kernel == 'mfma' or len(np.unique(slots)) == g['nparts']
    paint = np.full((g['rh'], g['rw']), -1, np.int32)
    if kernel == 'gen':
        d = _check_gen_plan(th, tw, rows, cols, n)      # asserts that the tiles cover every position exactly once
        assert d['tiles'] == g['nparts']
        for (ti, (y0, R, xb0, nxb)) in g['tiles'].items():
            if R:
                paint[y0:y0 + R, 32 * xb0:min(32 * (xb0 + nxb), g['vx0'])] = ti
            else:
                paint[y0:y0 + mt.V_ROWS, g['vx0'] + xb0] = ti
    elif kernel == 'mfma':
        (rb, na, npairs, ks) = (g['rb'], g['na'], g['np'], g['ks'])
        for t in range(na + 2 * npairs):
            if t < na:
                (y0, R, first, last) = (t * rb, rb, 3, 3)
            else:
                q = t - na
                base = rb * na + (2 * rb + 1) * (q >> 1)
                (y0, R, first, last) = (base, rb + 1, 3, 1) if q % 2 == 0 else (base + rb, rb + 1, 2, 3)
            for r in range(R):
                mask = first if r == 0 else (last if r == R - 1 else 3)
                for xb in range(2):
                    if (mask >> xb) & 1 and y0 + r < g['rh']:
                        assert (paint[y0 + r, 32 * xb:32 * xb + 32] == -1).all()
                        paint[y0 + r, 32 * xb:32 * xb + 32] = t * ks + (r * ks) // R
    else:
        for cb in range((g['rw'] + 63) // 64):
            for rb_ in range(g['nrb']):
                paint[44 * rb_:44 * rb_ + 44, 64 * cb:64 * cb + 64] = cb * g['nrb'] + rb_
    assert np.array_equal(paint, slots)


@pytest.mark.parametrize('run', [r for r in RUNS if r[1] == 'gen'], ids=[r[0] for r in RUNS if r[1] == 'gen'])
def test_general_kernel_lanes_visit_in_raster_order(run, monkeypatch):
    """"The first element visited wins" is no wrong rule for the general kernel: in every plan the GPU part runs, every lane of
    every wave hands its positions to tile_epilogue in increasing raster order, H form and V form, and the lanes' visits together
    are the map.  So the index clause of tile_epilogue's comparison (k_match_gen.hip:114, "elements are NOT visited in raster
    order here") decides nothing today -- a build without it gives the same records on every scene (tried) -- and guards a
    change of the visiting order; the comparisons BETWEEN lanes, waves and partials are the ones the scenes pin."""
    g = _geometry(run, monkeypatch)
    seen = np.zeros((g['rh'], g['rw']), np.int32)
    for tile in g['tiles']:
        for w in range(g['slices']):
            for hh in (0, 1):
                seq = mt.gen_lane_visits(g, tile, w, hh)
                idx = [y * g['rw'] + x for (y, x) in seq]
                assert idx == sorted(idx) and len(set(idx)) == len(idx), (run[0], tile, w, hh)
                for (y, x) in seq:
                    assert mt.partial_slot(g, y, x) == tile and mt.half_of(g, y, x) == hh
                    seen[y, x] += 1
    assert (seen == 1).all()


def test_grey_pixels_keep_their_value_as_lightness():
    """The device-fold tests feed the scenes as grey BGR frames: by the oracle, L of a grey pixel is its value, for all 256."""
    from oracle import pyoracle as po
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for hue_shift in (0, 30):
        assert np.array_equal(po.bgr2hls(np.ascontiguousarray(grey), hue_shift)[:, :, 1], grey[:, :, 0])


# ------------------------------------------------------------------ GPU ----
def deal(S, n, t):
    """Launch t of a batch of n frames over S scenes -> the scene of every frame.  Over launches(S, n) launches every scene sits in
    every lane of a 32-frame group (lane 0 and lane 31 among them)."""
    i = np.arange(n)
    if n < 32:
        return (t * n + i) % S
    return (i // 32 + t * ((n + 31) // 32) + 7 * (i % 32)) % S


def launches(S, n):
    return -(-S // n) if n < 32 else -(-S // ((n + 31) // 32))


def deal_tail(S, n, t):
    """n not a multiple of 32: over -(-S // (n % 32)) launches every scene sits in the last, partial 32-frame group."""
    m = n % 32
    pick = np.arange(n) % S
    pick[n - m:] = (t * m + np.arange(m)) % S
    return pick


def _assert_firsts(mv, mxx, myy, ref, pick, tag):
    """(max value, x, y) of every frame against the exact reference of its scene; values by their bits."""
    want = [ref['firsts'][s] for s in pick]
    wv = np.array([w[0] for w in want], np.float32)
    bad = np.nonzero((np.asarray(mv, np.float32).view(np.uint32) != wv.view(np.uint32))
                     | (np.asarray(mxx) != np.array([w[1] for w in want])) | (np.asarray(myy) != np.array([w[2] for w in want])))[0]
    if len(bad):
        i = int(bad[0])
        s = int(pick[i])
        raise AssertionError('%s: %d of %d frames differ; the first is frame %d = scene %d (%s, pasted at %s, ties %s): got (%r, x %d, y %d), '
                             'exact (%r, x %d, y %d)' % (tag, len(bad), len(pick), i, s, ref['families'][s], ref['anchors'][s], ref['planned'][s][:9],
                                                         float(mv[i]), int(mxx[i]), int(myy[i]), want[i][0], want[i][1], want[i][2]))


def _run_both(ctx, ref, pick, tag, check_info):
    """melf_match_ccoeff without a result map (production: the kernels' `if (result_map)` branches not taken) and with one; the map
    itself against the reference."""
    imgs = ref['imgs'][pick]
    (mv, mxx, myy, _none) = ctx.match_ccoeff(imgs, want_map=False)
    check_info(ctx.last_match())
    _assert_firsts(mv, mxx, myy, ref, pick, tag + ' without a map')
    (mv, mxx, myy, rmap) = ctx.match_ccoeff(imgs, want_map=True)
    check_info(ctx.last_match())
    _assert_firsts(mv, mxx, myy, ref, pick, tag + ' with a map')
    assert np.array_equal(rmap.view(np.uint32), ref['map'][pick].view(np.uint32)), tag


@pytest.fixture(scope='module')
def readers(tmp_path_factory):
    """Contexts with the lattice templates: 119 x 188 under default dispatch and each kernel forced, 33 x 33 under the general and the
    VALU kernel.  (MELF_MATCH is read when the context is created, MELF_MATCH_LAYOUT at every launch.)"""
    import os
    from meterelf_amd import _hip
    from tests.test_gpu_parity import _reader_with_template
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    saved = {k: os.environ.pop(k, None) for k in ('MELF_MATCH', 'MELF_MATCH_LAYOUT')}
    out = {}
    try:
        for (name, th, tw) in (('119', 119, 188), ('33', 33, 33)):
            for kind in ((None, 'fast', 'gen', 'dot4') if name == '119' else ('gen', 'dot4')):
                if kind is None:
                    os.environ.pop('MELF_MATCH', None)
                else:
                    os.environ['MELF_MATCH'] = kind
                out[(name, kind)] = _reader_with_template(tmp_path_factory.mktemp('ties_%s_%s' % (name, kind)), mt.lattice_template(th, tw))
    finally:
        os.environ.pop('MELF_MATCH', None)
        for (k, v) in saved.items():
            if v is not None:
                os.environ[k] = v
    yield out
    for r in out.values():
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize('rb,pairs,cols,ks', ALL_LAYOUTS, ids=lambda v: str(v))
def test_tuned_kernel_every_layout_ties(readers, monkeypatch, rb, pairs, cols, ks):
    """A: every instantiation of the tuned kernel, forced (MELF_MATCH=fast, MELF_MATCH_LAYOUT), on every scene of its shape."""
    sid = SID2 if cols == 250 else SID1
    ref = mt.scene_set(sid)
    monkeypatch.setenv('MELF_MATCH_LAYOUT', '%d,%d,%d' % (rb, pairs, ks))
    g = mt.geometry('mfma', mt.SHAPES[sid], len(ref['imgs']))

    def check_info(info):
        assert info['kernel'] == 'mfma' and info['rows_per_wave'] == rb and info['k_slices'] == ks, info
        assert (info['pair_waves'] > 0) == (pairs > 0 and cols == 250), info
        assert (info['full_waves'], info['pair_waves'], info['layout']) == (g['na'], 2 * g['np'], g['layout']), (info, g)
    _run_both(readers[('119', 'fast')].ctx, ref, np.arange(len(ref['imgs'])), 'tuned %s' % g['layout'], check_info)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [256, 1024], ids=lambda n: 'n%d_%s' % (n, EXPECTED_LAYOUT[n]))
def test_tuned_kernel_default_dispatch_ties(readers, monkeypatch, n):
    """B: default dispatch at the host-fed chunk size and at the headline batch; every scene in every lane of a frame group, and
    (n - 5 frames, the same layout) in the last, partial group."""
    monkeypatch.delenv('MELF_MATCH_LAYOUT', raising=False)
    ref = mt.scene_set(SID2)
    S = len(ref['imgs'])
    ctx = readers[('119', None)].ctx
    for (m, picks) in ((n, [deal(S, n, t) for t in range(launches(S, n))]), (n - 5, [deal_tail(S, n - 5, t) for t in range(-(-S // 27))])):
        seen = {lane: set() for lane in (0, 31, 'tail')}
        for pick in picks:
            (mv, mxx, myy, _none) = ctx.match_ccoeff(ref['imgs'][pick], want_map=False)
            info = ctx.last_match()
            assert (info['kernel'], info['layout'], info['n']) == ('mfma', EXPECTED_LAYOUT[n], m), info
            _assert_firsts(mv, mxx, myy, ref, pick, 'default dispatch n=%d %s' % (m, info['layout']))
            seen[0] |= set(pick[0::32].tolist())
            seen[31] |= set(pick[31::32].tolist())
            seen['tail'] |= set(pick[32 * (m // 32):].tolist())
        full = set(range(S))
        assert (seen[0] == full and seen[31] == full) if m == n else seen['tail'] == full, (m, {k: len(v) for (k, v) in seen.items()})


GEN_RUNS = [r for r in RUNS if r[1] == 'gen']


@pytest.mark.gpu
@pytest.mark.parametrize('run', GEN_RUNS, ids=[r[0] for r in GEN_RUNS])
def test_general_kernel_ties(readers, monkeypatch, run):
    """C: MELF_MATCH=gen on the config-4 crop at its four plans, on four V-form columns over six V-form row blocks, on two column
    blocks and a V-form column, and in sliced tiles at three frames."""
    (rid, _kernel, sid, n, _force, want) = run
    monkeypatch.delenv('MELF_MATCH_LAYOUT', raising=False)
    ref = mt.scene_set(sid)
    S = len(ref['imgs'])
    g = mt.geometry('gen', mt.SHAPES[sid], n)

    def check_info(info):
        assert (info['kernel'], info['layout'], info['n'], info['tiles']) == ('gen', g['layout'], n, g['nparts']), info
        assert info['layout'] == want if want is not None else info['slices'] > 1, info
    ctx = readers[('119' if mt.SHAPES[sid][0] == 119 else '33', 'gen')].ctx
    for t in range(launches(S, n)):
        _run_both(ctx, ref, deal(S, n, t), 'general %s launch %d' % (g['layout'], t), check_info)


@pytest.mark.gpu
@pytest.mark.parametrize('sid', [SID2, SID_33W])
def test_valu_kernel_ties(readers, monkeypatch, sid):
    """D: MELF_MATCH=dot4 on one column block of three row blocks, and on three column blocks of two row blocks (the partial
    slots are column-block-major there: the first maximum of the valu_block scenes lies in a higher slot than the second)."""
    monkeypatch.delenv('MELF_MATCH_LAYOUT', raising=False)
    ref = mt.scene_set(sid)

    def check_info(info):
        assert info['kernel'] == 'dot4', info
    _run_both(readers[('119' if sid == SID2 else '33', 'dot4')].ctx, ref, np.arange(len(ref['imgs'])), 'VALU kernel %s' % sid, check_info)


def _grey_frames(imgs, x0, y0):
    """The L images as grey BGR frames with a random margin around the crop."""
    (n, rows, cols) = imgs.shape
    rng = np.random.default_rng([n, rows, cols])
    frames = rng.integers(0, 256, size=(n, rows + 8, cols + 12, 3), dtype=np.uint8)
    frames[:, y0:y0 + rows, x0:x0 + cols, :] = imgs[:, :, :, None]
    return frames


def _read_frames_under(tmp_path, monkeypatch, kind, tpl, imgs):
    from tests.test_gpu_parity import _reader_with_template
    (x0, y0) = (6, 4)
    (rows, cols) = imgs.shape[1:]
    if kind is None:
        monkeypatch.delenv('MELF_MATCH', raising=False)
    else:
        monkeypatch.setenv('MELF_MATCH', kind)
    monkeypatch.delenv('MELF_MATCH_LAYOUT', raising=False)
    reader = _reader_with_template(tmp_path / ('fold_%s' % kind), tpl, dials_template_match_threshold=1,
                                   meter_rect={'top_left': [x0, y0], 'bottom_right': [x0 + cols, y0 + rows]})
    frames = _grey_frames(imgs, x0, y0)
    buf = _DevBuf(hip_runtime(), frames.nbytes)
    try:
        host = reader.read_frames(frames)         # the host-fed path: chunks of its own size
        buf.upload(frames)
        recs = reader.ctx.process_batch_dev(buf.p.value, len(frames), frames.shape[1], frames.shape[2])      # ONE launch of the batch
        info = reader.ctx.last_match()
        family = reader.ctx.last_dials()['family']
    finally:
        buf.free()
        reader.close()
    assert (info['rows'], info['cols'], info['n']) == (rows, cols, len(imgs)), info
    assert family == 'bgr', family
    for k in ('match_val', 'match_x', 'match_y'):
        assert host[k].tobytes() == recs[k].tobytes(), k
    return recs, info


@pytest.mark.gpu
@pytest.mark.parametrize('sid,kind,kernel', [(SID2, None, 'mfma'), (SID2, 'gen', 'gen'), (SID2, 'dot4', 'dot4'), (SID_33W, 'gen', 'gen'),
                                             (SID_33W, 'dot4', 'dot4')], ids=lambda v: str(v))
def test_device_fold_ties(tmp_path, monkeypatch, sid, kind, kernel):
    """E: the same scenes as grey BGR frames through read_frames and through one process_batch_dev call: the partials are folded by the
    dial kernel's prologue on the device (k_dials_body.inc), per lane and then by the DPP scan.  256 frames of the 250 x 250 crop (default dispatch: the tuned kernel in
    four K slices, 64 partials a frame); every scene of the 129-column map (the VALU kernel's column-block-major slots)."""
    ref = mt.scene_set(sid)
    S = len(ref['imgs'])
    pick = np.arange(256 if sid == SID2 else S) % S
    (recs, info) = _read_frames_under(tmp_path, monkeypatch, kind, ref['tpl'], ref['imgs'][pick])
    assert info['kernel'] == kernel and (kernel != 'mfma' or info['layout'] == EXPECTED_LAYOUT[256]), info
    _assert_firsts(recs['match_val'], recs['match_x'], recs['match_y'], ref, pick, 'device fold %s %s' % (sid, info['layout']))


@pytest.mark.gpu
def test_negative_map_ties(tmp_path, monkeypatch):
    """F: the 1 x 2 map of two equal negative values under the three kernels through melf_match_ccoeff (host fold) and through
    read_frames (device fold): (that value, 0, 0) -- no fold's initial value wins, and the second position does not."""
    from meterelf_amd import _hip
    from tests.test_gpu_parity import _reader_with_template
    (tpl, img) = mt.negative_scene()
    (_cc, _ws, rmap, firsts) = mx.exact_match(img[None], tpl)
    assert firsts[0][0] < 0 and firsts[0][1:] == (0, 0) and rmap[0, 0, 0] == rmap[0, 0, 1]
    n = 33          # two frame groups, the second with one frame
    imgs = np.ascontiguousarray(np.broadcast_to(img, (n,) + img.shape))
    ref = dict(firsts=firsts, families=['negative'], anchors=[[(0, 0), (0, 1)]], planned=[[(0, 0), (0, 1)]])
    pick = np.zeros(n, np.int64)
    default = _hip.match_gen_plan_query(*mt.NEGATIVE_SHAPE, n)[0]['default_kernel']
    monkeypatch.delenv('MELF_MATCH_LAYOUT', raising=False)
    for (kind, kernel) in (('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')):
        monkeypatch.setenv('MELF_MATCH', kind)
        reader = _reader_with_template(tmp_path / kind, tpl)
        try:
            for want_map in (False, True):
                (mv, mxx, myy, gmap) = reader.ctx.match_ccoeff(imgs, want_map=want_map)
                assert reader.ctx.last_match()['kernel'] == kernel
                _assert_firsts(mv, mxx, myy, ref, pick, 'negative map %s' % kernel)
                if want_map:
                    assert gmap.shape == (n, 1, 2) and (gmap.view(np.uint32) == rmap[0].view(np.uint32)[None]).all()
        finally:
            reader.close()
    for (kind, kernel) in ((None, default), ('gen', 'gen'), ('dot4', 'dot4')):
        (recs, info) = _read_frames_under(tmp_path, monkeypatch, kind, tpl, imgs)
        assert info['kernel'] == kernel, info
        _assert_firsts(recs['match_val'], recs['match_x'], recs['match_y'], ref, pick, 'negative map, device fold %s' % kernel)
