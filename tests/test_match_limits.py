"""Template match beyond 2^31: the oracle and all three match kernels against an exact reference, at the largest templates
a context accepts.

The match kernels admit every template with th * tw * 255^2 < 2^32 (mfma_match_ok, gen_match_ok) and form cc = sum T * L
modulo 2^32, converted UNSIGNED; the VALU kernel accumulates cc in uint32_t.  The only other limit on a context's template
is the VALU kernel's 64 KiB LDS tile (setup_device_tables), which allows 209 x 190, 159 x 256 and 291 x 128 (th x tw):
39 710, 40 704 and 37 248 pixels, cc up to 2.58e9, 2.65e9 and 2.42e9.  A kernel (or an oracle) that reads cc as signed, or
narrows an accumulator, a window sum or the LDS exchange of the K slices by one bit, is wrong only there.

The reference is tests/match_exact.py (int64, numpy only, written out as the definition); everything is compared bit for
bit -- no tolerance anywhere.  CPU part: the oracle equals the reference, the frames hold what they claim (shown by the
reference alone; the GPU tests import the same frames), the admission boundary.  GPU part: every match kernel and every
instantiation of the tuned one on batches of 40 frames whose cc lies in [2^31, 2^32), whole maps and first maxima of ALL
frames, and the full path with a match threshold that values from beyond 2^31 decide.
"""
import glob
import os

import numpy as np
import pytest

from tests import match_exact as mx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# setup_device_tables' rule for the VALU kernel's LDS tile (melf_internal.h)
MATCH_R = 11         # output rows per lane
MATCH_WAVES = 4      # waves per workgroup
MATCH_CBLK = 64      # output columns per workgroup


def lds_rule_ok(th, tw):
    ldsw = MATCH_CBLK // 4 + (tw + 3) // 4 + 1
    lds_rows = MATCH_R * MATCH_WAVES + th - 1
    return ldsw * lds_rows * 4 <= 64 * 1024


CASES = [(sid, v) for sid in mx.LIMIT_SHAPES for v in mx.VARIANTS]
CASE_IDS = ['%s_%s' % c for c in CASES]
# the three shapes of the general and the VALU kernel's tests (the fourth is the tuned kernel's single column block)
SHAPES3 = ('t209x190_i231x250', 't159x256_i175x288', 't291x128_i300x161')
CASES3 = [(sid, v) for sid in SHAPES3 for v in mx.VARIANTS]
CASE3_IDS = ['%s_%s' % c for c in CASES3]


# ------------------------------------------------------------------ CPU ----
def _oracle_equals_reference(imgs, tpl, ref=None):
    from oracle import pyoracle as po
    (_cc, _ws, rmap, firsts) = ref if ref is not None else mx.exact_match(imgs, tpl)
    for k in range(len(imgs)):
        (ev, ex, ey, emap) = po.match_ccoeff(imgs[k], tpl, want_map=True)
        assert np.array_equal(emap.view(np.uint32), rmap[k].view(np.uint32)), k
        assert (ev, ex, ey) == firsts[k], (k, (ev, ex, ey), firsts[k])
        assert po.match_ccoeff(imgs[k], tpl)[:3] == firsts[k], k      # without a map


def test_oracle_equals_reference_fixture_template():
    """The fixtures' template (119 x 188) on the L plane of a fixture crop, and random 0..255 content at 119 x 188: cc stays
    below 2^31, where the oracle's 32-bit loop always was exact."""
    from oracle import pyoracle as po
    pfile = os.path.join(GOLDEN, 'sample-images1', 'params.yml')
    op = po.Params(pfile)
    tpl = op.load_template()
    files = sorted(glob.glob(os.path.join(GOLDEN, 'sample-images1', '*.jpg')))
    crops = [po.crop_meter(po.decode_bgr(f), op) for f in files[2:4]]
    lplanes = np.stack([np.ascontiguousarray(po.bgr2hls(c, op.hue_shift)[:, :, 1]) for c in crops])
    assert lplanes.shape[1:] == (250, 250) and tpl.shape == (119, 188)
    _oracle_equals_reference(lplanes, tpl)
    rng = np.random.default_rng(119188)
    rtpl = rng.integers(0, 256, size=(119, 188), dtype=np.uint8)
    rimgs = rng.integers(0, 256, size=(2, 135, 220), dtype=np.uint8)
    ref = mx.exact_match(rimgs, rtpl)
    assert ref[0].max() < mx.TWO31
    _oracle_equals_reference(rimgs, rtpl, ref)


@pytest.mark.parametrize('sid,variant', CASES3, ids=CASE3_IDS)
def test_oracle_equals_reference_beyond_2_31(sid, variant):
    """orc_match_ccoeff on frames (a) to (f) of the largest templates a context accepts: map, value, x and y bit-equal to the
    exact reference.  (An int32_t accumulator converted as signed fails all six cases: at 209 x 190 every map value of frame (a)
    comes out 2^32 too low, -4.29e9 where the reference has values within +-1.5e4.)"""
    r = mx.limit_reference(sid, variant)
    idx = [r['roles'][name][0] for name in mx.ROLE_NAMES]
    ref = (r['cc'][idx], r['ws'][idx], r['map'][idx], [r['firsts'][k] for k in idx])
    _oracle_equals_reference(r['imgs'][idx], r['tpl'], ref)


@pytest.mark.parametrize('sid,variant', CASES, ids=CASE_IDS)
def test_limit_cases_hold_what_they_claim(sid, variant):
    """By the reference alone: the batch the GPU tests run does reach [2^31, 2^32) the way each frame's role says."""
    (th, tw, rows, cols) = mx.LIMIT_SHAPES[sid]
    r = mx.limit_reference(sid, variant)
    (cc, rmap, roles, imgs) = (r['cc'], r['map'], r['roles'], r['imgs'])
    (rh, rw) = (rows - th + 1, cols - tw + 1)
    assert imgs.shape == (mx.N_LIMIT, rows, cols) and cc.shape == (mx.N_LIMIT, rh, rw)
    assert th * tw * 65025 < mx.TWO32 and th * tw > 33026, 'admitted by the matrix-core kernels, and able to pass 2^31'
    assert lds_rule_ok(th, tw), 'a context accepts the template'
    assert 0 <= cc.min() and 2.3e9 < cc.max() < mx.TWO32
    for name in mx.ROLE_NAMES:
        (k0, k1) = roles[name]
        assert k0 < 32 <= k1 and np.array_equal(imgs[k0], imgs[k1]), 'in both 32-frame groups'
        assert np.array_equal(cc[k0], cc[k1])
    a = cc[roles['a'][0]]
    assert (a >= mx.TWO31).all()
    b = roles['b'][0]
    assert (imgs[b] == 255).all() and (cc[b] >= mx.TWO31).all() and cc[b].max() == cc.max()
    assert (r['ws'][b] == 255 * th * tw).all() and r['ws'].max() == 255 * th * tw
    assert len(np.unique(rmap[b])) == 1 and r['firsts'][b][1:] == (0, 0), 'every value ties: the first one wins'
    share = float((cc[roles['c'][0]] >= mx.TWO31).mean())
    assert 0.2 <= share <= 0.8, share
    d = roles['d'][0]
    assert r['firsts'][d][1:] == mx.PASTE_XY
    assert cc[d].min() < mx.TWO31 <= cc[d].max() and cc[d][mx.PASTE_XY[1], mx.PASTE_XY[0]] >= mx.TWO31
    e = roles['e'][0]
    nmax = int((rmap[e] == rmap[e].max()).sum())
    (ev, ex, ey) = r['firsts'][e]
    assert nmax >= 4 and (ex, ey) != (0, 0), (nmax, ex, ey)
    assert (cc[e] >= mx.TWO31).all()
    assert (cc[roles['f'][0]] < mx.TWO31).all()
    fill = [k for k in range(mx.N_LIMIT) if k % 32 >= len(mx.ROLE_NAMES)]
    assert (cc[fill] >= mx.TWO31).all()


def test_largest_templates_of_a_context():
    """The LDS rule, restated: the three shapes pass it and one more template row does not."""
    assert lds_rule_ok(209, 190) and not lds_rule_ok(210, 190)
    assert lds_rule_ok(159, 256) and not lds_rule_ok(160, 256)
    assert lds_rule_ok(291, 128) and not lds_rule_ok(292, 128)
    assert lds_rule_ok(119, 188)


def test_admission_boundary():
    """th * tw * 255^2 < 2^32 through melf_match_layout_query: 66 048 pixels are given to a matrix-core kernel, 66 240 (tuned
    kernel's class) and 66 304 (general kernel's) go to the VALU kernel.  Query only: no context of that size can exist."""
    from meterelf_amd import _hip
    assert 344 * 192 * 65025 < mx.TWO32 <= 345 * 192 * 65025
    assert 258 * 256 * 65025 < mx.TWO32 <= 259 * 256 * 65025
    for n in (1, 40, 1024):
        assert _hip.match_layout_query(344, 192, 344 + 20, 192 + 40, n)['kernel'] == 'mfma', n
        assert _hip.match_layout_query(345, 192, 345 + 20, 192 + 40, n)['kernel'] == 'dot4', n
        assert _hip.match_layout_query(258, 256, 258 + 20, 256 + 40, n)['kernel'] == 'gen', n
        assert _hip.match_layout_query(259, 256, 259 + 20, 256 + 40, n)['kernel'] == 'dot4', n
        (d, _tasks) = _hip.match_gen_plan_query(344, 192, 344 + 20, 192 + 40, n)     # the general kernel takes it too
        assert d['default_kernel'] in ('mfma', 'gen')
        with pytest.raises(Exception):
            _hip.match_gen_plan_query(345, 192, 345 + 20, 192 + 40, n)


def test_limit_shapes_dispatch():
    """What the GPU tests below expect of the planners for a batch of 40 (host logic): the tuned kernel's class holds 209 x 190 only;
    the 17 x 33 map runs K slices and one V-form column, the 10 x 34 map two V-form columns over five Toeplitz blocks."""
    from meterelf_amd import _hip
    n = mx.N_LIMIT
    for sid in ('t209x190_i231x250', 't209x190_i231x215'):
        assert _hip.match_layout_query(*mx.LIMIT_SHAPES[sid], n)['kernel'] == 'mfma'
    (d, _t) = _hip.match_gen_plan_query(*mx.LIMIT_SHAPES['t209x190_i231x250'], n)
    assert d['default_kernel'] == 'gen' and d['v_columns'] == 0 and d['nd'] == 7, d    # 80 waves would leave the chip idle: general kernel
    assert _hip.match_layout_query(*mx.LIMIT_SHAPES['t159x256_i175x288'], n)['kernel'] == 'gen'
    (d, _t) = _hip.match_gen_plan_query(*mx.LIMIT_SHAPES['t159x256_i175x288'], n)
    assert d['default_kernel'] == 'gen' and d['v_columns'] == 1 and d['slices'] > 1 and d['nd'] == 9, d
    assert _hip.match_layout_query(*mx.LIMIT_SHAPES['t291x128_i300x161'], n)['kernel'] == 'gen'
    (d, _t) = _hip.match_gen_plan_query(*mx.LIMIT_SHAPES['t291x128_i300x161'], n)
    assert d['default_kernel'] == 'gen' and d['v_columns'] == 2 and d['nd'] == 5, d


# ------------------------------------------------------------------ GPU ----
FORCED_LAYOUTS = ((2, 0, 1), (2, 3, 1), (3, 0, 1), (3, 2, 1), (4, 0, 1), (4, 1, 1), (5, 0, 1), (4, 0, 2), (4, 1, 2), (4, 0, 4), (4, 2, 4))


def _assert_equals_reference(got, r, tag):
    """(mv, mx, my, rmap) of melf_match_ccoeff against the exact reference: ALL frames, bit for bit."""
    (mv, mxx, myy, rmap) = got
    assert rmap.shape == r['map'].shape, tag
    same = rmap.view(np.uint32) == r['map'].view(np.uint32)
    if not same.all():
        (k, y, x) = (int(v[0]) for v in np.nonzero(~same))
        raise AssertionError('%s: %d of %d map values differ; the first at frame %d (y, x) = (%d, %d): got %r, exact %r, cc %d, ws %d'
                             % (tag, int((~same).sum()), same.size, k, y, x, float(rmap[k, y, x]), float(r['map'][k, y, x]),
                                int(r['cc'][k, y, x]), int(r['ws'][k, y, x])))
    for k in range(len(mv)):
        assert (float(mv[k]), int(mxx[k]), int(myy[k])) == r['firsts'][k], (tag, k)


@pytest.mark.gpu
@pytest.mark.parametrize('sid,variant', [(s, v) for s in ('t209x190_i231x250', 't209x190_i231x215') for v in mx.VARIANTS],
                         ids=lambda v: str(v))
def test_tuned_kernel_beyond_2_31(tmp_path, monkeypatch, sid, variant):
    """k_match_mfma in every instantiation (forced: MELF_MATCH=fast, MELF_MATCH_LAYOUT=rb,np,ks) with a 209 x 190 template on
    bright frames: two column blocks (map 23 x 61) and one (23 x 26); 209 template rows pad to 210 ... 240, so the padded-row path
    runs too."""
    from tests.test_gpu_parity import _reader_with_template
    (th, tw, rows, cols) = mx.LIMIT_SHAPES[sid]
    r = mx.limit_reference(sid, variant)
    monkeypatch.setenv('MELF_MATCH', 'fast')
    reader = _reader_with_template(tmp_path / 'fast', r['tpl'])
    seen = set()
    try:
        for (rb, pairs, ks) in FORCED_LAYOUTS:
            monkeypatch.setenv('MELF_MATCH_LAYOUT', '%d,%d,%d' % (rb, pairs, ks))
            got = reader.ctx.match_ccoeff(r['imgs'], want_map=True)
            info = reader.ctx.last_match()
            assert info['kernel'] == 'mfma' and info['rows_per_wave'] == rb and info['k_slices'] == ks, info
            assert (info['pair_waves'] > 0) == (pairs > 0 and cols - tw + 1 > 32), info
            assert info['th_pad'] % ks == 0 and info['th_pad'] > th, info
            seen.add(info['th_pad'])
            _assert_equals_reference(got, r, '%s %s layout %s' % (sid, variant, info['layout']))
    finally:
        reader.close()
    # 209 rows pad to 210 (3-row period) ... and, in four slices, to 240 with pairs (two column blocks) or 220 without
    assert 210 in seen and (240 if cols - tw + 1 > 32 else 220) in seen, seen


@pytest.mark.gpu
@pytest.mark.parametrize('sid,variant', CASES3, ids=CASE3_IDS)
def test_general_kernel_beyond_2_31(tmp_path, monkeypatch, sid, variant):
    """k_match_gen (MELF_MATCH=gen) at the three largest templates: two column blocks; one column block + one V-form column in K
    slices; five Toeplitz blocks per template row with two V-form columns.  Twice (the sliced tiles' work buffers are reused)."""
    from tests.test_gpu_parity import _reader_with_template
    r = mx.limit_reference(sid, variant)
    monkeypatch.setenv('MELF_MATCH', 'gen')
    reader = _reader_with_template(tmp_path / 'gen', r['tpl'])
    try:
        for rep in range(2):
            got = reader.ctx.match_ccoeff(r['imgs'], want_map=True)
            info = reader.ctx.last_match()
            assert info['kernel'] == 'gen' and info['n'] == mx.N_LIMIT and info['groups'] == 2, info
            if sid == 't159x256_i175x288':
                assert info['slices'] > 1 and info['v_columns'] == 1 and info['nd'] == 9, info
            elif sid == 't291x128_i300x161':
                assert info['v_columns'] == 2 and info['nd'] == 5, info
            else:
                assert info['v_columns'] == 0 and info['nd'] == 7, info
            _assert_equals_reference(got, r, '%s %s %s rep %d' % (sid, variant, info['layout'], rep))
    finally:
        reader.close()


@pytest.mark.gpu
def test_default_dispatch_beyond_2_31(tmp_path, monkeypatch):
    """No MELF_MATCH: 40 frames of 231 x 250 with the 209 x 190 template go to the general kernel (too few waves for the tuned one)."""
    from tests.test_gpu_parity import _reader_with_template
    monkeypatch.delenv('MELF_MATCH', raising=False)
    monkeypatch.delenv('MELF_MATCH_LAYOUT', raising=False)
    r = mx.limit_reference('t209x190_i231x250', 'bright')
    reader = _reader_with_template(tmp_path / 'default', r['tpl'])
    try:
        got = reader.ctx.match_ccoeff(r['imgs'], want_map=True)
        info = reader.ctx.last_match()
        assert info['kernel'] == 'gen', info
        _assert_equals_reference(got, r, 'default dispatch %s' % info['layout'])
    finally:
        reader.close()


@pytest.mark.gpu
@pytest.mark.parametrize('sid,variant', CASES3, ids=CASE3_IDS)
def test_valu_kernel_beyond_2_31(tmp_path, monkeypatch, sid, variant):
    """k_match (MELF_MATCH=dot4), whose uint32_t accumulator the context's LDS rule keeps below 2^32, against the reference --
    not only against another kernel."""
    from tests.test_gpu_parity import _reader_with_template
    r = mx.limit_reference(sid, variant)
    monkeypatch.setenv('MELF_MATCH', 'dot4')
    reader = _reader_with_template(tmp_path / 'dot4', r['tpl'])
    try:
        got = reader.ctx.match_ccoeff(r['imgs'], want_map=True)
        info = reader.ctx.last_match()
        assert info['kernel'] == 'dot4', info
        _assert_equals_reference(got, r, '%s %s dot4' % (sid, variant))
        (mv, mxx, myy, _none) = reader.ctx.match_ccoeff(r['imgs'], want_map=False)
        for k in range(mx.N_LIMIT):
            assert (float(mv[k]), int(mxx[k]), int(myy[k])) == r['firsts'][k], k
    finally:
        reader.close()


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [(None, 'gen'), ('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')], ids=lambda v: str(v))
def test_full_path_beyond_2_31(tmp_path, monkeypatch, kind, kernel):
    """read_frames with a 231 x 250 meter_rect inside 239 x 262 frames whose B = G = R = the batch's L planes (so L = (max + min) / 2
    is that plane), 209 x 190 template, under each match kernel: match_val, match_x, match_y of every record equal the reference's
    first maximum, and status and the rest equal the oracle's process_frames -- with a match threshold in the middle of the batch's
    values, so that (double) match_val < threshold is decided on values whose cc lies beyond 2^31."""
    from oracle import pyoracle as po
    from tests.test_gpu_parity import _compare_records, _reader_with_template
    sid = 't209x190_i231x250'
    (th, tw, rows, cols) = mx.LIMIT_SHAPES[sid]
    r = mx.limit_reference(sid, 'bright')
    vals = np.array([f[0] for f in r['firsts']], np.float64)
    threshold = int(np.floor(np.median(vals)))
    assert 8 <= int((vals < threshold).sum()) <= mx.N_LIMIT - 8
    (x0, y0) = (6, 4)
    rng = np.random.default_rng(239262)
    frames = rng.integers(0, 256, size=(mx.N_LIMIT, rows + 8, cols + 12, 3), dtype=np.uint8)
    frames[:, y0:y0 + rows, x0:x0 + cols, :] = r['imgs'][:, :, :, None]
    if kind is None:
        monkeypatch.delenv('MELF_MATCH', raising=False)
    else:
        monkeypatch.setenv('MELF_MATCH', kind)
    monkeypatch.delenv('MELF_MATCH_LAYOUT', raising=False)
    reader = _reader_with_template(tmp_path / 'full', r['tpl'], dials_template_match_threshold=threshold,
                                   meter_rect={'top_left': [x0, y0], 'bottom_right': [x0 + cols, y0 + rows]})
    try:
        recs = reader.read_frames(frames)
        info = reader.ctx.last_match()
    finally:
        reader.close()
    assert info['kernel'] == kernel and info['n'] == mx.N_LIMIT and (info['rows'], info['cols']) == (rows, cols), info
    for k in range(mx.N_LIMIT):
        assert (float(recs[k]['match_val']), int(recs[k]['match_x']), int(recs[k]['match_y'])) == r['firsts'][k], k
        assert (int(recs[k]['status']) == 1) == (vals[k] < threshold), (k, int(recs[k]['status']), vals[k], threshold)
    ores = po.process_frames(frames, po.Params(str(tmp_path / 'full' / 'params.yml')))
    _compare_records(recs, ores, tag='full path %s' % kernel)
