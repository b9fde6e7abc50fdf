"""YCbCr 4:4:0 (luma 1x2) and 4:1:1 (luma 4x1) JPEG files decoded and read on the GPU (melf_ctx_set_jpeg_samplings).

The reference never comes from the GPU (tests/jpeg_sampling_cases.py): a frame is Pillow's (libjpeg-turbo's) decode of the same bytes,
a record is the reader's on that frame.  Bar: every byte of every frame and of every record.  The files come from tests/jpeg_writer.py
and tests/jpeg_prog_writer.py, which start from coefficient blocks (Pillow writes neither layout from an RGB image here).

CPU part: the numpy restatement of the two upsamplers against Pillow (it pins the header's formulas), the probe with and without the
new bit, the declared exports.  GPU part: whole frames over sizes that cross MCU rows and columns, the Huffman paths, extreme chroma,
the switch off, mixed batches, progressive and oriented files, the three switches together, the meter_rect window against both fixture
parameter sets, get_meter_values."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_orient_cases as jc  # noqa: E402
from tests import jpeg_prog_writer as pw  # noqa: E402
from tests import jpeg_sampling_cases as sc  # noqa: E402
from tests import jpeg_writer as jw  # noqa: E402

GOLDEN = sc.GOLDEN
PFILES = {sd: os.path.join(GOLDEN, sd, 'params.yml') for sd in ('sample-images1', 'sample-images2')}
(TAKE_ORIENT, TAKE_PROG, TAKE_SAMP) = (1, 2, 4)
OLD_REASON = 'luma sampling other than 1x1, 2x1, 2x2'
# the 13 sizes of the reference check; the refusal cases' size; 4:1:1 across an MCU column (32 pixels); 4:4:0 across an MCU row (16)
SIZES = sc.SIZES13 + [(40, 56), (8, 31), (8, 32), (8, 33), (8, 65), (15, 8), (16, 8), (17, 8), (33, 8)]


@functools.lru_cache(None)
def _grids(size, sampling, seed=5):
    rng = np.random.default_rng(seed + 1000 * size[0] + size[1])
    return tuple(sc.image_coefs(sc.natural(rng, *size), sampling))


@functools.lru_cache(None)
def _file(size, sampling):
    return sc.write(list(_grids(size, sampling)), size, sampling)


# ------------------------------------------------------------------ CPU: the reference ----
@pytest.mark.parametrize('sampling', sc.LAYOUTS)
def test_numpy_upsamplers_equal_pillow(sampling):
    """include/meterelf_hip.h's formulas, in numpy on libjpeg's own component planes (each component's grid decoded as a greyscale
    file), against Pillow's decode of the colour file: all 13 sizes, every byte."""
    for size in sc.SIZES13:
        grids = list(_grids(size, sampling))
        ref = sc.pillow_bgr(_file(size, sampling))
        got = sc.upsampled_frame(grids, size, sampling)
        assert ref.shape == (size[0], size[1], 3) and np.array_equal(got, ref), (sampling, size, int((got != ref).sum()), np.argwhere(got != ref)[:3])


def test_the_rounding_terms_decide_bytes():
    """4:4:0 planes on which +1 / +2 (and the clamp to the last REAL row) decide: the restatement with either changed differs from
    Pillow, so the equality above is not vacuous."""
    size = (22, 33)
    grids = [np.zeros((s[0], s[1], 64), np.int16) for s in jw.grid_shape(size, '440')[1]]
    rng = np.random.default_rng(9)
    for g in grids[1:]:
        g[..., 0] = rng.integers(-60, 61, g.shape[:2])          # every chroma block another flat level
        g[..., 8] = rng.integers(-30, 31, g.shape[:2])          # and a vertical ramp inside it
    data = sc.write(grids, size, '440')
    ref = sc.pillow_bgr(data)
    assert np.array_equal(sc.upsampled_frame(grids, size, '440'), ref)
    (Y, Cb, Cr) = sc.component_planes(grids, size, '440')
    y = np.arange(size[0])
    cy = y >> 1

    def variant(P, bias_odd, last):
        far = np.where(y & 1, np.minimum(cy + 1, last), np.maximum(cy - 1, 0))
        return (3 * P[cy] + P[far] + np.where(y & 1, bias_odd, 1)[:, None]) >> 2
    ch = Cb.shape[0]
    assert ch == 11 and Cb.shape[0] == Cr.shape[0]
    assert np.array_equal(sc.ycc_to_bgr(Y, variant(Cb, 2, ch - 1), variant(Cr, 2, ch - 1)), ref)
    assert not np.array_equal(sc.ycc_to_bgr(Y, variant(Cb, 1, ch - 1), variant(Cr, 1, ch - 1)), ref)   # the odd rows' rounding term


# ------------------------------------------------------------------ CPU: the probe ----
def _refusal_cases():
    from tests.test_jpeg_streams import _refusal_cases
    return _refusal_cases()


def test_exports_and_enum_values():
    import inspect
    import re

    from meterelf_amd import MeterReader, _hip
    assert {'melf_ctx_set_jpeg_samplings', 'melf_ctx_get_jpeg_samplings'} <= set(_hip.EXPORTS)
    L = _hip.lib()
    assert L.melf_ctx_set_jpeg_samplings and L.melf_ctx_get_jpeg_samplings
    assert (_hip.JPEG_TAKE_ORIENTED, _hip.JPEG_TAKE_PROGRESSIVE, _hip.JPEG_TAKE_SAMPLINGS) == (1, 2, 4)
    header = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    assert re.search(r'MELF_JPEG_TAKE_ORIENTED = 1, MELF_JPEG_TAKE_PROGRESSIVE = 2, MELF_JPEG_TAKE_SAMPLINGS = 4\b', header)
    assert 'int melf_ctx_set_jpeg_samplings(melf_ctx* ctx, int on);' in header and 'int melf_ctx_get_jpeg_samplings(melf_ctx* ctx, int* on);' in header
    assert inspect.signature(MeterReader.__init__).parameters['jpeg_samplings'].default is False
    assert hasattr(MeterReader, 'set_jpeg_samplings')


def test_probe_refuses_both_layouts_without_the_bit_and_takes_them_with_it():
    from meterelf_amd import _hip
    cases = {c.name: c for c in _refusal_cases()}
    for name in ('4:4:0', '4:1:1'):
        data = cases[name].data
        assert _hip.jpeg_probe(data) == (40, 56, False, OLD_REASON)
        for flags in range(4):
            assert _hip.jpeg_probe_flags(data, flags) == (40, 56, 1, False, OLD_REASON), (name, flags)
        for flags in range(4, 8):
            assert _hip.jpeg_probe_flags(data, flags) == (40, 56, 1, True, ''), (name, flags)
        (H, W, o, ok) = _hip.jpeg_probe_flags_batch([data, data], TAKE_SAMP)
        assert list(ok) == [1, 1] and list(H) == [40, 40] and list(W) == [56, 56]
        assert list(_hip.jpeg_probe_flags_batch([data], 3)[3]) == [0]
    with pytest.raises(Exception):
        _hip.jpeg_probe_flags(cases['4:4:0'].data, 8)                 # no such switch


def test_probe_names_410_and_refuses_other_factors():
    """4:1:0 (luma 4x2: ten blocks an MCU) is refused by name with the bit on; other luma factors and subsampled chroma spellings stay
    refused; without the bit the text is today's for all of them."""
    from meterelf_amd import _hip
    base = bytearray(_file((16, 32), '411'))
    sof = base.index(b'\xff\xc0')

    def with_factors(luma, chroma=0x11):
        b = bytearray(base)
        assert b[sof + 11] == 0x41 and b[sof + 14] == 0x11 and b[sof + 17] == 0x11
        (b[sof + 11], b[sof + 14], b[sof + 17]) = (luma, chroma, chroma)
        return bytes(b)
    (_h, _w, _o, ok, why) = _hip.jpeg_probe_flags(with_factors(0x42), TAKE_SAMP)
    assert not ok and '4:1:0' in why, why
    assert _hip.jpeg_probe_flags(with_factors(0x42), 3)[3:] == (False, OLD_REASON)
    for luma in (0x14, 0x24, 0x44, 0x31, 0x13, 0x22 + 0x10):
        (_h, _w, _o, ok, why) = _hip.jpeg_probe_flags(with_factors(luma), TAKE_SAMP)
        assert not ok and 'luma sampling other than' in why and '4x1' in why, (hex(luma), why)
        assert _hip.jpeg_probe_flags(with_factors(luma), 0)[3:] == (False, OLD_REASON)
    for flags in (0, TAKE_SAMP):                                       # the "2x2 / 1x2 / 1x2" spelling of 4:2:2: chroma factors above 1
        (_h, _w, _o, ok, why) = _hip.jpeg_probe_flags(with_factors(0x22, 0x12), flags)
        assert not ok and 'subsampled chroma' in why, why
    assert _hip.jpeg_probe_flags(with_factors(0x41), TAKE_SAMP)[:4] == (16, 32, 1, True)
    assert _hip.jpeg_probe_flags(with_factors(0x12), TAKE_SAMP)[:4] == (16, 32, 1, True)


def test_the_bit_alone_changes_no_other_answer():
    from meterelf_amd import _hip
    seen = 0
    for c in _refusal_cases():
        if c.name in ('4:4:0', '4:1:1'):
            continue
        for flags in (0, TAKE_ORIENT, TAKE_PROG, 3):
            assert _hip.jpeg_probe_flags(c.data, flags | TAKE_SAMP) == _hip.jpeg_probe_flags(c.data, flags), (c.name, flags)
        seen += 1
    assert seen == 8
    for s in ('420', '422', '444', 'grey'):                            # and files of the four older samplings stay taken
        assert _hip.jpeg_probe_flags(_file((24, 40), s), TAKE_SAMP) == _hip.jpeg_probe_flags(_file((24, 40), s), 0) == (24, 40, 1, True, '')
    rng = np.random.default_rng(2)
    prog = pw.write_progressive(list(_grids((37, 53), '440')), (37, 53), '440', sc.QT, pw.PILLOW_COLOUR)
    assert _hip.jpeg_probe_flags(prog, TAKE_SAMP)[3] is False and 'progressive' in _hip.jpeg_probe_flags(prog, TAKE_SAMP)[4]
    assert _hip.jpeg_probe_flags(prog, TAKE_PROG)[3:] == (False, OLD_REASON)
    assert _hip.jpeg_probe_flags(prog, TAKE_PROG | TAKE_SAMP)[:4] == (37, 53, 1, True)
    tagged = jc.with_app1(_file((37, 53), '411'), jc.tiff_block(6, bool(rng.integers(0, 2))))
    assert _hip.jpeg_probe_flags(tagged, TAKE_SAMP)[2:4] == (6, False) and 'EXIF' in _hip.jpeg_probe_flags(tagged, TAKE_SAMP)[4]
    assert _hip.jpeg_probe_flags(tagged, TAKE_ORIENT | TAKE_SAMP)[:4] == (37, 53, 6, True)


def test_get_meter_values_asks_for_the_switch_unless_the_host_is_asked_for(monkeypatch):
    from meterelf_amd import _api, _engine, _params

    class Reader:
        jpeg_samplings = False

        def set_jpeg_samplings(self, on):
            self.jpeg_samplings = bool(on)
    monkeypatch.delenv('METERELF_JPEG_SAMPLING', raising=False)
    assert _api._jpeg_on_gpu('jpeg_samplings') and _api._with_jpeg_orientation(Reader()).jpeg_samplings
    params = _params.load(PFILES['sample-images1'])
    blob = _engine.make_blob(params)
    k_gpu = _api._reader_key(params, blob, 0)
    monkeypatch.setenv('METERELF_JPEG_SAMPLING', 'host')
    assert not _api._jpeg_on_gpu('jpeg_samplings') and not _api._with_jpeg_orientation(Reader()).jpeg_samplings
    assert _api._reader_key(params, blob, 0) != k_gpu                  # a reader made under one setting is never handed out under the other
    monkeypatch.setenv('METERELF_JPEG_SAMPLING', 'gpu')
    assert _api._reader_key(params, blob, 0) == k_gpu


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope='module')
def reader():
    from meterelf_amd import _hip
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    r = MeterReader(_params.load(PFILES['sample-images1']), jpeg_samplings=True)
    assert r.ctx.jpeg_samplings() and r.jpeg_samplings and not r.ctx.jpeg_orientation() and not r.ctx.jpeg_progressive()
    yield r
    r.close()


def _assert_equal_to_pillow(ctx, files):
    """files: (name, bytes, (H, W)); one decode call per size, every status 0 and every byte Pillow's."""
    by_size = {}
    for (name, data, size) in files:
        by_size.setdefault(size, []).append((name, data))
    n = 0
    for ((H, W), group) in by_size.items():
        (frames, status) = ctx.jpeg_decode([d for (_n, d) in group], H, W)
        for ((name, data), got, st) in zip(group, frames, status):
            ref = sc.pillow_bgr(data)
            assert st == 0, (name, int(st))
            assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:3])
            n += 1
    assert n == len(files)


@pytest.mark.gpu
@pytest.mark.parametrize('sampling', sc.LAYOUTS)
def test_small_frames_equal_pillow(reader, sampling):
    _assert_equal_to_pillow(reader.ctx, [('%s-%dx%d' % (sampling, *size), _file(size, sampling), size) for size in SIZES])


def _huffman_path_files():
    (H, W) = size = (37, 53)
    out = []
    big16 = (np.array(sc.q_ramp(3), np.int64) + (np.arange(64) // 8 + np.arange(64) % 8 >= 6) * 900).tolist()
    for sampling in sc.LAYOUTS:
        grids = list(_grids(size, sampling))
        ((my, mx), _s) = jw.grid_shape(size, sampling)
        out.append(('%s-rst-1' % sampling, sc.write(grids, size, sampling, restart=1), size))
        out.append(('%s-rst-row' % sampling, sc.write(grids, size, sampling, restart=mx), size))
        out.append(('%s-rst-mid-row' % sampling, sc.write(grids, size, sampling, restart=mx + 1), size))
        out.append(('%s-sof1' % sampling, sc.write(grids, size, sampling, layout=dict(sof=0xC1)), size))
        q16 = {0: (big16, True), 1: (sc.q_ramp(5), True)}
        g16 = sc.image_coefs(sc.natural(np.random.default_rng(16), H, W), sampling, q16)
        out.append(('%s-dqt16' % sampling, sc.write(g16, size, sampling, q16), size))
        for (k, sel) in enumerate(([(0, 1, 1), (1, 0, 0), (1, 0, 0)], [(0, 0, 1), (1, 1, 0), (1, 0, 1)], [(1, 1, 0), (0, 0, 0), (1, 1, 1)])):
            gs = jw.coefficients_from_image(sc.natural(np.random.default_rng(40 + k), H, W), sampling, [sc.QT[sel[c][0]][0] for c in range(3)])
            out.append(('%s-sel-%d' % (sampling, k), sc.write(gs, size, sampling, sel=sel), size))
    assert all((b'\xff\xdd' in d) == ('rst' in n) for (n, d, _s) in out)
    return out


@pytest.mark.gpu
def test_huffman_paths(reader):
    """k_jpeg_huff_rst (an interval of one MCU, of one MCU row, of one MCU more than a row), SOF1, 16-bit quantisation tables (entries
    above 255), Huffman and quantisation tables assigned crosswise."""
    _assert_equal_to_pillow(reader.ctx, _huffman_path_files())


@pytest.mark.gpu
@pytest.mark.parametrize('sampling', sc.LAYOUTS)
def test_a_scan_long_enough_for_the_1024_lane_kernel(reader, sampling):
    """A scan above 2 MB takes k_jpeg_huff<1024> (tests/test_jpeg_orient.py's size for that kernel): dense mid-size coefficients that
    keep every block inside the writer's range condition (jpeg_sampling_cases.dense_file)."""
    size = (1088, 1280)
    (data, scan) = sc.dense_file(size, sampling)
    assert 2100000 < scan < 3900000, scan                              # above half of what the kernel addresses with 512 lanes, below its limit
    _assert_equal_to_pillow(reader.ctx, [('%s-long' % sampling, data, size)])


def _extreme_chroma_files():
    """Chroma planes at constant 0, constant 255, and a checkerboard of the extremes the writer's range condition allows (DC of
    neighbouring blocks at the two ends, so that the filter of 4:4:0 mixes 0 and 255 across every block border and the rounding terms
    decide bytes), under a luma ramp."""
    out = []
    q8 = {0: ([8] * 64, False), 1: ([8] * 64, False)}
    for sampling in sc.LAYOUTS:
        for size in ((37, 53), (16, 65)):
            shapes = jw.grid_shape(size, sampling)[1]
            luma = np.zeros((shapes[0][0], shapes[0][1], 64), np.int16)
            luma[..., 0] = (np.arange(shapes[0][0])[:, None] * 7 + np.arange(shapes[0][1])[None, :] * 11) % 200 - 100
            luma[..., 1] = 9
            for (name, lo, hi) in (('zero', -128, -128), ('full', 127, 127), ('checker', -128, 127), ('near', -3, 2)):
                grids = [luma]
                for c in (1, 2):
                    g = np.zeros((shapes[c][0], shapes[c][1], 64), np.int16)
                    par = (np.arange(shapes[c][0])[:, None] + np.arange(shapes[c][1])[None, :] + c) & 1
                    g[..., 0] = np.where(par, hi, lo)                  # DC * 8 / 8 = the block's level around 128
                    if name == 'near':
                        g[..., 8] = np.where(par, 1, -1)               # a one-step vertical ramp: neighbouring rows one level apart
                    grids.append(g)
                out.append(('%s-%s-%dx%d' % (sampling, name, *size), sc.write(grids, size, sampling, q8), size))
    return out


@pytest.mark.gpu
def test_extreme_chroma_planes(reader):
    files = _extreme_chroma_files()
    ref = sc.pillow_bgr([d for (n, d, _s) in files if n.startswith('440-checker')][0])
    assert len(np.unique(ref.reshape(-1, 3), axis=0)) > 8              # the filter made intermediate levels: not a flat frame
    _assert_equal_to_pillow(reader.ctx, files)


@pytest.mark.gpu
def test_the_switch_off_every_entry_point_refuses(reader, tmp_path):
    """Status 1 and a zero-filled frame from the decode call (small files, the refusal cases' own among them), status 1 from the
    calls that read (fixture frames re-encoded in both layouts: the reading path needs the meter_rect inside the frame)."""
    from meterelf_amd import MeterReader, _hip, _params
    (h, w) = (40, 56)
    small = [_file((h, w), s) for s in sc.LAYOUTS] + [c.data for c in _refusal_cases() if c.name in ('4:4:0', '4:1:1')]
    (items, (H, W)) = _reencoded('sample-images1')
    files = [d for (_s, d) in items[:2]]
    paths = []
    for (k, d) in enumerate(files):
        paths.append(str(tmp_path / ('off%d.jpg' % k)))
        open(paths[-1], 'wb').write(d)
    plain = MeterReader(_params.load(PFILES['sample-images1']))
    try:
        assert not plain.ctx.jpeg_samplings() and not plain.jpeg_samplings
        (frames, status) = plain.ctx.jpeg_decode(small, h, w)
        assert (status == _hip.JPEG_UNSUPPORTED).all() and not frames.any()
        (frames, status) = plain.ctx.jpeg_decode(files, H, W)
        assert (status == _hip.JPEG_UNSUPPORTED).all() and not frames.any()
        (_recs, status) = plain.ctx.jpeg_process_batch(files, H, W)
        assert (status == _hip.JPEG_UNSUPPORTED).all()
        (_recs, status) = plain.ctx.jpeg_process_batch(files * 40, H, W)      # the chunked path
        assert (status == _hip.JPEG_UNSUPPORTED).all()
        (_recs, status, _hw) = plain.ctx.jpeg_process_files(paths)
        assert (status == _hip.JPEG_UNSUPPORTED).all()
        plain.ctx.jpeg_process_files_begin(paths)
        (_recs, status, _hw) = plain.ctx.jpeg_process_files_end()
        assert (status == _hip.JPEG_UNSUPPORTED).all()
        assert plain.read_jpeg_files(files) == [None] * len(files)
        (_r, ok) = plain.read_jpeg_paths_batch(paths)
        assert not ok.any()
    finally:
        plain.close()
    # the switch turned off again on the reader that had it on: the same; and not while a _begin call is in flight
    reader.set_jpeg_samplings(False)
    try:
        (frames, status) = reader.ctx.jpeg_decode(small, h, w)
        assert (status == _hip.JPEG_UNSUPPORTED).all() and not frames.any()
    finally:
        reader.set_jpeg_samplings(True)
    (frames, status) = reader.ctx.jpeg_decode(small, h, w)
    assert (status == 0).all() and all(np.array_equal(f, sc.pillow_bgr(d)) for (f, d) in zip(frames, small))
    reader.ctx.jpeg_process_files_begin(paths)
    with pytest.raises(Exception):
        reader.ctx.set_jpeg_samplings(False)
    (_recs, status, hw) = reader.ctx.jpeg_process_files_end()
    assert hw == (H, W) and (status == 0).all() and reader.ctx.jpeg_samplings()


@pytest.mark.gpu
def test_mixed_batch_in_one_call(reader):
    """4:2:0, 4:2:2, 4:4:4, grey, 4:4:0 and 4:1:1 files of one size interleaved in one call, one of another size, one cut short: frames
    and statuses in the caller's order."""
    from meterelf_amd import _hip
    size = (40, 56)
    kinds = ['420', '440', '422', '411', '444', 'grey', '411', '440', '420', '411', '440', 'grey']
    files = []
    for (k, s) in enumerate(kinds):
        rng = np.random.default_rng(300 + k)
        files.append(sc.natural_file(rng, size, s, restart=(3 if k % 5 == 1 else 0)))
    other = len(files)
    files.append(_file((37, 53), '440'))
    cut = len(files)
    whole = _file(size, '411')
    files.append(whole[:len(whole) - len(whole) // 3])
    files.append(_file(size, '440'))
    (frames, status) = reader.ctx.jpeg_decode(files, *size)
    want = np.zeros(len(files), np.int32)
    want[other] = _hip.JPEG_SIZE_MISMATCH
    want[cut] = _hip.JPEG_CORRUPT
    assert np.array_equal(status, want), status
    for (i, d) in enumerate(files):
        if want[i] == 0:
            ref = sc.pillow_bgr(d)
            assert np.array_equal(frames[i], ref), (i, int((frames[i] != ref).sum()))
        else:
            assert not frames[i].any(), i


def _prog_files():
    """Both layouts through the progressive writer with libjpeg's ten-scan colour script, with and without restart intervals, and the
    baseline file of the same coefficients."""
    out = []
    for sampling in sc.LAYOUTS:
        for size in ((37, 53), (16, 65)):
            grids = list(_grids(size, sampling))
            ((my, mx), _s) = jw.grid_shape(size, sampling)
            for (name, restart) in (('plain', 0), ('rst', [mx, 3, 2, 2, 3, 5, 1, 2, 2, 4])):
                data = pw.write_progressive(grids, size, sampling, sc.QT, pw.PILLOW_COLOUR, restart=restart)
                base = sc.write(pw.decoded_grids(grids, size, sampling, pw.PILLOW_COLOUR), size, sampling)
                out.append(('%s-%dx%d-%s' % (sampling, *size, name), data, base, size))
    return out


@pytest.mark.gpu
def test_progressive_files_of_both_layouts(reader):
    """A luma AC scan of a 4:1:1 file walks ceil(W / 8) real blocks a row across MCUs 4 blocks wide, of a 4:4:0 file ceil(H / 8) real
    block rows across MCUs 2 blocks tall (37 x 53 and 16 x 65 leave padded blocks in both): equal to Pillow, and to the baseline
    decode of the same coefficients."""
    files = _prog_files()
    assert len(files) == 8
    reader.set_jpeg_progressive(True)
    try:
        _assert_equal_to_pillow(reader.ctx, [(n, d, s) for (n, d, _b, s) in files])
        _assert_equal_to_pillow(reader.ctx, [(n + '-baseline', b, s) for (n, _d, b, s) in files])
        for (n, d, b, s) in files:
            assert np.array_equal(sc.pillow_bgr(d), sc.pillow_bgr(b)), n
    finally:
        reader.set_jpeg_progressive(False)
    # that switch off: the progressive ones are the host's again, the baseline ones are still taken
    (n, d, b, s) = files[0]
    (_f, status) = reader.ctx.jpeg_decode([d, b], *s)
    assert list(status) == [1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize('sampling', sc.LAYOUTS)
def test_oriented_files_of_both_layouts(reader, sampling):
    """Each of the eight codes at 37 x 53 stored: Pillow's decode permuted by the table."""
    (Hs, Ws) = size = (37, 53)
    plain = _file(size, sampling)
    groups = {}
    for code in jc.CODES:
        data = jc.with_app1(plain, jc.tiff_block(code, code % 2 == 0))
        groups.setdefault((Ws, Hs) if code >= 5 else (Hs, Ws), []).append((code, data))
    reader.set_jpeg_orientation(True)
    try:
        n = 0
        for ((Hu, Wu), items) in groups.items():
            (frames, status) = reader.ctx.jpeg_decode([d for (_c, d) in items], Hu, Wu)
            assert (status == 0).all(), (Hu, Wu, status)
            for ((code, d), got) in zip(items, frames):
                ref = jc.reference_frame(d, code)
                assert got.shape == ref.shape and np.array_equal(got, ref), (sampling, code, int((got != ref).sum()))
                n += 1
        assert n == 8
    finally:
        reader.set_jpeg_orientation(False)


@pytest.mark.gpu
def test_all_three_switches(reader):
    """A progressive 4:4:0 file (and a 4:1:1 one) with an EXIF code: taken only with all three switches on."""
    from meterelf_amd import _hip
    (Hs, Ws) = size = (37, 53)
    files = []
    for (sampling, code) in (('440', 6), ('411', 7)):
        grids = list(_grids(size, sampling))
        prog = pw.write_progressive(grids, size, sampling, sc.QT, pw.PILLOW_COLOUR, restart=[2, 3, 0, 0, 4, 0, 1, 0, 2, 0])
        files.append((jc.with_app1(prog, jc.tiff_block(code, False)), code))
    assert _hip.jpeg_probe_flags(files[0][0], 7)[:4] == (Hs, Ws, 6, True)
    for on in range(8):
        reader.set_jpeg_orientation(bool(on & 1))
        reader.set_jpeg_progressive(bool(on & 2))
        reader.set_jpeg_samplings(bool(on & 4))
        try:
            (H, W) = (Ws, Hs) if on & 1 else (Hs, Ws)
            (frames, status) = reader.ctx.jpeg_decode([d for (d, _c) in files], H, W)
            if on == 7:
                assert (status == 0).all(), status
                for ((d, code), got) in zip(files, frames):
                    assert np.array_equal(got, jc.reference_frame(d, code)), code
            else:
                assert (status == _hip.JPEG_UNSUPPORTED).all() and not frames.any(), (on, status)
        finally:
            reader.set_jpeg_orientation(False)
            reader.set_jpeg_progressive(False)
            reader.set_jpeg_samplings(True)


# ---- the meter_rect window and the records ----
@functools.lru_cache(None)
def _reencoded(sd, n=4):
    """n fixture frames of the set re-encoded in each layout: [(layout, bytes)], and the frames' (H, W)."""
    (_files, frames) = sc.fixture_frames(n, sd)
    return ([(s, sc.reencode(f, s)) for f in frames for s in sc.LAYOUTS], frames[0].shape[:2])


@pytest.mark.gpu
@pytest.mark.parametrize('sd', list(PFILES))
def test_window_and_records(sd, tmp_path):
    """melf_jpeg_process_batch decodes the meter_rect window only (16 pixels of margin, 16-aligned: for sample-images2 its left edge,
    48, is the middle of a 32-pixel MCU of a 4:1:1 file; for sample-images1 it is 32, an MCU corner): the records equal
    melf_process_batch's on Pillow's decode of the same bytes, bit for bit, from memory and from disk."""
    from meterelf_amd import MeterReader, _hip, _params
    params = _params.load(PFILES[sd])
    ((x0, y0), (x1, y1)) = params.meter_rect
    left = max(0, (x0 - 16) & ~15)
    assert (left % 32 != 0) == (sd == 'sample-images2'), (sd, left)
    (items, (H, W)) = _reencoded(sd)
    datas = [d for (_s, d) in items]
    assert len(datas) == 8 and all(_hip.jpeg_probe_flags(d, TAKE_SAMP)[:4] == (H, W, 1, True) for d in datas)
    r = MeterReader(params, jpeg_samplings=True)
    try:
        ref = r.ctx.process_batch(np.stack([sc.pillow_bgr(d) for d in datas]))
        assert (ref['status'] == _hip.FRAME_OK).sum() * 4 >= 3 * len(datas), ref['status']
        (recs, status) = r.ctx.jpeg_process_batch(datas, H, W)
        assert (status == 0).all(), status
        assert recs.tobytes() == ref.tobytes(), [i for i in range(len(datas)) if recs[i].tobytes() != ref[i].tobytes()]
        many = datas * 10                                              # 80 files: the chunked path
        (recs, status) = r.ctx.jpeg_process_batch(many, H, W)
        assert (status == 0).all() and recs.tobytes() == ref.tobytes() * 10
        paths = []
        for (k, d) in enumerate(datas):
            paths.append(str(tmp_path / ('w%d.jpg' % k)))
            open(paths[-1], 'wb').write(d)
        (recs, status, hw) = r.ctx.jpeg_process_files(paths)
        assert hw == (H, W) and (status == 0).all() and recs.tobytes() == ref.tobytes()
        got = r.read_jpeg_files(datas)
        assert all(g is not None and g.tobytes() == x.tobytes() for (g, x) in zip(got, ref))
        (r1, ok1) = r.read_jpeg_paths_batch(paths)
        assert ok1.all() and r1.tobytes() == ref.tobytes()
    finally:
        r.close()


@pytest.mark.gpu
def test_get_meter_values_reads_them_on_the_gpu(tmp_path, monkeypatch):
    """A directory mixing fixture files with their 4:4:0 / 4:1:1 re-encodings: the same values by default and under
    METERELF_JPEG_SAMPLING=host, and by default the host decoder is never called."""
    import meterelf_amd
    from meterelf_amd import _image
    (items, _hw) = _reencoded('sample-images1')
    (fixtures, _frames) = sc.fixture_frames(12)
    paths = []
    for (k, (s, d)) in enumerate(items):
        p = str(tmp_path / ('m%02d_%s.jpg' % (k, s)))
        open(p, 'wb').write(d)
        paths += [p, fixtures[4 + k]]
    calls = []
    real = _image.imread_bgr

    def counting(filename):
        calls.append(filename)
        return real(filename)
    monkeypatch.setattr(_image, 'imread_bgr', counting)
    monkeypatch.setenv('METERELF_CTX_CACHE', '0')
    monkeypatch.setenv('METERELF_JPEG_SAMPLING', 'host')
    host = list(meterelf_amd.get_meter_values(PFILES['sample-images1'], paths))
    assert sorted(calls) == sorted(paths[0::2])                        # the host branch: exactly the re-encoded files
    del calls[:]
    monkeypatch.delenv('METERELF_JPEG_SAMPLING')
    got = list(meterelf_amd.get_meter_values(PFILES['sample-images1'], paths))
    assert calls == []
    assert [g.filename for g in got] == paths
    for (g, h) in zip(got, host):
        assert g.meter_values == h.meter_values and g.value == h.value and (g.error is None) == (h.error is None)
    assert sum(g.error is None for g in got) * 4 >= 3 * len(got)
