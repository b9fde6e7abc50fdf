"""Multi-scan sequential JPEG files -- three scans of one component each -- decoded and read on the GPU (melf_ctx_set_jpeg_multiscan).

The reference never comes from the GPU (tests/jpeg_scans_cases.py): a frame is Pillow's (libjpeg-turbo's) decode of the same bytes, a
record is the reader's on that frame.  Bar: every byte of every frame and of every record.  The files are spliced from the
entropy-coded segments tests/jpeg_writer.py writes for each component's real-block grid as a greyscale file.

CPU part: Pillow decodes every multi-scan file like its interleaved twin, the probe with and without the bit, the refused scripts and
what Pillow makes of them, the scan plan swept on the host (tests/jpeg_scans_main.cpp, plain and under the host sanitizers).  GPU part:
whole frames over sizes that cut the MCU both ways, samplings, scan orders, restart plans and table plans; calls shared with every
other kind of file; the switches off; the meter_rect window beyond half the frame; every reading entry point; corrupt scans; and the
launches of a call without such files."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_orient_cases as jc  # noqa: E402
from tests import jpeg_prog_writer as pw  # noqa: E402
from tests import jpeg_sampling_cases as sc  # noqa: E402
from tests import jpeg_scans_cases as ms  # noqa: E402
from tests import jpeg_writer as jw  # noqa: E402

PFILE = os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml')
# what Pillow (libjpeg-turbo) does with the scripts the decoder refuses: it decodes every one of them without complaint
PILLOW_ON_REFUSALS = {
    'two components in a scan': 'decodes', 'component sent twice': 'decodes', 'ends before the third scan': 'decodes',
    'DQT behind the first SOS': 'decodes', 'segment behind the third scan': 'decodes', 'fourth scan': 'decodes'}


@functools.lru_cache(None)
def _cases(size):
    return ms.decode_cases(size)


def _flags_for(name):
    return ms.TAKE_MULTI | (ms.TAKE_SAMP if name.split('-')[1] in ('411', '440') else 0)


# ------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize('size', ms.SIZES, ids=lambda s: '%dx%d' % s)
def test_pillow_decodes_every_case_like_its_interleaved_twin(size):
    cases = _cases(size)
    assert len(cases) == 45 * len(ms.samplings_of(size))
    for (name, data, twin) in cases:
        assert data.count(b'\xff\xda') >= 3 and np.array_equal(sc.pillow_bgr(data), sc.pillow_bgr(twin)), name


def test_the_redefined_tables_decide_the_decode():
    """The 'redefined' plan is not vacuous: with the last definition of table 0 / 0 hoisted in front of all three scans the file no
    longer decodes to the twin's frame (Pillow raises or returns another frame)."""
    size = (37, 51)
    grids = ms.grids_for(size, '420')
    (tables, sof, hoist) = ms.table_plan('redefined')
    assert not hoist and len({(t[0], t[1]) for t in tables}) == 1 and len({repr(t[2:]) for t in tables}) == 3
    good = ms.write_multiscan(grids, size, '420', tables=tables, hoist=False)
    last = [tables[2]] * 3
    body = ms.write_multiscan(grids, size, '420', tables=last, hoist=True)
    sos = ms.segments(body)[-1][1]
    head_end = ms.segments(good)[-1][1]
    bad = body[:sos] + good[head_end:]                                 # the good file's scans behind a header that defines the last tables only
    try:
        same = np.array_equal(sc.pillow_bgr(bad), sc.pillow_bgr(good))
    except Exception:
        same = False
    assert not same


def test_exports_and_enum_values():
    import inspect
    import re

    from meterelf_amd import MeterReader, _hip
    assert {'melf_ctx_set_jpeg_multiscan', 'melf_ctx_get_jpeg_multiscan'} <= set(_hip.EXPORTS)
    L = _hip.lib()
    assert L.melf_ctx_set_jpeg_multiscan and L.melf_ctx_get_jpeg_multiscan
    assert _hip.JPEG_TAKE_MULTISCAN == 32
    header = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    assert re.search(r'MELF_JPEG_TAKE_MULTISCAN = 32\b', header)
    assert 'int melf_ctx_set_jpeg_multiscan(melf_ctx* ctx, int on);' in header and 'int melf_ctx_get_jpeg_multiscan(melf_ctx* ctx, int* on);' in header
    assert inspect.signature(MeterReader.__init__).parameters['jpeg_multiscan'].default is False
    assert hasattr(MeterReader, 'set_jpeg_multiscan')


@pytest.mark.parametrize('size', ms.SIZES, ids=lambda s: '%dx%d' % s)
def test_probe_refuses_every_case_without_the_bit_and_takes_it_with_it(size):
    from meterelf_amd import _hip
    for (name, data, twin) in _cases(size):
        fl = _flags_for(name)
        assert _hip.jpeg_probe(data) == (size[0], size[1], False, ms.OLD_REASON), name
        for flags in (0, fl & ~ms.TAKE_MULTI, 7, 7 | ms.TAKE_TABLES):
            assert _hip.jpeg_probe_flags(data, flags) == (size[0], size[1], 1, False, ms.OLD_REASON), (name, flags)
        assert _hip.jpeg_probe_flags(data, fl) == (size[0], size[1], 1, True, ''), name
        assert _hip.jpeg_probe_flags(twin, fl) == _hip.jpeg_probe_flags(twin, fl & ~ms.TAKE_MULTI) == (size[0], size[1], 1, True, ''), name
    datas = [d for (_n, d, _t) in _cases(size)[:45]]
    (H, W, _o, ok) = _hip.jpeg_probe_flags_batch(datas, ms.TAKE_MULTI)
    assert ok.all() and (H == size[0]).all() and (W == size[1]).all()
    assert not _hip.jpeg_probe_flags_batch(datas, 7)[3].any()


def test_refused_scripts_have_reasons_of_their_own_and_pillow_is_pinned():
    from meterelf_amd import _hip
    cases = ms.refusal_cases()
    assert set(cases) == set(PILLOW_ON_REFUSALS)
    reasons = {}
    pillow = {}
    for (name, data) in cases.items():
        assert _hip.jpeg_probe_flags(data, 0) == (37, 51, 1, False, ms.OLD_REASON), name
        (h, w, _o, ok, why) = _hip.jpeg_probe_flags(data, ms.TAKE_MULTI)
        assert (h, w) == (37, 51) and not ok and why and why != ms.OLD_REASON, (name, why)
        reasons[name] = why
        try:
            sc.pillow_bgr(data)
            pillow[name] = 'decodes'
        except Exception as e:
            pillow[name] = 'error: ' + type(e).__name__
    assert pillow == PILLOW_ON_REFUSALS
    assert reasons['fourth scan'] == reasons['segment behind the third scan']
    assert len(set(reasons.values())) == len(reasons) - 1, reasons


def test_tables_a_scan_needs_and_the_default_tables():
    """A scan whose table was never defined is refused by that name; with the default-tables bit the Annex K tables are filled in once,
    before the first scan; a file cut inside a scan is unreadable, as a truncated file ever was."""
    from meterelf_amd import _hip
    size = (37, 51)
    grids = ms.grids_for(size, '422')
    bare = ms.write_multiscan(grids, size, '422', omit=ms.ALL_TABLES)
    assert b'\xff\xc4' not in bare
    assert np.array_equal(sc.pillow_bgr(bare), sc.pillow_bgr(sc.write(grids, size, '422')))
    assert _hip.jpeg_probe_flags(bare, ms.TAKE_MULTI)[3:] == (False, ms.OLD_TABLE_REASON)
    assert _hip.jpeg_probe_flags(bare, ms.TAKE_TABLES)[3:] == (False, ms.OLD_REASON)
    assert _hip.jpeg_probe_flags(bare, ms.TAKE_MULTI | ms.TAKE_TABLES) == (37, 51, 1, True, '')
    (tables, sof, hoist) = ms.table_plan('ids23')
    high = ms.write_multiscan(grids, size, '422', tables=tables, sof=sof, omit=(('ac', 3),))
    assert _hip.jpeg_probe_flags(high, ms.TAKE_MULTI | ms.TAKE_TABLES)[3:] == (False, ms.OLD_TABLE_REASON)   # slots 2 and 3 receive nothing
    whole = ms.write_multiscan(grids, size, '422')
    (a, b) = ms.scan_offsets(whole)[1]
    assert _hip.jpeg_probe_flags(whole[:(a + b) // 2], ms.TAKE_MULTI)[:4] == (0, 0, 1, False)
    # an interleaved file that defines a table with id 2 stays refused whether or not the bit is on
    (dc, ac) = sc.std_tables()
    extra = jw.write_jpeg(grids, size, '422', sc.QT, {0: dc[0], 1: dc[1], 2: dc[0]}, {0: ac[0], 1: ac[1]})
    assert _hip.jpeg_probe_flags(extra, 0)[3:] == _hip.jpeg_probe_flags(extra, ms.TAKE_MULTI)[3:] == (False, 'Huffman table id above 1')


def test_the_bit_alone_changes_no_other_answer():
    from meterelf_amd import _hip
    from tests.test_jpeg_streams import _refusal_cases
    seen = 0
    for c in _refusal_cases():
        for flags in (0, 1, 2, 4, 7):
            (a, b) = (_hip.jpeg_probe_flags(c.data, flags | ms.TAKE_MULTI), _hip.jpeg_probe_flags(c.data, flags))
            assert a == b or b[4] == ms.OLD_REASON, (c.name, flags, a, b)
        seen += 1
    assert seen >= 8


def _compiler():
    for cxx in (os.environ.get('CXX'), '/opt/rocm/llvm/bin/clang++', 'g++', 'clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail('no C++ compiler for the stand-alone program')


@pytest.mark.parametrize('flags', [[], ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g']], ids=['plain', 'sanitizers'])
def test_the_scan_plan_swept_on_the_host(tmp_path, flags):
    """tests/jpeg_scans_main.cpp: windows, block addresses and areas of meterelf_amd/csrc/melf_jpeg_scans.h over every size 1..70 x 1..70,
    every sampling and every window, as an ordinary program."""
    exe = str(tmp_path / 'jpeg_scans_main')
    subprocess.check_call([_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + flags +
                          ['-I', os.path.join(ROOT, 'meterelf_amd', 'csrc'), os.path.join(ROOT, 'tests', 'jpeg_scans_main.cpp'), '-o', exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    (word, count) = out.stdout.decode().split()
    assert word == 'ok' and int(count) > 2000000


def test_get_meter_values_asks_for_the_switch_unless_the_host_is_asked_for(monkeypatch):
    """METERELF_JPEG_MULTISCAN: 'gpu' (the default, which the rate tool's one-file-in-a-call rows decide) or 'host'; the setting is part of
    the reader-cache key."""
    from meterelf_amd import _api, _engine, _params

    class Reader:
        jpeg_multiscan = False

        def set_jpeg_multiscan(self, on):
            self.jpeg_multiscan = bool(on)
    monkeypatch.delenv('METERELF_JPEG_MULTISCAN', raising=False)
    params = _params.load(PFILE)
    blob = _engine.make_blob(params)
    k_default = _api._reader_key(params, blob, 0)
    default_on = _api._jpeg_on_gpu('jpeg_multiscan')
    assert default_on
    assert _api._with_jpeg_orientation(Reader()).jpeg_multiscan == default_on
    monkeypatch.setenv('METERELF_JPEG_MULTISCAN', 'host')
    assert not _api._jpeg_on_gpu('jpeg_multiscan') and not _api._with_jpeg_orientation(Reader()).jpeg_multiscan
    k_host = _api._reader_key(params, blob, 0)
    monkeypatch.setenv('METERELF_JPEG_MULTISCAN', 'gpu')
    assert _api._jpeg_on_gpu('jpeg_multiscan') and _api._with_jpeg_orientation(Reader()).jpeg_multiscan
    assert _api._reader_key(params, blob, 0) != k_host                 # a reader made under one setting is never handed out under the other
    assert k_default == (_api._reader_key(params, blob, 0) if default_on else k_host)


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope='module')
def reader():
    from meterelf_amd import _hip
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    r = MeterReader(_params.load(PFILE), jpeg_multiscan=True, jpeg_samplings=True)
    assert r.ctx.jpeg_multiscan() and r.jpeg_multiscan and r.ctx.jpeg_samplings() and not r.ctx.jpeg_default_tables()
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize('size', ms.SIZES, ids=lambda s: '%dx%d' % s)
def test_frames_equal_pillow(reader, size):
    """melf_jpeg_decode_batch, one call for the size: every sampling, scan order, restart plan and table plan, every byte Pillow's."""
    cases = _cases(size)
    (frames, status) = reader.ctx.jpeg_decode([d for (_n, d, _t) in cases], *size)
    assert (status == 0).all(), [(n, int(s)) for ((n, _d, _t), s) in zip(cases, status) if s != 0][:5]
    for ((name, data, _twin), got) in zip(cases, frames):
        ref = sc.pillow_bgr(data)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:3])


def _shared_call(size=(37, 51)):
    """[(kind, bytes, EXIF code)] in a shuffled order: multi-scan, baseline, DHT-less, oriented and progressive files of one upright size."""
    rng = np.random.default_rng(77)
    files = []
    for (k, sampling) in enumerate(('420', '422', '444', '420', '422')):
        grids = ms.grids_for(size, sampling, seed=20 + k)
        files.append(('multi', ms.write_multiscan(grids, size, sampling, order=ms.ORDERS[k % 3], restarts=ms.restart_plan(ms.RESTARTS[k], size, sampling)), 1))
        files.append(('baseline', sc.write(grids, size, sampling, restart=(0, 3)[k % 2]), 1))
        files.append(('bare', ms.without_tables(grids, size, sampling), 1))
        files.append(('prog', pw.write_progressive(grids, size, sampling, sc.QT, pw.PILLOW_COLOUR), 1))
        files.append(('oriented', jc.with_app1(sc.write(grids, size, sampling), jc.tiff_block(3, bool(k % 2))), 3))
    files.append(('multi-bare', ms.write_multiscan(ms.grids_for(size, '422', seed=40), size, '422', omit=ms.ALL_TABLES), 1))
    files.append(('multi-oriented', jc.with_app1(ms.write_multiscan(ms.grids_for(size, '420', seed=41), size, '420'), jc.tiff_block(4, False)), 4))
    files.append(('grey', sc.write(ms.grids_for(size, 'grey', seed=42), size, 'grey'), 1))
    order = rng.permutation(len(files))
    return [files[i] for i in order]


@pytest.mark.gpu
def test_shared_calls_and_the_switches_off(reader):
    """One call mixes multi-scan files with baseline, DHT-less, oriented and progressive ones, all switches on: frames and statuses in the
    caller's order, each frame Pillow's.  With the two new switches off the same call gives the multi-scan and DHT-less files status
    1 and zero frames, and every other file the very frame it had."""
    from meterelf_amd import _hip
    size = (37, 51)
    files = _shared_call(size)
    datas = [d for (_k, d, _c) in files]
    reader.set_jpeg_orientation(True)
    reader.set_jpeg_progressive(True)
    reader.set_jpeg_default_tables(True)
    try:
        (on, status) = reader.ctx.jpeg_decode(datas, *size)
        assert (status == 0).all(), [(files[i][0], int(s)) for (i, s) in enumerate(status) if s]
        for ((kind, d, code), got) in zip(files, on):
            ref = jc.reference_frame(d, code) if code != 1 else sc.pillow_bgr(d)
            assert np.array_equal(got, ref), (kind, int((got != ref).sum()))
        reader.set_jpeg_multiscan(False)
        reader.set_jpeg_default_tables(False)
        (off, status) = reader.ctx.jpeg_decode(datas, *size)
        for ((kind, _d, _c), a, b, st) in zip(files, on, off, status):
            if kind.startswith('multi') or kind == 'bare':
                assert st == _hip.JPEG_UNSUPPORTED and not b.any(), (kind, int(st))
            else:
                assert st == 0 and np.array_equal(a, b), (kind, int(st))
    finally:
        reader.set_jpeg_orientation(False)
        reader.set_jpeg_progressive(False)
        reader.set_jpeg_default_tables(False)
        reader.set_jpeg_multiscan(True)


@pytest.mark.gpu
def test_corrupt_scans(reader):
    """A file cut inside its second scan, a restart marker missing from a chroma scan (the next one is then out of sequence), a code
    that does not exist in the third scan: each status 2 and a zero frame, the files on either side byte-equal to Pillow."""
    from meterelf_amd import _hip
    size = (37, 51)
    good = [ms.write_multiscan(ms.grids_for(size, s, seed=60 + k), size, s, restarts=(0, 2, 0)) for (k, s) in enumerate(('420', '422', '444', '420'))]
    whole = good[1]
    spans = ms.scan_offsets(whole)
    assert len(spans) == 3
    cut = whole[:(spans[1][0] + spans[1][1]) // 2]
    (a, b) = spans[1]
    at = whole.index(b'\xff\xd1', a, b)
    missing = whole[:at] + whole[at + 2:]                               # RST1 gone: RST2 follows RST0
    (a, b) = spans[2]
    mid = (a + b) // 2
    nocode = whole[:mid] + b'\xff\x00' * 8 + whole[mid + 16:]             # 64 one-bits: no code of either Annex K table is all ones
    files = [good[0], cut, good[1], missing, good[2], nocode, good[3]]
    (frames, status) = reader.ctx.jpeg_decode(files, *size)
    assert list(status) == [0, _hip.JPEG_CORRUPT, 0, _hip.JPEG_CORRUPT, 0, _hip.JPEG_CORRUPT, 0], status
    for (i, d) in enumerate(files):
        if i % 2:
            assert not frames[i].any(), i
        else:
            assert np.array_equal(frames[i], sc.pillow_bgr(d)), i


def _canvas_files(sampling):
    """A 960 x 1280 canvas with a golden frame at its bottom right, as a multi-scan file and as its interleaved twin (flat tables)."""
    (_paths, frames) = sc.fixture_frames(1)
    (h, w) = frames[0].shape[:2]
    (H, W) = (1280, 960)
    canvas = np.full((H, W, 3), 90, np.uint8)
    canvas[H - h:, W - w:] = frames[0]
    qt = {0: ([sc.FLAT_Q[0]] * 64, False), 1: ([sc.FLAT_Q[1]] * 64, False)}
    grids = sc.image_coefs(canvas, sampling, qt)
    return ((H, W), (W - w, H - h), ms.write_multiscan(grids, (H, W), sampling, qt, order=(2, 0, 1)), sc.write(grids, (H, W), sampling, qt))


@pytest.mark.gpu
@pytest.mark.parametrize('sampling', ['420', '422'])
def test_a_window_beyond_half_the_frame(sampling):
    """The meter_rect moved to the bottom right of a 960 x 1280 canvas: the window's left and top edges lie beyond half the frame, where a
    chroma scan's window (the file's divided by the sampling factors) is no subset of the luma window.  melf_jpeg_process_batch on the
    multi-scan file, on its interleaved twin, and the reader on Pillow's decode of the twin: identical records."""
    from meterelf_amd import MeterReader, _engine, _hip, _params
    params = _params.load(PFILE)
    ((H, W), (dx, dy), multi, twin) = _canvas_files(sampling)
    ((x0, y0), (x1, y1)) = params.meter_rect
    rect = _engine.Rect((x0 + dx, y0 + dy), (x1 + dx, y1 + dy))
    assert ((x0 + dx - 16) & ~15) > W // 2 and ((y0 + dy - 16) & ~15) > H // 2
    r = MeterReader(params, blob=_engine.make_blob(params, rect), jpeg_multiscan=True)
    try:
        ref = r.read_frames(np.stack([sc.pillow_bgr(twin)]))
        assert ref['status'][0] == _hip.FRAME_OK
        (recs, status) = r.ctx.jpeg_process_batch([multi, twin, multi], H, W)
        assert (status == 0).all(), status
        assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes() == ref[0].tobytes()
    finally:
        r.close()


@functools.lru_cache(None)
def _fixture_files(n=8):
    """n golden frames as multi-scan files (4:2:0 and 4:2:2 in turn, the scan orders and restart plans in turn) and their twins."""
    (paths, frames) = sc.fixture_frames(n)
    qt = {0: ([sc.FLAT_Q[0]] * 64, False), 1: ([sc.FLAT_Q[1]] * 64, False)}
    (multi, twins) = ([], [])
    for (k, f) in enumerate(frames):
        sampling = '422' if k % 2 else '420'
        size = f.shape[:2]
        grids = sc.image_coefs(f, sampling, qt)
        multi.append(ms.write_multiscan(grids, size, sampling, qt, order=ms.ORDERS[k % 3], restarts=ms.restart_plan(('none', 'row')[k // 2 % 2], size, sampling)))
        twins.append(sc.write(grids, size, sampling, qt))
    return (frames[0].shape[:2], multi, twins)


@pytest.mark.gpu
def test_whole_path_records_and_values(reader, tmp_path, monkeypatch):
    """Eight golden frames re-coded as multi-scan files through melf_jpeg_process_files, MeterReader.read_jpeg_paths and get_meter_values:
    records and values identical to their interleaved twins'; under METERELF_JPEG_MULTISCAN=host the same values, and the library gives
    the files status 1."""
    import meterelf_amd
    from meterelf_amd import MeterReader, _hip, _image, _params
    ((H, W), multi, twins) = _fixture_files()
    ref = reader.ctx.process_batch(np.stack([sc.pillow_bgr(d) for d in twins]))
    assert (ref['status'] == _hip.FRAME_OK).sum() * 4 >= 3 * len(twins), ref['status']
    (recs, status) = reader.ctx.jpeg_process_batch(twins, H, W)
    assert (status == 0).all() and recs.tobytes() == ref.tobytes()
    (recs, status) = reader.ctx.jpeg_process_batch(multi, H, W)
    assert (status == 0).all() and recs.tobytes() == ref.tobytes()
    (recs, status) = reader.ctx.jpeg_process_batch(multi * 10, H, W)          # 80 files: the chunked path
    assert (status == 0).all() and recs.tobytes() == ref.tobytes() * 10
    paths = []
    for (k, d) in enumerate(multi):
        paths.append(str(tmp_path / ('scans%d.jpg' % k)))
        open(paths[-1], 'wb').write(d)
    (recs, status, hw) = reader.ctx.jpeg_process_files(paths)
    assert hw == (H, W) and (status == 0).all() and recs.tobytes() == ref.tobytes()
    reader.ctx.jpeg_process_files_begin(paths)
    with pytest.raises(Exception):
        reader.ctx.set_jpeg_multiscan(False)                             # not while a _begin call is in flight
    (recs, status, hw) = reader.ctx.jpeg_process_files_end()
    assert (status == 0).all() and recs.tobytes() == ref.tobytes() and reader.ctx.jpeg_multiscan()
    got = reader.read_jpeg_paths(paths)
    assert all(g is not None and g.tobytes() == x.tobytes() for (g, x) in zip(got, ref))
    assert all(g is not None and g.tobytes() == x.tobytes() for (g, x) in zip(reader.read_jpeg_files(multi), ref))
    plain = MeterReader(_params.load(PFILE))
    try:
        (_r, status, _hw) = plain.ctx.jpeg_process_files(paths)
        assert (status == _hip.JPEG_UNSUPPORTED).all()
        assert plain.read_jpeg_paths(paths) == [None] * len(paths)
    finally:
        plain.close()
    calls = []
    real = _image.imread_bgr

    def counting(filename):
        calls.append(filename)
        return real(filename)
    monkeypatch.setattr(_image, 'imread_bgr', counting)
    monkeypatch.setenv('METERELF_CTX_CACHE', '0')
    monkeypatch.setenv('METERELF_JPEG_MULTISCAN', 'host')
    host = list(meterelf_amd.get_meter_values(PFILE, paths))
    assert sorted(calls) == sorted(paths)
    del calls[:]
    monkeypatch.delenv('METERELF_JPEG_MULTISCAN')
    got = list(meterelf_amd.get_meter_values(PFILE, paths))
    assert calls == [] and [g.filename for g in got] == paths
    names = reader.dial_names
    for (g, h, x) in zip(got, host, ref):
        assert g.meter_values == h.meter_values and g.value == h.value and (g.error is None) == (h.error is None)
        if g.error is None:
            assert all(g.meter_values[nm] == float(x['pos'][i]) for (i, nm) in enumerate(names))
    assert sum(g.error is None for g in got) * 4 >= 3 * len(got)


@pytest.mark.gpu
def test_a_call_without_such_files_launches_what_it_launched(reader):
    """melf_ctx_timings of a baseline-only call with the two switches off and on: the same launches of every kernel, the same records."""
    ((H, W), _multi, twins) = _fixture_files()
    ctx = reader.ctx
    seen = []
    ctx.set_profiling(1)
    try:
        for on in (False, True, False):
            reader.set_jpeg_multiscan(on)
            reader.set_jpeg_default_tables(on)
            ctx.timings()
            (recs, status) = ctx.jpeg_process_batch(twins, H, W)
            assert (status == 0).all()
            seen.append(({k: v[1] for (k, v) in ctx.timings().items()}, recs.tobytes()))
    finally:
        ctx.set_profiling(0)
        reader.set_jpeg_multiscan(True)
        reader.set_jpeg_default_tables(False)
    assert seen[0] == seen[1] == seen[2] and sum(seen[0][0].values()) > 0
