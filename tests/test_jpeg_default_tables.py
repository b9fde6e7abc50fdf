"""JPEG files that leave their Huffman tables out (Motion-JPEG frames of UVC webcams and AVI MJPG streams: no DHT segment), decoded on
the GPU with the T.81 Annex K tables as libjpeg-turbo decodes them (melf_ctx_set_jpeg_default_tables, MELF_JPEG_TAKE_DEFAULT_TABLES).

The reference never comes from the GPU: a frame is Pillow's (libjpeg-turbo's) decode of the same bytes.  The files come from
tests/jpeg_writer.py, coded with the Annex K tables and written without some or all of their DHT segments (its layout's `omit`).

CPU part: the four tables the parser installs against the ones an encoder writes (tests/jpeg_std_tables_main.cpp prints the header's,
plain and under the host sanitizers), Pillow's decode with and without the DHT segments, the probe with and without the bit, the
declared exports, the get_meter_values switch.  GPU part: whole frames byte-equal to Pillow, the UVC shape (4:2:2, restart interval, no
DHT), partial definitions, slot 2, the switch off, records through every reading entry point."""
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

from tests import jpeg_sampling_cases as sc  # noqa: E402
from tests import jpeg_scans_cases as ms  # noqa: E402
from tests import jpeg_writer as jw  # noqa: E402

PFILE = os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml')
PARTIAL = [ms.ALL_TABLES, (('dc', 1), ('ac', 1)), (('dc', 0),), (('ac', 1),), (('dc', 0), ('ac', 0))]


@functools.lru_cache(None)
def _grids(size, sampling):
    return tuple(ms.grids_for(size, sampling))


def _bare(size, sampling, omit=ms.ALL_TABLES, **kw):
    return ms.without_tables(list(_grids(size, sampling)), size, sampling, omit=omit, **kw)


def _compiler():
    for cxx in (os.environ.get('CXX'), '/opt/rocm/llvm/bin/clang++', 'g++', 'clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail('no C++ compiler for the stand-alone program')


# ------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize('flags', [[], ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g']], ids=['plain', 'sanitizers'])
def test_the_installed_tables_are_the_ones_an_encoder_writes(tmp_path, flags):
    """meterelf_amd/csrc/melf_jpeg_std_tables.h, printed by a program of its own, against jpeg_writer.standard_tables() (read out of a
    file Pillow writes): counts and symbols of all four tables."""
    exe = str(tmp_path / 'std_tables')
    subprocess.check_call([_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + flags +
                          ['-I', os.path.join(ROOT, 'meterelf_amd', 'csrc'), os.path.join(ROOT, 'tests', 'jpeg_std_tables_main.cpp'), '-o', exe])
    lines = subprocess.check_output([exe]).decode().splitlines()
    std = jw.standard_tables()
    seen = set()
    for line in lines:
        (head, vals) = line.split(' : ')
        (kind, tid, *counts) = head.split()
        spec = std[kind][int(tid)]
        assert [int(v) for v in counts] == list(spec[0][1:17]) and [int(v) for v in vals.split()] == list(spec[1]), (kind, tid)
        seen.add((kind, int(tid)))
    assert seen == {('dc', 0), ('dc', 1), ('ac', 0), ('ac', 1)}


def test_pillow_decodes_a_file_without_its_tables_like_the_file_with_them():
    for sampling in ('420', '422', '444', 'grey'):
        size = (37, 51)
        full = sc.write(list(_grids(size, sampling)), size, sampling)
        for omit in PARTIAL:
            if sampling == 'grey' and any(t == 1 for (_k, t) in omit):
                continue
            bare = _bare(size, sampling, omit)
            assert len(bare) < len(full) and np.array_equal(sc.pillow_bgr(bare), sc.pillow_bgr(full)), (sampling, omit)


def test_exports_and_enum_values():
    import inspect
    import re

    from meterelf_amd import MeterReader, _hip
    assert {'melf_ctx_set_jpeg_default_tables', 'melf_ctx_get_jpeg_default_tables'} <= set(_hip.EXPORTS)
    L = _hip.lib()
    assert L.melf_ctx_set_jpeg_default_tables and L.melf_ctx_get_jpeg_default_tables
    assert _hip.JPEG_TAKE_DEFAULT_TABLES == 16
    header = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    assert re.search(r'MELF_JPEG_TAKE_DEFAULT_TABLES = 16\b', header)
    assert 'int melf_ctx_set_jpeg_default_tables(melf_ctx* ctx, int on);' in header and 'int melf_ctx_get_jpeg_default_tables(melf_ctx* ctx, int* on);' in header
    assert inspect.signature(MeterReader.__init__).parameters['jpeg_default_tables'].default is False
    assert hasattr(MeterReader, 'set_jpeg_default_tables')


def test_probe_refuses_without_the_bit_and_takes_with_it():
    from meterelf_amd import _hip
    size = (37, 51)
    for sampling in ('420', '422', '444', 'grey'):
        for omit in PARTIAL:
            if sampling == 'grey' and any(t == 1 for (_k, t) in omit):
                continue
            data = _bare(size, sampling, omit, restart=3)
            assert _hip.jpeg_probe(data) == (37, 51, False, ms.OLD_TABLE_REASON)
            for flags in (0, 1, 2, 4, 7):
                assert _hip.jpeg_probe_flags(data, flags) == (37, 51, 1, False, ms.OLD_TABLE_REASON), (sampling, omit, flags)
                assert _hip.jpeg_probe_flags(data, flags | ms.TAKE_TABLES) == (37, 51, 1, True, ''), (sampling, omit, flags)
    data = _bare(size, '422')
    (H, W, _o, ok) = _hip.jpeg_probe_flags_batch([data, data], ms.TAKE_TABLES)
    assert list(ok) == [1, 1] and list(H) == [37, 37] and list(W) == [51, 51]
    assert list(_hip.jpeg_probe_flags_batch([data], 7)[3]) == [0]
    with pytest.raises(Exception):
        _hip.jpeg_probe_flags(data, 8)                                  # no such switch
    with pytest.raises(Exception):
        _hip.jpeg_probe_flags(data, 64)


def test_slots_2_and_3_receive_nothing_and_progressive_files_keep_their_answer():
    from meterelf_amd import _hip
    from tests import jpeg_prog_writer as pw
    size = (37, 51)
    grids = list(_grids(size, '420'))
    (dc, ac) = sc.std_tables()
    # luma on DC table 2, which no DHT defines: unsupported with or without the bit (as a file that defines it is: ids above 1)
    data = jw.write_jpeg(grids, size, '420', sc.QT, {2: dc[0], 1: dc[1]}, {0: ac[0], 1: ac[1]}, sel=[(0, 2, 0), (1, 1, 1), (1, 1, 1)],
                         layout=dict(sof=0xC1, omit=(('dc', 2),)))
    for flags in (0, ms.TAKE_TABLES):
        (_h, _w, _o, ok, why) = _hip.jpeg_probe_flags(data, flags)
        assert not ok and why, (flags, why)
    prog = pw.write_progressive(grids, size, '420', sc.QT, pw.PILLOW_COLOUR)
    assert _hip.jpeg_probe_flags(prog, ms.TAKE_PROG)[3] is True
    cut = bytearray()
    i = 2
    while prog[i + 1] != 0xDA:                                           # the same file without the DHT segments in front of its first scan
        L = (prog[i + 2] << 8) | prog[i + 3]
        if prog[i + 1] != 0xC4:
            cut += prog[i:i + 2 + L]
        i += 2 + L
    bare = prog[:2] + bytes(cut) + prog[i:]
    assert _hip.jpeg_probe_flags(bare, ms.TAKE_PROG) == _hip.jpeg_probe_flags(bare, ms.TAKE_PROG | ms.TAKE_TABLES)
    assert _hip.jpeg_probe_flags(bare, ms.TAKE_PROG | ms.TAKE_TABLES)[3] is False


def test_the_bit_alone_changes_no_other_answer():
    from meterelf_amd import _hip
    from tests.test_jpeg_streams import _refusal_cases
    seen = 0
    for c in _refusal_cases():
        for flags in (0, 1, 2, 4, 7):
            (a, b) = (_hip.jpeg_probe_flags(c.data, flags | ms.TAKE_TABLES), _hip.jpeg_probe_flags(c.data, flags))
            assert a == b or b[4] == ms.OLD_TABLE_REASON, (c.name, flags, a, b)
        seen += 1
    assert seen >= 8
    for s in ('420', '422', '444', 'grey'):
        full = sc.write(list(_grids((24, 40), s)), (24, 40), s)
        assert _hip.jpeg_probe_flags(full, ms.TAKE_TABLES) == _hip.jpeg_probe_flags(full, 0) == (24, 40, 1, True, '')


def test_get_meter_values_asks_for_the_switch_unless_the_host_is_asked_for(monkeypatch):
    from meterelf_amd import _api, _engine, _params

    class Reader:
        jpeg_default_tables = False

        def set_jpeg_default_tables(self, on):
            self.jpeg_default_tables = bool(on)
    monkeypatch.delenv('METERELF_JPEG_TABLES', raising=False)
    assert _api._jpeg_on_gpu('jpeg_default_tables') and _api._with_jpeg_orientation(Reader()).jpeg_default_tables
    params = _params.load(PFILE)
    blob = _engine.make_blob(params)
    k_gpu = _api._reader_key(params, blob, 0)
    monkeypatch.setenv('METERELF_JPEG_TABLES', 'host')
    assert not _api._jpeg_on_gpu('jpeg_default_tables') and not _api._with_jpeg_orientation(Reader()).jpeg_default_tables
    assert _api._reader_key(params, blob, 0) != k_gpu                  # a reader made under one setting is never handed out under the other
    monkeypatch.setenv('METERELF_JPEG_TABLES', 'gpu')
    assert _api._reader_key(params, blob, 0) == k_gpu


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope='module')
def reader():
    from meterelf_amd import _hip
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    r = MeterReader(_params.load(PFILE), jpeg_default_tables=True)
    assert r.ctx.jpeg_default_tables() and r.jpeg_default_tables and not r.ctx.jpeg_samplings() and not r.ctx.jpeg_progressive()
    yield r
    r.close()


def _assert_equal_to_pillow(ctx, files):
    by_size = {}
    for (name, data, size) in files:
        by_size.setdefault(size, []).append((name, data))
    for ((H, W), group) in by_size.items():
        (frames, status) = ctx.jpeg_decode([d for (_n, d) in group], H, W)
        for ((name, data), got, st) in zip(group, frames, status):
            ref = sc.pillow_bgr(data)
            assert st == 0, (name, int(st))
            assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:3])


@pytest.mark.gpu
def test_frames_without_tables_equal_pillow(reader):
    """The UVC shape -- 4:2:2, a restart interval, no DHT at all -- and every sampling at sizes that cut the MCU, with and without
    restart intervals (both Huffman kernels); a file that defines only DC 0 and AC 0; and the other partial definitions."""
    files = []
    for size in ((37, 51), (16, 16), (70, 19)):
        for sampling in ('422', '420', '444', 'grey'):
            for restart in (0, 2):
                files.append(('%s-%d-bare-%dx%d' % (sampling, restart, *size), _bare(size, sampling, restart=restart), size))
    size = (33, 130)
    files.append(('uvc', _bare(size, '422', restart=jw.grid_shape(size, '422')[0][1]), size))
    files.append(('only-dc0-ac0', _bare(size, '420', (('dc', 1), ('ac', 1))), size))
    for omit in PARTIAL[2:]:
        files.append(('partial-%s' % (omit,), _bare(size, '420', omit, restart=5), size))
    assert all(b'\xff\xc4' not in d for (n, d, _s) in files if 'bare' in n or n == 'uvc')
    _assert_equal_to_pillow(reader.ctx, files)


@pytest.mark.gpu
def test_the_switch_off_gives_status_1_and_slot_2_stays_unsupported(reader):
    from meterelf_amd import _hip
    size = (37, 51)
    bare = _bare(size, '422', restart=3)
    full = sc.write(list(_grids(size, '422')), size, '422', restart=3)
    (dc, ac) = sc.std_tables()
    slot2 = jw.write_jpeg(list(_grids(size, '422')), size, '422', sc.QT, {2: dc[0], 1: dc[1]}, {0: ac[0], 1: ac[1]},
                          sel=[(0, 2, 0), (1, 1, 1), (1, 1, 1)], layout=dict(sof=0xC1, omit=(('dc', 2),)))
    (frames, status) = reader.ctx.jpeg_decode([full, slot2, bare], *size)
    assert list(status) == [0, _hip.JPEG_UNSUPPORTED, 0] and not frames[1].any()
    assert np.array_equal(frames[0], frames[2]) and np.array_equal(frames[2], sc.pillow_bgr(bare))
    reader.set_jpeg_default_tables(False)
    try:
        assert not reader.ctx.jpeg_default_tables()
        (off, status) = reader.ctx.jpeg_decode([full, slot2, bare], *size)
        assert list(status) == [0, _hip.JPEG_UNSUPPORTED, _hip.JPEG_UNSUPPORTED] and not off[2].any()
        assert np.array_equal(off[0], frames[0])
    finally:
        reader.set_jpeg_default_tables(True)


@functools.lru_cache(None)
def _fixture_files(n=8):
    """n golden frames as writer files with their tables (the twins) and the same bytes without the DHT segments."""
    (paths, frames) = sc.fixture_frames(n)
    twins = [sc.reencode(f, '422' if k % 2 else '420') for (k, f) in enumerate(frames)]
    bare = []
    for d in twins:
        segs = ms.segments(d)
        bare.append(d[:2] + b''.join(d[a:b] for (m, a, b) in segs if m != 0xC4) + d[segs[-1][2]:])
    assert all(b'\xff\xc4' not in b[:ms.segments(b)[-1][2]] for b in bare)
    return (paths, frames[0].shape[:2], twins, bare)


@pytest.mark.gpu
def test_whole_path_records_and_values(reader, tmp_path, monkeypatch):
    """Eight golden frames without their DHT segments through melf_jpeg_process_files, MeterReader.read_jpeg_paths and get_meter_values:
    the records and values of their twins with tables; under METERELF_JPEG_TABLES=host the same values, from the host branch."""
    import meterelf_amd
    from meterelf_amd import MeterReader, _hip, _image, _params
    (_golden, (H, W), twins, bare) = _fixture_files()
    ref = reader.ctx.process_batch(np.stack([sc.pillow_bgr(d) for d in twins]))
    assert (ref['status'] == _hip.FRAME_OK).sum() * 4 >= 3 * len(twins), ref['status']
    (recs, status) = reader.ctx.jpeg_process_batch(bare, H, W)
    assert (status == 0).all() and recs.tobytes() == ref.tobytes()
    paths = []
    for (k, d) in enumerate(bare):
        paths.append(str(tmp_path / ('bare%d.jpg' % k)))
        open(paths[-1], 'wb').write(d)
    (recs, status, hw) = reader.ctx.jpeg_process_files(paths)
    assert hw == (H, W) and (status == 0).all() and recs.tobytes() == ref.tobytes()
    got = reader.read_jpeg_paths(paths)
    assert all(g is not None and g.tobytes() == x.tobytes() for (g, x) in zip(got, ref))
    assert all(g is not None and g.tobytes() == x.tobytes() for (g, x) in zip(reader.read_jpeg_files(bare), ref))
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
    monkeypatch.setenv('METERELF_JPEG_TABLES', 'host')
    host = list(meterelf_amd.get_meter_values(PFILE, paths))
    assert sorted(calls) == sorted(paths)
    del calls[:]
    monkeypatch.delenv('METERELF_JPEG_TABLES')
    got = list(meterelf_amd.get_meter_values(PFILE, paths))
    assert calls == [] and [g.filename for g in got] == paths
    names = reader.dial_names
    for (g, h, x) in zip(got, host, ref):
        assert g.meter_values == h.meter_values and g.value == h.value and (g.error is None) == (h.error is None)
        if g.error is None:
            assert all(g.meter_values[nm] == float(x['pos'][i]) for (i, nm) in enumerate(names))
    assert sum(g.error is None for g in got) * 4 >= 3 * len(got)
