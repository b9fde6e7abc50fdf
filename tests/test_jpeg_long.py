"""Baseline JPEG files without restart markers whose scan is longer than k_jpeg_huff addresses, decoded on the GPU chapter by chapter
(melf_ctx_set_jpeg_long_scans).

The reference never comes from the GPU: a frame is Pillow's (libjpeg-turbo's) decode of the same bytes, a record is the reader's on that
frame.  Bar: every byte of every frame and of every record, no tolerance.

CPU part: the chapter plan swept on the host (tests/jpeg_long_main.cpp, plain and under the host sanitizers, as an ordinary program),
the exports, the switch's row in get_meter_values' table and the reader-cache key.  GPU part: small files through 1 to 35 chapters at
three chapter lengths; the meter_rect window ending in the first, a middle and the last chapter; the real sizes (4.9 MB and 10.5 MB)
at the production length, which a context without the switch refuses; calls shared with every other kind of file; damaged long
files; the file-name entry points and get_meter_values; the switch's round trips."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_long_cases as lc  # noqa: E402
from tests import jpeg_orient_cases as jc  # noqa: E402
from tests import jpeg_sampling_cases as sc  # noqa: E402
from tests import jpeg_scans_cases as ms  # noqa: E402

PFILE = os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml')
CHAPTER_WANTS = (1, 100000, 200000)     # the rule's minimum (36 864 bytes) and two larger lengths (102 400 and 200 704)


# ------------------------------------------------------------------ CPU ----
def _compiler():
    for cxx in (os.environ.get('CXX'), '/opt/rocm/llvm/bin/clang++', 'g++', 'clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail('no C++ compiler for the stand-alone program')


@pytest.mark.parametrize('flags', [[], ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g']], ids=['plain', 'sanitizers'])
def test_the_chapter_plan_swept_on_the_host(tmp_path, flags):
    """tests/jpeg_long_main.cpp: segment lengths, chapters, segment ends and the 32-bit bound of meterelf_amd/csrc/melf_jpeg_long.h over
    scan lengths from 1 byte to the bound and chapter lengths from 1 byte up, as an ordinary program."""
    exe = str(tmp_path / 'jpeg_long_main')
    subprocess.check_call([_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + flags +
                          ['-I', os.path.join(ROOT, 'meterelf_amd', 'csrc'), os.path.join(ROOT, 'tests', 'jpeg_long_main.cpp'), '-o', exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    (word, count) = out.stdout.decode().split()
    assert word == 'ok' and int(count) > 500000


def test_the_restated_plan_is_the_headers():
    """tests/jpeg_long_cases.py restates the header's constants; the issue's figures follow from them."""
    import re
    text = open(os.path.join(ROOT, 'meterelf_amd', 'csrc', 'melf_jpeg_long.h')).read()
    assert re.search(r'constexpr uint32_t T = %d;' % lc.T, text)
    assert re.search(r'MIN_SEG_DWORDS = %d;' % lc.MIN_DWORDS, text) and re.search(r'MAX_SEG_DWORDS = %d;' % lc.MAX_DWORDS, text)
    assert 'MAX_SCAN_BYTES == 532774904ull' in text
    assert (lc.PRODUCTION, lc.MIN_CHAPTER) == (4091904, 36864)
    assert [lc.chapter_bytes(k) for k in CHAPTER_WANTS] == [36864, 102400, 200704]
    assert lc.chapter_bytes(36865) == 45056 and lc.chapter_bytes(10 ** 9) == lc.PRODUCTION
    assert -(-4929102 // lc.PRODUCTION) == 2 and -(-10523739 // lc.PRODUCTION) == 3   # the two real sizes of the GPU test


def test_exports_header_and_python_surface():
    import inspect

    from meterelf_amd import MeterReader, _hip
    assert {'melf_ctx_set_jpeg_long_scans', 'melf_ctx_get_jpeg_long_scans'} <= set(_hip.EXPORTS)
    L = _hip.lib()
    assert L.melf_ctx_set_jpeg_long_scans and L.melf_ctx_get_jpeg_long_scans
    header = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    assert 'int melf_ctx_set_jpeg_long_scans(melf_ctx* ctx, int on, int chapter_bytes);' in header
    assert 'int melf_ctx_get_jpeg_long_scans(melf_ctx* ctx, int* on, int* chapter_bytes);' in header
    assert inspect.signature(MeterReader.__init__).parameters['jpeg_long_scans'].default is False
    assert inspect.signature(MeterReader.set_jpeg_long_scans).parameters['chapter_bytes'].default == 0
    assert inspect.signature(_hip.Context.set_jpeg_long_scans).parameters['chapter_bytes'].default == 0
    assert ('jpeg_long_scans', None) in [(n, f) for (n, f, _d) in _hip.JPEG_SWITCHES]     # no probe flag
    # a NULL context is refused by both calls, without a GPU
    import ctypes as C
    (on, k) = (C.c_int(0), C.c_int(0))
    assert L.melf_ctx_set_jpeg_long_scans(None, 1, 0) != 0
    assert L.melf_ctx_get_jpeg_long_scans(None, C.byref(on), C.byref(k)) != 0


def test_the_new_kernel_has_no_scratch():
    """tools/kernel_meta.py on the built library: the chapter kernel exists once, for 1024 lanes, and keeps no private segment."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = {n: d for (n, d) in kernel_meta.kernel_metadata().items() if 'k_jpeg_chapters' in n}
    assert len(meta) == 1
    (d,) = meta.values()
    assert d.get('private_segment_fixed_size', 0) == 0 and d.get('max_flat_workgroup_size') == 1024 and d.get('wavefront_size', 64) == 64


def test_get_meter_values_row_key_and_default(monkeypatch):
    """JPEG_SWITCH_ENV has the row; METERELF_JPEG_LONG: 'gpu' or 'host', the committed default otherwise; the setting is part of the
    reader-cache key."""
    from meterelf_amd import _api, _engine, _params

    class Reader:
        jpeg_long_scans = False

        def set_jpeg_long_scans(self, on, chapter_bytes=0):
            self.jpeg_long_scans = bool(on)
    rows = [r for r in _api.JPEG_SWITCH_ENV if r[0] == 'jpeg_long_scans']
    assert len(rows) == 1 and rows[0][1] == 'METERELF_JPEG_LONG' and rows[0][2] in ('gpu', 'host') and rows[0][3] == b'long'
    assert len(_api.JPEG_SWITCH_ENV) == 7 and len({r[3] for r in _api.JPEG_SWITCH_ENV}) == 7
    default_on = rows[0][2] == 'gpu'
    monkeypatch.delenv('METERELF_JPEG_LONG', raising=False)
    params = _params.load(PFILE)
    blob = _engine.make_blob(params)
    k_default = _api._reader_key(params, blob, 0)
    assert _api._jpeg_on_gpu('jpeg_long_scans') == default_on
    assert _api._with_jpeg_orientation(Reader()).jpeg_long_scans == default_on
    monkeypatch.setenv('METERELF_JPEG_LONG', 'host')
    assert not _api._jpeg_on_gpu('jpeg_long_scans') and not _api._with_jpeg_orientation(Reader()).jpeg_long_scans
    k_host = _api._reader_key(params, blob, 0)
    monkeypatch.setenv('METERELF_JPEG_LONG', 'gpu')
    assert _api._jpeg_on_gpu('jpeg_long_scans') and _api._with_jpeg_orientation(Reader()).jpeg_long_scans
    k_gpu = _api._reader_key(params, blob, 0)
    assert k_gpu != k_host and k_default == (k_gpu if default_on else k_host)


def test_the_default_is_the_one_the_rate_file_dictates():
    """profiles/jpeg_long/jpeg_long_rate.txt, the row of ONE long file in a 256-file call: the default is 'gpu' exactly if that row is
    faster on the GPU than through the host branch."""
    import re

    from meterelf_amd import _api
    text = open(os.path.join(ROOT, 'profiles', 'jpeg_long', 'jpeg_long_rate.txt')).read()
    m = re.search(r'^\s*1 long file of 256\s*:\s*gpu\s+([0-9.]+) ms\s+host branch\s+([0-9.]+) ms', text, re.M)
    assert m, 'no 1-file row'
    default = next(r[2] for r in _api.JPEG_SWITCH_ENV if r[0] == 'jpeg_long_scans')
    assert default == ('gpu' if float(m.group(1)) < float(m.group(2)) else 'host')


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope='module')
def reader():
    from meterelf_amd import _hip
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    r = MeterReader(_params.load(PFILE), jpeg_long_scans=True, jpeg_samplings=True)
    assert r.ctx.jpeg_long_scans() and r.jpeg_long_scans and r.ctx.jpeg_long_chapter_bytes() == lc.PRODUCTION
    yield r
    r.close()


_refs = {}


def _ref(data):
    """Pillow's frame of a file, decoded once per module."""
    key = id(data)
    if key not in _refs:
        _refs[key] = (data, lc.pillow_bgr(data))
    return _refs[key][1]


def _decode_and_compare(ctx, named, shape):
    (frames, status) = ctx.jpeg_decode([d for (_n, d) in named], *shape)
    assert (status == 0).all(), [(n, int(s)) for ((n, _d), s) in zip(named, status) if s != 0][:5]
    for ((name, data), got) in zip(named, frames):
        ref = _ref(data)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:3])


@pytest.mark.gpu
@pytest.mark.parametrize('want', CHAPTER_WANTS)
def test_small_files_through_many_chapters(reader, want):
    """Whole-frame decodes of noise and natural images of three shapes in every sampling (4:4:0 and 4:1:1 included), qualities 75 to 100,
    optimised tables and not, with chapters of `want` bytes: the files span 2, 3 and at least 6 chapters, files below the chapter length
    share the calls (the ordinary kernel's), and three steered files sit at the plan's edges -- barely longer than one chapter, at most
    one segment short of two whole chapters, and one chapter only (longer than the chapter in the file, not without its stuffing)."""
    reader.set_jpeg_long_scans(True, want)
    try:
        k = reader.ctx.jpeg_long_chapter_bytes()
        assert k == lc.chapter_bytes(want) and reader.ctx.jpeg_long_scans()
        counts = []
        below = 0
        for shape in lc.SHAPES:
            named = list(lc.pool(shape))
            if shape == (251, 333):
                named += [('dense-' + s, sc.dense_file(shape, s)[0]) for s in sc.LAYOUTS]
            for (_name, d) in named:
                if lc.scan_lengths(d)[0] > k:
                    counts.append(lc.chapters(d, k))
                else:
                    below += 1
            _decode_and_compare(reader.ctx, named, shape)
        assert {2, 3} <= set(counts) and max(counts) >= 6 and below >= 1, (sorted(counts), below)
        seg = k // lc.T                                                      # bytes of a segment
        for (what, lo, hi, nchap) in (('barely longer than one chapter', k, k + seg, 2), ('a segment short of two chapters', 2 * k - seg, 2 * k, 2),
                                      ('one chapter only', k - 60, k, 1)):
            (data, shape) = lc.steered_file(lo, hi)
            (raw, clean) = lc.scan_lengths(data)
            assert raw > k and lo < clean <= hi and lc.chapters(data, k) == nchap, (what, raw, clean, k)
            small = lc.encode(lc.natural(np.random.default_rng(5), *shape)[..., 1], quality=60)
            assert lc.scan_lengths(small)[0] <= k
            _decode_and_compare(reader.ctx, [('small', small), (what, data), ('small again', small)], shape)
    finally:
        reader.set_jpeg_long_scans(True, 0)


def _window_files(n=4):
    """n golden frames re-encoded by Pillow at quality 100, 4:4:4, and for each the clean offset at which the meter_rect window's last
    MCU row ends, measured on a twin with a restart marker behind every MCU row: (frame size, files, [(lo, hi)] bounds of that offset).
    The twin's rows are the file's rows plus the bits that pad each row to a byte and the DC differences against a reset predictor:
    at most 4 bytes a row more or less."""
    import re

    from meterelf_amd import _params
    (_paths, frames) = sc.fixture_frames(n)
    (H, W) = frames[0].shape[:2]
    ((_x0, _y0), (_x1, y1)) = _params.load(PFILE).meter_rect
    rows = -(-min(H, (y1 + 16 + 15) & ~15) // 8)                            # melf_jpeg_orient_addr.h: window(); MCUs of 8 x 8
    assert 0 < rows < -(-H // 8)
    (files, ends) = ([], [])
    for f in frames:
        files.append(lc.encode(f, quality=100, subsampling='4:4:4'))
        twin = lc.encode(f, quality=100, subsampling='4:4:4', restart_marker_rows=1)
        parts = re.split(b'\xff[\xd0-\xd7]', twin[lc.scan_begin(twin):-2])
        assert len(parts) == -(-H // 8)
        e = sum(len(p.replace(b'\xff\x00', b'\xff')) for p in parts[:rows])
        ends.append((e - 4 * rows, e + 4 * rows))
    return ((H, W), files, ends)


@pytest.mark.gpu
def test_the_window_ends_in_the_first_a_middle_and_the_last_chapter(reader):
    """melf_jpeg_process_batch on golden frames at quality 100, 4:4:4 (133 to 142 KB of scan, the window's last MCU row ending near
    110 KB): chapters of 118 784 bytes leave that row in the first of two chapters, 61 440 in the middle one of three, 77 824 in the
    last of two -- asserted from the scan lengths and the window.  The records are those of the ordinary kernel on the same files and
    those of the reader on Pillow's frames."""
    ((H, W), files, ends) = _window_files()
    ref = reader.read_frames(np.stack([_ref(d) for d in files]))
    (recs, status) = reader.ctx.jpeg_process_batch(files, H, W)              # production: these files are the ordinary kernel's
    assert all(lc.scan_lengths(d)[0] <= lc.MAX_PAR_SCAN for d in files)
    assert (status == 0).all() and recs.tobytes() == ref.tobytes()
    try:
        for (want, where) in ((118784, 'first'), (61440, 'middle'), (77824, 'last'), (1, None)):
            reader.set_jpeg_long_scans(True, want)
            k = reader.ctx.jpeg_long_chapter_bytes()
            assert k == max(want, lc.MIN_CHAPTER)
            for (d, (lo, hi)) in zip(files, ends):
                nchap = lc.chapters(d, k)
                assert lc.scan_lengths(d)[0] > k and nchap >= 2
                c = lo // k
                if where is not None:
                    assert lo // k == hi // k                                 # the chapter that holds the row's end is certain
                    assert where == ('first' if c == 0 else 'last' if c == nchap - 1 else 'middle'), (want, c, nchap)
            (recs, status) = reader.ctx.jpeg_process_batch(files, H, W)
            assert (status == 0).all() and recs.tobytes() == ref.tobytes(), want
            got = reader.read_jpeg_files(files)
            assert all(g is not None and g.tobytes() == x.tobytes() for (g, x) in zip(got, ref)), want
    finally:
        reader.set_jpeg_long_scans(True, 0)


def _real_list(shape):
    """A noise file of the shape at quality 100, 4:4:4, between two small files of its size."""
    (H, W) = shape
    rng = np.random.default_rng(77)
    noise = lc.encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=100, subsampling='4:4:4')
    small = lc.encode(lc.natural(rng, H, W), quality=60, subsampling='4:4:4')
    return [small, noise, small]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,nchap', [((1000, 1200), 2), ((1500, 1700), 3)], ids=['4.9MB', '10.5MB'])
def test_real_sizes(reader, shape, nchap):
    """Scans of 4.9 and 10.5 MB at the production chapter length: two and three chapters, status 0 and Pillow's frame with the switch on;
    a context without the switch, and this context with the switch turned off again, answer [0, 1, 0] as before."""
    from meterelf_amd import MeterReader, _hip, _params
    files = _real_list(shape)
    (raw, clean) = lc.scan_lengths(files[1])
    assert raw > lc.MAX_PAR_SCAN and -(-clean // lc.PRODUCTION) == nchap, (raw, clean)
    assert reader.ctx.jpeg_long_chapter_bytes() == lc.PRODUCTION
    (frames, status) = reader.ctx.jpeg_decode(files, *shape)
    assert list(status) == [0, 0, 0], status
    ref = lc.pillow_bgr(files[1])
    assert np.array_equal(frames[1], ref), (int((frames[1] != ref).sum()), np.argwhere(frames[1] != ref)[:3])
    small = lc.pillow_bgr(files[0])
    assert np.array_equal(frames[0], small) and np.array_equal(frames[2], small)
    reader.set_jpeg_long_scans(False)
    try:
        assert not reader.ctx.jpeg_long_scans() and not reader.jpeg_long_scans
        (off, status) = reader.ctx.jpeg_decode(files, *shape)
        assert list(status) == [_hip.JPEG_OK, _hip.JPEG_UNSUPPORTED, _hip.JPEG_OK], status
        assert np.array_equal(off[0], small) and np.array_equal(off[2], small) and not off[1].any()
    finally:
        reader.set_jpeg_long_scans(True, 0)
    if nchap == 2:
        plain = MeterReader(_params.load(PFILE))
        try:
            assert not plain.ctx.jpeg_long_scans()
            (_f, status) = plain.ctx.jpeg_decode(files, *shape)
            assert list(status) == [_hip.JPEG_OK, _hip.JPEG_UNSUPPORTED, _hip.JPEG_OK], status
        finally:
            plain.close()


@pytest.mark.gpu
def test_mixed_call(reader):
    """One whole-frame call and one melf_jpeg_process_batch call with chapters of the minimum length, on golden frames: ordinary camera
    files, a file with restart intervals, long files (quality 100), a long file stored under EXIF orientation 6, a multi-scan file.
    Statuses in the caller's order; every frame Pillow's and the frame of the file decoded alone; every record the reader's on Pillow's
    frame and the record of the file read alone."""
    (paths, frames) = sc.fixture_frames(4)
    size = frames[0].shape[:2]
    qt = {0: ([sc.FLAT_Q[0]] * 64, False), 1: ([sc.FLAT_Q[1]] * 64, False)}
    files = [('ordinary', open(paths[0], 'rb').read(), 1),
             ('long', lc.encode(frames[1], quality=100, subsampling='4:4:4'), 1),
             ('restarts', lc.encode(frames[2], quality=90, subsampling='4:2:2', restart_marker_rows=1), 1),
             ('long-turned', jc.stored_under(frames[3], 6, quality=100, subsampling='4:4:4'), 6),
             ('multiscan', ms.write_multiscan(sc.image_coefs(frames[0], '420', qt), size, '420', qt), 1),
             ('long-422', lc.encode(frames[2], quality=100, subsampling='4:2:2'), 1),
             ('ordinary', open(paths[3], 'rb').read(), 1)]
    reader.set_jpeg_long_scans(True, 1)
    reader.set_jpeg_orientation(True)
    reader.set_jpeg_multiscan(True)
    try:
        k = reader.ctx.jpeg_long_chapter_bytes()
        assert k == lc.MIN_CHAPTER
        for (kind, d, _c) in files:
            if kind.startswith('long'):
                assert lc.scan_lengths(d)[0] > k and lc.chapters(d, k) >= 2, kind
            elif kind == 'ordinary':
                assert lc.scan_lengths(d)[0] <= k, kind
        assert b'\xff\xdd' in files[2][1]
        datas = [d for (_k, d, _c) in files]
        refs = [jc.reference_frame(d, code) if code != 1 else lc.pillow_bgr(d) for (_k, d, code) in files]
        (got, status) = reader.ctx.jpeg_decode(datas, *size)
        assert (status == 0).all(), [(files[i][0], int(s)) for (i, s) in enumerate(status) if s]
        (recs, rstatus) = reader.ctx.jpeg_process_batch(datas, *size)
        assert (rstatus == 0).all(), rstatus
        host = reader.read_frames(np.stack(refs))
        assert recs.tobytes() == host.tobytes()
        viafiles = reader.read_jpeg_files(datas)
        assert all(g is not None and g.tobytes() == x.tobytes() for (g, x) in zip(viafiles, host))
        for (i, (kind, d, _code)) in enumerate(files):
            assert np.array_equal(got[i], refs[i]), (kind, int((got[i] != refs[i]).sum()))
            (alone, st) = reader.ctx.jpeg_decode([d], *size)
            assert st[0] == 0 and np.array_equal(alone[0], got[i]), kind
            (rec1, st) = reader.ctx.jpeg_process_batch([d], *size)
            assert st[0] == 0 and rec1[0].tobytes() == recs[i].tobytes(), kind
    finally:
        reader.set_jpeg_orientation(False)
        reader.set_jpeg_multiscan(False)
        reader.set_jpeg_long_scans(True, 0)


@pytest.mark.gpu
def test_damaged_long_files_are_never_decoded_wrong(reader):
    """A long file of ten chapters of the minimum length, damaged in turn: a code that does not exist in chapter 0 and in chapter 4,
    3000 bytes removed from the end of the data (they run out in the last chapter), the last byte in front of EOI dropped.  The first
    three are MELF_JPEG_CORRUPT with a zero frame -- the cut one with melf_ctx_set_jpeg_truncated on as well --; the last is either
    refused or the frame Pillow decodes from the truncated file.  The files on either side stay exact.  Through the window-limited
    call a damaged chapter in front of the window is corrupt too."""
    from meterelf_amd import _hip
    size = (251, 333)
    good = dict(lc.pool(size))['noise-4:4:4-q100']
    reader.set_jpeg_long_scans(True, 1)
    try:
        k = reader.ctx.jpeg_long_chapter_bytes()
        b = lc.scan_begin(good)
        nchap = lc.chapters(good, k)
        assert k == lc.MIN_CHAPTER and nchap >= 8
        nocode = b'\xff\x00' * 8                                             # 64 one-bits: no Huffman code is all ones
        at0 = b + k // 2
        at4 = b + 4 * k + k // 2 + 4 * k // 200                               # (about one byte in 256 is a stuffed zero)
        assert 4 * k < len(good[b:at4].replace(b'\xff\x00', b'\xff')) < 5 * k - 64   # inside chapter 4, by clean bytes
        first = good[:at0] + nocode + good[at0 + 16:]
        middle = good[:at4] + nocode + good[at4 + 16:]
        cut = good[:-3002] + good[-2:]
        assert lc.scan_lengths(cut)[1] > (nchap - 1) * k                      # the data end inside the last chapter
        nibbled = good[:-3] + good[-2:]
        files = [good, first, good, middle, good, cut, good, nibbled]
        for truncated in (False, True):
            reader.set_jpeg_truncated(truncated)
            (frames, status) = reader.ctx.jpeg_decode(files, *size)
            assert list(status[:7]) == [0, _hip.JPEG_CORRUPT, 0, _hip.JPEG_CORRUPT, 0, _hip.JPEG_CORRUPT, 0], (truncated, status)
            for i in (1, 3, 5):
                assert not frames[i].any(), i
            for i in (0, 2, 4, 6):
                assert np.array_equal(frames[i], _ref(good)), i
            assert status[7] != 0 or np.array_equal(frames[7], lc.pillow_bgr(nibbled, truncated=True))
            assert status[7] == 0 or not frames[7].any()
    finally:
        reader.set_jpeg_truncated(False)
        reader.set_jpeg_long_scans(True, 0)
    # the window-limited decode: chapters of 61 440 bytes, the window's last row in chapter 1 of 3, the damage in chapter 0 and in front
    # of the window's first MCU row (row 18 of 80)
    ((H, W), wfiles, _ends) = _window_files(2)
    d = wfiles[1]
    at = lc.scan_begin(d) + 4000
    hurt = d[:at] + nocode + d[at + 16:]
    reader.set_jpeg_long_scans(True, 61440)
    try:
        (recs, status) = reader.ctx.jpeg_process_batch([wfiles[0], hurt, wfiles[0]], H, W)
        assert list(status) == [0, _hip.JPEG_CORRUPT, 0] and recs[0].tobytes() == recs[2].tobytes()
    finally:
        reader.set_jpeg_long_scans(True, 0)


@pytest.mark.gpu
def test_file_names_and_get_meter_values(reader, tmp_path, monkeypatch):
    """The 4.9 MB file and golden files by name: MeterReader.read_jpeg_paths reads them all on the GPU; get_meter_values gives the same
    values under METERELF_JPEG_LONG=gpu (no host decode) and =host (the long file through the host branch).  A pipelined
    melf_jpeg_process_batch call under MELF_JPEG_CHUNK gives the records of the one-piece calls."""
    import meterelf_amd
    from meterelf_amd import _image
    big = _real_list((1000, 1200))[1]
    golden = sc.golden_files()[2:6]
    paths = [str(tmp_path / 'long.jpg')] + golden[:2] + [str(tmp_path / 'long2.jpg')] + golden[2:]
    for p in (paths[0], paths[3]):
        open(p, 'wb').write(big)
    got = reader.read_jpeg_paths(paths)
    assert all(g is not None for g in got)
    host = reader.read_frames(np.stack([lc.pillow_bgr(big)]))
    assert got[0].tobytes() == got[3].tobytes() == host[0].tobytes()
    (recs, status, hw) = reader.ctx.jpeg_process_files([paths[0], paths[3]])
    assert hw == (1000, 1200) and (status == 0).all() and recs[0].tobytes() == host[0].tobytes()
    calls = []
    real = _image.imread_bgr

    def counting(filename):
        calls.append(filename)
        return real(filename)
    monkeypatch.setattr(_image, 'imread_bgr', counting)
    monkeypatch.setenv('METERELF_CTX_CACHE', '0')
    monkeypatch.setenv('METERELF_JPEG_LONG', 'host')
    via_host = list(meterelf_amd.get_meter_values(PFILE, paths))
    assert sorted(calls) == sorted([paths[0], paths[3]])
    del calls[:]
    monkeypatch.setenv('METERELF_JPEG_LONG', 'gpu')
    via_gpu = list(meterelf_amd.get_meter_values(PFILE, paths))
    assert calls == [] and [g.filename for g in via_gpu] == paths
    for (g, h) in zip(via_gpu, via_host):
        assert g.meter_values == h.meter_values and g.value == h.value and (g.error is None) == (h.error is None)
    assert sum(g.error is None for g in via_gpu) >= 3
    # pipelined: 100 files, long ones (three chapters of 61 440 bytes) and ordinary ones in turn
    ((H, W), wfiles, _ends) = _window_files()
    ordinary = [open(f, 'rb').read() for f in sc.fixture_frames(4)[0]]
    files = [(wfiles if i % 3 else ordinary)[i % 4] for i in range(100)]
    reader.set_jpeg_long_scans(True, 61440)
    try:
        (ref, rstat) = ([], [])
        for i in range(0, len(files), 50):
            (r, s) = reader.ctx.jpeg_process_batch(files[i:i + 50], H, W)
            ref.append(r)
            rstat.append(s)
        (ref, rstat) = (np.concatenate(ref), np.concatenate(rstat))
        assert (rstat == 0).all()
        monkeypatch.setenv('MELF_JPEG_CHUNK', '40')
        (recs, status) = reader.ctx.jpeg_process_batch(files, H, W)
        assert (status == 0).all() and recs.tobytes() == ref.tobytes()
    finally:
        reader.set_jpeg_long_scans(True, 0)


@pytest.mark.gpu
def test_switch_hygiene(reader):
    """Setter and getter round trips with the rounded chapter length; bad arguments; not while a _begin call is in flight; a call without
    a long file launches what it launched with the switch off."""
    from meterelf_amd import _hip
    ctx = reader.ctx
    L = _hip.lib()
    try:
        for (want, k) in ((0, lc.PRODUCTION), (1, 36864), (36864, 36864), (36865, 45056), (100000, 102400), (4091904, 4091904), (2 ** 31 - 1, lc.PRODUCTION)):
            ctx.set_jpeg_long_scans(True, want)
            assert ctx.jpeg_long_scans() and ctx.jpeg_long_chapter_bytes() == k, want
            ctx.set_jpeg_long_scans(True, k)                                  # the length in force is a fixed point
            assert ctx.jpeg_long_chapter_bytes() == k
        ctx.set_jpeg_long_scans(False, 100000)
        assert not ctx.jpeg_long_scans() and ctx.jpeg_long_chapter_bytes() == 102400
        ctx.set_jpeg_long_scans(True, 100000)
        with pytest.raises(Exception):
            ctx.set_jpeg_long_scans(True, -1)
        assert ctx.jpeg_long_scans() and ctx.jpeg_long_chapter_bytes() == 102400   # a refused call changes nothing
        assert L.melf_ctx_set_jpeg_long_scans(None, 1, 0) != 0
        assert L.melf_ctx_get_jpeg_long_scans(ctx._h, None, None) != 0
        assert not ctx.jpeg_truncated() and ctx.jpeg_samplings()                   # the other switches' bits are untouched
        paths = sc.golden_files()[2:6]
        ctx.set_jpeg_long_scans(True, 0)
        ctx.jpeg_process_files_begin(paths)
        with pytest.raises(Exception):
            ctx.set_jpeg_long_scans(False)
        ctx.jpeg_process_files_end()
        assert ctx.jpeg_long_scans()
        # launches of a call without a long file, switch off / on / off
        files = [open(p, 'rb').read() for p in paths]
        (H, W) = _hip.jpeg_probe(files[0])[:2]
        seen = []
        ctx.set_profiling(1)
        try:
            for on in (False, True, False):
                ctx.set_jpeg_long_scans(on, 0)
                ctx.timings()
                (recs, status) = ctx.jpeg_process_batch(files, H, W)
                assert (status == 0).all()
                seen.append(({name: v[1] for (name, v) in ctx.timings().items()}, recs.tobytes()))
        finally:
            ctx.set_profiling(0)
        assert seen[0] == seen[1] == seen[2] and sum(seen[0][0].values()) > 0
    finally:
        reader.set_jpeg_long_scans(True, 0)
