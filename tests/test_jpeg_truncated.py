"""Baseline JPEG files that end inside their scan, completed on the GPU as libjpeg completes them (melf_ctx_set_jpeg_truncated).

The reference never comes from the GPU: a frame is Pillow's (libjpeg-turbo's) decode of `data[:cut] + FF D9`, a record is the
reader's on the host decoder's frame.  Bar: every byte of every frame and of every record, for every cut inside the range where
libjpeg's range limit is a plain clamp (tests/jpeg_cut_cases.py: at most one cut in sixteen of a file may lie outside it, and that is
asserted wherever cuts are left out).

CPU part: the rule restated in Python equals Pillow at every cut; the walk of meterelf_amd/csrc/melf_jpeg_cut.h as a host program
(tests/jpeg_cut_main.cpp, plain and under the host sanitizers) gives the rule's blocks at every cut; interfaces; the code-object
notes of the built library.  GPU part: whole frames at every cut of small files of every sampling, with and without restart
intervals; the switch off; a camera frame; the meter_rect window with the cut before, inside and behind it; mixed calls, chunked;
what stays corrupt; an EOI in mid-scan; the other switches; launches."""
import functools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_cut_cases as cc  # noqa: E402
from tests import jpeg_orient_cases as jc  # noqa: E402
from tests import jpeg_prog_writer as pw  # noqa: E402
from tests import jpeg_sampling_cases as sc  # noqa: E402
from tests import jpeg_scans_cases as ms  # noqa: E402
from tests import jpeg_writer as jw  # noqa: E402

PFILE = os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml')
HUFF_GOLDEN = os.path.join(sc.GOLDEN, 'jpeg_cut', 'huff_kernel_resources.json')

# name -> (size, Pillow subsampling, restart interval in MCUs, greyscale)
SMALL = {
    '420': ((37, 51), '4:2:0', 0, False),
    '422': ((37, 51), '4:2:2', 0, False),
    '444': ((24, 40), '4:4:4', 0, False),
    '420-rst3': ((37, 51), '4:2:0', 3, False),
    'grey': ((16, 24), '4:4:4', 0, True),
    '420-rstrow': ((37, 51), '4:2:0', 4, False),   # one MCU row: ceil(51 / 16) MCUs
}
CPU_FILES = ['420', '422', '444', '420-rst3', 'grey']
GPU_FILES = ['420', '422', '444', '420-rst3', 'grey', '420-rstrow']


@functools.lru_cache(None)
def _small(name):
    """(bytes, parsed headers, the whole file decoded once) of a Pillow-written quality-90 file."""
    (size, sub, restart, grey) = SMALL[name]
    data = cc.pillow_file(size, sub, quality=90, restart=restart, grey=grey)
    p = cc.parse(data)
    assert p.size == size and p.restart == restart
    return (data, p, cc.decode(p))


@functools.lru_cache(None)
def _kept(name):
    """[(cut, grids, cut MCU)] of the file's cuts inside the range (the cap of one in sixteen is asserted there)."""
    (_data, p, d) = _small(name)
    return cc.in_range_cuts(p, d, cc.cuts(p))


# ------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize('name', CPU_FILES)
def test_the_rule_equals_pillow_at_every_cut(name):
    """Every cut from the first scan byte to the last: the rule's coefficient grids, written out as a complete file with the Annex K
    tables, decode to the very frame Pillow gives the truncated file.  Cuts outside the plain-clamp range are left out, at most one in
    sixteen."""
    (data, p, d) = _small(name)
    kept = _kept(name)
    assert len(cc.cuts(p)) > 100 and all(cm is not None for (_c, _g, cm) in kept)
    assert {cm for (_c, _g, cm) in kept} == set(range(p.my * p.mx))     # every MCU of the grid is the cut MCU of some cut
    done = {}
    for (cut, grids, cm) in kept:
        key = b''.join(g.tobytes() for g in grids)
        if key not in done:                                              # many cuts of one MCU give the same grids: decode them once
            done[key] = cc.pillow_bgr(cc.reencode(p, grids))
        ref = cc.reference(data, cut)
        assert np.array_equal(done[key], ref), (name, cut, cm, int((done[key] != ref).sum()))


def _compiler():
    for cxx in (os.environ.get('CXX'), '/opt/rocm/llvm/bin/clang++', 'g++', 'clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail('no C++ compiler for the stand-alone program')


@pytest.mark.parametrize('flags', [[], ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g']], ids=['plain', 'sanitizers'])
def test_the_walk_as_a_host_program(tmp_path, flags):
    """tests/jpeg_cut_main.cpp: melf_jpeg_cut.h's walk as an ordinary program, on every cut of the 37 x 51 4:2:0 file without restart
    intervals and with an interval of 3 MCUs, each case from a decoder state a few symbols before the stream's end (or from zero bits,
    where the cut MCU begins an interval that was not found), on a heap copy of exactly the stream's bytes.  Its blocks are the rule's."""
    exe = str(tmp_path / 'jpeg_cut_main')
    subprocess.check_call([_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + flags +
                          ['-I', os.path.join(ROOT, 'meterelf_amd', 'csrc'), os.path.join(ROOT, 'tests', 'jpeg_cut_main.cpp'), '-o', exe])
    for name in ('420', '420-rst3'):
        (_data, p, d) = _small(name)
        positions = cc.cuts(p)
        (text, cases) = cc.program_input(p, d, positions)
        path = str(tmp_path / (name + '.txt'))
        open(path, 'w').write(text)
        out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        lines = out.stdout.decode().split('\n')
        assert lines[-2] == 'done %d' % len(positions)
        at = 0
        bpm = len(p.layout)
        mid_block = 0
        for (n, (cut, first, k)) in enumerate(cases):
            (grids, cm, _bits) = cc.rule(p, d, cut)
            (word, idx, res, after) = lines[at].split()
            at += 1
            assert (word, int(idx), int(res), int(after)) == ('case', n, 1, (cm + 1) * bpm), (name, cut, lines[at - 1])
            mid_block += k > 0
            for nb in range(first, (cm + 1) * bpm):
                got = lines[at].split()
                at += 1
                assert got[0] == 'block' and int(got[1]) == nb
                (m, b) = divmod(nb, bpm)
                (c, y, x) = p.layout[b]
                (yy, xx) = divmod(m, p.mx)
                (h, v) = (jw.SAMPLING[p.sampling][1], jw.SAMPLING[p.sampling][2]) if c == 0 else (1, 1)
                want = grids[c][yy * v + y, xx * h + x].astype(np.int64)
                have = np.array([int(t) for t in got[2:]], np.int64)
                look = jw.ZIGZAG[k:] if nb == first else jw.ZIGZAG     # the walk joins the first block at coefficient k
                assert np.array_equal(have[look], want[look]), (name, cut, nb, k)
        assert mid_block * 2 > len(cases)                               # most cases join a block in its middle


def test_exports_header_and_defaults():
    import inspect

    from meterelf_amd import MeterReader, _hip
    names = {'melf_ctx_set_jpeg_truncated', 'melf_ctx_get_jpeg_truncated', 'melf_ctx_jpeg_truncated_files'}
    assert names <= set(_hip.EXPORTS)
    L = _hip.lib()
    assert all(getattr(L, n) for n in names)
    header = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    assert 'int melf_ctx_set_jpeg_truncated(melf_ctx* ctx, int on);' in header and 'int melf_ctx_get_jpeg_truncated(melf_ctx* ctx, int* on);' in header
    assert 'int melf_ctx_jpeg_truncated_files(const melf_ctx* ctx, int64_t* files, int reset);' in header
    assert inspect.signature(MeterReader.__init__).parameters['jpeg_truncated'].default is False
    assert hasattr(MeterReader, 'set_jpeg_truncated')
    for n in ('set_jpeg_truncated', 'jpeg_truncated', 'jpeg_truncated_files'):
        assert hasattr(_hip.Context, n)
    # no probe knows the switch: the flag set is what it was (bits 8 and 64 stay bad arguments)
    (data, _p, _d) = _small('420')
    for flag in (8, 64, 256):
        with pytest.raises(Exception):
            _hip.jpeg_probe_flags(data, flag)


def test_get_meter_values_asks_for_the_switch_unless_the_host_is_asked_for(monkeypatch):
    """METERELF_JPEG_TRUNCATED: 'gpu' (the default) or 'host'; the setting is part of the reader-cache key."""
    from meterelf_amd import _api, _engine, _params

    class Reader:
        jpeg_truncated = False

        def set_jpeg_truncated(self, on):
            self.jpeg_truncated = bool(on)
    monkeypatch.delenv('METERELF_JPEG_TRUNCATED', raising=False)
    params = _params.load(PFILE)
    blob = _engine.make_blob(params)
    k_default = _api._reader_key(params, blob, 0)
    assert _api._jpeg_on_gpu('jpeg_truncated') and _api._with_jpeg_orientation(Reader()).jpeg_truncated
    monkeypatch.setenv('METERELF_JPEG_TRUNCATED', 'host')
    assert not _api._jpeg_on_gpu('jpeg_truncated') and not _api._with_jpeg_orientation(Reader()).jpeg_truncated
    k_host = _api._reader_key(params, blob, 0)
    monkeypatch.setenv('METERELF_JPEG_TRUNCATED', 'gpu')
    assert _api._jpeg_on_gpu('jpeg_truncated') and _api._with_jpeg_orientation(Reader()).jpeg_truncated
    assert _api._reader_key(params, blob, 0) != k_host and k_default != k_host


def test_code_object_notes_of_the_built_library():
    """k_jpeg_cut_tail has no scratch and spills nothing; every k_jpeg_huff / k_jpeg_huff_rst instantiation has the registers, LDS and
    scratch -- and so the waves per SIMD -- of the build before the switch existed (tests/golden/jpeg_cut/huff_kernel_resources.json,
    read from that build with tools/kernel_meta.py)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    tail = [v for (k, v) in meta.items() if 'k_jpeg_cut_tail' in k]
    assert len(tail) == 1
    assert tail[0]['private_segment_fixed_size'] == 0 and tail[0]['vgpr_spill_count'] == 0 and tail[0]['sgpr_spill_count'] == 0
    want = json.load(open(HUFF_GOLDEN))
    assert set(want) == {'k_jpeg_huffILi512E', 'k_jpeg_huffILi1024E', 'k_jpeg_huff_rstILi256E'}
    for (tag, figures) in want.items():
        got = [v for (k, v) in meta.items() if tag in k]
        assert len(got) == 1, tag
        assert {f: got[0][f] for f in figures} == figures, (tag, got[0])


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope='module')
def reader():
    from meterelf_amd import _hip
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    plain = MeterReader(_params.load(PFILE))
    assert not plain.jpeg_truncated and not plain.ctx.jpeg_truncated()   # off by default
    plain.close()
    r = MeterReader(_params.load(PFILE), jpeg_truncated=True)
    assert r.ctx.jpeg_truncated() and r.jpeg_truncated and not r.ctx.jpeg_multiscan()
    yield r
    r.close()


def _decode(ctx, files, size, calls_of=1024):
    (frames, status) = ([], [])
    for i in range(0, len(files), calls_of):
        (f, s) = ctx.jpeg_decode(files[i:i + calls_of], *size)
        frames.append(f)
        status.append(s)
    return (np.concatenate(frames), np.concatenate(status))


@pytest.mark.gpu
@pytest.mark.parametrize('name', GPU_FILES)
def test_every_cut_decodes_to_pillows_frame(reader, name):
    """melf_jpeg_decode_batch with the switch on, every in-range cut of a small file (the bytes up to the cut, nothing behind them):
    status 0, every byte Pillow's, and the counter says every file was completed under the rule.  The 1.1 KB scans spread over about
    30 Huffman segments, so the cuts fall into first, middle and last segments; the sizes cut the MCU grid in both directions."""
    (data, p, _d) = _small(name)
    kept = _kept(name)
    files = [data[:cut] for (cut, _g, _cm) in kept]
    reader.ctx.jpeg_truncated_files(reset=True)
    (frames, status) = _decode(reader.ctx, files, p.size)
    assert (status == 0).all(), [(kept[i][0], int(s)) for (i, s) in enumerate(status) if s][:5]
    assert reader.ctx.jpeg_truncated_files() == len(files)
    assert reader.ctx.jpeg_truncated_files(reset=True) == len(files) and reader.ctx.jpeg_truncated_files() == 0
    for ((cut, _g, cm), got) in zip(kept, frames):
        ref = cc.reference(data, cut)
        assert np.array_equal(got, ref), (name, cut, cm, int((got != ref).sum()), np.argwhere(got != ref)[:3].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['420', '420-rst3'])
def test_the_switch_off_every_cut_is_corrupt(reader, name):
    """The same call with the switch off: every file MELF_JPEG_CORRUPT with a zero frame, as ever, and nothing counted.  As ever, too,
    the exception: a cut inside the last MCU's last blocks, where the segment decoders' 32 bits of over-run into the scan area's zero
    padding complete the last MCU by themselves -- status 0 and Pillow's frame, with the switch or without (tests/test_jpeg.py has
    always allowed a truncated file either answer).  Those are cuts of the last MCU only, fewer than one in sixteen."""
    from meterelf_amd import _hip
    (data, p, _d) = _small(name)
    kept = _kept(name)
    files = [data[:cut] for (cut, _g, _cm) in kept]
    reader.set_jpeg_truncated(False)
    try:
        reader.ctx.jpeg_truncated_files(reset=True)
        (frames, status) = _decode(reader.ctx, files, p.size)
        assert reader.ctx.jpeg_truncated_files() == 0
    finally:
        reader.set_jpeg_truncated(True)
    ok = status == 0
    print('%s: %d of %d cuts completed by the zero padding alone with the switch off' % (name, int(ok.sum()), len(files)))
    assert (status[~ok] == _hip.JPEG_CORRUPT).all() and not frames[~ok].any()
    assert ok.sum() * 16 <= len(files)
    for i in np.flatnonzero(ok):
        (cut, _g, cm) = kept[i]
        assert cm == p.my * p.mx - 1 and np.array_equal(frames[i], cc.reference(data, cut)), (name, cut, cm)


@functools.lru_cache(None)
def _camera():
    """One fixture frame (640 x 480 pixels) as a writer file with the flat tables (its scan is long: segments above the minimum length)."""
    (paths, frames) = sc.fixture_frames(1)
    data = sc.reencode(frames[0], '420')
    p = cc.parse(data)
    return (data, p, cc.decode(p))


@pytest.mark.gpu
def test_a_camera_frame_cut_at_ten_places(reader):
    (data, p, d) = _camera()
    assert p.size[0] * p.size[1] == 640 * 480 and p.scan_end - p.scan_begin > 20000
    positions = [int(v) for v in np.linspace(p.scan_begin + 1, p.scan_end - 1, 10)]
    kept = cc.in_range_cuts(p, d, positions)
    assert len(kept) == 10
    reader.ctx.jpeg_truncated_files(reset=True)
    (frames, status) = reader.ctx.jpeg_decode([data[:cut] for (cut, _g, _cm) in kept], *p.size)
    assert (status == 0).all() and reader.ctx.jpeg_truncated_files(reset=True) == 10
    for ((cut, _g, cm), got) in zip(kept, frames):
        ref = cc.reference(data, cut)
        assert np.array_equal(got, ref), (cut, cm, int((got != ref).sum()), np.argwhere(got != ref)[:3].tolist())


def _window_cuts(p, d, params):
    """Cut positions of a camera file whose cut MCU lies before the meter_rect window's rows, inside the window, and well behind its
    last row plus the decoder's margin."""
    ((x0, y0), (x1, y1)) = params.meter_rect
    row_of = lambda cut: cc.rule(p, d, cut)[1] // p.mx   # noqa: E731
    cuts = cc.cuts(p)
    pick = {}
    for cut in cuts[::97]:
        r = row_of(cut) * 16
        kind = 'before' if r + 16 <= y0 - 32 else 'inside' if y0 <= r and r + 16 <= y1 else 'behind' if r >= y1 + 80 else None
        if kind:
            pick.setdefault(kind, []).append(cut)
    return {k: [v[len(v) // 3], v[2 * len(v) // 3]] for (k, v) in pick.items()}


@pytest.mark.gpu
def test_the_windowed_path_reads_like_the_host_decoder(reader, tmp_path):
    """melf_jpeg_process_batch and read_jpeg_paths on a camera file cut before the meter_rect window, inside it and behind it: records
    equal to the reader's on the host decoder's frame.  Behind the window the answer is the same with the switch off, and the counter
    does not move: the window-limited decode never looked there."""
    from meterelf_amd import _image
    (data, p, d) = _camera()
    picks = _window_cuts(p, d, reader.params)
    assert set(picks) == {'before', 'inside', 'behind'}
    (H, W) = p.size
    for kind in ('before', 'inside', 'behind'):
        kept = cc.in_range_cuts(p, d, picks[kind])
        assert len(kept) == 2
        files = [data[:cut] for (cut, _g, _cm) in kept]
        paths = []
        for (k, f) in enumerate(files):
            paths.append(str(tmp_path / ('%s%d.jpg' % (kind, k))))
            open(paths[-1], 'wb').write(f)
        host = np.stack([_image.imread_bgr(q) for q in paths])
        for (h, (cut, _g, _cm)) in zip(host, kept):
            assert np.array_equal(h, cc.reference(data, cut))            # the host decoder is libjpeg too
        ref = reader.read_frames(host)
        reader.ctx.jpeg_truncated_files(reset=True)
        (recs, status) = reader.ctx.jpeg_process_batch(files, H, W)
        assert (status == 0).all() and recs.tobytes() == ref.tobytes(), (kind, status)
        counted = reader.ctx.jpeg_truncated_files(reset=True)
        got = reader.read_jpeg_paths(paths)
        assert all(g is not None and g.tobytes() == x.tobytes() for (g, x) in zip(got, ref)), kind
        reader.ctx.jpeg_truncated_files(reset=True)
        if kind == 'behind':
            assert counted == 0
            reader.set_jpeg_truncated(False)
            try:
                (recs0, status0) = reader.ctx.jpeg_process_batch(files, H, W)
            finally:
                reader.set_jpeg_truncated(True)
            assert (status0 == 0).all() and recs0.tobytes() == ref.tobytes()
        else:
            assert counted == len(files), (kind, counted)


def _mixed_call():
    """[(kind, bytes, expected status, reference frame or None)]: whole and cut files of one size with a cut progressive file, a cut
    multi-scan file, a file cut in its headers, garbage and a file of another size among them."""
    from meterelf_amd import _hip
    size = (37, 51)
    items = []
    for (k, name) in enumerate(('420', '422', '420-rst3', '420-rstrow')):
        (data, p, _d) = _small(name)
        kept = _kept(name)
        items.append(('whole-' + name, data, 0, sc.pillow_bgr(data)))
        for (cut, _g, _cm) in (kept[len(kept) // 5], kept[len(kept) // 2], kept[-1 - k]):
            items.append(('cut-%s-%d' % (name, cut), data[:cut], 0, cc.reference(data, cut)))
    grids = ms.grids_for(size, '420', seed=70)
    prog = pw.write_progressive(grids, size, '420', sc.QT, pw.PILLOW_COLOUR)
    multi = ms.write_multiscan(grids, size, '420')
    spans = ms.scan_offsets(multi)
    (data, p, _d) = _small('420')
    items.insert(3, ('cut-progressive', prog[:len(prog) - len(prog) // 3], _hip.JPEG_CORRUPT, None))
    items.insert(6, ('cut-multiscan', multi[:(spans[2][0] + spans[2][1]) // 2], _hip.JPEG_CORRUPT, None))
    items.insert(8, ('cut-in-headers', data[:p.scan_begin - 20], _hip.JPEG_CORRUPT, None))
    items.insert(9, ('garbage', b'garbage' * 40, _hip.JPEG_CORRUPT, None))
    other = sc.natural_file(np.random.default_rng(9), (24, 40), '420')
    items.insert(12, ('other-size', other, _hip.JPEG_SIZE_MISMATCH, None))
    return (size, items)


@pytest.mark.gpu
def test_a_mixed_call_of_whole_and_cut_files(reader):
    (size, items) = _mixed_call()
    reader.set_jpeg_progressive(True)
    reader.set_jpeg_multiscan(True)
    try:
        reader.ctx.jpeg_truncated_files(reset=True)
        (frames, status) = reader.ctx.jpeg_decode([d for (_k, d, _s, _r) in items], *size)
        assert [int(s) for s in status] == [s for (_k, _d, s, _r) in items], [(k, int(a)) for ((k, _d, s, _r), a) in zip(items, status) if a != s]
        assert reader.ctx.jpeg_truncated_files(reset=True) == sum(k.startswith('cut-4') for (k, _d, _s, _r) in items)
        for ((kind, _d, _s, ref), got) in zip(items, frames):
            assert (np.array_equal(got, ref) if ref is not None else not got.any()), kind
    finally:
        reader.set_jpeg_progressive(False)
        reader.set_jpeg_multiscan(False)


@pytest.mark.gpu
@pytest.mark.parametrize('chunk', ['96', '40,260'])
def test_chunked_calls_equal_the_one_piece_call(reader, monkeypatch, chunk):
    """melf_jpeg_process_batch on a list of whole and cut camera files with a file cut in its headers, garbage and a file of another
    size among them: calls of at most 64 files (one piece each) and the same list in one pipelined call under MELF_JPEG_CHUNK give
    the same statuses and records, and count the same files."""
    from meterelf_amd import _hip
    (data, p, d) = _camera()
    (H, W) = p.size
    picks = _window_cuts(p, d, reader.params)
    kept = cc.in_range_cuts(p, d, picks['before'] + picks['inside'])
    cut_files = [data[:cut] for (cut, _g, _cm) in kept]
    files = []
    for k in range(300):
        files.append(cut_files[k % len(cut_files)] if k % 7 == 3 else data)
    files[20] = data[:p.scan_begin - 20]
    files[150] = b'garbage' * 40
    files[151] = sc.natural_file(np.random.default_rng(9), (24, 40), '420')
    reader.ctx.jpeg_truncated_files(reset=True)
    (ref, rstat) = ([], [])
    for i in range(0, len(files), 64):
        (r, s) = reader.ctx.jpeg_process_batch(files[i:i + 64], H, W)
        ref.append(r)
        rstat.append(s)
    (ref, rstat) = (np.concatenate(ref), np.concatenate(rstat))
    ncut = sum(1 for k in range(300) if k % 7 == 3 and k not in (20, 150, 151))
    assert reader.ctx.jpeg_truncated_files(reset=True) == ncut
    assert rstat[20] == _hip.JPEG_CORRUPT and rstat[150] == _hip.JPEG_CORRUPT and rstat[151] == _hip.JPEG_SIZE_MISMATCH and (rstat == 0).sum() == 297
    monkeypatch.setenv('MELF_JPEG_CHUNK', chunk)
    (got, gstat) = reader.ctx.jpeg_process_batch(files, H, W)
    assert np.array_equal(gstat, rstat) and reader.ctx.jpeg_truncated_files(reset=True) == ncut
    ok = rstat == 0
    assert got[ok].tobytes() == ref[ok].tobytes()
    host = reader.read_frames(np.stack([sc.pillow_bgr(data), cc.reference(data, kept[3 % len(kept)][0])]))
    assert got[0].tobytes() == host[0].tobytes() and got[3].tobytes() == host[1].tobytes()


@pytest.mark.gpu
def test_still_corrupt_with_the_switch_on(reader):
    """An impossible code in mid-stream, a middle restart interval that runs out of data, one RSTn too many, a scan ended by a DHT marker:
    MELF_JPEG_CORRUPT and a zero frame with the switch on as with it off, the files on either side exact."""
    from meterelf_amd import _hip
    size = (37, 51)
    rng = np.random.default_rng(21)
    grids = sc.image_coefs(sc.natural(rng, *size), '420')
    good = sc.write(grids, size, '420')
    p = cc.parse(good)
    mid = (p.scan_begin + p.scan_end) // 2
    nocode = good[:mid] + b'\xff\x00' * 8 + good[mid + 16:]               # 64 one-bits: no code of either Annex K table is all ones
    rst = sc.write(grids, size, '420', restart=5)                          # 12 MCUs: intervals of 5, 5 and 2
    pr = cc.parse(rst)
    (a, b) = (rst.index(b'\xff\xd0', pr.scan_begin), rst.index(b'\xff\xd1', pr.scan_begin))
    short_middle = rst[:a + 2] + rst[b:]                                   # the second interval empty: its lane finds 2 MCUs of data for 5
    surplus = rst[:b] + b'\xff\xd1' + rst[b:pr.scan_end] + b'\xff\xd2' + rst[pr.scan_end:]   # thirteenth MCU's worth of markers: one RSTn too many
    dht = good[:mid] + b'\xff\xc4\x00\x02' + good[p.scan_end:]             # the scan ends at a DHT marker, half way
    files = [good, nocode, rst, short_middle, good, surplus, rst, dht, good]
    want = [0, 2, 0, 2, 0, 2, 0, 2, 0]
    for on in (True, False):
        reader.set_jpeg_truncated(on)
        try:
            reader.ctx.jpeg_truncated_files(reset=True)
            (frames, status) = reader.ctx.jpeg_decode(files, *size)
            assert [int(s) for s in status] == [_hip.JPEG_CORRUPT if w else 0 for w in want], (on, status)
            assert reader.ctx.jpeg_truncated_files() == 0
            for (i, f) in enumerate(files):
                assert (not frames[i].any()) if want[i] else np.array_equal(frames[i], sc.pillow_bgr(f)), (on, i)
        finally:
            reader.set_jpeg_truncated(True)


@pytest.mark.gpu
def test_an_eoi_in_mid_scan_with_bytes_behind_it(reader):
    """FF D9 spliced into the scan, the rest of the file behind it: the frame of the file cut there."""
    for name in ('420', '420-rst3'):
        (data, p, _d) = _small(name)
        kept = _kept(name)
        pick = [kept[len(kept) // 4], kept[len(kept) // 2], kept[3 * len(kept) // 4]]
        files = [data[:cut] + b'\xff\xd9' + data[cut:] for (cut, _g, _cm) in pick]
        reader.ctx.jpeg_truncated_files(reset=True)
        (frames, status) = reader.ctx.jpeg_decode(files, *p.size)
        assert (status == 0).all() and reader.ctx.jpeg_truncated_files(reset=True) == len(files)
        for ((cut, _g, _cm), got) in zip(pick, frames):
            assert np.array_equal(got, cc.reference(data, cut)), (name, cut)


def _some_cuts(data, n=6):
    """(parsed, [(cut, grids, cut MCU)]): n evenly spaced in-range cuts of a file (the cap applies to the ones tried)."""
    p = cc.parse(data)
    d = cc.decode(p)
    positions = [int(v) for v in np.linspace(p.scan_begin + 1, p.scan_end - 1, 16)]
    kept = cc.in_range_cuts(p, d, positions)
    return (p, kept[::max(1, len(kept) // n)][:n])


@pytest.mark.gpu
def test_with_the_other_switches(reader):
    """A handful of cuts each: EXIF orientation 6 with that switch, a 4:4:0 and a 4:1:1 file, a file without DHT segments, and a file with
    tables of its own whose all-zero codes are not the Annex K symbols (the all-zero AC code carries a run)."""
    size = (37, 51)
    rng = np.random.default_rng(33)
    img = sc.natural(rng, *size)
    # orientation 6: the stored frame is 51 x 37; the reference is Pillow's frame of the cut file, turned as cv2.imread turns it
    stored = np.ascontiguousarray(jc.unorient(img, 6))
    plain = sc.write(sc.image_coefs(stored, '420'), stored.shape[:2], '420')
    (p, kept) = _some_cuts(plain)
    tagged = jc.with_app1(plain, jc.tiff_block(6, False))
    shift = len(tagged) - len(plain)
    reader.set_jpeg_orientation(True)
    try:
        reader.ctx.jpeg_truncated_files(reset=True)
        (frames, status) = reader.ctx.jpeg_decode([tagged[:cut + shift] for (cut, _g, _cm) in kept], *size)
        assert (status == 0).all() and reader.ctx.jpeg_truncated_files(reset=True) == len(kept)
        for ((cut, _g, _cm), got) in zip(kept, frames):
            assert np.array_equal(got, np.ascontiguousarray(jc.orient(cc.reference(tagged, cut + shift), 6))), ('orient', cut)
    finally:
        reader.set_jpeg_orientation(False)
    reader.set_jpeg_samplings(True)
    try:
        for sampling in ('440', '411'):
            data = sc.write(sc.image_coefs(img, sampling), size, sampling)
            (p, kept) = _some_cuts(data)
            (frames, status) = reader.ctx.jpeg_decode([data[:cut] for (cut, _g, _cm) in kept], *size)
            assert (status == 0).all() and reader.ctx.jpeg_truncated_files(reset=True) == len(kept)
            for ((cut, _g, _cm), got) in zip(kept, frames):
                assert np.array_equal(got, cc.reference(data, cut)), (sampling, cut)
    finally:
        reader.set_jpeg_samplings(False)
    reader.set_jpeg_default_tables(True)
    try:
        data = ms.without_tables(sc.image_coefs(img, '422'), size, '422')
        assert b'\xff\xc4' not in data
        (p, kept) = _some_cuts(data)
        (frames, status) = reader.ctx.jpeg_decode([data[:cut] for (cut, _g, _cm) in kept], *size)
        assert (status == 0).all() and reader.ctx.jpeg_truncated_files(reset=True) == len(kept)
        for ((cut, _g, _cm), got) in zip(kept, frames):
            assert np.array_equal(got, cc.reference(data, cut)), ('bare', cut)
    finally:
        reader.set_jpeg_default_tables(False)
    (data, zero_syms) = _own_tables_file(img, size)
    std = jw.standard_tables()
    assert zero_syms['ac'] != std['ac'][0][1][0] and zero_syms['ac'] >> 4 and zero_syms['dc'] != std['dc'][0][1][0]
    (p, kept) = _some_cuts(data)
    (frames, status) = reader.ctx.jpeg_decode([data[:cut] for (cut, _g, _cm) in kept], *size)
    assert (status == 0).all() and reader.ctx.jpeg_truncated_files(reset=True) == len(kept)
    for ((cut, _g, _cm), got) in zip(kept, frames):
        assert np.array_equal(got, cc.reference(data, cut)), ('own tables', cut)


def _own_tables_file(img, size):
    """A 4:4:4 file with one DC and one AC table of its own whose FIRST codes (the all-zero ones) are DC category 2 and the AC symbol
    run 2 / size 1: a zero-filled block is then -3 at DC and a -1 at every third coefficient, the last run overshooting the block."""
    std = jw.standard_tables()
    dc_syms = [2] + [s for s in std['dc'][0][1] if s != 2]
    ac_syms = [0x21] + [s for s in std['ac'][0][1] if s != 0x21]
    dc = ([0, 0] + [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1] + [0, 0, 0], dc_syms)          # lengths 2 .. 13, one code each: complete but for all-ones
    bits = list(std['ac'][0][0])
    ac = (bits, ac_syms)
    qt = {0: (sc.q_ramp(1, 2), False)}
    grids = jw.coefficients_from_image(img, '444', [qt[0][0]] * 3)
    data = jw.write_jpeg(grids, size, '444', qt, {0: dc}, {0: ac}, sel=[(0, 0, 0)] * 3)
    return (data, {'dc': dc_syms[0], 'ac': ac_syms[0]})


@pytest.mark.gpu
def test_a_call_without_a_cut_file_launches_what_it_launched(reader):
    """melf_ctx_timings of a call of whole files with the switch off, on and off: the same launches of every kernel, the same records,
    nothing counted."""
    (paths, _frames) = sc.fixture_frames(8)
    files = [open(f, 'rb').read() for f in paths]
    from meterelf_amd import _hip
    (H, W) = _hip.jpeg_probe(files[0])[:2]
    ctx = reader.ctx
    seen = []
    ctx.set_profiling(1)
    try:
        for on in (False, True, False):
            reader.set_jpeg_truncated(on)
            ctx.timings()
            ctx.jpeg_truncated_files(reset=True)
            (recs, status) = ctx.jpeg_process_batch(files, H, W)
            assert (status == 0).all() and ctx.jpeg_truncated_files() == 0
            seen.append(({k: v[1] for (k, v) in ctx.timings().items()}, recs.tobytes()))
    finally:
        ctx.set_profiling(0)
        reader.set_jpeg_truncated(True)
    assert seen[0] == seen[1] == seen[2] and sum(seen[0][0].values()) > 0
