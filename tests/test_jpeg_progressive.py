"""Progressive JPEG files (SOF2) decoded on the GPU (melf_ctx_set_jpeg_progressive, k_jpeg_prog_scan, melf_jpeg_prog.h).

The reference never comes from the GPU: a frame is Pillow's (libjpeg-turbo's) decode of the same bytes, a coefficient area is the
grids the test-side writer (tests/jpeg_prog_writer.py) was given, a record is the reader's on the host decoder's frame.  Bar: every
byte of every frame, coefficient and record.

CPU part: the probe with flags, the writer against Pillow (a progressive file of any script decodes to the pixels of the baseline file
of the same coefficient grids), refusals by reason, header fuzz, and the decoder body on the host (jpeg_prog_main.cpp, plain and under
the host sanitizers, on every script case and on a few hundred damaged copies).  GPU part: Pillow's files and the writer's against
Pillow, mixed calls in several chunkings, the switch off, the file-name calls and get_meter_values, and the damaged files' status.

EOB runs: category c needs a run of 2^c blocks whose band is empty, so category 14 needs 16 384 blocks in one scan (a 1024 x 1024 grey
image).  The cases stop at what a 64 x 64 grey image reaches: 64 blocks, categories 0..6.
"""
import collections
import functools
import glob
import io
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_orient_cases as jc  # noqa: E402
from tests import jpeg_prog_writer as pw  # noqa: E402
from tests import jpeg_writer as jw  # noqa: E402
from tests.test_jpeg import _encode, _natural_image, _pillow_bgr  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PFILE = os.path.join(GOLDEN, 'sample-images1', 'params.yml')
TAKE_PROG = 2
TAKE_ORIENT = 1
Case = collections.namedtuple('Case', 'name data size sampling coefs script decoded stats')

# sizes whose padded and real block grids differ (and one whole-MCU greyscale)
GEOMETRIES = [((24, 40), '420'), ((33, 47), '420'), ((17, 16), '422'), ((9, 1), '444'), ((1, 1), '444'), ((16, 16), 'grey')]
SUBSAMPLING = {'grey': None, '444': '4:4:4', '422': '4:2:2', '420': '4:2:0'}


def _q(step, base=2):
    (i, j) = np.mgrid[0:8, 0:8]
    return np.minimum(base + step * (i + j), 255).reshape(64).tolist()


QT = {0: (_q(2), False), 1: (_q(3, 3), False)}


def _coefs(rng, size, sampling):
    nc = jw.SAMPLING[sampling][0]
    img = _natural_image(rng, *size)
    return jw.coefficients_from_image(img[..., 1] if nc == 1 else img, sampling, [QT[0][0], QT[1][0], QT[1][0]][:nc])


# ------------------------------------------------------------------ scan scripts ----
def _script_spectral(nc, dc_interleaved=True):
    comps = tuple(range(nc))
    s = [(comps, 0, 0, 0, 0)] if dc_interleaved else [((c,), 0, 0, 0, 0) for c in comps]
    for c in comps:
        s += [((c,), 1, 5, 0, 0), ((c,), 6, 63, 0, 0)]
    return s


def _script_successive(nc):
    comps = tuple(range(nc))
    s = [(comps, 0, 0, 0, 3)]
    for c in comps:
        s.append(((c,), 1, 63, 0, 3))
    for al in (2, 1, 0):
        s.append((comps, 0, 0, al + 1, al))
        for c in comps:
            s.append(((c,), 1, 63, al + 1, al))
    return s


def _script_bands_of_one(nc, total):
    """DC, the chroma components in one band each, luma in bands of width 1 and one last band: `total` scans."""
    comps = tuple(range(nc))
    s = [(comps, 0, 0, 0, 0)] + [((c,), 1, 63, 0, 0) for c in comps[1:]]
    singles = total - len(s) - 1
    s += [((0,), k, k, 0, 0) for k in range(1, singles + 1)]
    s.append(((0,), singles + 1, 63, 0, 0))
    assert len(s) == total
    return s


def _history_blocks(coefs):
    """Every component's block (0, 0) (and every fourth block) rebuilt so that a refinement scan 1 -> 0 of the band 1..63 meets: a
    run of more than sixteen zero-history positions that crosses coefficients with history (ZRL, correction bits behind it), a new
    coefficient right after fifteen zeros of history, and a band tail under an EOB run that still holds coefficients with history."""
    out = [g.copy() for g in coefs]
    for g in out:
        flat = g.reshape(-1, 64)
        for b in range(0, flat.shape[0], 4):
            zz = np.zeros(64, np.int16)
            zz[0] = flat[b, 0]
            zz[2] = 3; zz[5] = -2; zz[9] = 6          # history (non-zero at Al = 1) inside the first long run
            zz[24] = 1                                  # new, 21 zero-history positions behind the band's start: ZRL over history
            zz[30] = -5                                 # history
            zz[41] = -1                                 # new, exactly 15 zero-history positions behind 24 (25..40 without 30)
            zz[50] = 2; zz[58] = -4                     # history in the tail, under the EOB
            blk = np.zeros(64, np.int16)
            blk[jw.ZIGZAG] = zz
            flat[b] = blk
    return out


def _eob_case():
    """64 x 64 grey, three luma bands: runs of 1, 2, 4, 8 and 16 empty bands (1..5), a run of 32 (6..20), a run of all 64 (21..63)."""
    size = (64, 64)
    g = np.zeros((8, 8, 64), np.int16)
    flat = g.reshape(64, 64)
    flat[:, 0] = np.arange(64) - 30
    z = jw.ZIGZAG
    at = 0
    for run in (1, 2, 4, 8, 16):
        at += run
        flat[at, z[5]] = 3          # the band's last coefficient: the block ends the run and needs no end of band itself
        at += 1
    flat[at:, z[3]] = -2            # the rest of band 1..5: no run
    flat[at:, z[5]] = 1
    flat[32:, z[6]] = 2             # band 6..20: the first 32 blocks empty, the others full to the band's end
    flat[32:, z[20]] = -1
    script = [((0,), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((0,), 6, 20, 0, 0), ((0,), 21, 63, 0, 0)]
    return ('eob-runs', size, 'grey', [g], script, {})


@functools.lru_cache(None)
def _cases():
    rng = np.random.default_rng(20261)
    out = []

    def add(name, size, sampling, coefs, script, **kw):
        stats = {}
        data = pw.write_progressive(coefs, size, sampling, QT, script, stats=stats, **kw)
        out.append(Case(name, data, size, sampling, coefs, script, pw.decoded_grids(coefs, size, sampling, script), stats))

    for (size, sampling) in GEOMETRIES:
        nc = jw.SAMPLING[sampling][0]
        tag = '%s-%dx%d' % (sampling, size[0], size[1])
        coefs = _coefs(rng, size, sampling)
        add('spectral-' + tag, size, sampling, coefs, _script_spectral(nc))
        add('spectral-dc-apart-' + tag, size, sampling, coefs, _script_spectral(nc, False))
        add('successive-' + tag, size, sampling, coefs, _script_successive(nc))
        add('bands-31-' + tag, size, sampling, coefs, _script_bands_of_one(nc, 31))
        add('bands-32-' + tag, size, sampling, coefs, _script_bands_of_one(nc, 32))
        add('history-' + tag, size, sampling, _history_blocks(coefs), _script_successive(nc))
        script = _script_successive(nc)
        add('ids-2-3-' + tag, size, sampling, coefs, script, tabsel=[{c: ((2, 3) if c == 0 else (3, 2)) for c in s[0]} for s in script])
        add('restart-1-' + tag, size, sampling, coefs, script, restart=1)
        add('restart-7-' + tag, size, sampling, coefs, _script_spectral(nc), restart=[7 if k % 2 else 5 for k in range(len(_script_spectral(nc)))])
    (name, size, sampling, coefs, script, kw) = _eob_case()
    add(name, size, sampling, coefs, script, **kw)
    return out


def _area_order(grids, size, sampling):
    """The grids in the decoder's block order: (MCU * blocks per MCU + block in the MCU) * 64."""
    (nc, hs, vs) = jw.SAMPLING[sampling]
    ((my, mx), _shapes) = jw.grid_shape(size, sampling)
    if nc == 1:
        return np.ascontiguousarray(grids[0].reshape(my * mx, 64)).astype('<i2')
    luma = grids[0].reshape(my, vs, mx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, vs * hs, 64)
    return np.ascontiguousarray(np.concatenate([luma] + [g.reshape(my * mx, 1, 64) for g in grids[1:]], axis=1)).astype('<i2')


def _baseline_of(case):
    """jpeg_writer's baseline file of the grids a decoder holds after the case's script."""
    nc = len(case.coefs)
    dc = jw.tables_from_lengths({4: list(range(12))})
    ac = jw.tables_from_lengths({8: [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]})
    return jw.write_jpeg(case.decoded, case.size, case.sampling, QT, {0: dc, 1: dc}, {0: ac, 1: ac}, sel=[(0, 0, 0), (1, 1, 1), (1, 1, 1)][:nc])


def _pillow_progressive_files():
    """(name, bytes, (H, W)): Pillow's own progressive files over samplings and restart options."""
    rng = np.random.default_rng(77)
    out = []
    for (H, W) in [(24, 40), (33, 47)]:
        for (mode, sub) in SUBSAMPLING.items():
            for extra in ({}, {'restart_marker_blocks': 3}, {'restart_marker_rows': 1}, {'optimize': True}):
                img = _natural_image(rng, H, W)
                kw = dict(quality=90, progressive=True, **extra)
                data = _encode(np.ascontiguousarray(img[..., 1]), **kw) if sub is None else _encode(img, subsampling=sub, **kw)
                out.append(('%s-%dx%d-%s' % (mode, H, W, sorted(extra)), data, (H, W)))
    return out


# ------------------------------------------------------------------ CPU: the probe ----
def test_probe_flags_takes_pillows_progressive_files():
    from meterelf_amd import _hip
    files = _pillow_progressive_files()
    for (name, data, (H, W)) in files:
        assert _hip.jpeg_probe_flags(data, TAKE_PROG) == (H, W, 1, True, ''), name
        assert _hip.jpeg_probe_flags(data, TAKE_PROG | TAKE_ORIENT) == (H, W, 1, True, ''), name
        (h0, w0, ok0, why0) = _hip.jpeg_probe(data)
        assert (h0, w0, ok0) == (H, W, False) and 'progressive' in why0, name
        (h1, w1, o1, ok1, why1) = _hip.jpeg_probe_flags(data, 0)
        assert (h1, w1, o1, ok1) == (H, W, 1, False) and 'progressive' in why1, name
    # with an orientation tag: each switch alone is not enough
    tagged = jc.encode(jc.natural(24, 40), 6, quality=90, progressive=True)
    assert _hip.jpeg_probe_flags(tagged, TAKE_PROG | TAKE_ORIENT)[:4] == (24, 40, 6, True)
    (H, W, o, ok, why) = _hip.jpeg_probe_flags(tagged, TAKE_PROG)
    assert (H, W, o, ok) == (24, 40, 6, False) and 'EXIF' in why
    (H, W, o, ok, why) = _hip.jpeg_probe_flags(tagged, TAKE_ORIENT)
    assert (H, W, o, ok) == (24, 40, 6, False) and 'progressive' in why
    # the batch form: the same answers
    datas = [d for (_n, d, _s) in files] + [tagged, b'junk']
    (hs, ws, os_, oks) = _hip.jpeg_probe_flags_batch(datas, TAKE_PROG)
    assert list(oks) == [1] * len(files) + [0, 0] and list(os_) == [1] * len(files) + [6, 1]
    assert [(int(h), int(w)) for (h, w) in zip(hs, ws)][:len(files)] == [s for (_n, _d, s) in files]
    assert {'melf_jpeg_probe_flags', 'melf_jpeg_probe_flags_batch', 'melf_ctx_set_jpeg_progressive', 'melf_ctx_get_jpeg_progressive'} <= set(_hip.EXPORTS)


def test_probe_flags_zero_is_the_oriented_probe_on_the_stream_cases():
    from meterelf_amd import _hip
    from tests import test_jpeg_streams as ts
    cases = ts._equality_cases() + ts._refusal_cases()
    assert len(cases) > 100
    for case in cases:
        assert _hip.jpeg_probe_flags(case.data, 0) == _hip.jpeg_probe_oriented(case.data), case.name
        (H, W, ok, why) = _hip.jpeg_probe(case.data)
        assert _hip.jpeg_probe_flags(case.data, 0) == (H, W, 1, ok, why), case.name
        # a baseline file is judged alike whatever is taken
        assert _hip.jpeg_probe_flags(case.data, TAKE_PROG)[:4] == (H, W, 1, ok), case.name


def test_reader_switch_is_off_by_default():
    import inspect

    from meterelf_amd import MeterReader
    assert inspect.signature(MeterReader.__init__).parameters['jpeg_progressive'].default is False
    hdr = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    assert '#define MELF_JPEG_PROG_SCANS_MAX 32' in hdr and 'MELF_JPEG_TAKE_ORIENTED = 1' in hdr and 'MELF_JPEG_TAKE_PROGRESSIVE = 2' in hdr


# ------------------------------------------------------------------ CPU: the writer against the reference ----
def test_writer_files_decode_like_the_baseline_file_of_the_same_grids():
    """The condition that makes the writer a source of test inputs: Pillow decodes every case's progressive file to exactly the
    pixels it decodes from jpeg_writer's baseline file of the same coefficient grids."""
    for case in _cases():
        assert np.array_equal(_pillow_bgr(case.data), _pillow_bgr(_baseline_of(case))), case.name


def test_cases_hold_what_they_claim():
    from meterelf_amd import _hip
    by = {c.name: c for c in _cases()}
    for c in _cases():
        (H, W, o, ok, why) = _hip.jpeg_probe_flags(c.data, TAKE_PROG)
        assert (H, W, o, ok, why) == (c.size[0], c.size[1], 1, True, ''), (c.name, why)
        assert len(c.script) <= 32
    assert by['eob-runs'].stats['eob_categories'] == set(range(7))
    assert len(by['bands-31-420-24x40'].script) == 31 and len(by['bands-32-grey-16x16'].script) == 32
    h = by['history-420-33x47'].stats
    assert h['zrl_over_history'] > 0 and h['new_after_15'] > 0 and h['zrl_refine'] > 0
    # every scan defines the ids it uses anew: one id with different code lengths in two scans
    specs = by['successive-420-24x40'].stats['specs']
    assert len({tuple(t[('ac', 0)][0]) for t in specs if ('ac', 0) in t}) > 1
    assert any(('ac', 3) in t for t in by['ids-2-3-420-24x40'].stats['specs']) and any(('dc', 2) in t for t in by['ids-2-3-420-24x40'].stats['specs'])
    # a restart interval that does not divide the scan's block count: 24 x 40 in 4:2:0 has 15 luma and 6 chroma blocks
    assert pw.real_blocks((24, 40), '420') == [(3, 5), (2, 3), (2, 3)]


# ------------------------------------------------------------------ CPU: refusals ----
def _refusals():
    rng = np.random.default_rng(5)
    (size, sampling) = ((24, 40), '420')
    coefs = _coefs(rng, size, sampling)
    good = _script_successive(3)
    w = lambda script, **kw: pw.write_progressive(coefs, size, sampling, QT, script, check=False, **kw)   # noqa: E731
    luma_left_at_1 = [s for s in pw.PILLOW_COLOUR if not (s[0] == (0,) and s[3] == 1 and s[1] == 1)] + [((0,), 1, 5, 1, 0)]
    return [
        ('luma 6..63 left at Al = 1', w(luma_left_at_1), 'incomplete'),
        ('cut after the fifth scan', w(pw.PILLOW_COLOUR[:5]), 'incomplete'),
        ('33 scans', w(_script_bands_of_one(3, 33)), 'MELF_JPEG_PROG_SCANS_MAX'),
        ('Al = Ah - 2', w([((0, 1, 2), 0, 0, 0, 3), ((0, 1, 2), 0, 0, 3, 1)] + good[1:]), 'Al is not Ah - 1'),
        ('AC before DC', w([((0,), 1, 63, 0, 0)] + _script_spectral(3)), "before the component's first DC scan"),
        ('Ss = 0, Se = 5', w([((0,), 0, 5, 0, 0)] + _script_spectral(3)), 'band is not DC alone'),
        ('DQT after the first SOS', w(_script_spectral(3), dqt_after_first_sos=True), 'quantisation table defined after the first scan'),
        ('SOF10', w(_script_spectral(3), sof=0xCA), 'progressive / lossless / arithmetic'),
        ('a band sent twice', w(_script_spectral(3) + [((1,), 1, 5, 0, 0)]), 'already sent'),
    ] + [('SOF0 behind the first scan, ' + name, _with_second_sof(w(_script_spectral(3)), sampling_bytes), 'second frame header')
         for (name, sampling_bytes) in (('luma 0x1', (0x01, 0x11, 0x11)), ('luma 4x4', (0x44, 0x11, 0x11)), ('chroma 2x2', (0x22, 0x22, 0x22)),
                                        ('the same frame again', (0x22, 0x11, 0x11)))]


def _with_second_sof(data, sampling_bytes, marker=0xC0):
    """data with a frame header of 24 x 40, three components of the given sampling bytes, between its first scan and what follows."""
    (_a, e) = _scan_ranges(data)[0]
    f = bytes([8, 0, 24, 0, 40, 3]) + b''.join(bytes([c + 1, sampling_bytes[c], min(c, 1)]) for c in range(3))
    return data[:e] + jw._segment(marker, f) + data[e:]


def test_refusals_name_the_rule():
    from meterelf_amd import _hip
    for (name, data, reason) in _refusals():
        (H, W, o, ok, why) = _hip.jpeg_probe_flags(data, TAKE_PROG)
        assert not ok and reason in why and (H, W) == (24, 40), (name, why)
    # the luma-left-at-1 script is what it says: Pillow's script with the last luma refinement narrowed to 1..5
    assert _hip.jpeg_probe_flags(pw.write_progressive(_coefs(np.random.default_rng(5), (24, 40), '420'), (24, 40), '420', QT, pw.PILLOW_COLOUR),
                                 TAKE_PROG)[3]


def test_a_table_marker_turned_into_a_frame_marker_is_refused():
    """One byte of damage the random flips rarely make: the C4 of a DHT between two scans read as C0, C1 or C2 -- a second frame
    header whose 'sampling factors' are table bytes.  Never taken, never a crash."""
    from meterelf_amd import _hip
    for base in (_cases()[2].data, _pillow_progressive_files()[9][1]):
        first_sos = base.index(b'\xff\xda')
        marks = [i for i in range(first_sos, len(base) - 1) if base[i] == 0xFF and base[i + 1] == 0xC4]
        assert len(marks) >= 3
        for m in marks:
            for sof in (0xC0, 0xC1, 0xC2, 0xC9):
                b = bytearray(base)
                b[m + 1] = sof
                (H, W, o, ok, why) = _hip.jpeg_probe_flags(bytes(b), TAKE_PROG)
                assert not ok and (why or H == 0), (m, sof, why)


def test_get_meter_values_leaves_progressive_files_to_the_host_unless_asked(monkeypatch):
    from meterelf_amd import _api

    class Reader:
        jpeg_progressive = False
        jpeg_orientation = False

        def set_jpeg_progressive(self, on):
            self.jpeg_progressive = bool(on)

        def set_jpeg_orientation(self, on):
            self.jpeg_orientation = bool(on)
    monkeypatch.delenv('METERELF_JPEG_PROGRESSIVE', raising=False)
    assert not _api._jpeg_on_gpu('jpeg_progressive') and not _api._with_jpeg_orientation(Reader()).jpeg_progressive
    monkeypatch.setenv('METERELF_JPEG_PROGRESSIVE', 'host')
    assert not _api._with_jpeg_orientation(Reader()).jpeg_progressive
    monkeypatch.setenv('METERELF_JPEG_PROGRESSIVE', 'gpu')
    assert _api._jpeg_on_gpu('jpeg_progressive') and _api._with_jpeg_orientation(Reader()).jpeg_progressive


def test_probe_survives_mutated_progressive_headers():
    """Truncations and byte flips of a progressive file's headers (the segments between its scans included) only ever answer no --
    or yes: the parser is a pure function of the bytes and never reads outside them."""
    from meterelf_amd import _hip
    rng = np.random.default_rng(991)
    for base in (_cases()[2].data, _pillow_progressive_files()[9][1]):
        # where the header segments are: the file's start, and every DHT / SOS between the scans
        marks = [i for i in range(len(base) - 1) if base[i] == 0xFF and base[i + 1] in (0xC4, 0xDA, 0xDD, 0xC2, 0xDB)]
        spots = sorted({p for m in marks for p in range(m, min(m + 40, len(base)))})
        for cut in list(range(0, min(len(base), 900), 5)) + [len(base) - 1, len(base) - 2]:
            r = _hip.jpeg_probe_flags(base[:cut] if cut else b'\xff', TAKE_PROG)
            assert isinstance(r[3], bool) and (r[3] is False or cut >= len(base) - 2)
        for _ in range(3000):
            b = bytearray(base)
            for _k in range(int(rng.integers(1, 6))):
                b[spots[int(rng.integers(0, len(spots)))]] = int(rng.integers(0, 256))
            r = _hip.jpeg_probe_flags(bytes(b), TAKE_PROG)
            assert isinstance(r[3], bool) and (r[3] or r[4])
            # bytes exactly to the end of an allocation of their own
            arr = np.frombuffer(bytes(b), np.uint8).copy()
            assert _hip.jpeg_probe_flags(arr, TAKE_PROG)[:4] == r[:4]


# ------------------------------------------------------------------ CPU: the decoder body on the host ----
def _scan_ranges(data):
    """[begin, end) of the entropy-coded bytes of every scan of a file."""
    out = []
    i = 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF
        (m, L) = (data[i + 1], (data[i + 2] << 8) | data[i + 3])
        if m == 0xD9:
            break
        i += 2 + L
        if m == 0xDA:
            j = i
            while not (data[j] == 0xFF and data[j + 1] not in (0x00, 0xFF) and not 0xD0 <= data[j + 1] <= 0xD7):
                j += 1
            out.append((i, j))
            i = j
    return out


@functools.lru_cache(None)
def _damaged(n_per=6, seed=4711):
    """[(case, bytes)], made ONCE and used by the host program's test and by the GPU test alike: copies of the case files damaged
    INSIDE their scans: one to three entropy-coded bytes replaced (never an FF, the byte behind
    one, or by an FF: the markers, the stuffing and so the scans' extents stay, what changes is what the decoder reads in them), or
    the file cut inside a scan.  Such a file is still one the parser takes, or one whose bytes end inside a scan: status 0 or 2."""
    rng = np.random.default_rng(seed)
    out = []
    for c in _cases():
        ranges = _scan_ranges(c.data)
        spots = [i for (a, e) in ranges for i in range(a, e) if c.data[i] != 0xFF and c.data[i - 1] != 0xFF]
        assert len(ranges) == len(c.script) and spots
        for k in range(n_per):
            b = bytearray(c.data)
            if k % 3 == 2:
                (a, e) = ranges[int(rng.integers(0, len(ranges)))]
                b = b[:int(rng.integers(a, e + 1))]
            else:
                for _ in range(int(rng.integers(1, 4))):
                    b[spots[int(rng.integers(0, len(spots)))]] = int(rng.integers(0, 255))
            out.append((c, bytes(b)))
    return out


ROCM_CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _build_host_program(tmp_path):
    """jpeg_prog_main.cpp with the ROCm clang++ (or $CXX; g++ where there is neither), plain and under the host sanitizers, each with
    the header's plain host paths and with the GPU build's paths (-DMELF_JP_HOST_STAGED)."""
    cxx = os.environ.get('CXX') or (ROCM_CLANG if os.path.exists(ROCM_CLANG) else 'g++')
    src = os.path.join(ROOT, 'tests', 'jpeg_prog_main.cpp')
    exes = {}
    for (tag, flags) in (('plain', ['-O2']), ('san', ['-O1', '-g', '-fno-sanitize-recover=all', '-fsanitize=address,undefined'])):
        for (kind, define) in (('', []), ('_staged', ['-DMELF_JP_HOST_STAGED'])):
            exes[tag + kind] = os.path.join(str(tmp_path), 'jpeg_prog_' + tag + kind)
            subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror'] + flags + define + ['-o', exes[tag + kind], src])
    return exes


def _run_host_program(exe, manifest):
    env = {k: v for (k, v) in os.environ.items() if k != 'LD_PRELOAD'}
    p = subprocess.run([exe, manifest], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    return (p.returncode, p.stdout.decode(), p.stderr.decode())


@functools.lru_cache(None)
def _host_program_verdict():
    """Builds the host program and runs it on every script case, on Pillow's files and on the damaged list, in all four builds; what
    each run answered.  Made once: the GPU test of the damaged files asks for it before it sends them anywhere."""
    import tempfile
    tmp = tempfile.mkdtemp(prefix='jpeg_prog_')
    exes = _build_host_program(tmp)
    lines = []
    for (k, c) in enumerate(_cases()):
        (fj, fe) = (os.path.join(tmp, 'c%03d.jpg' % k), os.path.join(tmp, 'c%03d.i16' % k))
        open(fj, 'wb').write(c.data)
        _area_order(c.decoded, c.size, c.sampling).tofile(fe)
        lines.append('%s %s' % (fj, fe))
    for (k, (_n, data, _s)) in enumerate(_pillow_progressive_files()):
        fj = os.path.join(tmp, 'p%03d.jpg' % k)
        open(fj, 'wb').write(data)
        lines.append('%s -' % fj)
    good = os.path.join(tmp, 'good.txt')
    open(good, 'w').write('\n'.join(lines) + '\n')
    dl = []
    for (k, (_c, data)) in enumerate(_damaged()):
        fj = os.path.join(tmp, 'd%03d.jpg' % k)
        open(fj, 'wb').write(data)
        dl.append('%s -' % fj)
    bad = os.path.join(tmp, 'damaged.txt')
    open(bad, 'w').write('\n'.join(dl) + '\n')
    out = {}
    for tag in sorted(exes):
        out[tag] = (_run_host_program(exes[tag], good), _run_host_program(exes[tag], bad))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    return (len(lines), out)


def _assert_host_program_clean():
    (ngood, verdict) = _host_program_verdict()
    ndam = len(_damaged())
    assert ndam >= 300 and set(verdict) == {'plain', 'plain_staged', 'san', 'san_staged'}
    answers = set()
    for (tag, ((rc, out, err), (rcd, outd, errd))) in verdict.items():
        assert rc == 0 and err == '', (tag, out[-3000:], err[-3000:])
        assert out.splitlines()[-1] == 'files %d, ok %d, corrupt 0, mismatches 0' % (ngood, ngood), (tag, out[-2000:])
        assert rcd == 0 and errd == '', (tag, outd[-3000:], errd[-3000:])
        last = outd.splitlines()[-1].replace(',', '').split()
        (files, ok, corrupt) = (int(last[1]), int(last[3]), int(last[5]))
        assert files == ndam and ok + corrupt == files and corrupt > files // 4, (tag, last)     # not vacuous: damage was seen
        answers.add(tuple(ln.split()[-1] for ln in outd.splitlines()[:-1]))
    assert len(answers) == 1      # the plain and the staged paths, with and without sanitizers, answer alike file by file


def test_decoder_body_on_the_host():
    """melf_jpeg_prog.h compiled alone, plain and under the host sanitizers, with its plain host paths and with the GPU build's paths
    (16-byte stream lines, staged AC refinement blocks) on buffers sized as the library sizes them: every script case decodes to
    exactly the writer's grids (in the decoder's block order), Pillow's files decode, and on the damaged copies the decoder
    terminates with 'corrupt' or 'ok'."""
    _assert_host_program_clean()


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope='module')
def reader():
    from meterelf_amd import _hip
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    r = MeterReader(_params.load(PFILE), jpeg_progressive=True)
    assert r.ctx.jpeg_progressive() and r.jpeg_progressive and not r.ctx.jpeg_orientation()
    yield r
    r.close()


def _assert_frames_equal_pillow(ctx, files):
    by_size = {}
    for (name, data, size) in files:
        by_size.setdefault(size, []).append((name, data))
    for ((H, W), group) in by_size.items():
        (frames, status) = ctx.jpeg_decode([d for (_n, d) in group], H, W)
        for ((name, data), got, st) in zip(group, frames, status):
            ref = _pillow_bgr(data)
            assert st == 0, (name, int(st))
            assert np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:3])


@pytest.mark.gpu
@pytest.mark.parametrize('quality', [50, 90, 100])
def test_pillow_progressive_files_decode_like_pillow(reader, quality):
    rng = np.random.default_rng(1000 + quality)
    files = []
    for (H, W) in [(24, 40), (33, 47), (1, 1), (9, 1), (16, 17), (96, 128)]:
        for (mode, sub) in SUBSAMPLING.items():
            for extra in ({}, {'restart_marker_blocks': 3}, {'restart_marker_rows': 1}, {'optimize': True}):
                img = _natural_image(rng, H, W)
                kw = dict(quality=quality, progressive=True, **extra)
                data = _encode(np.ascontiguousarray(img[..., 1]), **kw) if sub is None else _encode(img, subsampling=sub, **kw)
                files.append(('%s-%dx%d-%s' % (mode, H, W, sorted(extra)), data, (H, W)))
    _assert_frames_equal_pillow(reader.ctx, files)


@pytest.mark.gpu
def test_writer_script_cases_decode_like_pillow(reader):
    _assert_frames_equal_pillow(reader.ctx, [(c.name, c.data, c.size) for c in _cases()])


def _fixture_files(n):
    from PIL import Image
    src = []
    for f in jc.golden_files():
        with Image.open(f) as im:
            src.append((f, im.size))
    size = max(set(s for (_, s) in src), key=[s for (_, s) in src].count)
    return ([f for (f, s) in src if s == size][:n], (size[1], size[0]))


def _resave(path, **kw):
    from PIL import Image
    buf = io.BytesIO()
    with Image.open(path) as im:
        im.save(buf, 'JPEG', quality=95, progressive=True, **kw)
    return buf.getvalue()


@functools.lru_cache(None)
def _mixed_list():
    """About 200 files at the fixtures' size and what each must come back as: (bytes, status with both switches on, progressive?)."""
    (src, (H, W)) = _fixture_files(66)
    rng = np.random.default_rng(31)
    items = []
    for (k, f) in enumerate(src):
        items.append((open(f, 'rb').read(), 0, False))
        items.append((_resave(f), 0, True))
        items.append((_resave(f, restart_marker_rows=1) if k % 2 else _resave(f, restart_marker_blocks=40), 0, True))
    items.insert(20, (jc.stored_under(src[3], 6, quality=95, progressive=True), 0, True))
    items.insert(90, (jc.stored_under(src[4], 3, quality=95, progressive=True), 0, True))
    items.insert(130, (_encode(_natural_image(rng, 48, 64), progressive=True), 3, True))
    whole = _resave(src[5])
    sos = [i for i in range(len(whole) - 1) if whole[i] == 0xFF and whole[i + 1] == 0xDA]
    items.insert(60, (whole[:(sos[3] + sos[4]) // 2], 2, True))          # truncated in its fourth scan
    from PIL import Image
    buf = io.BytesIO()
    with Image.open(src[6]) as im:
        im.convert('L').save(buf, 'JPEG', quality=95, progressive=True)
    items.insert(170, (buf.getvalue(), 0, True))
    return (items, (H, W))


def _host_records(reader, datas):
    """The reader's records on the host decoder's frames (Pillow + exif_transpose), one call."""
    from PIL import Image, ImageOps
    frames = []
    for d in datas:
        with Image.open(io.BytesIO(d)) as im:
            frames.append(np.ascontiguousarray(np.asarray(ImageOps.exif_transpose(im).convert('RGB'), np.uint8)[:, :, ::-1]))
    return reader.read_frames(np.stack(frames))


@pytest.mark.gpu
def test_mixed_call_in_every_chunking_and_with_the_switch_off(reader, monkeypatch):
    (items, (H, W)) = _mixed_list()
    datas = [d for (d, _s, _p) in items]
    want = np.array([s for (_d, s, _p) in items])
    good = np.flatnonzero(want == 0)
    ref = _host_records(reader, [datas[i] for i in good])
    reader.set_jpeg_orientation(True)
    try:
        for chunk in ('', '64,300', '40'):
            if chunk:
                monkeypatch.setenv('MELF_JPEG_CHUNK', chunk)
            else:
                monkeypatch.delenv('MELF_JPEG_CHUNK', raising=False)
            for _twice in range(2):
                (recs, status) = reader.ctx.jpeg_process_batch(datas, H, W)
                assert list(status) == list(want), (chunk, np.flatnonzero(status != want), status[status != want])
                assert recs[good].tobytes() == ref.tobytes(), (chunk, [int(i) for (k, i) in enumerate(good) if recs[i].tobytes() != ref[k].tobytes()])
        # the progressive switch off: those files are the host's, everything else is as it was
        reader.set_jpeg_progressive(False)
        monkeypatch.delenv('MELF_JPEG_CHUNK', raising=False)
        (recs, status) = reader.ctx.jpeg_process_batch(datas, H, W)
        prog = np.array([p for (_d, _s, p) in items])
        assert (status[prog] == 1).all() and (status[~prog] == 0).all()
        keep = np.flatnonzero(~prog)
        pos = {int(i): k for (k, i) in enumerate(good)}
        assert recs[keep].tobytes() == ref[[pos[int(i)] for i in keep]].tobytes()
    finally:
        reader.set_jpeg_progressive(True)
        reader.set_jpeg_orientation(False)


@pytest.mark.gpu
def test_file_name_calls_and_get_meter_values(reader, tmp_path, monkeypatch):
    import meterelf_amd
    from meterelf_amd import _api, _hip
    (src, (H, W)) = _fixture_files(30)
    paths = []
    for (k, f) in enumerate(src[:12]):
        p = str(tmp_path / ('prog%02d.jpg' % k))
        open(p, 'wb').write(_resave(f, **({'restart_marker_rows': 2} if k % 3 == 0 else {})))
        paths.append(p)
    ref = _host_records(reader, [open(p, 'rb').read() for p in paths])
    (recs, status, hw) = reader.ctx.jpeg_process_files(paths)
    assert hw == (H, W) and (status == _hip.JPEG_OK).all(), (hw, status)
    assert recs.tobytes() == ref.tobytes()
    reader.ctx.jpeg_process_files_begin(paths[:7])
    reader.ctx.jpeg_process_files_begin(paths[7:])
    with pytest.raises(Exception):
        reader.ctx.set_jpeg_progressive(False)       # not while a _begin call is in flight
    (ra, sa, _hwa) = reader.ctx.jpeg_process_files_end()
    (rb, sb, _hwb) = reader.ctx.jpeg_process_files_end()
    assert (sa == 0).all() and (sb == 0).all() and ra.tobytes() + rb.tobytes() == ref.tobytes()
    got = reader.read_jpeg_files([open(p, 'rb').read() for p in paths[:5]])
    assert all(g is not None and g.tobytes() == r.tobytes() for (g, r) in zip(got, ref[:5]))
    # get_meter_values over a list mixing them with baseline fixtures: the values of the host branch, and no host decode
    mixed = [x for pair in zip(paths, src[12:24]) for x in pair]
    monkeypatch.setenv('METERELF_CTX_CACHE', '0')
    monkeypatch.setenv('METERELF_JPEG_PROGRESSIVE', 'host')
    host = list(meterelf_amd.get_meter_values(PFILE, mixed))
    monkeypatch.setenv('METERELF_JPEG_PROGRESSIVE', 'gpu')
    decoded_on_host = []
    real = _api.ImageFile.get_frame

    def spy(self):
        decoded_on_host.append(self.filename)
        return real(self)
    monkeypatch.setattr(_api.ImageFile, 'get_frame', spy)
    got = list(meterelf_amd.get_meter_values(PFILE, mixed))
    assert decoded_on_host == []
    assert [g.filename for g in got] == mixed
    for (g, h) in zip(got, host):
        assert g.meter_values == h.meter_values and g.value == h.value and (g.error is None) == (h.error is None)
    assert sum(g.error is None for g in got) * 4 >= 3 * len(got)


@pytest.mark.gpu
def test_damaged_files_come_back_corrupt_or_decoded(reader):
    """The very damaged copies the host program ran on (_damaged(): one list, made once), once through jpeg_decode, and only after
    that program was clean on them in all its builds: the call returns, every file is 0 (decoded) or 2 (corrupt), and a good file
    in the same call still equals Pillow.  This asserts the error reporting; it searches for nothing."""
    _assert_host_program_clean()
    by_size = {}
    for (c, data) in _damaged():
        by_size.setdefault(c.size, (c, []))[1].append(data)
    assert sum(len(v[1]) for v in by_size.values()) == len(_damaged())
    for ((H, W), (first, datas)) in by_size.items():
        (frames, status) = reader.ctx.jpeg_decode(datas + [first.data], H, W)
        assert set(int(s) for s in status[:-1]) <= {0, 2}, status
        assert status[-1] == 0 and np.array_equal(frames[-1], _pillow_bgr(first.data))
        assert all((frames[k] == 0).all() for k in np.flatnonzero(status[:-1] != 0)[:20])
