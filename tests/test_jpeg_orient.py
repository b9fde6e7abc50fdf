"""JPEG files that carry an EXIF orientation, decoded and read on the GPU (melf_ctx_set_jpeg_orientation, k_jpeg_color_exif).

The reference never comes from the GPU (tests/jpeg_orient_cases.py): a frame is Pillow's decode of the same bytes permuted in numpy by
the orientation table of include/meterelf_hip.h -- decode first, permute afterwards, as cv2.imread does --, a record is the reader's on
the frame the host decoder (imread_bgr: Pillow + exif_transpose) returns.  Bar: every byte of every frame and of every record.

CPU part: the probe that takes the tag, the window of the stored frame (melf_jpeg_orient_addr.h swept by jpeg_orient_window_main.cpp),
and get_meter_values' switch with stand-in readers.  GPU part: whole frames over codes x samplings x sizes, mixed batches, restart
intervals and the 1024-lane Huffman kernel, the full path through both library paths and the file-name calls, windows at the frame's
edges, get_meter_values.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import frame_cases as fc  # noqa: E402
from tests import jpeg_orient_cases as jc  # noqa: E402

GOLDEN = jc.GOLDEN
PFILE = os.path.join(GOLDEN, 'sample-images1', 'params.yml')


# ------------------------------------------------------------------ CPU: probe ----
def test_probe_oriented_returns_the_code_and_the_stored_size():
    from meterelf_amd import _hip
    img = jc.natural(24, 40)
    plain = jc.encode(img, None, quality=90)                       # no APP1 at all
    assert _hip.jpeg_probe_oriented(plain)[:4] == (24, 40, 1, True)
    for code in jc.CODES:
        for data in (jc.encode(img, code, quality=90), jc.with_app1(plain, jc.tiff_block(code, False)), jc.with_app1(plain, jc.tiff_block(code, True))):
            (H, W, o, ok, why) = _hip.jpeg_probe_oriented(data)
            assert (H, W, o, ok, why) == (24, 40, code, True, ''), (code, H, W, o, ok, why)
            # the old probe's answer does not change: a tag above 1 is unsupported there
            (H1, W1, ok1, why1) = _hip.jpeg_probe(data)
            assert (H1, W1) == (24, 40) and ok1 == (code == 1) and (ok1 or 'EXIF' in why1)
    for bad in (0, 9, 65535):                                      # outside 1..8: left alone, as Pillow and cv2 leave it
        for be in (False, True):
            assert _hip.jpeg_probe_oriented(jc.with_app1(plain, jc.tiff_block(bad, be)))[:4] == (24, 40, 1, True), (bad, be)
    for junk in (b'II\x2a\x00', b'XX' + jc.tiff_block(6, False)[2:], jc.tiff_block(6, False)[:14]):   # unreadable TIFF blocks
        assert _hip.jpeg_probe_oriented(jc.with_app1(plain, junk))[:4] == (24, 40, 1, True)
    # progressive: not for the decoder, with or without a tag; the code is still reported
    (H, W, o, ok, why) = _hip.jpeg_probe_oriented(jc.encode(img, 6, quality=90, progressive=True))
    assert (H, W, o, ok) == (24, 40, 6, False) and 'progressive' in why
    assert _hip.jpeg_probe_oriented(b'not a jpeg at all')[2:4] == (1, False)
    # the batch form: the same answers
    files = [jc.encode(img, code, quality=90) for code in jc.CODES] + [plain, b'junk']
    (hs, ws, os_, oks) = _hip.jpeg_probe_oriented_batch(files)
    assert list(os_) == list(jc.CODES) + [1, 1] and list(oks) == [1] * 9 + [0] and list(hs[:9]) == [24] * 9 and list(ws[:9]) == [40] * 9


def test_orientation_table_of_the_test_support():
    """tests/jpeg_orient_cases.orient against Pillow's own transposition (what imread_bgr applies): the reference of every GPU test."""
    import io

    from PIL import Image, ImageOps
    img = jc.natural(13, 17)
    for code in jc.CODES:
        im = Image.open(io.BytesIO(jc.encode(img, code, quality=100, subsampling='4:4:4')))
        stored = np.asarray(im.convert('RGB'))
        up = np.asarray(ImageOps.exif_transpose(im).convert('RGB'))
        assert np.array_equal(jc.orient(stored, code), up), code
        assert np.array_equal(jc.orient(jc.unorient(img, code), code), img), code


# ------------------------------------------------------------------ CPU: the window ----
def test_stored_window_sweep(tmp_path):
    """melf_jpeg_orient_addr.h on the host, plain and under the host sanitizers: for every code, stored size 1..40 x 1..40 and rectangle
    of a coarse grid the window lies in the stored frame, starts on a multiple of 16, holds the rectangle's stored pixels and 16 more
    on every side that is no frame edge (and at most the alignment's 15 beyond that); code 1 is the upright rule to the pixel."""
    out = fc.build_and_run(tmp_path, os.environ.get('CXX', 'g++'), os.path.join(ROOT, 'tests', 'jpeg_orient_window_main.cpp'), 'jpeg_orient_window',
                           [], ['-fsanitize=address,undefined'])
    lines = out.splitlines()
    assert lines[-1] == 'failures 0', lines[-5:]
    (cases, whole) = (int(lines[-2].split()[1].rstrip(',')), int(lines[-2].split()[-1]))
    assert cases > 1000000 and 0 < whole < cases     # not vacuous: windows smaller than the frame were seen too


# ------------------------------------------------------------------ CPU: get_meter_values' switch ----
class _SwitchReader:
    """A CPU stand-in that takes no file on the 'GPU' (everything goes through the host branch) and records the switch."""
    made = []

    def __init__(self, params, device=0, blob=None, ctx=None):
        self.dial_names = params.dial_names
        self.jpeg_orientation = False
        self.asked = []
        self.ctx = None
        _SwitchReader.made.append(self)

    def set_jpeg_orientation(self, on):
        self.asked.append(bool(on))
        self.jpeg_orientation = bool(on)

    def close(self):
        pass

    def read_jpeg_paths(self, paths):
        return [None] * len(paths)

    def read_many(self, images, cropped=None):
        from meterelf_amd import _hip
        return list(np.zeros(len(images), _hip.RESULT_DTYPE))


def test_get_meter_values_asks_for_the_switch(tmp_path, monkeypatch):
    from PIL import Image

    from meterelf_amd import _api, _engine, _params
    f = str(tmp_path / 'a.png')
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(f)
    monkeypatch.setattr(_api, 'MeterReader', _SwitchReader)
    del _SwitchReader.made[:]
    monkeypatch.delenv('METERELF_JPEG_ORIENT', raising=False)
    assert len(list(_api.get_meter_values(PFILE, [f]))) == 1
    assert [r.asked for r in _SwitchReader.made] == [[True]]
    monkeypatch.setenv('METERELF_JPEG_ORIENT', 'host')
    assert len(list(_api.get_meter_values(PFILE, [f]))) == 1
    assert [r.asked for r in _SwitchReader.made] == [[True], []]
    # the fan-out's workers make their readers the same way
    monkeypatch.setenv('METERELF_DEVICES', '0,0')
    monkeypatch.delenv('METERELF_JPEG_ORIENT', raising=False)
    del _SwitchReader.made[:]
    assert len(list(_api.get_meter_values(PFILE, [f, f, f]))) == 3
    assert _SwitchReader.made and all(r.asked == [True] for r in _SwitchReader.made)
    # the cache: a reader made under one setting is never handed out under the other
    params = _params.load(PFILE)
    blob = _engine.make_blob(params)
    monkeypatch.delenv('METERELF_JPEG_ORIENT', raising=False)
    k_gpu = _api._reader_key(params, blob, 0)
    monkeypatch.setenv('METERELF_JPEG_ORIENT', 'host')
    k_host = _api._reader_key(params, blob, 0)
    monkeypatch.setenv('METERELF_JPEG_ORIENT', 'gpu')
    assert k_gpu != k_host and _api._reader_key(params, blob, 0) == k_gpu
    # ... also through _acquire_reader / _release_reader, with the stand-in as "the real reader"
    monkeypatch.setattr(_api, '_REAL_READER', _SwitchReader)
    monkeypatch.setattr(_api, '_idle_readers', {})
    r_gpu = _api._acquire_reader(params, 0)
    assert r_gpu.asked == [True]
    _api._release_reader(r_gpu)
    monkeypatch.setenv('METERELF_JPEG_ORIENT', 'host')
    r_host = _api._acquire_reader(params, 0)
    assert r_host is not r_gpu and r_host.asked == []
    _api._release_reader(r_host)
    monkeypatch.setenv('METERELF_JPEG_ORIENT', 'gpu')
    assert _api._acquire_reader(params, 0) is r_gpu and r_gpu.asked == [True]
    monkeypatch.setattr(_api, '_idle_readers', {})


def test_reader_switch_is_off_by_default():
    """MeterReader's signature: jpeg_orientation=False (no GPU: the signature alone)."""
    import inspect

    from meterelf_amd import MeterReader, _hip
    assert inspect.signature(MeterReader.__init__).parameters['jpeg_orientation'].default is False
    assert {'melf_jpeg_probe_oriented', 'melf_ctx_set_jpeg_orientation', 'melf_ctx_get_jpeg_orientation'} <= set(_hip.EXPORTS)


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope='module')
def reader():
    from meterelf_amd import _hip
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    from meterelf_amd import MeterReader, _params
    r = MeterReader(_params.load(PFILE), jpeg_orientation=True)
    assert r.ctx.jpeg_orientation() and r.jpeg_orientation
    yield r
    r.close()


MODES = {'grey': None, '4:4:4': '4:4:4', '4:2:2': '4:2:2', '4:2:0': '4:2:0'}
# stored H x W: whole MCUs of every sampling; partial MCUs (and rows of 3 * 17 = 51 and 3 * 13 = 39 bytes: no dword alignment); one
# block; one pixel -- each in both axis orders, so that every code sees it as its stored AND as its upright size
SIZES = [(32, 48), (48, 32), (24, 40), (40, 24), (13, 17), (17, 13), (8, 8), (1, 1)]


def _encode_mode(img, code, mode, **kw):
    if MODES[mode] is None:
        return jc.encode(np.ascontiguousarray(img[..., 1]), code, **kw)
    return jc.encode(img, code, subsampling=MODES[mode], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', list(MODES))
def test_whole_frames_of_every_code_sampling_and_size(reader, mode):
    """melf_jpeg_decode_batch with the switch on: every code x size of one sampling, every frame byte-equal to Pillow's decode
    permuted by the table.  Files of one upright size share a call (codes 1-4 of H x W with codes 5-8 of W x H)."""
    from meterelf_amd import _hip
    groups = {}
    for (H, W) in SIZES:
        for code in jc.CODES:
            data = _encode_mode(jc.natural(H, W), code, mode, quality=90)
            assert _hip.jpeg_probe_oriented(data)[:4] == (H, W, code, True)
            groups.setdefault((W, H) if code >= 5 else (H, W), []).append((code, data))
    total = 0
    for ((Hu, Wu), items) in groups.items():
        (frames, status) = reader.ctx.jpeg_decode([d for (_, d) in items], Hu, Wu)
        assert (status == _hip.JPEG_OK).all(), (Hu, Wu, status)
        for ((code, d), got) in zip(items, frames):
            ref = jc.reference_frame(d, code)
            assert ref.shape == got.shape and np.array_equal(got, ref), (mode, Hu, Wu, code, int((got != ref).sum()), np.argwhere(got != ref)[:3])
            total += 1
    assert total == len(SIZES) * 8


@pytest.mark.gpu
def test_mixed_batch_in_one_call(reader):
    """All eight codes interleaved with upright files, not grouped by class, samplings mixed; one file of another upright size and one
    corrupt file.  Frames in the caller's order; with the switch OFF the same call gives what it always gave."""
    from meterelf_amd import _hip
    (H, W) = (32, 48)
    order = [6, 1, 3, None, 8, 2, 1, 5, 7, 4, None, 6, 3, 1, 8, 5, 2, 7, 4, 1]
    modes = list(MODES)
    files = []
    for (k, code) in enumerate(order):
        img = jc.natural(H, W) if (code or 1) < 5 else jc.natural(W, H)      # stored 48 x 32 for the transposing codes
        img = np.roll(img, 3 * k, axis=1)                                      # every file its own content
        files.append(_encode_mode(img, code, modes[k % 4], quality=85))
    other = len(files)
    files.append(jc.encode(jc.natural(24, 40), None, quality=85))             # another upright size, no tag
    corrupt = len(files)
    big = jc.encode(np.ascontiguousarray(jc.unorient(jc.natural(H, W), 6)), 6, quality=100, subsampling='4:4:4')
    files.append(big[:len(big) - len(big) // 3])                               # headers whole, the scan cut short
    files.append(_encode_mode(jc.natural(W, H), 6, '4:2:0', quality=85))
    codes = [c or 1 for c in order] + [1, 6, 6]
    (frames, status) = reader.ctx.jpeg_decode(files, H, W)
    want = np.zeros(len(files), np.int32)
    want[other] = _hip.JPEG_SIZE_MISMATCH
    want[corrupt] = _hip.JPEG_CORRUPT
    assert np.array_equal(status, want), status
    for (i, d) in enumerate(files):
        if want[i] == 0:
            ref = jc.reference_frame(d, codes[i])
            assert np.array_equal(frames[i], ref), (i, codes[i], int((frames[i] != ref).sum()))
    assert not frames[other].any()
    # the switch off: exactly the old statuses -- every tagged file unsupported --, and the upright files decode as ever
    reader.ctx.set_jpeg_orientation(False)
    try:
        (frames0, status0) = reader.ctx.jpeg_decode(files, H, W)
    finally:
        reader.ctx.set_jpeg_orientation(True)
    old = np.array([_hip.JPEG_UNSUPPORTED if c != 1 else _hip.JPEG_OK for c in codes], np.int32)
    old[other] = _hip.JPEG_SIZE_MISMATCH
    assert np.array_equal(status0, old), status0
    for (i, d) in enumerate(files):
        if old[i] == 0:
            assert np.array_equal(frames0[i], jc.pillow_bgr(d)), i
        else:
            assert not frames0[i].any(), i


@pytest.mark.gpu
def test_restart_intervals_and_the_1024_lane_huffman_kernel(reader):
    """k_jpeg_huff_rst under code 6 (restart intervals, Pillow writes them), and k_jpeg_huff<1024> under code 3: a 3.3 MB scan of
    noise at quality 100, the size tests/test_jpeg.py::test_long_scans uses for that kernel (a scan above 2 MB takes 1024 lanes)."""
    from meterelf_amd import _hip
    (H, W) = (120, 200)
    img = jc.natural(W, H)                                                     # stored 200 x 120, upright 120 x 200
    files = [jc.encode(img, 6, quality=80, subsampling='4:2:0', restart_marker_blocks=3),
             jc.encode(img, 6, quality=80, subsampling='4:4:4', restart_marker_rows=1),
             jc.encode(np.ascontiguousarray(img[..., 1]), 6, quality=60, restart_marker_blocks=5),
             jc.encode(jc.natural(H, W), 4, quality=70, subsampling='4:2:2', restart_marker_blocks=1),
             jc.encode(jc.natural(H, W), None, quality=70, subsampling='4:2:0', restart_marker_blocks=2)]
    assert all(b'\xff\xdd' in f for f in files)
    (frames, status) = reader.ctx.jpeg_decode(files, H, W)
    assert (status == _hip.JPEG_OK).all(), status
    for (d, code, got) in zip(files, (6, 6, 6, 4, 1), frames):
        assert np.array_equal(got, jc.reference_frame(d, code)), code
    rng = np.random.default_rng(77)
    (H, W) = (800, 1000)
    noise = jc.encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), 3, quality=100, subsampling='4:4:4')
    assert len(noise) > 2100000                                                # above half of what the kernel addresses: 1024 lanes
    small = jc.encode(jc.natural(H, W), 3, quality=60, subsampling='4:4:4')
    (frames, status) = reader.ctx.jpeg_decode([small, noise], H, W)
    assert (status == _hip.JPEG_OK).all(), (len(noise), status)
    assert np.array_equal(frames[0], jc.reference_frame(small, 3)) and np.array_equal(frames[1], jc.reference_frame(noise, 3))


# ---- the full path: files whose upright frames are the golden camera frames ----
FULL_CODES = (3, 6, 8, 2, None)     # None: an upright file without a tag


def _full_path_files(tmp_path, n, pick=None):
    """n files from the golden sample-images1 frames of the common size, file k stored under FULL_CODES[k % 5] (or pick(k)), quality
    95.  Returns (paths, bytes, upright (H, W))."""
    from PIL import Image
    src = []
    for f in jc.golden_files():
        with Image.open(f) as im:
            if im.size == (480, 640) or im.size == (640, 480):
                src.append((f, im.size))
    size = max(set(s for (_, s) in src), key=[s for (_, s) in src].count)
    src = [f for (f, s) in src if s == size]
    (paths, datas) = ([], [])
    for k in range(n):
        code = pick(k) if pick else FULL_CODES[k % len(FULL_CODES)]
        data = jc.stored_under(src[k % len(src)], code, quality=95)
        p = str(tmp_path / ('f%03d_%s.jpg' % (k, code)))
        with open(p, 'wb') as fh:
            fh.write(data)
        paths.append(p)
        datas.append(data)
    return (paths, datas, (size[1], size[0]))


def _reference_records(reader, paths):
    """reader.read_many on the host decoder's frames, one call for the list; and how many of them the reading path read."""
    from meterelf_amd import _hip
    from meterelf_amd._image import imread_bgr
    ref = np.array(reader.read_many([imread_bgr(p) for p in paths]), dtype=_hip.RESULT_DTYPE)
    return ref


def _oracle_reads(paths):
    """The CPU oracle on the imread_bgr frames: how many of the files are read without error."""
    from meterelf_amd import _hip, _params
    from meterelf_amd._image import imread_bgr
    from tests import helpers
    orc = helpers.OracleReader(_params.load(PFILE))
    recs = orc.read_frames(np.stack([imread_bgr(p) for p in paths]))
    return int((recs['status'] == _hip.FRAME_OK).sum())


@pytest.mark.gpu
def test_full_path_one_piece_and_chunked(reader, tmp_path):
    """melf_jpeg_process_batch on 8 files (the one-piece path) and on 72 (the chunked path; codes 3, 6, 8, 2 and upright files in one
    call): every status OK, every record the reference's, byte for byte."""
    from meterelf_amd import _hip
    (paths, datas, (H, W)) = _full_path_files(tmp_path, 72)
    distinct = paths[:40]                                       # the golden frames repeat behind that: the oracle sees each once
    assert _oracle_reads(distinct) * 4 >= 3 * len(distinct)
    ref = _reference_records(reader, paths)
    assert (ref['status'] == _hip.FRAME_OK).sum() * 4 >= 3 * len(paths)
    for n in (8, 72):
        (recs, status) = reader.ctx.jpeg_process_batch(datas[:n], H, W)
        assert (status == _hip.JPEG_OK).all(), (n, status)
        assert recs.tobytes() == ref[:n].tobytes(), (n, np.flatnonzero([a.tobytes() != b.tobytes() for (a, b) in zip(recs, ref[:n])]))
    # the reader's own list call groups by upright size
    got = reader.read_jpeg_files(datas[:10])
    assert all(g is not None and g.tobytes() == r.tobytes() for (g, r) in zip(got, ref[:10]))


@pytest.mark.gpu
def test_full_path_file_names_and_two_calls_in_flight(reader, tmp_path):
    """melf_jpeg_process_files, and _begin / _end with two calls in flight: the same records, H_used / W_used the upright size."""
    from meterelf_amd import _hip
    (paths, datas, (H, W)) = _full_path_files(tmp_path, 70)
    ref = _reference_records(reader, paths)
    assert (ref['status'] == _hip.FRAME_OK).sum() * 4 >= 3 * len(paths)
    (recs, status, hw) = reader.ctx.jpeg_process_files(paths)
    assert hw == (H, W) and (status == _hip.JPEG_OK).all(), (hw, status)
    assert recs.tobytes() == ref.tobytes()
    (a, b) = (paths[:66], paths[66:] + paths[5:40])
    reader.ctx.jpeg_process_files_begin(a)
    reader.ctx.jpeg_process_files_begin(b)
    (ra, sa, hwa) = reader.ctx.jpeg_process_files_end()
    (rb, sb, hwb) = reader.ctx.jpeg_process_files_end()
    assert hwa == (H, W) and hwb == (H, W) and (sa == 0).all() and (sb == 0).all()
    assert ra.tobytes() == ref[:66].tobytes() and rb.tobytes() == np.concatenate([ref[66:], ref[5:40]]).tobytes()
    (r1, ok1) = reader.read_jpeg_paths_batch(paths[:12])
    assert ok1.all() and r1.tobytes() == ref[:12].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('edge', ['left', 'top', 'right', 'bottom'])
def test_window_at_the_frame_edges(tmp_path, edge):
    """A context whose meter_rect touches one frame edge (the fixture's rectangle moved there, the golden frames' content moved
    with it), files under codes 6 and 7 and upright: the stored window is clamped at another stored edge for each code."""
    from PIL import Image

    from meterelf_amd import MeterReader, _hip, _params
    from meterelf_amd._engine import make_blob
    from meterelf_amd._types import Rect
    params = _params.load(PFILE)
    ((x0, y0), (x1, y1)) = params.meter_rect
    sizes = [Image.open(f).size for f in jc.golden_files()]
    (W, H) = max(set(sizes), key=sizes.count)                                 # the fixture's common frame size
    src = [f for (f, s) in zip(jc.golden_files(), sizes) if s == (W, H)][:6]
    (dx, dy) = {'left': (-x0, 0), 'top': (0, -y0), 'right': (W - x1, 0), 'bottom': (0, H - y1)}[edge]
    rect = Rect((x0 + dx, y0 + dy), (x1 + dx, y1 + dy))
    assert 0 in rect.top_left or rect.bottom_right[0] == W or rect.bottom_right[1] == H
    (paths, datas) = ([], [])
    for (k, f) in enumerate(src):
        frame = np.roll(np.asarray(Image.open(f).convert('RGB')), (dy, dx), axis=(0, 1))
        data = jc.stored_under(np.ascontiguousarray(frame), (6, 7, None)[k % 3], quality=95)
        p = str(tmp_path / ('e%d.jpg' % k))
        with open(p, 'wb') as fh:
            fh.write(data)
        paths.append(p)
        datas.append(data)
    r = MeterReader(params, blob=make_blob(params, rect), jpeg_orientation=True)
    try:
        ref = _reference_records(r, paths)
        assert (ref['status'] == _hip.FRAME_OK).sum() * 4 >= 3 * len(paths), ref['status']
        (recs, status) = r.ctx.jpeg_process_batch(datas, H, W)
        assert (status == _hip.JPEG_OK).all(), status
        assert recs.tobytes() == ref.tobytes()
    finally:
        r.close()


@pytest.mark.gpu
def test_get_meter_values_reads_oriented_files_on_the_gpu(tmp_path, monkeypatch):
    """A directory mixing upright and orientation-6 files: get_meter_values returns what the host branch returns
    (METERELF_JPEG_ORIENT=host), and no file of it reaches the host decoder."""
    import meterelf_amd
    from meterelf_amd import _api
    (paths, _datas, _hw) = _full_path_files(tmp_path, 40, pick=lambda k: 6 if k % 3 == 1 else None)
    monkeypatch.setenv('METERELF_CTX_CACHE', '0')
    monkeypatch.setenv('METERELF_JPEG_ORIENT', 'host')
    host = list(meterelf_amd.get_meter_values(PFILE, paths))
    monkeypatch.delenv('METERELF_JPEG_ORIENT')
    decoded_on_host = []
    real = _api.ImageFile.get_frame

    def spy(self):
        decoded_on_host.append(self.filename)
        return real(self)
    monkeypatch.setattr(_api.ImageFile, 'get_frame', spy)
    got = list(meterelf_amd.get_meter_values(PFILE, paths))
    assert decoded_on_host == []
    assert [g.filename for g in got] == paths
    for (g, h) in zip(got, host):
        assert g.meter_values == h.meter_values and g.value == h.value and (g.error is None) == (h.error is None)
    assert sum(g.error is None for g in got) * 4 >= 3 * len(got)
