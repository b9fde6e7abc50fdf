"""tools/frame_rates.py, what the six frame-format rate tools share, and the tools themselves at their smallest size.

The tools do not import tests/frame_cases.py (it pulls in pytest and the fixtures), so frame_rates.py states the integer YUV -> BGR
conversion and the layouts once more, in torch.  The CPU tests here pin both to frame_cases: to_bgr byte-equal to yuv_to_bgr under
every matrix and subsampling, the layout writers byte-equal to the builders.  The GPU test runs each tool once."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, 'tools')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402

SUBSAMPLINGS = ((0, 0), (1, 0), (0, 1), (1, 1))


@pytest.fixture(scope='module')
def fr():
    """tools/frame_rates.py.  It imports torch: the library is loaded first, as everywhere in this suite (tests.helpers.hip_runtime)."""
    _hip.lib()
    pytest.importorskip('torch')
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import frame_rates
    return frame_rates


@pytest.fixture(scope='module')
def frames():
    """Two 8 x 12 BGR frames and their planes at every subsampling (numpy; left unchanged)."""
    bgr = np.random.default_rng(11).integers(0, 256, (2, 8, 12, 3), dtype=np.uint8)
    return bgr, {s: fc.bgr_to_yuv(bgr, *s) for s in SUBSAMPLINGS}


def test_import_touches_no_device():
    """Importing frame_rates creates no context and needs no device: a child process that sees none imports it."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES='')
    p = subprocess.run([sys.executable, '-c', 'import frame_rates'], cwd=TOOLS, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout == b''


def test_matrix_table_is_the_tests(fr):
    assert fr.MATRIX == fc.MATRIX
    assert {_hip.YUV_MATRIX_CODES[k]: v for (k, v) in fr.STANDARD.items()} == fc.STANDARD


@pytest.mark.parametrize('matrix', sorted(fc.MATRIX))
@pytest.mark.parametrize('sub', SUBSAMPLINGS)
def test_to_bgr_equals_yuv_to_bgr(fr, matrix, sub):
    """Random 8 x 12 planes, and the 64 triples with Y, U, V in {0, 16, 235, 255} (16 chroma corners under each Y), which clamp
    at both ends: byte-equal to tests/frame_cases.yuv_to_bgr."""
    import torch
    (sx, sy) = sub
    rng = np.random.default_rng(100 * matrix + 10 * sx + sy)
    (Y, U, V) = (rng.integers(0, 256, (3, 8, 12), dtype=np.uint8), rng.integers(0, 256, (3, 8 >> sy, 12 >> sx), dtype=np.uint8),
                 rng.integers(0, 256, (3, 8 >> sy, 12 >> sx), dtype=np.uint8))
    # the corner triples: one 2 x 2 block of equal Y per chroma pair, so that every subsampling holds all of them
    ends = (0, 16, 235, 255)
    (cu, cv) = [a.reshape(1, 4, 4) for a in np.meshgrid(ends, ends, indexing='ij')]
    cY = np.stack([np.full((8, 8), y, np.uint8) for y in ends])
    (cU, cV) = [np.repeat(np.repeat(c, 2 >> sy, axis=1), 2 >> sx, axis=2).repeat(4, axis=0).astype(np.uint8) for c in (cu, cv)]
    clamped = set()
    for (y, u, v) in ((Y, U, V), (cY, cU, cV)):
        want = fc.yuv_to_bgr(y, u, v, sx, sy, matrix)
        got = fr.to_bgr(torch.from_numpy(y), torch.from_numpy(u), torch.from_numpy(v), sx, sy, matrix)
        assert got.dtype == torch.uint8 and got.device.type == 'cpu'
        assert np.array_equal(got.numpy(), want), (matrix, sub)
        clamped |= {int(want.min()), int(want.max())}
    assert clamped >= {0, 255}


@pytest.mark.parametrize('fmt', ['nv12', 'i420', 'nv16', 'i422', 'i444', 'nv24'])
def test_write_yuv_equals_builders(fr, frames, fmt):
    import torch
    (sx, sy, step, _vfirst) = fc.YUV_PLANAR_FORMATS[fmt]
    (Y, U, V) = frames[1][(sx, sy)]
    want = fc.conventional_yuv_planar(Y, U, V, fmt)
    if (sx, sy) == (1, 1):
        assert np.array_equal(want, fc.conventional420(Y, U, V, fmt))
    assert want.shape[1] == fr.yuv_rows(8, sx, sy) == fc.rows_of(fmt, 8)
    out = torch.full(want.shape, 7, dtype=torch.uint8)
    fr.write_yuv(out, *[torch.from_numpy(p) for p in (Y, U, V)], semi=step == 2)
    assert np.array_equal(out.numpy(), want)
    # and back: the planes of the array, as the tools' record checks read them
    for (g, w) in zip(fr.yuv_planes(out, 8, sx, sy, semi=step == 2), (Y, U, V)):
        assert np.array_equal(g.numpy(), w)


@pytest.mark.parametrize('fmt', ['yuyv', 'uyvy', 'yvyu'])
def test_write_422_equals_packed422(fr, frames, fmt):
    import torch
    (Y, U, V) = frames[1][(1, 0)]
    out = torch.full((2, 8, 12, 2), 7, dtype=torch.uint8)
    fr.write_422(out, *[torch.from_numpy(p) for p in (Y, U, V)], fmt)
    assert np.array_equal(out.numpy(), fc.packed422(Y, U, V, fmt))


def test_write_planes_equals_to_planes(fr, frames):
    import torch
    bgr = frames[0]
    out = torch.full((2, 3, 8, 12), 7, dtype=torch.uint8)
    fr.write_planes(out, torch.from_numpy(bgr))
    assert np.array_equal(out.numpy(), fc.to_planes(bgr, 'rgb'))


def test_orders(fr):
    rows = ['a', 'b', 'c']
    assert [fr.forward_reversed(rows, r) for r in range(3)] == [rows, rows[::-1], rows]
    assert [fr.rotated(rows, r) for r in range(4)] == [rows, ['b', 'c', 'a'], ['c', 'a', 'b'], rows]


def test_print_table(fr, capsys):
    """The columns and widths of the tables under profiles/: the spread one character narrower than its title."""
    rows = [('BGR, x', None), ('NV12, y', None)]
    times = {'BGR, x': [0.25, 0.2, 0.3], 'NV12, y': [0.5, 0.5, 0.75]}
    kern = {'BGR, x': {'k_lplane': 0.05}, 'NV12, y': {'k_lplane': 0.0625, 'k_dials': 0.04}}
    fr.print_table('head', rows, times, rows[0], fr.kernel_columns(kern) + [('bytes', 6, lambda name: '%d' % len(name))], name=('row', 10))
    assert capsys.readouterr().out.splitlines() == [
        'head',
        '| row        |  ms/step |          spread |  vs BGR | k_lplane ms | k_dials ms |  bytes |',
        '|------------|----------|-----------------|---------|-------------|------------|--------|',
        '| BGR, x     |   0.2500 | 0.2000..0.3000 |  1.000x |      0.0500 |     0.0000 |      6 |',
        '| NV12, y    |   0.5000 | 0.5000..0.7500 |  2.000x |      0.0625 |     0.0400 |      7 |']


# --------------------------------------------------------------------------------------------------------------- GPU ---------
SMALL = ['--batch', '64', '--nbuf', '2', '--steps', '2', '--warmup', '2', '--rounds', '2']
YUV_PLANAR_ROWS = ['BGR, melf_process_batch_dev', 'NV12, melf_process_yuv_dev'] + ['%s, melf_process_yuv_planar_dev' % f for f in ('I422', 'NV16', 'I444', 'NV24')]
# tool: (arguments, the lines that say its records were checked or its frames counted, the rows of its table)
TOOL_RUNS = {
    'pixel_format_rate.py': (SMALL[:2] + SMALL[4:], [r'frames read: \d+ of 64'],
                             ['BGR, melf_process_batch_dev'] + ['%s, melf_process_frames_dev' % f for f in ('BGR', 'RGB', 'BGRA', 'RGBA')]
                             + ['torch RGBA -> packed BGR (conversion alone)', 'torch RGB -> packed BGR (conversion alone)', 'HLS crops, melf_read_dials']),
    'yuv_rate.py': (SMALL, [r'frames read: \d+ of 128; NV12 records == BGR records'],
                    ['BGR, melf_process_batch_dev', 'NV12, melf_process_yuv_dev', 'I420, melf_process_yuv_dev']),
    'yuv422_rate.py': (SMALL, [r'frames read: \d+ of 128; YUYV records == BGR records'], ['BGR, melf_process_batch_dev', 'YUYV, melf_process_yuv422_dev']),
    'yuv_matrix_rate.py': (SMALL, [r"library: .*; frames encoded with bt601"], list(_hip.YUV_MATRIX_CODES)),
    'planar_rate.py': (SMALL, [r'frames read: \d+ of 128; records of all three rows identical'],
                       ['BGR, melf_process_batch_dev', 'RGB planes, melf_process_planes_dev', 'RGB planes, permute().contiguous() + frames_dev']),
    'yuv_planar_rate.py': (SMALL, [r'%s: \d+ of 64 frames of the first batch read; records == those of its BGR conversion' % f
                                   for f in ('NV12', 'I422', 'NV16', 'I444', 'NV24')], YUV_PLANAR_ROWS),
}


@pytest.mark.gpu
def test_tools_run():
    """The six tools one after the other, each a fresh process, at 64 frames (two 32-frame match groups) x 2 buffers (the smallest
    rotation).  The first tool that fails or does not end stops the loop: nothing further is started on the GPU."""
    outputs = {}
    for (tool, (argv, _lines, _rows)) in TOOL_RUNS.items():
        try:
            p = subprocess.run([sys.executable, os.path.join(TOOLS, tool)] + argv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
        except subprocess.TimeoutExpired as e:
            pytest.fail('%s did not end in 180 s: %r' % (tool, (e.stdout or b'')[-3000:]))
        assert p.returncode == 0, (tool, p.returncode, p.stdout[-3000:], p.stderr[-3000:])
        outputs[tool] = p.stdout.decode()
    for (tool, (_argv, lines, rows)) in TOOL_RUNS.items():
        out = outputs[tool].splitlines()
        for pattern in lines:
            assert any(re.fullmatch(pattern, ln) for ln in out), (tool, pattern, outputs[tool])
        table = [ln.split('|')[1].strip() for ln in out if ln.startswith('| ')]
        for name in rows:
            assert name in table, (tool, name, outputs[tool])
