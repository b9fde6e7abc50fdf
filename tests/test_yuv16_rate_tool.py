"""tools/yuv16_rate.py at its smallest size, as tests/test_rate_tools.py runs the six tools of the 8-bit layouts: one fresh process,
64 frames (two 32-frame match groups) x 2 buffers (the smallest rotation).  What the run covers that nothing else does: the int16
view of the tool's (N, rows, W, 2) byte tensors, the byte shifts that make I010 of I420, the reduce-to-NV12 row with one scratch
batch per caller stream, and the tool's own check -- before it times anything -- that the 16-bit rows' records of every batch are
byte for byte the 8-bit rows'."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'yuv16_rate.py')
SMALL = ['--batch', '64', '--nbuf', '2', '--steps', '2', '--warmup', '2', '--rounds', '2']
ROWS = ['NV12, melf_process_yuv_dev', 'I420, melf_process_yuv_dev', 'P010, melf_process_yuv16_dev', 'I010, melf_process_yuv16_dev',
        'P010 -> NV12 pass + melf_process_yuv_dev', 'P010 -> NV12 pass (conversion alone)']


@pytest.mark.gpu
def test_tool_runs():
    try:
        p = subprocess.run([sys.executable, TOOL] + SMALL, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.fail('yuv16_rate.py did not end in 180 s: %r' % ((e.stdout or b'')[-3000:],))
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    text = p.stdout.decode()
    out = text.splitlines()
    m = [re.fullmatch(r"(\d+) of 128 frames read; the 16-bit rows' records == their 8-bit rows'", ln) for ln in out]
    m = [x for x in m if x]
    # the frames are the fixture's, shifted by at most 8 pixels: the siblings' recorded runs read all of them through their YUV
    # encodings (profiles/yuv_planar_frames/yuv_planar_rate.txt, profiles/yuv422_frames/yuv422_rate.txt); at least three quarters
    # keeps a tool that compares failure records with failure records from passing
    assert len(m) == 1 and int(m[0].group(1)) >= 96, text
    assert any(re.fullmatch(r'match kernel: \S+; dial kernel of the last 16-bit call: .*yuv16_step1.*', ln) for ln in out), text
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out if ln.startswith('| ')}
    for name in ROWS:
        assert name in table, (name, text)
        assert float(table[name][0]) > 0.0, (name, text)
    # the library's kernels ran in the rows that call it, and only there (columns: ms/step, spread, vs NV12, k_lplane, k_dials)
    for name in ROWS[:5]:
        assert float(table[name][3]) > 0.0 and float(table[name][4]) > 0.0, (name, text)
    assert float(table[ROWS[5]][3]) == 0.0 and float(table[ROWS[5]][4]) == 0.0, text
