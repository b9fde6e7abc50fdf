"""tools/packed32_rate.py at its smallest size, as tests/test_yuv422_10_rate_tool.py runs its sibling: one fresh process, 64 frames (two
32-frame match groups) x 2 buffers (the smallest rotation).  What the run covers that nothing else does: the tool's packing of VUYA,
Y410 and X2RGB10 words on the device, its unpack-to-i444 row with one scratch batch per caller stream, and the tool's own check --
before it times anything -- that the in-place rows' records of every batch are byte for byte the i444 row's."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'packed32_rate.py')
SMALL = ['--batch', '64', '--nbuf', '2', '--steps', '2', '--warmup', '2', '--rounds', '2']
ROWS = ['BGRA, melf_process_frames_dev', 'VUYA, melf_process_packed32_dev', 'Y410, melf_process_packed32_dev',
        'X2RGB10, melf_process_packed32_dev', 'Y410 -> i444 pass + melf_process_yuv_planar_dev', 'Y410 -> i444 pass (unpacking alone)']


@pytest.mark.gpu
def test_tool_runs():
    try:
        p = subprocess.run([sys.executable, TOOL] + SMALL, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.fail('packed32_rate.py did not end in 180 s: %r' % ((e.stdout or b'')[-3000:],))
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    text = p.stdout.decode()
    out = text.splitlines()
    m = [re.fullmatch(r"(\d+) of 128 frames read; the in-place rows' records == the i444 row's", ln) for ln in out]
    m = [x for x in m if x]
    # the frames are the fixture's, shifted by at most 8 pixels: the siblings' recorded runs read all of them through their YUV
    # encodings; at least three quarters (the siblings' cap) keeps a tool that compares failure records with failure records from
    # passing
    assert len(m) == 1 and int(m[0].group(1)) >= 96, text
    assert any(re.fullmatch(r'match kernel: \S+; dial kernel of the last call: .*p32.*', ln) for ln in out), text
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out if ln.startswith('| ')}
    for name in ROWS:
        assert name in table, (name, text)
        assert float(table[name][0]) > 0.0, (name, text)
    # the library's kernels ran in the rows that call it, and only there (columns: ms/step, spread, vs BGRA, k_lplane, k_dials)
    for name in ROWS[:5]:
        assert float(table[name][3]) > 0.0 and float(table[name][4]) > 0.0, (name, text)
    assert float(table[ROWS[5]][3]) == 0.0 and float(table[ROWS[5]][4]) == 0.0, text
