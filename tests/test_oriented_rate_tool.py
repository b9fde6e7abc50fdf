"""tools/oriented_rate.py at its smallest size, as tests/test_frame_list_rate_tool.py runs its sibling: one fresh process, 64 frames
(two 32-frame match groups) x 2 buffers (the smallest rotation).  What the run covers that nothing else does: stored torch batches
through melf_process_oriented_dev on two caller streams in rotation, beside torch.rot90 / flip of the same batches, and the tool's
own check -- before it times anything -- that the records of the oriented rows, the rot90 rows and the list rows of every batch are
byte for byte the upright rows'."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'oriented_rate.py')
SMALL = ['--batch', '64', '--nbuf', '2', '--steps', '2', '--warmup', '2', '--rounds', '2']
CASES = {'BGR rot180': 'melf_process_frames_dev', 'BGR rot90cw': 'melf_process_frames_dev', 'BGRA rot90cw': 'melf_process_frames_dev',
         'NV12 rot90cw': 'melf_process_yuv_dev', 'P010 rot90cw': 'melf_process_yuv16_dev'}


def rows_of(case):
    return ['%s (a) upright, %s' % (case, CASES[case]), '%s (b) stored, melf_process_oriented_dev' % case,
            '%s (c) torch rot90/flip + %s' % (case, CASES[case]), '%s (d) upright list, melf_process_frame_list_dev' % case]


@pytest.mark.gpu
def test_tool_runs():
    env = {k: v for (k, v) in os.environ.items() if k != 'MELF_LIB_PATH'}
    try:
        p = subprocess.run([sys.executable, TOOL] + SMALL, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.fail('oriented_rate.py did not end in 180 s: %r' % ((e.stdout or b'')[-3000:],))
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    text = p.stdout.decode()
    out = text.splitlines()
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out if ln.startswith('| ')}
    for case in CASES:
        # the tool's own records check passed, with at least three quarters of the frames read (so that failure records are not
        # compared with failure records)
        m = [re.fullmatch(r"%s: (\d+) of 128 frames read; the records of \(b\), \(c\) and \(d\) == the upright row's" % case, ln) for ln in out]
        m = [x for x in m if x]
        assert len(m) == 1 and int(m[0].group(1)) >= 96, text
        rows = rows_of(case)
        for name in rows:
            assert name in table, (name, text)
            assert float(table[name][0]) > 0.0, (name, text)
        # columns: ms/step, spread, vs (a), k_gather, k_lplane, k_dials.  MELF_K_GATHER shows up in rows (b) -- k_orient_tiles -- and
        # (d) -- k_gather_rows -- only; the reading kernels in every row
        (a, b, c, d) = (table[name] for name in rows)
        assert float(b[3]) > 0.0 and float(d[3]) > 0.0 and float(a[3]) == 0.0 and float(c[3]) == 0.0, text
        for row in (a, b, c, d):
            assert float(row[4]) > 0.0 and float(row[5]) > 0.0, text
        assert any(re.fullmatch(r'%s: \(b\)/\(a\) \d+\.\d+   \(c\)/\(b\) \d+\.\d+ .* orient / gather \d+\.\d+' % case, ln) for ln in out), text
