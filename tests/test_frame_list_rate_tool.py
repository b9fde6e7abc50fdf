"""tools/frame_list_rate.py at its smallest size, as tests/test_packed32_rate_tool.py runs its sibling: one fresh process, 64 frames
(two 32-frame match groups) x 2 buffers (the smallest rotation).  What the run covers that nothing else does: lists of separately
cloned torch tensors through melf_process_frame_list_dev on two caller streams in rotation, the diagnostic build's gather-alone
entry point, and the tool's own check -- before it times anything -- that the list rows' records of every batch are byte for byte
the contiguous rows'."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'frame_list_rate.py')
SMALL = ['--batch', '64', '--nbuf', '2', '--steps', '2', '--warmup', '2', '--rounds', '2']
ENTRY = {'BGR': 'melf_process_frames_dev', 'NV12': 'melf_process_yuv_dev', 'P010': 'melf_process_yuv16_dev'}


def rows_of(fmt):
    return ['%s (a) contiguous, %s' % (fmt, ENTRY[fmt]), '%s (b) list, melf_process_frame_list_dev' % fmt,
            '%s (c) torch.stack + %s' % (fmt, ENTRY[fmt]), '%s (d) gather kernel alone' % fmt]


@pytest.mark.gpu
def test_tool_runs():
    env = {k: v for (k, v) in os.environ.items() if k != 'MELF_LIB_PATH'}   # the tool picks the diagnostic build itself
    try:
        p = subprocess.run([sys.executable, TOOL] + SMALL, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.fail('frame_list_rate.py did not end in 180 s: %r' % ((e.stdout or b'')[-3000:],))
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    text = p.stdout.decode()
    out = text.splitlines()
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out if ln.startswith('| ')}
    for fmt in ENTRY:
        # the tool's own records check passed, with at least three quarters of the frames read (so that failure records are not
        # compared with failure records)
        m = [re.fullmatch(r"%s: (\d+) of 128 frames read; the list row's and the stack row's records == the contiguous row's" % fmt, ln) for ln in out]
        m = [x for x in m if x]
        assert len(m) == 1 and int(m[0].group(1)) >= 96, text
        rows = rows_of(fmt)
        for name in rows:
            assert name in table, (name, text)
            assert float(table[name][0]) > 0.0, (name, text)
        # columns: ms/step, spread, vs (a), k_gather, k_lplane, k_dials, gather GB/s.  The gather kernel shows up in rows (b) and (d)
        # only, the reading kernels in (a), (b) and (c) only
        (a, b, c, d) = (table[name] for name in rows)
        assert float(b[3]) > 0.0 and float(d[3]) > 0.0 and float(a[3]) == 0.0 and float(c[3]) == 0.0, text
        for row in (a, b, c):
            assert float(row[4]) > 0.0 and float(row[5]) > 0.0, text
        assert float(d[4]) == 0.0 and float(d[5]) == 0.0 and float(d[6]) > 0.0, text
        assert any(re.fullmatch(r'%s: \(b\)/\(a\) \d+\.\d+   \(c\)/\(b\) \d+\.\d+ .*' % fmt, ln) for ln in out), text
