"""tools/jpeg_orient_rate.py at its smallest size, as tests/test_oriented_rate_tool.py runs its sibling: one fresh process, 96-file
calls (the chunked path of melf_jpeg_process_batch) over 2 windows of 16 distinct files.  What the run covers that nothing else does:
the tool's own check -- before it times anything -- that the records of the files stored under orientations 6 and 3 are byte for byte
the host branch's for the same files, and the colour stage's time per call from melf_ctx_timings in every GPU row."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'jpeg_orient_rate.py')
SMALL = ['--batch', '96', '--nbuf', '2', '--distinct', '16', '--steps', '2', '--warmup', '1', '--rounds', '2', '--host-steps', '1']
GPU_ROWS = ['(a)  upright files, switch on', '(a0) upright files, switch off', '(b6) stored under 6 (rot90cw), switch on',
            '(b3) stored under 3 (rot180), switch on']


@pytest.mark.gpu
def test_tool_runs():
    env = {k: v for (k, v) in os.environ.items() if k not in ('MELF_LIB_PATH', 'METERELF_DECODE_THREADS')}
    try:
        p = subprocess.run([sys.executable, TOOL] + SMALL, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.fail('jpeg_orient_rate.py did not end in 180 s: %r' % ((e.stdout or b'')[-3000:],))
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    text = p.stdout.decode()
    out = text.splitlines()
    # the tool's own records check passed, with at least three quarters of the files read (failure records compared with failure
    # records would show nothing)
    for tag in (r'\(b6\)', r'\(b3\)', r'\(a\) '):
        m = [x for x in (re.match(r"%s: (\d+) of 96 files read; the records == the host branch's" % tag, ln) for ln in out) if x]
        assert len(m) == 1 and int(m[0].group(1)) >= 72, (tag, text)
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out if ln.startswith('| ')}
    # columns: ms/step, spread, vs (a), k_jpeg_huff, k_jpeg_idct, k_jpeg_color (ms per call)
    for name in GPU_ROWS:
        assert name.strip() in table or name in table, (name, text)
        row = table.get(name, table.get(name.strip()))
        assert float(row[0]) > 0.0 and all(float(row[k]) > 0.0 for k in (3, 4, 5)), (name, text)
    host = [n for n in table if n.startswith('(c6) host branch') or n.startswith('(c3) host branch')]
    assert len(host) == 2 and all(float(table[n][0]) > 0.0 and float(table[n][5]) == 0.0 for n in host), text
    assert sum(bool(re.match(r'orientation [63]: \(b\) \d+\.\d+ ms a call = \d+ files/s; \(b\)/\(a\) \d+\.\d+; host branch \(c\) .* \(c\)/\(b\) \d+\.\d+; colour stage \d+\.\d+ ms', ln))
               for ln in out) == 2, text
