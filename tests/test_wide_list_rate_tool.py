"""tools/wide_list_rate.py at its smallest size, as tests/test_wide_rate_tool.py runs its sibling: one fresh process, 64 frames (two
32-frame match groups) x 2 buffers (the smallest rotation).  What the run covers that nothing else does: the tool's lists of
separately cloned frames and planes of 16-bit, float16 and float32 samples in both layouts, its stack-and-read rows with one scratch
batch per caller stream, and the tool's own check -- before it times anything of a group -- that the records of every list row and
every stack row, of every batch, are byte for byte the batch row's."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'wide_list_rate.py')
SMALL = ['--batch', '64', '--nbuf', '2', '--steps', '2', '--warmup', '2', '--rounds', '2']
GROUPS = [(kind, layout) for kind in ('u16', 'f16', 'f32') for layout in ('hwc', 'chw')]


@pytest.mark.gpu
def test_tool_runs():
    try:
        p = subprocess.run([sys.executable, TOOL] + SMALL, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail('wide_list_rate.py did not end in 300 s: %r' % ((e.stdout or b'')[-3000:],))
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    text = p.stdout.decode()
    out = text.splitlines()
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out if ln.startswith('| ')}
    for (kind, layout) in GROUPS:
        tag = '%s %s' % (kind, layout)
        m = [re.fullmatch(r"%s: (\d+) of 128 frames read; the records of the other rows == row \(a\)'s" % tag, ln) for ln in out]
        m = [x for x in m if x]
        # the frames are the fixture's, shifted by at most 8 pixels; at least three quarters (the siblings' cap) keeps a tool that
        # compares failure records with failure records from passing
        assert len(m) == 1 and int(m[0].group(1)) >= 96, (tag, text)
        rows = ['(a) %s batch, melf_process_wide_dev' % tag, '(b) %s frame list, melf_process_wide_list_dev' % tag,
                '(d) %s torch.stack of the frames + (a)' % tag]
        if layout == 'chw':
            rows += ['(c) %s plane list, melf_process_wide_plane_list_dev' % tag, '(e) %s torch.stack of the planes + (a)' % tag]
        for name in rows:
            assert name in table, (name, text)
            # columns: ms/step, spread, vs (a), k_gather, k_lplane, k_dials: every row is timed, and in every row the narrowing kernel
            # and the reading kernels ran
            assert float(table[name][0]) > 0.0, (name, text)
            assert float(table[name][3]) > 0.0 and float(table[name][4]) > 0.0 and float(table[name][5]) > 0.0, (name, text)
        planes = r'   \(c\)/\(b\) \d+\.\d+   \(e\)/\(c\) \d+\.\d+' if layout == 'chw' else ''
        assert any(re.fullmatch(r'  %s +\(b\)/\(a\) \d+\.\d+   \(d\)/\(b\) \d+\.\d+%s   \(a\) \d+\.\d+ ms, its turns \d+\.\d+\.\.\d+\.\d+.*' % (tag, planes), ln)
                   for ln in out), (tag, text)
