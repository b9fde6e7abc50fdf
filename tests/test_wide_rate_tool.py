"""tools/wide_rate.py at its smallest size, as tests/test_packed32_rate_tool.py runs its sibling: one fresh process, 64 frames (two
32-frame match groups) x 2 buffers (the smallest rotation).  What the run covers that nothing else does: the tool's making of 16-bit,
float16 and float32 frames on the device in both layouts, its convert-and-read rows with one scratch batch per caller stream, and the
tool's own check -- before it times anything of a group -- that the wide rows' records of every batch are byte for byte the 8-bit
row's."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'wide_rate.py')
SMALL = ['--batch', '64', '--nbuf', '2', '--steps', '2', '--warmup', '2', '--rounds', '2']
GROUPS = [(kind, layout) for kind in ('u16', 'f16', 'f32') for layout in ('hwc', 'chw')]


@pytest.mark.gpu
def test_tool_runs():
    try:
        p = subprocess.run([sys.executable, TOOL] + SMALL, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail('wide_rate.py did not end in 300 s: %r' % ((e.stdout or b'')[-3000:],))
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    text = p.stdout.decode()
    out = text.splitlines()
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out if ln.startswith('| ')}
    for (kind, layout) in GROUPS:
        tag = '%s %s' % (kind, layout)
        m = [re.fullmatch(r"%s: (\d+) of 128 frames read; the wide rows' records == the 8-bit row's" % tag, ln) for ln in out]
        m = [x for x in m if x]
        # the frames are the fixture's, shifted by at most 8 pixels; at least three quarters (the siblings' cap) keeps a tool that
        # compares failure records with failure records from passing
        assert len(m) == 1 and int(m[0].group(1)) >= 96, (tag, text)
        family = 'planar' if layout == 'chw' else 'packed3'
        assert any(re.fullmatch(r'%s: match kernel: \S+; dial kernel of the last wide call: .*%s.*' % (tag, family), ln) for ln in out), (tag, text)
        name8 = 'melf_process_frames_dev' if layout == 'hwc' else 'melf_process_planes_dev'
        rows = ['(a) %s uint8, %s' % (tag, name8), '(b) %s, melf_process_wide_dev' % tag, '(c) %s -> uint8 pass + %s' % (tag, name8),
                '%s -> uint8 pass (conversion alone)' % tag]
        for name in rows:
            assert name in table, (name, text)
            assert float(table[name][0]) > 0.0, (name, text)
        # columns: ms/step, spread, vs (a), k_gather, k_lplane, k_dials.  The narrowing kernel ran in row (b) and only there; the
        # reading kernels in (a), (b) and (c); none of the library's in the conversion alone
        gather = [float(table[name][3]) for name in rows]
        assert gather[1] > 0.0 and gather[0] == gather[2] == gather[3] == 0.0, (tag, text)
        for name in rows[:3]:
            assert float(table[name][4]) > 0.0 and float(table[name][5]) > 0.0, (name, text)
        assert float(table[rows[3]][4]) == 0.0 and float(table[rows[3]][5]) == 0.0, (tag, text)
        assert any(re.fullmatch(r'  %s +\(b\) takes \d+\.\d+ times \(a\); \(c\) takes \d+\.\d+ times \(b\).*' % tag, ln) for ln in out), (tag, text)
