"""tools/jpeg_sampling_rate.py's table and closing lines, from made-up times (no GPU: the tool's report() alone, the way the rows of
profiles/jpeg_sampling/jpeg_sampling_rate.txt are printed), and its command line."""
import importlib.util
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, 'tools')


def _tool():
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    spec = importlib.util.spec_from_file_location('jpeg_sampling_rate', os.path.join(TOOLS, 'jpeg_sampling_rate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_format(capsys):
    t = _tool()
    gpu = list(t.GPU_ROWS)
    host = [n % 8 for n in t.HOST_ROWS]
    times = {gpu[0]: [2.0, 2.2, 2.1], gpu[1]: [2.4, 2.5, 2.6], gpu[2]: [3.0, 3.1, 3.2], gpu[3]: [1.9, 2.0, 2.1], host[0]: [700.0, 720.0], host[1]: [690.0, 710.0]}
    kern = {n: {'k_jpeg_huff': 1.0 + k, 'k_jpeg_idct': 0.25, 'k_jpeg_color': 0.5 * (k + 1)} for (k, n) in enumerate(gpu)}
    t.report('header line', gpu, host, times, kern, 1024)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == 'header line'
    head = [c.strip() for c in out[1].split('|')[1:-1]]
    assert head == ['row', 'ms/step', 'spread', 'vs (a)', 'k_jpeg_huff ms', 'k_jpeg_idct ms', 'k_jpeg_color ms']
    assert set(out[2]) == {'|', '-'} and len(out[2]) == len(out[1])
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out[3:9]}
    assert list(table) == [n.strip() for n in gpu + host]
    assert table[gpu[0]] == ['2.1000', '2.0000..2.2000', '1.000x', '1.0000', '0.2500', '0.5000']
    assert table[gpu[2]] == ['3.1000', '3.0000..3.2000', '1.476x', '3.0000', '0.2500', '1.5000']
    assert table[host[0]][:3] == ['710.0000', '700.0000..720.0000', '338.095x'] and table[host[0]][3:] == ['0.0000'] * 3
    assert re.match(r'\(a\) 2\.1000 ms a call = 487619 files/s \(spread of its rounds 9\.5 %\); \(e\) 2\.0000 ms a call = 512000 files/s$', out[9]), out[9]
    assert re.match(r'4:4:0: 2\.5000 ms a call = 409600 files/s; vs \(a\) 1\.190; host branch 710\.0 ms a call = 1442 files/s, 284 times as long; '
                    r'colour stage 1\.0000 ms a call against 0\.5000 for 4:2:2$', out[10]), out[10]
    assert out[11].startswith('4:1:1: 3.1000 ms a call') and out[11].endswith('colour stage 1.5000 ms a call against 0.5000 for 4:2:2')
    assert len(out) == 12


def test_rows_are_the_ones_the_profile_names():
    t = _tool()
    assert [n[:4] for n in t.GPU_ROWS] == ['(a) ', '(b) ', '(c) ', '(e) '] and [n[:4] for n in t.HOST_ROWS] == ['(db)', '(dc)']
    assert t.KERNELS == ('k_jpeg_huff', 'k_jpeg_idct', 'k_jpeg_color')
    text = open(os.path.join(ROOT, 'profiles', 'jpeg_sampling', 'jpeg_sampling_rate.txt')).read()
    for n in t.GPU_ROWS:
        assert '| %s' % n.strip() in text, n
