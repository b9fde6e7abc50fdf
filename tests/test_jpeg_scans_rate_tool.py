"""tools/jpeg_scans_rate.py's table and closing lines, from made-up times (no GPU: the tool's report() alone, the way the rows of
profiles/jpeg_scans/jpeg_scans_rate.txt are printed), its rows, and its command line."""
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, 'tools')


def _tool():
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    spec = importlib.util.spec_from_file_location('jpeg_scans_rate', os.path.join(TOOLS, 'jpeg_scans_rate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _made_up(t, m1, m0):
    gpu = list(t.GPU_ROWS)
    host = [n % 8 for n in t.HOST_ROWS]
    mix = [t.MIX_ROWS[0] % 256, t.MIX_ROWS[1]]
    times = {n: [2.0 + 0.5 * k, 2.2 + 0.5 * k, 2.1 + 0.5 * k] for (k, n) in enumerate(gpu)}
    times.update({host[0]: [700.0, 720.0], host[1]: [690.0, 710.0], mix[0]: m1, mix[1]: m0})
    kern = {n: {'k_jpeg_huff': 1.0 + k, 'k_jpeg_idct': 0.25, 'k_jpeg_color': 0.5} for (k, n) in enumerate(gpu)}
    return (gpu, host, mix, times, kern)


def test_table_format(capsys):
    t = _tool()
    (gpu, host, mix, times, kern) = _made_up(t, [1.0, 1.1, 1.2], [3.0, 3.1, 3.2])
    t.report('header line', gpu, host, mix, times, kern, 1024)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == 'header line'
    head = [c.strip() for c in out[1].split('|')[1:-1]]
    assert head == ['row', 'ms/step', 'spread', 'vs (a0)', 'k_jpeg_huff ms', 'k_jpeg_idct ms', 'k_jpeg_color ms']
    assert set(out[2]) == {'|', '-'} and len(out[2]) == len(out[1])
    table = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out[3:14]}
    assert list(table) == [n.strip() for n in gpu + host + mix]
    assert table[gpu[0]] == ['2.1000', '2.0000..2.2000', '1.000x', '1.0000', '0.2500', '0.5000']
    assert table[gpu[2]] == ['3.1000', '3.0000..3.2000', '1.476x', '3.0000', '0.2500', '0.5000']
    assert table[host[0]][:3] == ['710.0000', '700.0000..720.0000', '338.095x'] and table[host[0]][3:] == ['0.0000'] * 3
    assert re.match(r'\(a0\) 2\.1000 ms a call = 487619 files/s \(spread of its rounds 9\.5 %\); \(a2\) 2\.6000; \(e\) 5\.1000 ms a call = 200784 files/s$', out[14]), out[14]
    assert re.match(r'multi-scan: 4:2:0 3\.1000 ms a call = 330323 files/s, 1\.476 of its twin; 4:2:2 3\.6000 ms, 1\.385 of its twin; '
                    r'host branch 710\.0 ms a call = 1442 files/s, 229 times as long$', out[15]), out[15]
    assert out[16].startswith('without DHT: 4:2:0 4.1000 ms a call') and out[16].endswith('host branch 700.0 ms a call = 1463 files/s, 171 times as long')
    assert out[17] == ('one multi-scan file in a call: 1.1000 ms on the GPU (rounds 1.0000..1.2000) against 3.1000 ms through the host branch '
                       '(rounds 3.0000..3.2000): no longer, the switch may be on by default')
    assert len(out) == 18


def test_the_decision_line_says_opt_in_when_the_gpu_call_is_longer(capsys):
    t = _tool()
    (gpu, host, mix, times, kern) = _made_up(t, [4.0, 4.1, 4.2], [3.0, 3.1, 3.2])
    t.report('h', gpu, host, mix, times, kern, 1024)
    assert capsys.readouterr().out.splitlines()[-1].endswith(': longer, the switch stays opt-in')


def test_rows_are_the_ones_the_profile_names():
    t = _tool()
    assert [n[:4] for n in t.GPU_ROWS] == ['(a0)', '(a2)', '(b0)', '(b2)', '(c0)', '(c2)', '(e) ']
    assert [n[:4] for n in t.HOST_ROWS] == ['(hb)', '(hc)'] and [n[:4] for n in t.MIX_ROWS] == ['(m1)', '(m0)']
    assert t.KERNELS == ('k_jpeg_huff', 'k_jpeg_idct', 'k_jpeg_color')
    text = open(os.path.join(ROOT, 'profiles', 'jpeg_scans', 'jpeg_scans_rate.txt')).read()
    for n in t.GPU_ROWS:
        assert '| %s' % n.strip() in text, n
    assert 'one multi-scan file in a call:' in text


def test_command_line():
    out = subprocess.run([sys.executable, os.path.join(TOOLS, 'jpeg_scans_rate.py'), '--help'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    for opt in ('--steps', '--warmup', '--rounds', '--batch', '--distinct', '--host-steps', '--mix', '--parent-root', '--parent-turns'):
        assert opt in text, opt
