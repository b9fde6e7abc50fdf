"""tools/jpeg_long_rate.py's tables and closing lines, from made-up times (no GPU: the tool's report() alone, the way the rows of
profiles/jpeg_long/jpeg_long_rate.txt are printed), its rows, and its command line."""
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
    spec = importlib.util.spec_from_file_location('jpeg_long_rate', os.path.join(TOOLS, 'jpeg_long_rate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _made_up(t, one_gpu, one_host):
    full = [(t.FULL_ROW % (64, '4.9 MB'), [30.0, 28.5, 29.0], {'k_jpeg_huff': 20.25, 'k_jpeg_idct': 2.5, 'k_jpeg_color': 1.125}, [570.0]),
            (t.FULL_ROW % (256, '10.5 MB'), [250.0, 240.0, 245.0], {'k_jpeg_huff': 200.0, 'k_jpeg_idct': 10.0}, [4800.0])]
    mix = [(1, 256, one_gpu, one_host), (8, 256, [9.0, 8.0], [30.0, 31.0]), (32, 256, [20.0, 21.0], [100.0, 99.0])]
    return (full, mix)


def test_table_format(capsys):
    t = _tool()
    (full, mix) = _made_up(t, [3.5, 3.25, 3.75], [11.0, 10.5, 12.0])
    t.report('header line', full, mix, 8)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == 'header line'
    head = [c.strip() for c in out[1].split('|')[1:-1]]
    assert head == ['row', 'gpu ms', 'gpu calls', 'k_jpeg_huff ms', 'k_jpeg_idct ms', 'k_jpeg_color ms', 'host branch ms, 8 threads', 'host / gpu']
    assert set(out[2]) == {'|', '-'} and len(out[2]) == len(out[1]) == len(out[3]) == len(out[4])
    rows = {ln.split('|')[1].strip(): [c.strip() for c in ln.split('|')[2:-1]] for ln in out[3:5]}
    assert rows['(f)  64 files of 4.9 MB'] == ['28.500', '28.500..30.000', '20.250', '2.500', '1.125', '570.0', '20.0x']
    assert rows['(f) 256 files of 10.5 MB'] == ['240.000', '240.000..250.000', '200.000', '10.000', '0.000', '4800.0', '20.0x']
    assert out[5] == 'name lists through read_jpeg_paths, best of the calls (all calls in brackets):'
    assert out[6] == ' 1 long file of 256 : gpu 3.250 ms  host branch 10.500 ms  (gpu 3.500 3.250 3.750; host branch 11.000 10.500 12.000)'
    assert out[7].startswith(' 8 long files of 256 : gpu 8.000 ms  host branch 30.000 ms') and out[8].startswith('32 long files of 256 : gpu 20.000 ms')
    assert out[9] == "one long file in a list: 3.250 ms on the GPU against 10.500 ms through the host branch: faster, METERELF_JPEG_LONG defaults to 'gpu'"
    assert len(out) == 10
    # the row the default is read from (tests/test_jpeg_long.py) is this one
    assert re.search(r'^\s*1 long file of 256\s*:\s*gpu\s+([0-9.]+) ms\s+host branch\s+([0-9.]+) ms', out[6]).groups() == ('3.250', '10.500')


def test_the_decision_line_says_host_when_the_gpu_list_is_not_faster(capsys):
    t = _tool()
    (full, mix) = _made_up(t, [12.0, 12.5], [11.0, 10.5])
    t.report('h', full, mix, 8)
    out = capsys.readouterr().out.splitlines()
    assert out[-2].endswith("not faster, METERELF_JPEG_LONG defaults to 'host'")
    assert out[-1] == 'the switch pays from 8 long files in a list on'


def test_rows_are_the_ones_the_profile_names():
    t = _tool()
    assert t.KERNELS == ('k_jpeg_huff', 'k_jpeg_idct', 'k_jpeg_color')
    assert [tag for (_s, tag) in t.SIZES] == ['4.9 MB', '10.5 MB'] and [s for (s, _t) in t.SIZES] == [(1000, 1200), (1500, 1700)]
    text = open(os.path.join(ROOT, 'profiles', 'jpeg_long', 'jpeg_long_rate.txt')).read()
    for n in (64, 256):
        for (_s, tag) in t.SIZES:
            assert '| %s' % (t.FULL_ROW % (n, tag)) in text, (n, tag)
    for nlong in (1, 8, 32):
        assert (t.MIX_ROW % (nlong, '' if nlong == 1 else 's', 256)) + ' : gpu' in text, nlong
    assert 'one long file in a list:' in text


def test_command_line():
    out = subprocess.run([sys.executable, os.path.join(TOOLS, 'jpeg_long_rate.py'), '--help'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    for opt in ('--steps', '--warmup', '--counts', '--mix', '--mix-long', '--distinct', '--parent-root', '--parent-turns'):
        assert opt in text, opt
