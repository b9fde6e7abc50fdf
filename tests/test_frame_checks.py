"""The six descriptor checks of meterelf_amd/csrc/melf_frame_checks.h -- pure functions of a melf_*_frames descriptor -- swept on the
CPU by tests/frame_checks_main.cpp.  No GPU: the checks sit in front of every kernel and decide what the kernels' bounds tests may
rely on, and the overflow rejection of check_yuv is tested here and nowhere else.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import frame_cases as fc  # noqa: E402

# check: (messages it can give, forms the sweep must see accepted: format codes and plane orders / sub_x, sub_y, c_step and order /
# sub_y, c_step, order and shift 0, 2, 8 / the six plane orders)
CHECKS = {'check_frames': (8, 4), 'check_yuv': (13, 3), 'check_yuv422': (11, 3), 'check_yuv_planar': (17, 16), 'check_yuv16': (20, 24),
          'check_planes': (10, 6)}


def test_frame_checks_sweep(tmp_path):
    """tests/frame_checks_main.cpp, plain and under the host sanitizers (no check may overflow on any descriptor, the hand-written
    ones at the ends of 32 and 64 bits included): for every accepted descriptor the samples the public header's addressing gives
    end at (n - 1) * frame_stride + extent, none lies before the base and no two share a byte; every rejected one has an accepted
    neighbour that loosens what its message names.  Not vacuous: every check accepted descriptors of every form, every message of
    every check was produced, and the program ends with `failures 0`."""
    out = fc.build_and_run(tmp_path, os.environ.get('CXX', 'g++'), os.path.join(ROOT, 'tests', 'frame_checks_main.cpp'), 'frame_checks', [],
                           ['-fsanitize=address,undefined'])
    lines = out.splitlines()
    assert lines[-1] == 'failures 0', lines[-1]
    heads = {}
    for (i, ln) in enumerate(lines):
        m = re.match(r'(check_\w+) +accepted (\d+), forms (\d+) of (\d+), messages (\d+) of (\d+),', ln)
        if m:
            heads[m.group(1)] = (i, [int(x) for x in m.groups()[1:]])
    assert set(heads) == set(CHECKS), heads
    for (name, (nmsg, nforms)) in CHECKS.items():
        (i, (accepted, forms, of_forms, msgs, of_msgs)) = heads[name]
        assert accepted > 0 and (forms, of_forms) == (nforms, nforms) and (msgs, of_msgs) == (nmsg, nmsg), (name, lines[i])
        counts = [re.match(r' +(\d+)  \S', ln) for ln in lines[i + 1:i + 1 + nmsg]]
        assert all(counts) and all(int(c.group(1)) > 0 for c in counts), (name, lines[i + 1:i + 1 + nmsg])
    # the messages the program knows are the header's: every string a check returns, and no other
    hdr = open(os.path.join(ROOT, 'meterelf_amd', 'csrc', 'melf_frame_checks.h')).read()
    returned = set(re.findall(r'return "([^"]+)";', hdr)) | set(re.findall(r'UNKNOWN_YUV_MATRIX = "([^"]+)";', hdr))
    printed = {re.match(r' +\d+  (.*)$', ln).group(1) for ln in lines if re.match(r' +\d+  \S', ln)}
    assert returned == printed, returned ^ printed
