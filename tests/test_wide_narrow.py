"""The narrowing rule, the addresses and the descriptor check of the wide RGB frames (melf_process_wide*) on the CPU: the host-and-device
headers meterelf_amd/csrc/melf_narrow.h and melf_narrow_addr.h and check_wide of melf_frame_checks.h, compiled into stand-alone
programs under the host sanitizers and run alone.  No GPU: the kernel calls the same functions (tests/test_wide_frames.py runs it)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import wide_cases as wc  # noqa: E402


@pytest.fixture(scope='module')
def narrow_exe(tmp_path_factory):
    return wc.build(tmp_path_factory.mktemp('wide_narrow'), 'wide_narrow_main')


def test_narrowing_equals_numpy(narrow_exe, tmp_path):
    """Every byte tests/wide_narrow_main.cpp writes -- all 65 536 f16 and all 65 536 bf16 patterns under three (scale, offset, rounding)
    triples, all u16 values at shifts 0, 2, 4, 6, 8, and the directed float32 set: exact ties at scale 1, the special values, and for
    scale 58.395, offset 123.675 the values within 64 ulps of a rounding boundary for which fused arithmetic gives ANOTHER byte (at
    least 64 per rounding mode, asserted in wide_cases.f32_sets) -- equals numpy's float32 x * s, then + o, rint / floor, NaN to 0,
    clip."""
    allbits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    (records, want) = ([], [])
    for type_ in (wc.F16, wc.BF16):
        x32 = wc.widen(allbits, type_)
        for (s, o, r) in wc.TRIPLES:
            records.append(wc.pattern_record(type_, 0, s, o, r, 0))
            want.append(wc.narrow_float(x32, s, o, r))
    for shift in wc.SHIFTS:
        records.append(wc.pattern_record(wc.U16, shift, 0.0, 0.0, 'nearest', 0))
        want.append(wc.narrow_u16(allbits, shift))
    sets = wc.f32_sets()
    for (s, o, r, v) in sets:
        records.append(wc.pattern_record(wc.F32, 0, s, o, r, len(v)) + v.astype('<f4').tobytes())
        want.append(wc.narrow_float(v, s, o, r))
    (fin, fout) = (tmp_path / 'sets.bin', tmp_path / 'bytes.bin')
    fin.write_bytes(b''.join(records))
    out = wc.run([narrow_exe, 'patterns', str(fin), str(fout)])
    assert re.search(r'patterns: %d sets, %d samples' % (len(want), sum(len(w) for w in want)), out), out
    got = np.frombuffer(fout.read_bytes(), np.uint8)
    want = np.concatenate(want)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), bad[:10], got[bad[:10]], want[bad[:10]])
    # not vacuous: the non-fusion sets hold what a fused multiply-add gets wrong, and the sets exercise both clamps and the middle
    for (s, o, r, v) in sets[-2:]:
        assert (wc.narrow_float(v, s, o, r) != wc.fused_byte(v, s, o, r)).all() and len(v) >= 64
    assert {0, 1, 127, 128, 254, 255} <= set(np.unique(want).tolist())


def test_loads_stay_inside_the_frame(narrow_exe):
    """Frames that end exactly at the end of their malloc block and start one sample into it, narrowed through the host packer's code
    path under AddressSanitizer: W in {1, 5, 16, 17, 250}, crops that touch the right and bottom edges, padded pitches, 3 and 4
    channels in both orders, planar, every sample type.  Every staged byte is the sample the public header's addressing names, and
    the address header's pieces load samples in [0, extent) that are exactly the crop's, each once."""
    out = wc.run([narrow_exe, 'bounds'])
    m = re.search(r'bounds: (\d+) frames, (\d+) pieces \((\d+) of them tails\), (\d+) samples loaded', out)
    assert m and int(m.group(1)) == 4 * 5 * 5 * 2 * 2 * 2 * 2 and int(m.group(3)) > 0 and int(m.group(4)) > 0, out


def test_descriptor_checks(tmp_path):
    """tests/wide_checks_main.cpp under the host sanitizers: check_wide over accepted descriptors (2-byte alignment only among them)
    and one mutation per rejection, each with exactly its message; every message of the table was produced, and the table is the
    header's."""
    out = wc.run([wc.build(tmp_path, 'wide_checks_main')])
    m = re.search(r'check_wide accepted (\d+) \((\d+) of them at a base with the sample\'s own alignment only\)', out)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, out
    printed = dict((msg, int(cnt)) for (cnt, msg) in re.findall(r'^ +(\d+)  (\S.*)$', out, re.M))
    hdr = open(os.path.join(ROOT, 'meterelf_amd', 'csrc', 'melf_frame_checks.h')).read()
    table = re.search(r'WIDE_MESSAGES\[WIDE_MSGS\] = \{(.*?)\};', hdr, re.S).group(1)
    messages = re.findall(r'"([^"]+)"', table)
    assert len(messages) == 18 and set(printed) == set(messages) and all(c > 0 for c in printed.values()), printed
