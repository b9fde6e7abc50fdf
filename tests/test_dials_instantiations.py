"""The dial reader (meterelf_amd/csrc/k_dials.hip, k_dials_body.inc): every instantiation production can pick, launched, ASSERTED
to be the one that ran (melf_ctx_last_dials) and compared -- the way tests/test_match_layouts.py does it for the template match
and tests/test_fused_variants.py for the fused mask.

launch_dials picks one of twelve kernel families from the frames' layout and one of six row counts NR (32, 40, 48, 52, 56, 64)
from ws_max, the context's largest dial window (2 R + 5 rows): 72 kernels.  The fixtures' dials give NR 48 and 52 only, so:

* the sweep: eleven contexts whose largest dial has R = 13 .. 29, both ends of every NR class, each with a 9-row dial beside it;
  every family on the same twelve frames.  Packed BGR against the oracle (tests/test_gpu_parity.py's bars), the HLS crops
  against the oracle, every other family byte for byte against read_frames of the packed BGR frame its conversion defines (the
  contract and the restatements of the format modules, imported from them);
* the crop's edges: the exact path of a window that leaves the crop's columns, and the right-edge shift of the four-pixel fetch
  (cstart / cshift of k_yneedle and k_yp_needle<1, *>, mstart / mshifted of k_p422_needle), every family, at both parities of
  the crop's origin.

The loads themselves are checked on the CPU: tests/frame_src_bounds_main.cpp compiles melf_frame_src.h for the host and runs every
source type against frames malloc'd to exactly their extent, under the host sanitizers (test_frame_src_bounds_sweep), and
tests/prep_bounds_main.cpp sweeps the prep arms' address functions (melf_prep_addr.h, shared with the kernels) the same way
(test_prep_bounds_sweep).  On the GPU the edge cases then
run once more on frames cut to the crop's last row and column, every family's device copy ending where its allocation ends.

CPU tests check the inputs: the oracle reads every frame at every geometry, the outer rows of each NR class carry part of the
reading, the matches land where the edge cases need them, and the shifts the edge cases are there for do act.

The last GPU test asserts that the (family, NR) pairs launched and asserted by this module are all 72, from a list written out
by hand.  It runs whatever of the sweep has not run yet (each geometry runs once per session), so it also holds when selected
alone.
"""
import copy
import functools
import glob
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests.test_gpu_parity import POS_TOL, REJECTED, _compare_records  # noqa: E402

SD = 'sample-images1'
NFRAMES = 12
(RECT_X0, RECT_Y0, RECT_Y1) = (50, 160, 410)   # sample-images1's meter_rect: (50, 160)-(300, 410)

# ---- the table under test, written out by hand (nothing here comes from the library) ----
NR_CLASSES = (32, 40, 48, 52, 56, 64)
FAMILIES = ('hls', 'bgr', 'packed3', 'packed4', 'nv12', 'i420', 'p422', 'yp_sub0_step1', 'yp_sub0_step2', 'yp_sub1_step1',
            'yp_sub1_step2', 'planar')
ALL_PAIRS = frozenset([
    ('hls', 32), ('hls', 40), ('hls', 48), ('hls', 52), ('hls', 56), ('hls', 64),
    ('bgr', 32), ('bgr', 40), ('bgr', 48), ('bgr', 52), ('bgr', 56), ('bgr', 64),
    ('packed3', 32), ('packed3', 40), ('packed3', 48), ('packed3', 52), ('packed3', 56), ('packed3', 64),
    ('packed4', 32), ('packed4', 40), ('packed4', 48), ('packed4', 52), ('packed4', 56), ('packed4', 64),
    ('nv12', 32), ('nv12', 40), ('nv12', 48), ('nv12', 52), ('nv12', 56), ('nv12', 64),
    ('i420', 32), ('i420', 40), ('i420', 48), ('i420', 52), ('i420', 56), ('i420', 64),
    ('p422', 32), ('p422', 40), ('p422', 48), ('p422', 52), ('p422', 56), ('p422', 64),
    ('yp_sub0_step1', 32), ('yp_sub0_step1', 40), ('yp_sub0_step1', 48), ('yp_sub0_step1', 52), ('yp_sub0_step1', 56),
    ('yp_sub0_step1', 64),
    ('yp_sub0_step2', 32), ('yp_sub0_step2', 40), ('yp_sub0_step2', 48), ('yp_sub0_step2', 52), ('yp_sub0_step2', 56),
    ('yp_sub0_step2', 64),
    ('yp_sub1_step1', 32), ('yp_sub1_step1', 40), ('yp_sub1_step1', 48), ('yp_sub1_step1', 52), ('yp_sub1_step1', 56),
    ('yp_sub1_step1', 64),
    ('yp_sub1_step2', 32), ('yp_sub1_step2', 40), ('yp_sub1_step2', 48), ('yp_sub1_step2', 52), ('yp_sub1_step2', 56),
    ('yp_sub1_step2', 64),
    ('planar', 32), ('planar', 40), ('planar', 48), ('planar', 52), ('planar', 56), ('planar', 64),
])
# the families whose four-pixel fetch reads chroma pairs (and so has a right-edge shift), by what the shift is called
SUBSAMPLED = ('nv12', 'i420', 'p422', 'yp_sub1_step1', 'yp_sub1_step2')
# the largest dial's R per context: ws_max = 2 R + 5 = 31, 33, 39, 41, 47, 49, 51, 53, 55, 57, 63 -- both ends of every NR class
R_MAXES = (13, 14, 17, 18, 21, 22, 23, 24, 25, 26, 29)
CLASS_UPPER_R = (13, 17, 21, 23, 25, 29)   # the largest R of each NR class


def expected_nr(ws_max):
    """The class table of launch_dials, restated: the smallest instantiated row count that holds ws_max rows."""
    for nr in (32, 40, 48, 52, 56):
        if ws_max <= nr:
            return nr
    return 64


def py_round(v):
    return int(round(v))   # Python's round, half to even: what the parameters' loader uses


def dial_radius(nd):
    return py_round(nd['diameter'] / 2.0) + nd['dist_from_center'] + nd['circle_thickness'] - 1


def ws_max_of(data):
    return max(2 * dial_radius(nd) + 5 for nd in data['needle_data'])


# ---- the contexts' parameters ----
@functools.lru_cache(maxsize=None)
def _fixture_data():
    import yaml
    with open(os.path.join(GOLDEN, SD, 'params.yml')) as fp:
        return yaml.safe_load(fp)


def sweep_data(r_max):
    """sample-images1 with dial 1 grown or shrunk to R = r_max, dials 0 and 3 cut to R <= r_max, dial 2 a 9-row window (R = 2)."""
    data = copy.deepcopy(_fixture_data())
    nd = data['needle_data']
    nd[1]['circle_thickness'] = r_max - 11
    for k in (0, 3):
        nd[k]['circle_thickness'] -= max(dial_radius(nd[k]) - r_max, 0)
    nd[2].update(diameter=2, dist_from_center=0, circle_thickness=2)
    assert dial_radius(nd[1]) == r_max and dial_radius(nd[2]) == 2 and ws_max_of(data) == 2 * r_max + 5
    assert all(dial_radius(d) <= r_max and d['circle_thickness'] >= 1 for d in nd)
    return data


EDGE_KINDS = ('leave', 'near', 'flush')


def edge_data(kind, k, x0=RECT_X0):
    """sample-images1 with a crop of tw + k columns from frame column x0.  'leave': dial 0's window leaves the crop on the left
    and dial 3's on the right (the windows of test_dial_window_fetch_edge_paths (b)); 'near': the fixture's dials, dial 3's window
    inside the crop with its last pieces within 8 pixels of the crop's right edge; 'flush': dial 3 moved three columns further
    right, so that its last piece ends on the template's last column."""
    data = copy.deepcopy(_fixture_data())
    tw = data['dials_template_size'][0]
    data['meter_rect'] = {'top_left': [x0, RECT_Y0], 'bottom_right': [x0 + tw + k, RECT_Y1]}
    nd = data['needle_data']
    if kind == 'leave':
        nd[0]['center'][0] = 18.0
        nd[3]['center'][0] = tw - 17.5
    elif kind == 'flush':
        nd[3]['center'][0] += 3.0
    else:
        assert kind == 'near'
    return data


_TMP = []


def _params_dir(data, tag):
    """data as a params.yml beside the fixture's template, in a directory of this session's own."""
    import atexit
    import yaml
    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix='dials_inst_'))
        atexit.register(shutil.rmtree, _TMP[0], ignore_errors=True)
    d = os.path.join(_TMP[0], tag)
    if not os.path.isdir(d):
        os.makedirs(d)
        with open(os.path.join(d, 'params.yml'), 'w') as fp:
            yaml.safe_dump(data, fp)
        shutil.copy(os.path.join(GOLDEN, SD, data['dials_template']), os.path.join(d, data['dials_template']))
    return os.path.join(d, 'params.yml')


def _oparams(data, tag):
    from oracle import pyoracle as po
    return po.Params(_params_dir(data, tag))


# ---- the frames ----
def _streak(frame, ox, oy, angle, colour):
    """The streak painter of test_read_dials_random_geometries (three pixels wide, along a ray from the dial's centre), here from
    radius 14 to 30 of the ray at `angle` (turns, clockwise from north: get_angle_by_vector's): it hangs on the needle and crosses
    the outer rings of every NR class."""
    a = 2 * np.pi * angle
    (dx, dy) = (np.sin(a), -np.cos(a))
    for t in np.linspace(14, 30, 64):
        for w in (-1, 0, 1):
            frame[int(oy + t * dy - w * dx), int(ox + t * dx + w * dy)] = colour


@functools.lru_cache(maxsize=None)
def sweep_frames():
    """The first twelve same-sized good fixture frames, shifted and with +-2 noise (frame_cases.synth; its constant frame
    is given a slot of its own and dropped).  The fixture's needle of dial 1 ends at radius 21, so every second frame gets a
    streak of the dial's own colour from the needle into the rings beyond, 0.02 turn off the needle's angle: without it the rows
    that only the larger NR classes hold would not bear on any reading (test_outer_rows_bear_on_the_reading)."""
    from meterelf_amd._image import imread_bgr
    from oracle import pyoracle as po
    files = [f for f in sorted(glob.glob(os.path.join(GOLDEN, SD, '*.jpg'))) if os.path.basename(f) not in REJECTED]
    frames = [imread_bgr(f) for f in files]
    shapes = [f.shape for f in frames]
    twelve = [f for f in frames if f.shape == max(set(shapes), key=shapes.count)][:NFRAMES]
    assert len(twelve) == NFRAMES
    out = np.delete(fc.synth(twelve[:4] + [twelve[0]] + twelve[4:], NFRAMES + 1, 11), 4, axis=0)
    assert out.shape == (NFRAMES, 640, 480, 3)
    ores = po.process_frames(out, _oparams(_fixture_data(), 'fixture'))
    (cx, cy) = _fixture_data()['needle_data'][1]['center']
    for i in range(0, NFRAMES, 2):
        o = ores[i]
        assert o.status == 0
        (ox, oy) = (RECT_X0 + o.match_x + cx, RECT_Y0 + o.match_y + cy)
        core = out[i, int(oy) - 2:int(oy) + 3, int(ox) - 2:int(ox) + 3].reshape(-1, 3)
        _streak(out[i], ox, oy, o.angle[1] + 0.02, np.rint(core.mean(axis=0)).astype(np.uint8))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sweep_oracle(r_max):
    from oracle import pyoracle as po
    return po.process_frames(sweep_frames(), _oparams(sweep_data(r_max), 'r%d' % r_max))


@functools.lru_cache(maxsize=None)
def edge_frames(k, x0=RECT_X0):
    """sweep_frames with frame i rolled left by its own match_x and right by i % (k + 1) (+ x0 - 50): in a crop of tw + k columns
    from column x0 the matches land on crop columns 0 .. k."""
    src = sweep_frames()
    ores = sweep_oracle(21)
    out = np.stack([np.roll(src[i], i % (k + 1) - ores[i].match_x + x0 - RECT_X0, axis=1) for i in range(NFRAMES)])
    out.setflags(write=False)
    return out


def edge_match_x(k):
    return [i % (k + 1) for i in range(NFRAMES)]


@functools.lru_cache(maxsize=None)
def edge_oracle(kind, k, x0=RECT_X0):
    from oracle import pyoracle as po
    return po.process_frames(edge_frames(k, x0), _oparams(edge_data(kind, k, x0), '%s_k%d_x%d' % (kind, k, x0)))


def dial3_lanes(data, match_x):
    """Dial 3's window and the first frame column fx0 of each of its sixteen lanes' four pixels (k_dials_body.inc), with xlim and
    mlim, the crop's right edge in whole chroma pairs / macropixels."""
    nd = data['needle_data'][3]
    tw = data['dials_template_size'][0]
    (x0, x1) = (data['meter_rect']['top_left'][0], data['meter_rect']['bottom_right'][0])
    R = dial_radius(nd)
    (wx0, ws) = (py_round(nd['center'][0]) - R - 2, 2 * R + 5)
    npiece = (ws + 3) >> 2
    fx0 = [x0 + match_x + wx0 + 4 * min(pc, npiece - 1) for pc in range(16)]
    return dict(wx0=wx0, ws=ws, npiece=npiece, tw=tw, fx0=fx0, xlim=(x1 + 1) & ~1, mlim=(x1 + 1) >> 1,
                quads=wx0 >= 0 and wx0 + 4 * npiece <= tw)


def shifts_of(g):
    """(fx0 odd, chroma samples the 4:2:0 / 4:2:2 planar fetch is moved left, macropixels the packed 4:2:2 fetch is moved left)
    per lane: cstart = min(fx0 >> 1, (xlim >> 1) - 4), mstart = min(fx0 >> 1, mlim - 3)."""
    return [(fx & 1, (fx >> 1) - min(fx >> 1, (g['xlim'] >> 1) - 4), (fx >> 1) - min(fx >> 1, g['mlim'] - 3)) for fx in g['fx0']]


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_class_table_and_geometries():
    assert len(ALL_PAIRS) == 72 and ALL_PAIRS == {(f, nr) for f in FAMILIES for nr in NR_CLASSES}
    assert tuple(_hip.DIALS_FAMILIES) == FAMILIES
    ws = [ws_max_of(sweep_data(r)) for r in R_MAXES]
    assert ws == [31, 33, 39, 41, 47, 49, 51, 53, 55, 57, 63]
    assert [expected_nr(w) for w in ws] == [32, 40, 40, 48, 48, 52, 52, 56, 56, 64, 64]
    assert [expected_nr(2 * r + 5) for r in CLASS_UPPER_R] == list(NR_CLASSES)
    # the fixtures themselves: the two classes every other test runs in
    assert expected_nr(ws_max_of(_fixture_data())) == 48
    for r in R_MAXES:   # the library's loader sees the same windows
        from meterelf_amd import _params
        p = _params.load(_params_dir(sweep_data(r), 'r%d' % r))
        assert len(p.dial_names) == 4


def test_header_enum_matches_the_python_names():
    import re
    with open(os.path.join(ROOT, 'include', 'meterelf_hip.h')) as fp:
        text = fp.read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r'\bMELF_DIALS_([A-Z0-9_]+) = (\d+)', text)}
    assert values.pop('FAMILIES') == 12
    assert [k.lower() for (k, _v) in sorted(values.items(), key=lambda kv: kv[1])] == list(FAMILIES)
    assert sorted(values.values()) == list(range(12))


def test_oracle_reads_every_frame_at_every_geometry():
    from meterelf_amd._image import imread_bgr
    from oracle import pyoracle as po
    files = [f for f in sorted(glob.glob(os.path.join(GOLDEN, SD, '*.jpg'))) if os.path.basename(f) not in REJECTED]
    plain = [imread_bgr(f) for f in files[:40]]
    plain = np.stack([f for f in plain if f.shape == (640, 480, 3)][:NFRAMES])
    assert len(plain) == NFRAMES
    for r in R_MAXES:
        op = _oparams(sweep_data(r), 'r%d' % r)
        assert [o.status for o in po.process_frames(plain, op)] == [0] * NFRAMES, r      # the fixture frames as they are
        assert [o.status for o in sweep_oracle(r)] == [0] * NFRAMES, r                   # ... and as the sweep uses them


def test_outer_rows_bear_on_the_reading():
    """For each NR class: dial 1's position at the class's largest R differs from its position at the previous class's largest R on
    at least half of the frames -- by a million times the comparison's tolerance, not by rounding."""
    for (prev, upper) in zip(CLASS_UPPER_R[:-1], CLASS_UPPER_R[1:]):
        (a, b) = (sweep_oracle(prev), sweep_oracle(upper))
        differing = sum(abs(a[i].pos[1] - b[i].pos[1]) > 1e6 * POS_TOL for i in range(NFRAMES))
        assert 2 * differing >= NFRAMES, (upper, differing)


@pytest.mark.parametrize('kind', EDGE_KINDS)
def test_edge_matches_land_on_the_crop_columns(kind):
    for x0 in (RECT_X0, RECT_X0 + 1):
        for k in range(4):
            ores = edge_oracle(kind, k, x0)
            assert [o.match_x for o in ores] == edge_match_x(k), (kind, k, x0)
            assert [o.status for o in ores] == [0] * NFRAMES, (kind, k, x0)


def test_edge_geometries_reach_the_paths():
    """What each kind of edge context is there for, from its geometry."""
    for x0 in (RECT_X0, RECT_X0 + 1):
        for k in range(4):
            # 'leave': dials 0 and 3 leave the crop (quads == false), dials 1 and 2 stay inside
            data = edge_data('leave', k, x0)
            tw = data['dials_template_size'][0]
            inside = []
            for nd in data['needle_data']:
                R = dial_radius(nd)
                wx0 = py_round(nd['center'][0]) - R - 2
                inside.append(wx0 >= 0 and wx0 + 4 * ((2 * R + 5 + 3) >> 2) <= tw)
            assert inside == [False, True, True, False]
            assert py_round(data['needle_data'][0]['center'][0]) - dial_radius(data['needle_data'][0]) - 2 < 0
            # 'near' and 'flush': dial 3's window takes the four-pixel fetch, and in some frame of the context a lane's first pixel
            # lies within 8 pixels of the crop's right edge (of the edge itself: xlim, the edge rounded up to a whole pair, is
            # one further for the odd widths, and the fixture's dial 3 then stays exactly 8 short of it)
            x1 = data['meter_rect']['bottom_right'][0]
            for kind in ('near', 'flush'):
                lanes = [dial3_lanes(edge_data(kind, k, x0), mx) for mx in sorted(set(edge_match_x(k)))]
                for g in lanes:
                    assert g['quads'] and g['wx0'] >= 0 and g['wx0'] + 4 * g['npiece'] <= g['tw']
                    assert all(fx + 4 <= x1 for fx in g['fx0'])
                assert any(fx + 8 > x1 for g in lanes for fx in g['fx0']), (kind, k, x0)
                if kind == 'flush':
                    assert any(fx + 8 > g['xlim'] for g in lanes for fx in g['fx0']), (kind, k, x0)
    # The shift proper acts only when a lane's first chroma pair lies within three pairs of the edge: never for the fixture's
    # dial 3 (its last piece starts 7 columns short of the template's last, 7 + k - match_x short of the crop's) ...
    for x0 in (RECT_X0, RECT_X0 + 1):
        for k in range(4):
            for mx in range(k + 1):
                assert all(s[1] == 0 and s[2] == 0 for s in shifts_of(dial3_lanes(edge_data('near', k, x0), mx)))
    # ... which is what 'flush' is for: every context has a frame whose chroma fetch shifts, and over the contexts it shifts by one
    # and by two samples, at even and at odd fx0, at both parities of the crop's origin; the macropixel fetch (which only an even fx0
    # can move, by one) shifts at both origins too
    seen_c = set()
    seen_m = set()
    for x0 in (RECT_X0, RECT_X0 + 1):
        for k in range(4):
            here = [s for mx in edge_match_x(k) for s in shifts_of(dial3_lanes(edge_data('flush', k, x0), mx))]
            assert any(s[1] > 0 for s in here), (k, x0)
            assert all(s[1] <= (1 if s[0] else 2) and s[2] <= (0 if s[0] else 1) for s in here)   # what the loads can undo
            seen_c |= {(x0 & 1, s[0], s[1]) for s in here if s[1] > 0}
            seen_m |= {(x0 & 1, s[2]) for s in here if s[2] > 0}
    assert {(p, odd) for (p, odd, _n) in seen_c} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {n for (_p, _o, n) in seen_c} == {1, 2}
    assert seen_m == {(0, 1), (1, 1)}


def rocm_clangxx():
    """The ROCm tree's clang++ and include directory, from the hipcc meterelf_amd/csrc/Makefile builds with (HIPCC, else
    /opt/rocm/bin/hipcc)."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(hipcc) or hipcc)))
    cxx = os.path.join(rocm, 'llvm', 'bin', 'clang++')
    assert os.path.isfile(cxx), 'no clang++ beside %s (looked for %s): the dial sources cannot be compiled for the host' % (hipcc, cxx)
    return cxx, os.path.join(rocm, 'include')


def test_frame_src_bounds_sweep(tmp_path):
    """tests/frame_src_bounds_main.cpp: the dial sources of melf_frame_src.h, compiled for the host and run on frames malloc'd to
    exactly the descriptor's extent, over the sweep the program's head lists: no load leaves the allocation (the sanitizer's red
    zones), every unpacked pixel equals px of the same source and plain indexing of the planes, and every source type took the
    window fetch, the exact path and -- where it has one -- the load moved left at the crop's right edge.  Only `alignment` is
    dropped from the sanitizers: the sources load unaligned dwords on purpose."""
    (cxx, inc) = rocm_clangxx()
    out = fc.build_and_run(tmp_path, cxx, os.path.join(ROOT, 'tests', 'frame_src_bounds_main.cpp'), 'frame_src_bounds',
                           ['-D__HIP_PLATFORM_AMD__', '-I' + inc], ['-fsanitize=address,undefined', '-fno-sanitize=alignment'])
    assert out.count('windows: quads') == 15, out   # the fifteen source types


def test_prep_bounds_sweep(tmp_path):
    """tests/prep_bounds_main.cpp: every load of the prep kernels' 8-bit arms lies inside a buffer of exact extent, over the sweep
    the program's head lists, and every arm took each of its three paths.  The addresses, spans and guards are those of
    meterelf_amd/csrc/melf_prep_addr.h, the functions the kernels and the launcher compute them with."""
    out = fc.build_and_run(tmp_path, os.environ.get('CXX', 'g++'), os.path.join(ROOT, 'tests', 'prep_bounds_main.cpp'), 'prep_bounds', [],
                           ['-fsanitize=address,undefined'])
    assert out.count('lanes: row-safe') == 10, out   # the ten arms


# ------------------------------------------------------------------------------------------------------------- GPU ---------
SEEN = set()       # (family, NR) pairs this module launched and asserted
_SWEPT = {}        # r_max -> None, or the failure of its run


class _Ctx:
    """A reader for one parameter file, and the assertion that follows every call."""

    def __init__(self, data, tag):
        from meterelf_amd import MeterReader, _params
        if _hip.device_count() < 1:
            pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
        self.ws_max = ws_max_of(data)
        self.nr = expected_nr(self.ws_max)
        self.reader = MeterReader(_params.load(_params_dir(data, tag)))
        self.ctx = self.reader.ctx
        self.tag = tag

    def close(self):
        self.reader.close()

    def ran(self, family):
        got = self.ctx.last_dials()
        assert got == dict(family=family, nr=self.nr, ws_max=self.ws_max), (self.tag, family, got)
        SEEN.add((got['family'], got['nr']))

    def read_bgr(self, bgr):
        recs = self.reader.read_frames(bgr)
        self.ran('bgr')
        return recs


def _dev(make_buf, call):
    buf = make_buf()
    try:
        return call(buf.d.value)
    finally:
        buf.free()


_CONVERTED = {}   # the forward conversions of ONE set of frames (the sweep's eleven contexts share theirs, an edge case's three kinds too)


def _converted(bgr, key):
    """(Y, U, V, the packed BGR frames the conversion makes of them) of the frames bgr for chroma subsampling key."""
    if _CONVERTED.get('frames') is not bgr:
        _CONVERTED.clear()
        _CONVERTED['frames'] = bgr
    if key not in _CONVERTED:
        if key == '420':
            (Y, U, V) = fc.F420.from_bgr(bgr)
            _CONVERTED[key] = (Y, U, V, fc.F420.bgr_of(Y, U, V))
        elif key == '422':
            (Y, U, V) = fc.F422.from_bgr(bgr)
            _CONVERTED[key] = (Y, U, V, fc.F422.bgr_of(Y, U, V))
        else:
            assert key == '444'
            (Y, U, V) = fc.bgr_to_yuv(bgr, 0, 0)
            _CONVERTED[key] = (Y, U, V, fc.yuv_to_bgr(Y, U, V, 0, 0))
    return _CONVERTED[key]


def _run_families(c, bgr, rng, families, want_match_x=None, at_end=False):
    """Every family named, host and device path, byte for byte against read_frames of the packed BGR frames its conversion
    defines; melf_ctx_last_dials after every call.  want_match_x: where the converted frames, too, have to match.  at_end: the
    device path alone, every family's device copy ending where its allocation ends (frame_cases.DevBuf.at_end)."""
    ctx = c.ctx
    wants = {}
    devbuf = fc.DevBuf.at_end if at_end else fc.DevBuf

    def packed_dev(v):
        return _dev(lambda: devbuf(v.ptr, v.extent),
                    lambda d: ctx.process_frames_dev(d, v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride))

    def want_of(key):
        if key not in wants:
            wants[key] = c.read_bgr(bgr if key == 'bgr' else _converted(bgr, key)[3])
            if want_match_x is not None:
                assert [int(x) for x in wants[key]['match_x']] == want_match_x, (c.tag, key)
            assert (wants[key]['status'] == _hip.FRAME_OK).all(), (c.tag, key)
        return wants[key].tobytes()

    def check(family, fmt, wb, host, dev):
        if not at_end:
            assert host().tobytes() == wb, (c.tag, fmt, 'host')
            c.ran(family)
        assert dev().tobytes() == wb, (c.tag, fmt, 'device')
        c.ran(family)

    for (fmt, family) in (('rgb', 'packed3'), ('bgra', 'packed4'), ('rgba', 'packed4')):
        if family in families:
            (arr, f) = fc.to_layout(bgr, fmt, 5, rng)
            check(family, fmt, want_of('bgr'), lambda: c.reader.read_frame_views(arr, f),
                  lambda: packed_dev(_hip.frames_view(arr, f)))
    for fmt in ('nv12', 'i420'):
        if fmt in families:
            (Y, U, V, _b) = _converted(bgr, '420')
            v = _hip.yuv_frames_view(fc.conventional420(Y, U, V, fmt, 10 if fmt == 'nv12' else 0, rng), fmt)
            check(fmt, fmt, want_of('420'), lambda: ctx.process_yuv(v.ptr, v.descriptor()),
                  lambda: _dev(lambda: devbuf(v.ptr, v.extent), lambda d: ctx.process_yuv_dev(d, v.descriptor())))
    if 'p422' in families:
        (Y, U, V, _b) = _converted(bgr, '422')
        for fmt in ('yuyv', 'uyvy'):
            v = _hip.yuv422_frames_view(fc.conventional422(Y, U, V, fmt, 6, rng), fmt)
            check('p422', fmt, want_of('422'), lambda: ctx.process_yuv422(v.ptr, v.descriptor()),
                  lambda: _dev(lambda: devbuf(v.ptr, v.extent), lambda d: ctx.process_yuv422_dev(d, v.descriptor())))
    for (fmt, family) in (('i422', 'yp_sub1_step1'), ('nv16', 'yp_sub1_step2'), ('i444', 'yp_sub0_step1'), ('nv24', 'yp_sub0_step2')):
        if family in families:
            (sx, sy, step, _vf) = fc.YUV_PLANAR_FORMATS[fmt]
            assert (sx, sy, step) == (int(family[6]), 0, int(family[-1]))
            # (4:2:2: packed and planar formats are made by one forward conversion and expected from one restatement,
            # tests/frame_cases.py's, at (sub_x, sub_y) = (1, 0) -- so the planar formats share their expected records)
            key = '422' if sx else '444'
            (Y, U, V, _b) = _converted(bgr, key)
            v = _hip.yuv_planar_frames_view(fc.conventional_yuv_planar(Y, U, V, fmt, 0, rng), fmt)
            check(family, fmt, want_of(key), lambda: ctx.process_yuv_planar(v.ptr, v.descriptor()),
                  lambda: _dev(lambda: devbuf(v.ptr, v.extent), lambda d: ctx.process_yuv_planar_dev(d, v.descriptor())))
    if 'planar' in families:
        v = _hip.planar_frames_view(fc.to_planes(bgr, 'rgb', rng), 'rgb')
        check('planar', 'rgb planes', want_of('bgr'), lambda: ctx.process_planes(v.ptr, v.descriptor()),
              lambda: _dev(lambda: fc.DevBuf.at_end(v.ptr, v.extent), lambda d: ctx.process_planes_dev(d, v.descriptor())))


def test_forward_conversions_agree():
    """_run_families shares one set of expected records between the packed and the planar 4:2:2 formats.  Both families' input
    and expected frames now come from one function each (frame_cases.bgr_to_yuv, yuv_to_bgr), so this only holds the 4:2:2 record
    to (sub_x, sub_y) = (1, 0): the packed family's converters are those functions at that subsampling."""
    bgr = np.ascontiguousarray(sweep_frames()[:1, 200:264, 100:164])
    (a, b) = (fc.F422.from_bgr(bgr), fc.bgr_to_yuv(bgr, 1, 0))
    assert all(np.array_equal(p, q) for (p, q) in zip(a, b))
    assert np.array_equal(fc.F422.bgr_of(*a), fc.yuv_to_bgr(*b, 1, 0))


def _sweep_one(r_max):
    from oracle import pyoracle as po
    data = sweep_data(r_max)
    bgr = sweep_frames()
    ores = sweep_oracle(r_max)
    op = _oparams(data, 'r%d' % r_max)
    c = _Ctx(data, 'r%d' % r_max)
    try:
        assert c.ctx.last_dials()['ws_max'] == 2 * r_max + 5
        # (a) packed BGR, host-fed and from device memory, against the oracle
        recs = c.read_bgr(bgr)
        _compare_records(recs, ores, tag='r%d' % r_max)
        dev = _dev(lambda: fc.DevBuf(bgr.ctypes.data, bgr.nbytes), lambda d: c.ctx.process_batch_dev(d, NFRAMES, *bgr.shape[1:3]))
        c.ran('bgr')
        assert dev.tobytes() == recs.tobytes()
        # (b) the oracle's HLS crops of the same frames
        (th, tw) = op.template_size
        crops = []
        for (i, o) in enumerate(ores):
            hls = po.bgr2hls(po.crop_meter(bgr[i], op), op.hue_shift)
            crops.append(hls[o.match_y:o.match_y + th, o.match_x:o.match_x + tw])
        got = c.ctx.read_dials(np.stack(crops))
        c.ran('hls')
        for i in range(NFRAMES):
            o = po.read_dials(crops[i], op)
            assert int(got[i]['status']) == o.status == 0, i
            assert np.allclose(got[i]['pos'][:4], list(o.pos)[:4], rtol=0, atol=POS_TOL), i
            assert np.allclose(got[i]['angle'][:4], list(o.angle)[:4], rtol=0, atol=POS_TOL), i
            assert abs(float(got[i]['value']) - o.value) < 1e-8 and int(float(got[i]['value'])) == int(o.value), i
        # (c) every other family
        _run_families(c, bgr, np.random.default_rng(r_max), FAMILIES)
    finally:
        c.close()


def _sweep(r_max):
    if r_max not in _SWEPT:
        try:
            _sweep_one(r_max)
            _SWEPT[r_max] = None
        except BaseException as e:
            _SWEPT[r_max] = e
            raise
    elif _SWEPT[r_max] is not None:
        raise _SWEPT[r_max]


@pytest.mark.gpu
@pytest.mark.parametrize('r_max', R_MAXES)
def test_every_family_at_every_window_class(r_max):
    _sweep(r_max)
    assert {(f, expected_nr(2 * r_max + 5)) for f in FAMILIES} <= SEEN


@pytest.mark.gpu
@pytest.mark.parametrize('x0', (RECT_X0, RECT_X0 + 1))
@pytest.mark.parametrize('k', range(4))
@pytest.mark.parametrize('kind', EDGE_KINDS)
def test_crop_edge_paths(kind, k, x0):
    """x0 = 51, the crop's origin at the other parity: the families that read chroma pairs.  Then the same frames cut to the crop's
    bottom row and right column (the width rounded up to even), every family's device copy ending where its allocation ends: the
    last frame matches at the crop's last column (match_x = k), so its windows' last pieces -- the exact path of the window that
    leaves the crop, the chroma and macropixel fetches moved left -- lie against the buffer's last bytes."""
    data = edge_data(kind, k, x0)
    bgr = edge_frames(k, x0)
    tag = '%s_k%d_x%d' % (kind, k, x0)
    c = _Ctx(data, tag)
    try:
        assert c.nr == 48
        recs = c.read_bgr(bgr)
        _compare_records(recs, edge_oracle(kind, k, x0), tag=tag)
        assert [int(x) for x in recs['match_x']] == edge_match_x(k)
        families = [f for f in FAMILIES if x0 == RECT_X0 or f in SUBSAMPLED]
        _run_families(c, bgr, np.random.default_rng(7 + k), families, want_match_x=edge_match_x(k))
        x1 = data['meter_rect']['bottom_right'][0]
        assert edge_match_x(k)[-1] == k == x1 - x0 - data['dials_template_size'][0]
        cut = np.ascontiguousarray(bgr[:, :RECT_Y1, :(x1 + 1) & ~1])
        _run_families(c, cut, np.random.default_rng(70 + k), families, want_match_x=edge_match_x(k), at_end=True)
    finally:
        c.close()


@pytest.mark.gpu
def test_all_72_instantiations_were_launched_and_asserted():
    for r_max in R_MAXES:
        _sweep(r_max)
    assert SEEN == ALL_PAIRS, sorted(ALL_PAIRS - SEEN)
