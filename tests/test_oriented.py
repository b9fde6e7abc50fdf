"""Frames stored rotated or mirrored (EXIF orientations 1-8): melf_process_oriented / melf_process_oriented_dev, melf_orient_frames,
MeterReader.read_oriented_frames, the address functions of melf_orient_addr.h and the kernel k_orient_tiles.

The parity bar everywhere is byte equality of the records with the family's own _dev call on the upright batch: there is no
tolerance.  The stored batch is made from the upright one, plane by plane, under the inverse orientation (oriented_cases.
stored_batch); in every parity test at least three quarters of the upright batch's records are FRAME_OK (frame_cases.synth makes
every ninth frame constant: 29 of 33 read), so failure records are not compared with failure records."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import frame_list_cases as flc  # noqa: E402
from tests import oriented_cases as oc  # noqa: E402
from tests.frame_cases import env  # noqa: E402,F401
from tests.test_frame_list import COUNTED, ok_enough  # noqa: E402

KERNEL = 'k_orient_tiles'
N = 33   # one 32-frame match group plus one
ERR_INVALID = -1   # MELF_ERR_INVALID
NAMES = ('normal', 'mirror', 'rot180', 'flip', 'transpose', 'rot90cw', 'transverse', 'rot90ccw')
ORIENTABLE = [(lay, fmt) for (lay, fmt) in flc.FORMATS if lay in oc.FAMILIES]
ONE_PER_FAMILY = [(lay, fmt) for (lay, fmt) in flc.ONE_PER_FAMILY if lay in oc.FAMILIES]


# ------------------------------------------------------------------------------------------------------------------- CPU ---
def test_orient_runs_on_the_cpu(tmp_path):
    """tests/orient_runs_main.cpp, plain and under the host sanitizers: the six families under the eight codes over small
    descriptors, the oriented plan executed through the functions of melf_orient_addr.h -- the kernel's own -- on frames malloc'd to
    exactly the extent, against stage_plan plus a plain row copy of the naively oriented frame.  Every accepted (family, code) pair
    saw more than 200 cases, more than 50 of them with an odd crop origin and more than 50 touching an edge of the oriented frame."""
    from tests import test_dials_instantiations as di
    (cxx, inc) = di.rocm_clangxx()
    out = fc.build_and_run(tmp_path, cxx, os.path.join(ROOT, 'tests', 'orient_runs_main.cpp'), 'orient_runs', ['-D__HIP_PLATFORM_AMD__', '-I' + inc],
                           ['-fsanitize=address,undefined'])
    seen = {(m.group(1), int(m.group(2))): tuple(int(m.group(k)) for k in (3, 4, 5, 6))
            for m in re.finditer(r'family (\w+) code (\d): cases (\d+) odd_origin (\d+) edge (\d+) rejected (\d+)', out)}
    assert sorted(seen) == sorted((fam, code) for fam in ('frames', 'yuv', 'yuv_planar', 'yuv16', 'packed32', 'planes') for code in oc.CODES), out
    for ((fam, code), (cases, odd, edge, rejected)) in seen.items():
        assert cases > 200 and odd > 50 and edge > 50, (fam, code, out)
        assert (rejected > 0) == (fam in ('yuv_planar', 'yuv16') and code >= 5), (fam, code, out)   # 4:2:2 and 4:4:0 do not transpose
    assert 'packed 4:2:2 families: rejected 16 of 16' in out


def test_orientation_table_against_pillow():
    """oriented_cases.orient is Pillow's transpose under the mapping ImageOps.exif_transpose uses, and INVERSE undoes it."""
    from PIL import Image
    T = Image.Transpose if hasattr(Image, 'Transpose') else Image
    method = {2: T.FLIP_LEFT_RIGHT, 3: T.ROTATE_180, 4: T.FLIP_TOP_BOTTOM, 5: T.TRANSPOSE, 6: T.ROTATE_270, 7: T.TRANSVERSE, 8: T.ROTATE_90}
    a = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    assert oc.orient(a, 1).tobytes() == a.tobytes()
    for code in oc.CODES:
        if code > 1:
            want = np.asarray(Image.fromarray(a).transpose(method[code]))
            got = oc.orient(a, code)
            assert got.shape == want.shape and np.array_equal(got, want), code
        assert np.array_equal(oc.orient(oc.orient(a, oc.inverse(code)), code), a), code
    assert oc.INVERSE == {6: 8, 8: 6}


def test_exports_enum_and_names():
    """The three entry points are exported and listed; the enum's values are the EXIF codes; _hip.ORIENTATIONS names them."""
    L = _hip.lib()
    text = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    for name in ('melf_process_oriented', 'melf_process_oriented_dev', 'melf_orient_frames'):
        assert hasattr(L, name) and name in _hip.EXPORTS and ('int %s(' % name) in text, name
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'MELF_ORIENT_(\w+) = (\d)', text)}
    assert codes == dict(zip(NAMES, oc.CODES)) == _hip.ORIENTATIONS
    assert 'MELF_K_COUNT = 10' in text and _hip.K_COUNT == 10 and _hip.ABI_VERSION == 3
    assert '"rotate by 90 / 180 / 270 degrees clockwise to display" is 6 / 3 / 8' in text


class StandIn:
    """A context that records what read_oriented_frames hands to the library"""

    def __init__(self):
        self.calls = []

    def process_oriented(self, family, desc, orientation, ptr):
        self.calls.append(('host', family, desc, orientation, ptr))
        return np.zeros(desc.n, _hip.RESULT_DTYPE)


def stand_in_reader():
    from meterelf_amd import MeterReader
    r = MeterReader.__new__(MeterReader)
    r.device = 0
    r.ctx = StandIn()
    return r


def test_read_oriented_frames_with_a_stand_in():
    """What reaches the library for names and ints, and every ValueError (stand-in context: nothing reaches a library)."""
    r = stand_in_reader()
    (H, W) = (12, 16)
    bgr = np.zeros((2, H, W + 2, 3), np.uint8)[:, :, :W]   # padded rows, read in place
    for (code, name) in zip(oc.CODES, NAMES):
        for given in (code, name, name.upper(), np.int64(code)):
            assert len(r.read_oriented_frames(bgr, 'views', 'bgr', given)) == 2
            (kind, family, d, got, ptr) = r.ctx.calls[-1]
            assert (kind, family, got, ptr) == ('host', 'views', code, bgr.ctypes.data) and type(got) is int
            assert (d.pixel_format, d.n, d.H, d.W, d.row_pitch) == (_hip.PIX_BGR, 2, H, W, (W + 2) * 3)
    nv12 = np.zeros((1, H * 3 // 2, W), np.uint8)
    r.read_oriented_frames(nv12, 'yuv', 'nv12', 'rot90cw', matrix='bt709')
    (_k, family, d, got, _p) = r.ctx.calls[-1]
    assert (family, got, d.matrix, d.format) == ('yuv', 6, _hip.YUV_BT709_LIMITED, _hip.YUV_NV12)
    i422 = np.zeros((1, 2 * H, W), np.uint8)
    r.read_oriented_frames(i422, 'yuv_planar', 'i422', 'rot180')
    assert r.ctx.calls[-1][1:4:2] == ('yuv_planar', 3)
    p210 = np.zeros((1, 2 * H, W), np.uint16)
    r.read_oriented_frames(p210, 'yuv16', 'p210', 4, matrix='bt709')
    calls = len(r.ctx.calls)
    for bad in (0, 9, -1, 'upright', 'rot90', None, 2.0, True):
        with pytest.raises(ValueError, match='orientation'):
            r.read_oriented_frames(bgr, 'views', 'bgr', bad)
    with pytest.raises(ValueError, match='layout'):
        r.read_oriented_frames(bgr, 'bayer', 'bgr', 3)
    for layout in ('yuv422', 'yuv422_10'):
        with pytest.raises(ValueError, match='cannot be oriented in place'):
            r.read_oriented_frames(bgr, layout, 'yuyv', 3)
    with pytest.raises(ValueError, match='transposes the frame'):
        r.read_oriented_frames(i422, 'yuv_planar', 'i422', 'transpose')
    with pytest.raises(ValueError, match='transposes the frame'):
        r.read_oriented_frames(p210, 'yuv16', 'p210', 6, matrix='bt709')
    with pytest.raises(ValueError, match='takes no matrix'):
        r.read_oriented_frames(bgr, 'views', 'bgr', 3, matrix='bt709')
    with pytest.raises(ValueError, match='would have to be copied'):
        r.read_oriented_frames(np.zeros((2, H, 2 * W, 3), np.uint8)[:, :, ::2], 'views', 'bgr', 3)   # pixels six bytes apart
    with pytest.raises(ValueError, match='out= takes the records of device frames only'):
        r.read_oriented_frames(bgr, 'views', 'bgr', 3, out=np.zeros(4))
    assert len(r.ctx.calls) == calls


def orient_kernels(lib=None):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    return {k: d for (k, d) in kernel_meta.kernel_metadata(lib).items() if 'orient' in k}


def test_kernel_metadata_and_names():
    """The four k_orient_tiles instantiations are in the product library and in the diagnostic one: wave size 64, no private
    segment, no spilled registers, LDS within 64 KB; their names -- argument and template types included -- contain neither
    `gather` nor `k_plane_rows` nor any substring the other metadata tests count kernels by."""
    src = open(os.path.join(ROOT, 'meterelf_amd', 'csrc', 'k_orient.hip')).read()
    assert '\n%s(' % KERNEL in src
    for lib in (None, os.path.join(ROOT, 'meterelf_amd', 'csrc', 'libmeterelf_hip_diag.so')):
        new = orient_kernels(lib)
        assert len(new) == 4 and all(KERNEL in k for k in new), (lib, list(new))
        assert sorted(re.search(r'k_orient_tilesILi(\d)E', k).group(1) for k in new) == ['1', '2', '3', '4'], list(new)
        for (name, d) in new.items():
            for sub in COUNTED + ('gather', 'k_plane_rows'):
                assert sub not in name, (name, sub)
            assert d['wavefront_size'] == 64 and d.get('private_segment_fixed_size', 0) == 0, d
            assert d.get('vgpr_spill_count', 0) == 0 and d.get('sgpr_spill_count', 0) == 0, d
            assert 0 < d['group_segment_fixed_size'] <= 65536, d


# ------------------------------------------------------------------------------------------------------------------- GPU ---
@pytest.fixture(scope='module')
def src():
    return flc.synth_source(N)


def tight_descriptor(name, n, H, W):
    """(family, the tight descriptor) of the stage-entry test's layouts"""
    hw = H * W
    return {
        'bgr': lambda: ('views', _hip.MelfFrames(_hip.PIX_BGR, n, H, W, W * 3, hw * 3)),
        'bgra': lambda: ('views', _hip.MelfFrames(_hip.PIX_BGRA, n, H, W, W * 4, hw * 4)),
        'planar-rgb': lambda: ('planar', _hip.MelfPlanarFrames(n, H, W, 0, 2 * hw, hw, 0, W, 3 * hw)),
        'nv12': lambda: ('yuv', _hip.MelfYuvFrames(_hip.YUV_NV12, 0, n, H, W, 0, W, W, hw, hw + 1, hw * 3 // 2)),
        'i420': lambda: ('yuv', _hip.MelfYuvFrames(_hip.YUV_I420, 0, n, H, W, 0, W, W // 2, hw, hw + hw // 4, hw * 3 // 2)),
        'i444': lambda: ('yuv_planar', _hip.MelfYuvPlanarFrames(0, n, H, W, 0, 0, 1, 0, W, W, hw, 2 * hw, 3 * hw)),
        'p010': lambda: ('yuv16', _hip.MelfYuv16Frames(3, n, H, W, 1, 2, 8, 0, 2 * W, 2 * W, 2 * hw, 2 * hw + 2, 3 * hw)),
    }[name]()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['bgr', 'bgra', 'planar-rgb', 'nv12', 'i420', 'i444', 'p010'])
def test_orient_frames_bytes(env, name):  # noqa: F811
    """melf_orient_frames against oriented_cases.orient of every plane: codes 2-8 (and 1), three frames of random bytes at padded
    pitches and strides, H and W each from 2, 6, 64 (the tile), 66 and 130 (more than two tiles)."""
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(7)
    for H in (2, 6, 64, 66, 130):
        for W in (2, 6, 64, 66, 130):
            (family, tight) = tight_descriptor(name, 3, H, W)
            d = oc.relayout(family, tight, H, W, pad=1)
            assert d.frame_stride > oc.frame_extent(family, d) and oc.plane_table(family, d)[0][4] > oc.plane_table(family, tight)[0][4]
            planes = [rng.integers(0, 256, (3, rows, cols, eb), dtype=np.uint8) for (_o, rows, cols, eb, _p, _f) in oc.plane_table(family, d)]
            buf = oc.pack(family, d, planes, rng)
            for code in oc.CODES:
                want = oc.tight_oriented(family, d, buf, code)
                got = ctx.orient_frames(family, d, code, buf.ctypes.data, want.nbytes)
                assert got.tobytes() == want.tobytes(), (name, H, W, code)


def upright(src, layout, fmt, n, seed=5):  # noqa: F811
    """(the view of the upright batch of n frames, its descriptor, its bytes); the array stays alive with the view"""
    (arr, view, _kw) = flc.make(src, layout, fmt, np.random.default_rng(seed))
    v = view(arr[:n])
    assert not v.copied and v.n == n
    return v, flc.descriptor(v), oc.as_buffer(v)


def can_transpose(layout, d):
    return not ((layout == 'yuv_planar' and d.sub_x != d.sub_y) or (layout == 'yuv16' and d.sub_y != 1))


def oriented_dev(ctx, layout, d_up, up_buf, code, pad=0, **kw):
    """melf_process_oriented_dev on the stored batch of an upright one, the stored batch a device allocation of exactly its extent"""
    (d, buf) = oc.stored_batch(layout, d_up, up_buf, code, pad, np.random.default_rng(code))
    dev = fc.DevBuf(buf.ctypes.data, len(buf))
    try:
        return ctx.process_oriented_dev(layout, d, code, dev.d.value, **kw)
    finally:
        dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', ORIENTABLE, ids=['%s-%s' % lf for lf in ORIENTABLE])
def test_parity_every_format(env, src, layout, fmt):  # noqa: F811
    """Every format name of the six families, 1 frame and 33, under rot180 (3) and rot90cw (6): the records equal the family's _dev
    call on the upright batch.  A subsampling that does not transpose (4:2:2, 4:4:0) is MELF_ERR_INVALID under 6."""
    ctx = env['sample-images1']['reader'].ctx
    for n in (1, N):
        (v, d_up, up_buf) = upright(src, layout, fmt, n)
        whole = fc.DevBuf(v.ptr, v.extent)
        try:
            want = flc.dev_batch(ctx, layout, whole.d.value, d_up)
        finally:
            whole.free()
        if n > 1:
            ok_enough(want)
        for code in (3, 6):
            if code == 6 and not can_transpose(layout, d_up):
                with pytest.raises(_hip.HipError, match='sub_x == sub_y'):
                    ctx.process_oriented_dev(layout, d_up, code, v.ptr)   # (a host address: the call does not get as far as reading it)
                continue
            got = oriented_dev(ctx, layout, d_up, up_buf, code)
            assert got.tobytes() == want.tobytes(), (layout, fmt, n, code)


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', ONE_PER_FAMILY, ids=['%s-%s' % lf for lf in ONE_PER_FAMILY])
def test_parity_every_code(env, src, layout, fmt):  # noqa: F811
    """One format per family under all eight codes, tight and padded pitches; the host call's records equal the device call's."""
    ctx = env['sample-images1']['reader'].ctx
    (v, d_up, up_buf) = upright(src, layout, fmt, N)
    whole = fc.DevBuf(v.ptr, v.extent)
    try:
        want = flc.dev_batch(ctx, layout, whole.d.value, d_up)
    finally:
        whole.free()
    ok_enough(want)
    for code in oc.CODES:
        for pad in (0, 1):
            got = oriented_dev(ctx, layout, d_up, up_buf, code, pad)
            assert got.tobytes() == want.tobytes(), (layout, fmt, code, pad)
        (d, buf) = oc.stored_batch(layout, d_up, up_buf, code, 1, np.random.default_rng(code))
        assert ctx.process_oriented(layout, d, code, buf.ctypes.data).tobytes() == want.tobytes(), (layout, fmt, code, 'host')


GEOMETRY = {
    # (oriented frames cut to (H, W), rolled by (dy, dx)), meter_rect, codes
    'odd-origin': (((412, 302), (1, 1)), (51, 161, 301, 411), (2, 3, 5, 6)),
    'far-edges': (((410, 300), (0, 0)), (50, 160, 300, 410), (3, 4, 6, 8)),
    'origin-at-end-of-buffer': (((410, 300), (-160, -50)), (0, 0, 250, 250), (3, 6, 7, 8)),
}
GEOMETRY_FORMATS = [('views', 'bgr'), ('views', 'bgra'), ('yuv', 'nv12'), ('yuv', 'i420'), ('yuv16', 'p010'), ('packed32', 'y410'), ('planar', 'rgb')]


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(GEOMETRY))
def test_geometry(tmp_path, case):
    """Rectangles on the oriented frame (frame_cases.params_with_rect): an odd origin; oriented frames cut to 410 x 300 so that the
    rect touches both far edges; and a rect at (0, 0) under codes 3, 6, 7 and 8 with the stored batch the last thing in its
    allocation (DevBuf.at_end), so that the crop's source ends at the buffer's last byte.  The last frame reads FRAME_OK.  (A
    correct kernel stays inside every buffer: nothing is provoked.)"""
    from meterelf_amd import MeterReader
    (((H, W), (dy, dx)), rect, codes) = GEOMETRY[case]
    (base, _mx, _my) = fc.corner_frames()
    bgr = np.ascontiguousarray(np.roll(base, (dy, dx), axis=(1, 2))[:, :H, :W])
    source = flc.Source(bgr)
    r = MeterReader(fc.params_with_rect(tmp_path, 'sample-images1', rect, case))
    try:
        for (layout, fmt) in GEOMETRY_FORMATS:
            (v, d_up, up_buf) = upright(source, layout, fmt, len(bgr), seed=1)
            whole = fc.DevBuf(v.ptr, v.extent)
            try:
                want = flc.dev_batch(r.ctx, layout, whole.d.value, d_up)
            finally:
                whole.free()
            assert int(want['status'][-1]) == _hip.FRAME_OK
            ok_enough(want)
            for code in codes:
                (d, buf) = oc.stored_batch(layout, d_up, up_buf, code, 0)
                assert len(buf) == oc.batch_extent(layout, d)
                dev = fc.DevBuf.at_end(buf.ctypes.data, len(buf), 0)
                try:
                    got = r.ctx.process_oriented_dev(layout, d, code, dev.d.value)
                finally:
                    dev.free()
                assert got.tobytes() == want.tobytes(), (case, layout, fmt, code)
    finally:
        r.close()


@pytest.mark.gpu
def test_the_orientation_is_timed_as_the_gather(env, src):  # noqa: F811
    """melf_ctx_timings: code 1 launches no MELF_K_GATHER kernel (it is the family's in-place call), codes 2-8 one per call."""
    ctx = env['sample-images1']['reader'].ctx
    (v, d_up, up_buf) = upright(src, 'views', 'bgr', N)
    try:
        ctx.set_profiling(1)
        ctx.timings()
        for code in oc.CODES:
            oriented_dev(ctx, 'views', d_up, up_buf, code)
            t = ctx.timings()
            assert t['k_gather'][1] == (0 if code == 1 else 1) and t['k_dials'][1] == 1, (code, t)
            assert code == 1 or t['k_gather'][0] > 0
    finally:
        ctx.set_profiling(0)


@pytest.mark.gpu
def test_two_chunks(env, src):  # noqa: F811
    """1025 frames of 412 x 302 BGR (33 distinct ones tiled) run as two chunks of the lane's staged batch: two launches of the
    kernel, and every record correct."""
    ctx = env['sample-images1']['reader'].ctx
    few = np.ascontiguousarray(src.bgr[:, :412, :302])
    d33 = _hip.MelfFrames(_hip.PIX_BGR, N, 412, 302, 302 * 3, 412 * 302 * 3)
    whole = fc.DevBuf(few.ctypes.data, few.nbytes)
    try:
        want33 = flc.dev_batch(ctx, 'views', whole.d.value, d33)
    finally:
        whole.free()
    ok_enough(want33)
    n = 1025
    reps = -(-n // N)
    stored = np.ascontiguousarray(np.tile(oc.orient(few, oc.inverse(6), axes=(1, 2)), (reps, 1, 1, 1))[:n])
    d = _hip.MelfFrames(_hip.PIX_BGR, n, 302, 412, 412 * 3, 412 * 302 * 3)
    dev = fc.DevBuf(stored.ctypes.data, stored.nbytes)
    try:
        ctx.set_profiling(1)
        ctx.timings()
        got = ctx.process_oriented_dev('views', d, 6, dev.d.value)
        t = ctx.timings()
    finally:
        ctx.set_profiling(0)
        dev.free()
    assert t['k_gather'][1] == 2 and t['k_dials'][1] == 2, t
    assert got.tobytes() == np.tile(want33, reps)[:n].tobytes()


@pytest.mark.gpu
def test_two_caller_streams(env, src):  # noqa: F811
    """Two caller streams with two different stored batches (two orientations of two different upright batches), frames-resident
    mode off and on, records to a device buffer: each call gets its own records."""
    from meterelf_amd import MeterReader
    hip = fc.hip_rt()
    rsz = _hip.RESULT_DTYPE.itemsize
    r = MeterReader(env['sample-images1']['params'])
    (v, d_up, up_buf) = upright(src, 'yuv', 'nv12', N)
    # the second upright batch: the first in reverse order
    rev_buf = np.ascontiguousarray(up_buf.reshape(N, -1)[::-1]).reshape(-1)
    whole = fc.DevBuf(v.ptr, v.extent)
    streams = [C.c_void_p(), C.c_void_p()]
    d_res = C.c_void_p()
    devs = []
    try:
        want = flc.dev_batch(r.ctx, 'yuv', whole.d.value, d_up)
        ok_enough(want)
        assert len(set(x.tobytes() for x in want)) > N // 2   # the records tell the frames apart
        for s in streams:
            assert hip.hipStreamCreate(C.byref(s)) == 0
        assert hip.hipMalloc(C.byref(d_res), C.c_size_t(4 * N * rsz)) == 0
        calls = []
        for (i, (ub, code)) in enumerate([(up_buf, 6), (rev_buf, 3), (up_buf, 7), (rev_buf, 8)]):
            (d, buf) = oc.stored_batch('yuv', d_up, ub, code, i % 2)
            devs.append(fc.DevBuf(buf.ctypes.data, len(buf)))
            calls.append((d, code, devs[-1].d.value, want if ub is up_buf else want[::-1]))
        for resident in (False, True):
            r.ctx.set_frames_resident(resident)
            assert hip.hipMemset(d_res, 0, C.c_size_t(4 * N * rsz)) == 0
            for (i, (d, code, ptr, _w)) in enumerate(calls):
                r.ctx.process_oriented_dev('yuv', d, code, ptr, d_results_ptr=d_res.value + i * N * rsz, want_host=False, stream=streams[i % 2].value)
            r.ctx.sync()
            got = np.zeros(4 * N, _hip.RESULT_DTYPE)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), d_res, C.c_size_t(got.nbytes), 2) == 0
            for (i, (_d, code, _p, w)) in enumerate(calls):
                assert got[i * N:(i + 1) * N].tobytes() == w.tobytes(), (resident, i, code)
        r.ctx.set_frames_resident(False)
    finally:
        r.ctx.sync()
        r.close()
        if d_res.value:
            hip.hipFree(d_res)
        for s in streams:
            if s.value:
                hip.hipStreamDestroy(s)
        for b in devs:
            b.free()
        whole.free()


@pytest.mark.gpu
def test_argument_errors(env, src):  # noqa: F811
    """MELF_ERR_INVALID with a message that says which rule, before anything is launched or copied; n == 0 passes."""
    ctx = env['sample-images1']['reader'].ctx
    L = ctx._L
    (v, d_up, _buf) = upright(src, 'views', 'bgr', 4)
    out = np.zeros(4, _hip.RESULT_DTYPE)
    tight = np.zeros(4 * v.H * v.W * 3, np.uint8)

    def call(family, d, code, ptr, entry='dev', out_ptr=out.ctypes.data):
        dref = C.byref(d) if d is not None else None
        if entry == 'host':
            rc = L.melf_process_oriented(ctx._h, family, dref, code, C.c_void_p(ptr), C.c_void_p(out_ptr))
        elif entry == 'stage':
            rc = L.melf_orient_frames(ctx._h, family, dref, code, C.c_void_p(ptr), C.c_void_p(tight.ctypes.data if out_ptr else None), tight.nbytes)
        else:
            rc = L.melf_process_oriented_dev(ctx._h, family, dref, code, C.c_void_p(ptr), None, C.c_void_p(out_ptr), None)
        return rc, L.melf_last_error().decode()
    i422 = _hip.MelfYuvPlanarFrames(0, 4, 12, 16, 1, 0, 1, 0, 16, 8, 192, 288, 384)
    p210 = _hip.MelfYuv16Frames(3, 4, 12, 16, 0, 2, 8, 0, 32, 32, 384, 386, 768)
    yuyv = _hip.MelfYuv422Frames(0, 0, 4, 12, 16, 0, 32, 384)
    y210 = _hip.MelfYuv422_10Frames(1, 3, 4, 12, 16, 0, 64, 768)
    ctx.set_profiling(1)
    ctx.timings()
    before = fc.launch_counts(ctx)
    for entry in ('dev', 'host', 'stage'):
        for code in (0, 9, -1):
            (rc, msg) = call(0, d_up, code, v.ptr, entry)
            assert rc == ERR_INVALID and 'orientation outside 1 .. 8' in msg, (entry, code, msg)
        for (family, d) in ((2, yuyv), (5, y210)):
            for code in (1, 3, 6):
                (rc, msg) = call(family, d, code, v.ptr, entry)
                assert rc == ERR_INVALID and 'not a permutation' in msg, (entry, family, code, msg)
        for family in (-1, 8):
            (rc, msg) = call(family, d_up, 3, v.ptr, entry)
            assert rc == ERR_INVALID and 'unknown family' in msg, (entry, family, msg)
        (rc, msg) = call(3, i422, 5, v.ptr, entry)
        assert rc == ERR_INVALID and 'sub_x == sub_y' in msg, (entry, msg)
        (rc, msg) = call(4, p210, 6, v.ptr, entry)
        assert rc == ERR_INVALID and 'sub_y == 1' in msg, (entry, msg)
        (rc, msg) = call(0, None, 3, v.ptr, entry)
        assert rc == ERR_INVALID and 'descriptor is NULL' in msg, (entry, msg)
        (rc, msg) = call(0, d_up, 3, None, entry)
        assert rc == ERR_INVALID and 'frames pointer is NULL' in msg, (entry, msg)
        if entry != 'dev':   # (the device call's out_host may be NULL: the records stay in HBM)
            (rc, msg) = call(0, d_up, 3, v.ptr, entry, out_ptr=None)
            assert rc == ERR_INVALID and 'out_host is NULL' in msg, (entry, msg)
        empty = oc.copy_desc(d_up)
        empty.n = 0
        assert call(0, empty, 3, None, entry)[0] == 0
    rc = L.melf_orient_frames(ctx._h, 0, C.byref(d_up), 3, C.c_void_p(v.ptr), C.c_void_p(tight.ctypes.data), tight.nbytes - 1)
    assert rc == ERR_INVALID and 'out_bytes' in L.melf_last_error().decode()
    rc = L.melf_process_oriented_dev(None, 0, C.byref(d_up), 3, C.c_void_p(v.ptr), None, C.c_void_p(out.ctypes.data), None)
    assert rc == ERR_INVALID and 'ctx is NULL' in L.melf_last_error().decode()
    assert fc.launch_counts(ctx) == before
    ctx.set_profiling(0)


@pytest.mark.gpu
def test_an_oriented_frame_too_small_for_the_crop(env):  # noqa: F811
    """The oriented frame must hold the crop and the template as the family's call requires of an upright frame: a stored 640 x 20
    batch is 20 x 640 under rot90cw, and gives the family's own error, from both calls."""
    ctx = env['sample-images1']['reader'].ctx
    (H, W) = (640, 20)
    d = _hip.MelfFrames(_hip.PIX_BGR, 2, H, W, W * 3, H * W * 3)
    frames = np.zeros(2 * H * W * 3, np.uint8)
    upright_d = _hip.MelfFrames(_hip.PIX_BGR, 2, W, H, H * 3, H * W * 3)
    dev = fc.DevBuf(frames.ctypes.data, frames.nbytes)
    try:
        with pytest.raises(_hip.HipError) as own:
            flc.dev_batch(ctx, 'views', dev.d.value, upright_d)
        for call in (lambda: ctx.process_oriented_dev('views', d, 6, dev.d.value), lambda: ctx.process_oriented('views', d, 6, frames.ctypes.data)):
            with pytest.raises(_hip.HipError) as e:
                call()
            assert str(e.value) == str(own.value) and 'smaller than the dials template' in str(e.value)
    finally:
        dev.free()


@pytest.mark.gpu
def test_read_oriented_frames_in_a_torch_process():
    """MeterReader.read_oriented_frames with a CUDA tensor batch, orientation='rot90cw' and out=, against read_frame_views of
    torch.rot90(frames, -1, (1, 2)).contiguous(), and the other layouts and the host path, in a child process that imports torch
    first (tests/frame_cases.py says why)."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'oriented_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch oriented path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
