"""Frames in separate allocations: melf_process_frame_list / melf_process_frame_list_dev, MeterReader.read_frame_list, the staging
plans of melf_stage_plan.h and the gather kernel k_gather_rows.

The parity bar everywhere is byte equality of the records with the family's own call on one contiguous batch holding the same
frames in list order: there is no tolerance.  In every parity test at least three quarters of the reference batch's records are
FRAME_OK (frame_cases.synth makes every ninth frame constant: 29 of 33 read), so failure records are not compared with failure
records."""
import ctypes as C
import os
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
from tests.frame_cases import env  # noqa: E402,F401

KERNEL = 'k_gather_rows'
# the substrings existing metadata tests count kernels by: the new kernel's name may contain none of them
COUNTED = ('k_dials', 'k_prep_lplane', 'k_needles', 'k_yneedle', 'k_lplane_yuv', 'k_match_yuv', 'k_yuv2bgr', 'k_lplane_px4', 'k_match_px4',
           'k_p422_', 'k_yp_', 'k_y16_', 'k_v210_', 'k_y210_', 'k_p32_', 'k_planar_', 'k_match_mfma', 'k_match_gen', 'k_fused_mask', 'k_jpeg_',
           'k_bgr2hls', 'k_stream_probe')
N = 33   # one 32-frame match group plus one
ERR_INVALID = -1   # MELF_ERR_INVALID


def ok_enough(want):
    assert 4 * int((want['status'] == _hip.FRAME_OK).sum()) >= 3 * len(want), want['status']


# ------------------------------------------------------------------------------------------------------------------- CPU ---
def test_stage_runs_on_the_cpu(tmp_path):
    """tests/stage_runs_main.cpp, plain and under the host sanitizers: every family's plan over small descriptors, its row runs
    executed through the functions of melf_gather_addr.h -- the kernel's own -- on frames malloc'd to exactly the extent.  Every
    family saw accepted cases with odd origins and with rectangles touching the frame's edges."""
    import re
    from tests import test_dials_instantiations as di
    (cxx, inc) = di.rocm_clangxx()
    out = fc.build_and_run(tmp_path, cxx, os.path.join(ROOT, 'tests', 'stage_runs_main.cpp'), 'stage_runs', ['-D__HIP_PLATFORM_AMD__', '-I' + inc],
                           ['-fsanitize=address,undefined'])
    seen = {m.group(1): tuple(int(m.group(k)) for k in (2, 3, 4, 5, 6))
            for m in re.finditer(r'family (\w+): cases (\d+) odd_origin (\d+) edge (\d+) rejected \d+ full_pieces (\d+) tail_pieces (\d+)', out)}
    assert sorted(seen) == sorted(['frames', 'yuv', 'yuv422', 'yuv_planar', 'yuv16', 'yuv422_10', 'packed32', 'planes']), out
    for (fam, (cases, odd, edge, full, tail)) in seen.items():
        assert cases > 1000 and odd > 100 and edge > 100 and full > 0 and tail > 0, (fam, out)


def gather_kernels(lib=None):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    return {k: d for (k, d) in kernel_meta.kernel_metadata(lib).items() if 'gather' in k}


def test_kernel_name_collides_with_no_counted_substring():
    """The metadata tests of the other kernels count kernels by substrings of their names: the gather kernel's name -- in the source
    and as the library exports it -- contains none of them, so a rename cannot silently break those counts."""
    src = open(os.path.join(ROOT, 'meterelf_amd', 'csrc', 'k_gather.hip')).read()
    assert '\n%s(' % KERNEL in src
    names = list(gather_kernels()) + [KERNEL]
    assert len(names) == 2 and KERNEL in names[0]
    for name in names:
        for sub in COUNTED:
            assert sub not in name, (name, sub)


def test_gather_kernel_metadata():
    """k_gather_rows is in the product library and in the diagnostic one, once each: wave size 64, no private segment, no spilled
    registers."""
    for lib in (None, os.path.join(ROOT, 'meterelf_amd', 'csrc', 'libmeterelf_hip_diag.so')):
        new = gather_kernels(lib)
        assert len(new) == 1 and KERNEL in list(new)[0], (lib, list(new))
        (d,) = new.values()
        assert d['wavefront_size'] == 64 and d.get('private_segment_fixed_size', 0) == 0, d
        assert d.get('vgpr_spill_count', 0) == 0 and d.get('sgpr_spill_count', 0) == 0, d


def test_exports_and_codes():
    """The two entry points are exported, the diagnostic gather-alone entry is not; the family codes are the header's."""
    import re
    L = _hip.lib()
    assert hasattr(L, 'melf_process_frame_list') and hasattr(L, 'melf_process_frame_list_dev')
    if 'MELF_LIB_PATH' not in os.environ:
        assert not hasattr(L, 'melf_gather_frame_list_dev')
    text = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'MELF_LIST_(\w+) = (\d)', text)}
    assert codes == {'frames': 0, 'yuv': 1, 'yuv422': 2, 'yuv_planar': 3, 'yuv16': 4, 'yuv422_10': 5, 'packed32': 6, 'planes': 7}
    assert sorted(_hip.LIST_FAMILIES.values()) == list(range(8)) and set(_hip.LIST_FAMILIES) == set(flc.ENTRY)
    assert 'frames in separate allocations: melf_process_frame_list*; a frame\'s planes in separate allocations are still not there' in text


# ------------------------------------------------------------------------------------------------------------------- GPU ---
@pytest.fixture(scope='module')
def src():
    return flc.synth_source(N)


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', flc.FORMATS, ids=['%s-%s' % lf for lf in flc.FORMATS])
def test_parity(env, src, layout, fmt):  # noqa: F811
    """Every family, every format name its view function accepts, 1 frame and 33: every frame a device allocation of its own of
    exactly one frame's extent, allocated in shuffled order with spacers of differing sizes between them (the addresses are not one
    stride apart: asserted); the records of melf_process_frame_list_dev equal the family's _dev call on the contiguous copy."""
    ctx = env['sample-images1']['reader'].ctx
    (arr, view, _kw) = flc.make(src, layout, fmt, np.random.default_rng(5))
    for n in (1, N):
        v = view(arr[:n])
        assert not v.copied and v.n == n
        desc = flc.descriptor(v)
        whole = fc.DevBuf(v.ptr, v.extent)
        frames = flc.DevFrames(v, np.random.default_rng(n))
        try:
            want = flc.dev_batch(ctx, layout, whole.d.value, desc)
            ok_enough(want)
            if n > 1:
                assert len(set(frames.spread())) > 1, 'the frames lie one stride apart'
            desc.frame_stride = 0   # not looked at
            got = ctx.process_frame_list_dev(layout, desc, frames.ptrs)
            assert got.tobytes() == want.tobytes(), (layout, fmt, n)
        finally:
            frames.free()
            whole.free()


@pytest.mark.gpu
def test_the_table_is_what_is_read(env, src):  # noqa: F811
    """The list reversed, and a list with one pointer repeated, give the correspondingly permuted and repeated records."""
    ctx = env['sample-images1']['reader'].ctx
    (arr, view, _kw) = flc.make(src, 'views', 'bgr', np.random.default_rng(5))
    v = view(arr)
    desc = flc.descriptor(v)
    whole = fc.DevBuf(v.ptr, v.extent)
    frames = flc.DevFrames(v, np.random.default_rng(2))
    try:
        want = flc.dev_batch(ctx, 'views', whole.d.value, desc)
        ok_enough(want)
        assert len(set(r.tobytes() for r in want)) > N // 2   # the records tell the frames apart
        assert ctx.process_frame_list_dev('views', desc, frames.ptrs[::-1]).tobytes() == want[::-1].tobytes()
        order = list(range(N))
        order[7] = order[20] = 3
        assert ctx.process_frame_list_dev('views', desc, [frames.ptrs[i] for i in order]).tobytes() == want[order].tobytes()
    finally:
        frames.free()
        whole.free()


ENDS_PHASES = {'views-bgr': (0, 1, 2, 3), 'views-bgra': (0,), 'yuv-nv12': (0, 1, 2, 3), 'yuv-i420': (0, 1, 2, 3), 'yuv422-yuyv': (0,),
               'yuv_planar-i422': (0, 1, 2, 3), 'yuv_planar-nv24': (0, 1, 2, 3), 'yuv16-p010': (0, 2), 'yuv422_10-v210': (0,), 'yuv422_10-y210': (0,),
               'packed32-y410': (0,), 'planar-rgb': (0, 1, 2, 3)}


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', flc.RUN_SHAPES, ids=['%s-%s' % lf for lf in flc.RUN_SHAPES])
def test_per_frame_ends_of_mappings(tmp_path, layout, fmt):
    """frame_cases.ENDS_CASES: meter_rect ending on the frame's last row and column, and the odd-origin variant.  EVERY frame of the
    list ends where its own allocation ends (DevBuf.at_end), at every base phase the family's check accepts: a load past any single
    frame's extent would leave its mapping.  One format per distinct shape of the row runs.  The last frame reads FRAME_OK and the
    records equal read_frames of the BGR frames.  (A correct kernel stays inside every buffer: nothing is provoked.)"""
    from meterelf_amd import MeterReader
    (base, _mx, _my) = fc.corner_frames()
    for (case, ((H, W), (dx, dy))) in enumerate(fc.ENDS_CASES):
        params = fc.params_with_rect(tmp_path, 'sample-images1', (50 + dx, 160 + dy, 300 + dx, 410 + dy), 'ends%d' % case)
        bgr = np.ascontiguousarray(np.roll(base, (dy, dx), axis=(1, 2))[:, :H, :W])
        source = flc.Source(bgr)
        (arr, view, _kw) = flc.make(source, layout, fmt, np.random.default_rng(case))
        v = view(arr)
        assert not v.copied
        desc = flc.descriptor(v)
        r = MeterReader(params)
        try:
            want = r.read_frames(flc.reference_bgr(source, layout, fmt))   # the BGR reference of the family's contract
            assert int(want['status'][-1]) == _hip.FRAME_OK
            ok_enough(want)
            for phase in ENDS_PHASES['%s-%s' % (layout, fmt)]:
                frames = flc.DevFrames(v, np.random.default_rng(phase), at_end=True, phase=phase)
                try:
                    assert all(p % 4 == phase for p in frames.ptrs)
                    got = r.ctx.process_frame_list_dev(layout, desc, frames.ptrs)
                finally:
                    frames.free()
                assert got.tobytes() == want.tobytes(), (layout, fmt, case, phase)
        finally:
            r.close()


@pytest.mark.gpu
def test_lanes_and_ordering(env, src):  # noqa: F811
    """Two caller streams alternately, four calls with different lists, frames-resident mode off and on; two calls back to back on
    one stream with different lists (the lane's staging buffer is reused); and a list whose frames are written by a copy enqueued on
    the same stream just before the call.  Every call's records equal the contiguous read's."""
    from meterelf_amd import MeterReader
    hip = fc.hip_rt()
    rsz = _hip.RESULT_DTYPE.itemsize
    (arr, view, _kw) = flc.make(src, 'yuv', 'nv12', np.random.default_rng(5))
    v = view(arr)
    desc = flc.descriptor(v)
    r = MeterReader(env['sample-images1']['params'])
    whole = fc.DevBuf(v.ptr, v.extent)
    frames = flc.DevFrames(v, np.random.default_rng(4))
    streams = [C.c_void_p(), C.c_void_p()]
    d_res = C.c_void_p()
    late = None
    try:
        want = flc.dev_batch(r.ctx, 'yuv', whole.d.value, desc)
        ok_enough(want)
        orders = [list(range(N)), list(range(N))[::-1], [(7 * i) % N for i in range(N)], [(5 * i + 3) % N for i in range(N)]]
        for s in streams:
            assert hip.hipStreamCreate(C.byref(s)) == 0
        assert hip.hipMalloc(C.byref(d_res), C.c_size_t(4 * N * rsz)) == 0

        def fetch():
            got = np.zeros(4 * N, _hip.RESULT_DTYPE)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), d_res, C.c_size_t(got.nbytes), 2) == 0
            assert hip.hipMemset(d_res, 0, C.c_size_t(got.nbytes)) == 0
            return got
        for resident in (False, True):
            r.ctx.set_frames_resident(resident)
            for (i, order) in enumerate(orders):
                r.ctx.process_frame_list_dev('yuv', desc, [frames.ptrs[k] for k in order], d_results_ptr=d_res.value + i * N * rsz, want_host=False,
                                             stream=streams[i % 2].value)
            r.ctx.sync()
            got = fetch()
            for (i, order) in enumerate(orders):
                assert got[i * N:(i + 1) * N].tobytes() == want[order].tobytes(), (resident, i)
            # back to back on one stream: the second call's gather overwrites the staged batch the first call's kernels read
            for (i, order) in enumerate(orders[:2]):
                r.ctx.process_frame_list_dev('yuv', desc, [frames.ptrs[k] for k in order], d_results_ptr=d_res.value + i * N * rsz, want_host=False,
                                             stream=streams[0].value)
            r.ctx.sync()
            got = fetch()
            for (i, order) in enumerate(orders[:2]):
                assert got[i * N:(i + 1) * N].tobytes() == want[order].tobytes(), (resident, 'back to back', i)
            # frames written on the stream just before the call: a zeroed allocation filled by an asynchronous copy from the
            # contiguous batch; the gather must see the copy's bytes
            late = fc.DevBuf(np.zeros(v.extent, np.uint8).ctypes.data, v.extent)
            assert hip.hipMemcpyAsync(late.d, whole.d, C.c_size_t(v.extent), 3, streams[1]) == 0
            got = r.ctx.process_frame_list_dev('yuv', desc, [late.d.value + k * v.frame_stride for k in range(N)], stream=streams[1].value)
            assert got.tobytes() == want.tobytes(), (resident, 'written just before')
            late.free()
            late = None
        r.ctx.set_frames_resident(False)
    finally:
        r.ctx.sync()
        r.close()
        if late is not None:
            late.free()
        if d_res.value:
            hip.hipFree(d_res)
        for s in streams:
            if s.value:
                hip.hipStreamDestroy(s)
        frames.free()
        whole.free()


@pytest.mark.gpu
def test_argument_errors(env, src):  # noqa: F811
    """MELF_ERR_INVALID with a message that names the frame's index or the rule; n == 0 succeeds.  Nothing is launched."""
    ctx = env['sample-images1']['reader'].ctx
    L = ctx._L
    (arr, view, _kw) = flc.make(src, 'yuv422', 'yuyv', np.random.default_rng(5))
    v = view(arr[:4])
    desc = flc.descriptor(v)
    good = [v.ptr + i * v.frame_stride for i in range(4)]   # host addresses: no call below gets as far as reading them
    out = np.zeros(4, _hip.RESULT_DTYPE)

    def call(family, d, ptrs, host=False):
        table = flc.pointer_table(ptrs) if ptrs is not None else None
        dref = C.byref(d) if d is not None else None
        if host:
            rc = L.melf_process_frame_list(ctx._h, family, dref, table, out.ctypes.data_as(C.c_void_p))
        else:
            rc = L.melf_process_frame_list_dev(ctx._h, family, dref, table, None, out.ctypes.data_as(C.c_void_p), None)
        return rc, L.melf_last_error().decode()
    ctx.set_profiling(1)
    ctx.timings()
    before = fc.launch_counts(ctx)
    for host in (False, True):
        (rc, msg) = call(2, None, good, host)
        assert rc == ERR_INVALID and 'descriptor is NULL' in msg, msg
        (rc, msg) = call(2, desc, [good[0], good[1], None, good[3]], host)
        assert rc == ERR_INVALID and 'frame 2 of the list' in msg and 'NULL' in msg, msg
        (rc, msg) = call(2, desc, [good[0], good[1] + 2, good[2], good[3]], host)
        assert rc == ERR_INVALID and 'frame 1 of the list' in msg and '4-byte aligned base' in msg, msg
        for family in (-1, 8):
            (rc, msg) = call(family, desc, good, host)
            assert rc == ERR_INVALID and 'unknown family' in msg, msg
        bad = flc.descriptor(v)
        bad.W = v.W + 1   # odd
        (rc, msg) = call(2, bad, good, host)
        assert rc == ERR_INVALID and 'even width' in msg, msg
        (rc, msg) = call(2, desc, None, host)
        assert rc == ERR_INVALID and 'array of frame pointers is NULL' in msg, msg
        empty = flc.descriptor(v)
        empty.n = 0
        (rc, msg) = call(2, empty, None, host)
        assert rc == 0
    assert fc.launch_counts(ctx) == before
    ctx.set_profiling(0)
    assert _hip.ABI_VERSION == 3


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', flc.ONE_PER_FAMILY, ids=['%s-%s' % lf for lf in flc.ONE_PER_FAMILY])
def test_host_lists(env, src, layout, fmt):  # noqa: F811
    """A list of separately allocated numpy arrays through melf_process_frame_list equals the family's host call on their stack
    (and that equals the device call: the host path's records do not change)."""
    ctx = env['sample-images1']['reader'].ctx
    (arr, view, _kw) = flc.make(src, layout, fmt, np.random.default_rng(5))
    v = view(arr)
    desc = flc.descriptor(v)
    want = flc.host_batch(ctx, layout, v.ptr, desc)
    ok_enough(want)
    ext = flc.frame_extent(v)
    flat = np.lib.stride_tricks.as_strided(np.frombuffer((C.c_uint8 * v.extent).from_address(v.ptr), np.uint8), shape=(v.n, ext),
                                           strides=(v.frame_stride, 1))
    raw = [np.empty(ext + 64 + 16 * (i % 5), np.uint8) for i in range(v.n)]      # allocations of differing sizes
    copies = [b[-b.ctypes.data % 16:][:ext] for b in raw]                         # exactly the extent, aligned as the batch is
    for (c, f) in zip(copies, flat):
        c[...] = f
    got = ctx.process_frame_list(layout, desc, [c.ctypes.data for c in copies])
    assert got.tobytes() == want.tobytes(), (layout, fmt)


@pytest.mark.gpu
def test_gather_is_timed(env, src):  # noqa: F811
    """melf_ctx_timings counts one k_gather launch per list call (per 1024-frame chunk) and none for a batch call."""
    ctx = env['sample-images1']['reader'].ctx
    (arr, view, _kw) = flc.make(src, 'views', 'bgr', np.random.default_rng(5))
    v = view(arr)
    desc = flc.descriptor(v)
    whole = fc.DevBuf(v.ptr, v.extent)
    try:
        ctx.set_profiling(1)
        ctx.timings()
        flc.dev_batch(ctx, 'views', whole.d.value, desc)
        assert ctx.timings()['k_gather'][1] == 0
        ctx.process_frame_list_dev('views', desc, [whole.d.value + i * v.frame_stride for i in range(N)])
        t = ctx.timings()
        assert t['k_gather'][1] == 1 and t['k_gather'][0] > 0 and t['k_dials'][1] == 1
    finally:
        ctx.set_profiling(0)
        whole.free()


@pytest.mark.gpu
def test_read_frame_list_in_a_torch_process():
    """MeterReader.read_frame_list with separately allocated torch device tensors, views into one big tensor in reverse order, host
    lists, out=, and its ValueErrors, one format per family, in a child process that imports torch first (tests/frame_cases.py says
    why)."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'frame_list_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch frame list path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
