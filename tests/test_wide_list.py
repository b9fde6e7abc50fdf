"""RGB frames of wide samples in separate allocations, and wide planar frames whose planes are (melf_process_wide_list*,
melf_process_wide_plane_list*, melf_wide_list_to_bgr, MeterReader.read_wide_frame_list / read_wide_plane_list).

The contract (include/meterelf_hip.h): the records are byte-identical to melf_process_wide(_dev) on one contiguous batch holding the
same samples in list order; from each frame pointer one frame's extent is readable, from each plane pointer (H - 1) * row_pitch +
W * sample size bytes, and nothing more.

CPU tests: the stand-alone program tests/wide_list_main.cpp under the host sanitizers (exact-extent frames and planes through the
packers and the kernels' address functions; the two checks swept, every message counted), the prototypes against the header, the
argument errors of the two reader methods with a stand-in context.  GPU tests: the list kernels alone over a shape sweep
(melf_wide_list_to_bgr, byte for byte numpy's), the records of 33 fixture frames in every sample type, lists longer than a chunk,
which kernel ran, rejected calls, and torch tensors, caller streams and frames-resident mode in a child process that imports torch
first (tests/frame_cases.py says why)."""
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
from tests import wide_cases as wc  # noqa: E402
from tests import wide_list_cases as wl  # noqa: E402
from tests.frame_cases import env  # noqa: E402,F401

NEW = ('melf_process_wide_list', 'melf_process_wide_list_dev', 'melf_process_wide_plane_list', 'melf_process_wide_plane_list_dev',
       'melf_wide_list_to_bgr')


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_wide_lists_on_the_cpu(tmp_path):
    """tests/wide_list_main.cpp under -fsanitize=address,undefined: every frame and plane in a malloc block of exactly its extent,
    through the host packers and the kernels' address functions, against the batch packer; the two checks swept, all nine messages
    of their tables produced."""
    exe = wc.build(tmp_path, 'wide_list_main')
    out = wc.run([exe, 'extents'])
    assert 'extents: 2240 geometries' in out, out
    out = wc.run([exe, 'checks'])
    assert 'messages 9 of 9' in out, out


def test_prototypes_match_the_header(tmp_path):
    """The five functions as the header declares them (a C program assigns each to a pointer of the documented type: a prototype
    that differed would not compile), the descriptor and the version they leave alone, and the bindings."""
    src = tmp_path / 'wide_list.c'
    src.write_text(
        '#include <stdio.h>\n#include "meterelf_hip.h"\n'
        'int (*a)(melf_ctx*, const melf_wide_frames*, const void* const*, void*, melf_result*, void*) = melf_process_wide_list_dev;\n'
        'int (*b)(melf_ctx*, const melf_wide_frames*, const void* const*, melf_result*) = melf_process_wide_list;\n'
        'int (*c)(melf_ctx*, const melf_wide_frames*, const void* const*, int, void*, melf_result*, void*) = melf_process_wide_plane_list_dev;\n'
        'int (*d)(melf_ctx*, const melf_wide_frames*, const void* const*, int, melf_result*) = melf_process_wide_plane_list;\n'
        'int (*e)(melf_ctx*, const melf_wide_frames*, const void* const*, int, uint8_t*) = melf_wide_list_to_bgr;\n'
        'int main(void){printf("%zu %d %d %d\\n", sizeof(melf_wide_frames), MELF_ABI_VERSION, MELF_K_COUNT, MELF_K_GATHER);'
        'return !(a && b && c && d && e);}\n')
    obj = tmp_path / 'wide_list.o'
    subprocess.check_call(['gcc', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(obj)])
    exe = tmp_path / 'wide_list'
    stub = tmp_path / 'stubs.c'
    stub.write_text(''.join('int %s(void){return 0;}\n' % name for name in NEW))
    subprocess.check_call(['gcc', str(obj), str(stub), '-o', str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b'104', b'3', b'10', b'9']
    assert _hip.ABI_VERSION == 3 and C.sizeof(_hip.MelfWideFrames) == 104
    L = _hip.lib()
    vp = C.c_void_p
    W = C.POINTER(_hip.MelfWideFrames)
    want = {NEW[0]: [vp, W, vp, vp], NEW[1]: [vp, W, vp, vp, vp, vp], NEW[2]: [vp, W, vp, C.c_int, vp], NEW[3]: [vp, W, vp, C.c_int, vp, vp, vp],
            NEW[4]: [vp, W, vp, C.c_int, vp]}
    for name in NEW:
        assert name in _hip.EXPORTS and hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == want[name], name
    text = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    assert 'wide frames in the frame lists' not in text and 'MELF_LIST_WIDE' not in text
    import re
    assert len(re.findall(r'MELF_LIST_(\w+) = (\d)', text)) == 8   # no family code for the wide lists


class StandIn:
    """a context that records what would reach the library"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name, args, kw))
            return np.zeros(args[0].n, _hip.RESULT_DTYPE)
        return call


def stand_in_reader():
    from meterelf_amd import MeterReader
    r = MeterReader.__new__(MeterReader)
    r.device = 0
    r.ctx = StandIn()
    return r


class FakeDevice:
    def __init__(self, index):
        (self.type, self.index) = ('cuda', index)

    def __eq__(self, other):
        return isinstance(other, FakeDevice) and other.index == self.index


class FakeTensor:
    """What the view functions look at of a torch tensor on a GPU, over a numpy array's memory: nothing here is ever read"""
    __module__ = 'torch'

    def __init__(self, a, index=0):
        (self.a, self.dtype, self.device, self.shape, self.ndim) = (a, 'torch.' + str(a.dtype), FakeDevice(index), a.shape, a.ndim)

    def stride(self):
        return tuple(st // self.a.itemsize for st in self.a.strides)

    def data_ptr(self):
        return self.a.ctypes.data

    def __getitem__(self, key):
        return FakeTensor(self.a[key], self.device.index)


def test_read_wide_frame_list_with_a_stand_in():
    """What reaches the library -- the descriptor of one frame with n the list's length, the addresses in list order -- and every
    ValueError, before any library call."""
    r = stand_in_reader()
    (H, W) = (6, 10)
    # (H, W, 3) float32 frames, one of them a crop of a larger array: same pitch needed, so all are crops of equally wide arrays
    bigs = [np.zeros((H + 2, W + 3, 3), np.float32) for _ in range(4)]
    frames = [b[1:1 + H, 2:2 + W] for b in bigs]
    got = r.read_wide_frame_list(frames, 'hwc', 'rgb', scale=(1.0, 2.0, 3.0), rounding='floor')
    assert len(got) == 4
    ((name, (desc, ptrs), kw),) = r.ctx.calls
    assert name == 'process_wide_list' and not kw
    assert ptrs == [f.ctypes.data for f in frames] and ptrs[0] == bigs[0].ctypes.data + ((W + 3) + 2) * 12
    assert (desc.n, desc.H, desc.W, desc.layout, desc.pixel_format, desc.sample_type, desc.row_pitch, desc.rounding) == (
        4, H, W, _hip.WIDE_PACKED, _hip.PIX_RGB, _hip.WIDE_F32, (W + 3) * 12, _hip.ROUND_FLOOR)
    assert list(desc.scale) == [3.0, 2.0, 1.0] and (desc.reserved, desc.reserved2) == (0, 0)
    # planar uint16 frames
    r.ctx.calls.clear()
    chw = [np.zeros((3, H, W), np.uint16) for _ in range(3)]
    r.read_wide_frame_list(chw, 'chw', 'gbr', shift=4)
    ((name, (desc, ptrs), kw),) = r.ctx.calls
    P = H * W * 2
    assert (desc.n, desc.layout, desc.shift, desc.g_offset, desc.b_offset, desc.r_offset, desc.row_pitch) == (3, _hip.WIDE_PLANAR, 4, 0, P, 2 * P, W * 2)
    assert ptrs == [a.ctypes.data for a in chw]
    r.ctx.calls.clear()
    assert len(r.read_wide_frame_list([], 'chw', shift=8)) == 0 and not r.ctx.calls
    f32 = [np.zeros((3, H, W), np.float32) for _ in range(3)]
    for (args, kw, msg) in (
            (([f32[0], f32[1][:, :-1]], 'chw'), {}, 'frame 1 of the list differs from frame 0 in H: 5, not 6'),
            (([f32[0], f32[1], np.zeros((3, H, W + 2), np.float32)[:, :, :W]], 'chw'), {}, 'frame 2 of the list differs from frame 0 in b_offset: 576, not 480'),
            (([f32[0], np.zeros((3, H, W), np.float16)], 'chw'), {}, 'frame 1 of the list differs from frame 0 in sample_type'),
            (([f32[0], f32[1][:, :, ::2]], 'chw'), {}, 'frame 1 of the list: the strides .* do not fit melf_wide_frames'),
            (([f32[0], np.zeros((H, W, 3), np.float32).transpose(2, 0, 1)], 'chw'), {}, 'frame 1 of the list: the strides'),
            (([np.zeros((2, 3, H, W), np.float32)], 'chw'), {}, r'frame 0 of the list must be one frame, \(C, H, W\)'),
            (([np.zeros((H, W), np.float32)], 'hwc'), {}, r'frame 0 of the list must be one frame, \(H, W, C\)'),
            (([f32[0]], 'nchw'), {}, 'layout'),
            (([f32[0]], 'chw'), dict(shift=8), 'frame 0 of the list: float frames take no shift'),
            (([chw[0]], 'chw'), {}, 'frame 0 of the list: integer frames need shift'),
            (([f32[0].astype(np.float64)], 'chw'), {}, 'must be uint16, float16'),
            ((f32, 'chw'), dict(out=np.zeros(3)), 'out= takes the records of device frames only'),
            (([f32[0], FakeTensor(f32[1])], 'chw'), {}, 'frame 1 of the list is in device memory, frame 0 in host memory'),
            (([FakeTensor(f32[0]), f32[1]], 'chw'), {}, 'frame 1 of the list is in host memory, frame 0 in device memory'),
            (([FakeTensor(f32[0]), FakeTensor(f32[1], 1)], 'chw'), {}, 'frame 1 of the list differs from frame 0 in device: 1, not 0'),
            (([FakeTensor(f32[0], 1), FakeTensor(f32[1], 1)], 'chw'), {}, 'frames are on cuda:1, the reader on cuda:0')):
        with pytest.raises(ValueError, match=msg):
            r.read_wide_frame_list(*args, **kw)
    assert not r.ctx.calls


def test_read_wide_plane_list_with_a_stand_in():
    """The plane table in B, G, R slots for every channel order, one descriptor with zero offsets; every ValueError names frame and
    plane."""
    r = stand_in_reader()
    (H, W) = (5, 9)
    def plane(dtype=np.uint16, pad=3):   # noqa: E306
        return np.zeros((H, W + pad), dtype)[:, :W]
    for order in ('rgb', 'bgr', 'gbr'):
        r.ctx.calls.clear()
        frames = [tuple(plane() for _ in range(3)) for _ in range(4)]
        r.read_wide_plane_list(frames, order, shift=2)
        ((name, (desc, table, nplanes), kw),) = r.ctx.calls
        assert name == 'process_wide_plane_list' and nplanes == 3 and not kw
        assert table == [fr[order.index(ch)].ctypes.data for fr in frames for ch in 'bgr'], order
        assert (desc.n, desc.H, desc.W, desc.layout, desc.sample_type, desc.shift, desc.row_pitch, desc.b_offset, desc.g_offset, desc.r_offset) == (
            4, H, W, _hip.WIDE_PLANAR, _hip.WIDE_U16, 2, (W + 3) * 2, 0, 0, 0)
    # scale and offset in the order of channel_order -> B, G, R
    r.ctx.calls.clear()
    r.read_wide_plane_list([tuple(plane(np.float32) for _ in range(3))], 'gbr', scale=(1.0, 2.0, 3.0), offset=(4.0, 5.0, 6.0))
    desc = r.ctx.calls[0][1][0]
    assert (list(desc.scale), list(desc.offset), desc.sample_type, desc.row_pitch) == ([2.0, 1.0, 3.0], [5.0, 4.0, 6.0], _hip.WIDE_F32, (W + 3) * 4)
    r.ctx.calls.clear()
    assert len(r.read_wide_plane_list([], 'rgb', shift=8)) == 0
    ok = tuple(plane() for _ in range(3))
    for (frames, kw, msg) in (
            ([ok, ok[:2]], dict(shift=8), 'frame 1 of the list has 2 planes'),
            ([ok, (ok[0], ok[1], plane(pad=5))], dict(shift=8), 'frame 1, plane 2 of the list differs from frame 0, plane 0 in row_pitch: 28, not 24'),
            ([ok, (ok[0], plane(np.float16), ok[2])], dict(shift=8), 'frame 1, plane 1 of the list: float frames take no shift'),
            ([(ok[0], ok[1][:-1], ok[2])], dict(shift=8), r'frame 0, plane 1 of the list differs from frame 0, plane 0 in shape: \(4, 9\), not \(5, 9\)'),
            ([(ok[0], ok[1][:, ::2], ok[2])], dict(shift=8), 'frame 0, plane 1 of the list: the strides .* do not fit melf_wide_frames'),
            ([(ok[0], ok[1][::-1], ok[2])], dict(shift=8), 'frame 0, plane 1 of the list: the strides'),
            ([(ok[0], np.zeros((1, H, W), np.uint16), ok[2])], dict(shift=8), 'frame 0, plane 1 of the list must be a 2-D'),
            ([(ok[0], ok[1].astype(np.uint8), ok[2])], dict(shift=8), 'frame 0, plane 1 of the list: wide frames must be uint16'),
            ([ok], {}, 'frame 0, plane 0 of the list: integer frames need shift'),
            ([ok], dict(shift=8, channel_order='rgba'), 'does not name three planes'),
            ([ok], dict(shift=8, out=np.zeros(1)), 'out= takes the records of device frames only'),
            ([(ok[0], FakeTensor(ok[1]), ok[2])], dict(shift=8), 'frame 0, plane 1 of the list is in device memory, frame 0, plane 0 in host memory'),
            ([tuple(FakeTensor(p) for p in ok), (FakeTensor(ok[0]), FakeTensor(ok[1], 1), FakeTensor(ok[2]))], dict(shift=8),
             'frame 1, plane 1 of the list is on cuda:1, frame 0, plane 0 on cuda:0'),
            ([tuple(FakeTensor(p, 1) for p in ok)], dict(shift=8), 'frames are on cuda:1, the reader on cuda:0')):
        with pytest.raises(ValueError, match=msg):
            r.read_wide_plane_list(frames, **dict(dict(channel_order='rgb'), **kw))
    # a float plane with a differing dtype among float planes
    with pytest.raises(ValueError, match='frame 0, plane 2 of the list differs from frame 0, plane 0 in dtype'):
        r.read_wide_plane_list([(plane(np.float32), plane(np.float32), plane(np.float16, pad=15))], 'rgb')
    assert not r.ctx.calls


# ------------------------------------------------------------------------------------------------------------- GPU ---------
@pytest.mark.gpu
@pytest.mark.parametrize('type_', [wc.U16, wc.F16, wc.BF16, wc.F32], ids=['u16', 'f16', 'bf16', 'f32'])
def test_stage_parity_of_the_list_kernels(env, type_):  # noqa: F811
    """melf_wide_list_to_bgr over wide_list_cases.SHAPES: every frame of a list, every plane of a plane list in a device allocation
    of exactly its readable extent (the entry point's contract); the bytes equal numpy's narrowing of the samples exactly.  u16 at
    shifts 0 and 8; the float types under the three triples of wide_cases.TRIPLES and with one triple per channel (scale and offset
    by position); NaN, +-inf and negative values in the first and last sample of a row and in its tail piece."""
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(100 + type_)
    calls = 0
    for (planar, order, H, W, pad) in wl.SHAPES:
        samples = wl.random_samples(type_, planar, len(order), 2, H, W, rng)
        (frames, planes, geom) = wl.separate(samples, planar, order, type_, pad)
        for rule in wl.rules(type_):
            want = wl.narrowed_bgr(samples, planar, order, type_, rule)
            desc = wl.descriptor(type_, geom, rule)
            got = ctx.wide_list_to_bgr(desc, [f.ctypes.data for f in frames])
            assert np.array_equal(got, want), ('frames', planar, order, H, W, pad, rule, np.argwhere(got != want)[:4])
            calls += 1
            if planar:
                desc = wl.descriptor(type_, dict(geom, b_offset=0, g_offset=0, r_offset=0), rule)
                got = ctx.wide_list_to_bgr(desc, [p.ctypes.data for fr in planes for p in fr], 3)
                assert np.array_equal(got, want), ('planes', H, W, pad, rule, np.argwhere(got != want)[:4])
                calls += 1
    assert calls == len(wl.SHAPES) * len(wl.rules(type_)) * 6 // 5   # a fifth of the shapes are planar: those twice


# (sample type, shift)
RECORD_TYPES = [(wc.U16, 8), (wc.F16, 0), (wc.BF16, 0), (wc.F32, 0)]


@pytest.fixture(scope='module')
def cut():
    """the 33 synthetic fixture frames' top-left part that holds meter_rect (50, 160)-(300, 410)"""
    bgr = flc.synth_source().bgr
    assert bgr.shape[0] == 33
    return np.ascontiguousarray(bgr[:, :412, :302])


@pytest.mark.gpu
@pytest.mark.parametrize('planar', [False, True], ids=['packed', 'planar'])
@pytest.mark.parametrize('type_,shift', RECORD_TYPES, ids=['u16>>8', 'f16', 'bf16', 'f32'])
def test_records_of_lists_equal_the_batch(env, cut, type_, shift, planar):  # noqa: F811
    """33 fixture frames as wide frames, each placed so that it ends where its own device allocation ends, at a base with the
    sample's own alignment only, in shuffled allocations: melf_process_wide_list_dev and melf_process_wide_list give the records of
    melf_process_wide on the stacked batch, byte for byte; planar frames also through the plane lists, every plane an allocation of
    its own that ends with the plane's last sample."""
    ctx = env['sample-images1']['reader'].ctx
    case = wl.fixture_case(cut, type_, shift, planar)
    want = ctx.process_wide(case.buf.ctypes.data, case.desc)
    assert 4 * int((want['status'] == _hip.FRAME_OK).sum()) >= 3 * len(want), want['status']
    assert len(set(r.tobytes() for r in want)) > len(want) // 2   # the records tell the frames apart
    phase = 2 if case.ss == 2 else 0
    frames = flc.DevFrames(case.view, np.random.default_rng(3), at_end=True, phase=phase)
    try:
        assert all(p % 4 == phase for p in frames.ptrs) and len(set(frames.spread())) > 1
        got = ctx.process_wide_list_dev(case.list_desc, frames.ptrs)
        assert got.tobytes() == want.tobytes(), 'device list'
        order = list(range(len(want)))[::-1]
        order[5] = order[20] = 2   # reversed, one frame repeated
        got = ctx.process_wide_list_dev(case.list_desc, [frames.ptrs[i] for i in order])
        assert got.tobytes() == want[order].tobytes(), 'device list, permuted'
    finally:
        frames.free()
    got = ctx.process_wide_list(case.list_desc, [f.ctypes.data for f in case.host_frames])
    assert got.tobytes() == want.tobytes(), 'host list'
    if not planar:
        return
    bufs = [[fc.DevBuf.at_end(p.ctypes.data, p.nbytes, phase) for p in fr] for fr in case.host_planes]
    try:
        ptrs = [b.d.value for fr in bufs for b in fr]
        got = ctx.process_wide_plane_list_dev(case.plane_desc, ptrs)
        assert got.tobytes() == want.tobytes(), 'device plane list'
    finally:
        for fr in bufs:
            for b in fr:
                b.free()
    got = ctx.process_wide_plane_list(case.plane_desc, [p.ctypes.data for fr in case.host_planes for p in fr])
    assert got.tobytes() == want.tobytes(), 'host plane list'


@pytest.mark.gpu
def test_lists_longer_than_a_chunk_and_which_kernel_ran(env, cut):  # noqa: F811
    """1030 pointers cycling over the 33 frames (frames may repeat): two chunks, the records the 33 tiled, on the device and from
    the host; the same for a plane list whose three slots all name one plane (planes may alias).  With profiling on, a wide-list
    call launches one MELF_K_GATHER kernel per chunk and otherwise what the batch call launches."""
    ctx = env['sample-images1']['reader'].ctx
    n = 1030
    cyc = [i % 33 for i in range(n)]
    case = wl.fixture_case(cut, wc.U16, 8, True)
    want = ctx.process_wide(case.buf.ctypes.data, case.desc)
    frames = flc.DevFrames(case.view, np.random.default_rng(8))
    bufs = [fc.DevBuf(fr[1].ctypes.data, fr[1].nbytes) for fr in case.host_planes]   # the G planes
    ctx.set_profiling(1)
    try:
        dev = fc.DevBuf(case.buf.ctypes.data, case.buf.nbytes)
        try:
            ctx.timings()
            ctx.process_wide_dev(dev.d.value, case.desc)
            batch_counts = fc.launch_counts(ctx)
        finally:
            dev.free()
        got = ctx.process_wide_list_dev(case.list_desc, frames.ptrs)
        assert fc.launch_counts(ctx) == batch_counts and batch_counts['k_gather'] == 1, batch_counts
        assert got.tobytes() == want.tobytes()
        long_desc = wl.with_n(case.list_desc, n)
        got = ctx.process_wide_list_dev(long_desc, [frames.ptrs[i] for i in cyc])
        t = fc.launch_counts(ctx)
        assert t['k_gather'] == 2 and t['k_dials'] == 2, t
        assert got.tobytes() == want[cyc].tobytes(), 'device list of 1030'
        got = ctx.process_wide_list(long_desc, [case.host_frames[i].ctypes.data for i in cyc])
        assert got.tobytes() == want[cyc].tobytes(), 'host list of 1030'
        # aliased planes: B = G = R = the frame's G plane; the reference is the batch of frames with three such planes
        ggg = wl.fixture_case(cut[..., [1, 1, 1]], wc.U16, 8, True)
        want_g = ctx.process_wide(ggg.buf.ctypes.data, ggg.desc)
        ctx.timings()
        got = ctx.process_wide_plane_list_dev(wl.with_n(case.plane_desc, n), [bufs[i].d.value for i in cyc for _k in range(3)])
        t = fc.launch_counts(ctx)
        assert t['k_gather'] == 2 and t['k_dials'] == 2, t
        assert got.tobytes() == want_g[cyc].tobytes(), 'aliased planes'
        got = ctx.process_wide_plane_list(case.plane_desc, [fr[1].ctypes.data for fr in case.host_planes for _k in range(3)])
        assert got.tobytes() == want_g.tobytes(), 'aliased planes, host'
    finally:
        ctx.set_profiling(0)
        frames.free()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_rejected_lists_launch_nothing(env, cut):  # noqa: F811
    """MELF_ERR_INVALID with the checks' messages from all five entry points, the index of the offending frame and plane in front,
    before anything is launched; n == 0 passes."""
    ctx = env['sample-images1']['reader'].ctx
    case = wl.fixture_case(cut[:3], wc.F32, 0, True)
    packed = wl.fixture_case(cut[:3], wc.F32, 0, False)
    fp = [f.ctypes.data for f in case.host_frames]
    pp = [p.ctypes.data for fr in case.host_planes for p in fr]
    ctx.set_profiling(1)
    try:
        fc.launch_counts(ctx)   # (reading the counts resets them: what an earlier test left is read away first)
        before = fc.launch_counts(ctx)
        assert not any(before.values()), before

        def every_list_call(desc, ptrs, msg):
            for call in (lambda: ctx.process_wide_list(desc, ptrs), lambda: ctx.process_wide_list_dev(desc, ptrs),
                         lambda: ctx.wide_list_to_bgr(desc, ptrs)):
                with pytest.raises(_hip.HipError, match=msg):
                    call()

        def every_plane_call(desc, ptrs, msg, nplanes=3):
            for call in (lambda: ctx.process_wide_plane_list(desc, ptrs, nplanes), lambda: ctx.process_wide_plane_list_dev(desc, ptrs, nplanes),
                         lambda: ctx.wide_list_to_bgr(desc, ptrs, nplanes)):
                with pytest.raises(_hip.HipError, match=msg):
                    call()
        every_list_call(case.list_desc, [fp[0], 0, fp[2]], 'frame 1 of the list: frame pointer of wide frames is NULL')
        every_list_call(case.list_desc, [fp[0], fp[1], fp[2] + 2], 'frame 2 of the list: wide frames need frame pointers that are multiples')
        every_list_call(wl.changed(case.list_desc, H=0), fp, 'bad batch shape of wide frames')
        every_list_call(wl.changed(case.list_desc, row_pitch=case.list_desc.row_pitch + 2), fp, 'multiples of the sample size')
        every_list_call(wl.changed(case.list_desc, sample_type=4), fp, 'unknown sample_type')
        every_plane_call(case.plane_desc, pp[:4] + [0] + pp[5:], 'frame 1, plane 1 of the list: plane pointer of wide frames is NULL')
        every_plane_call(case.plane_desc, pp[:8] + [pp[8] + 1], 'frame 2, plane 2 of the list: wide frames need plane pointers that are multiples')
        every_plane_call(wl.changed(case.plane_desc, g_offset=4), pp, 'b_offset, g_offset and r_offset must be 0')
        every_plane_call(case.plane_desc, pp[:6], 'nplanes of a wide plane list must be 3', nplanes=2)
        every_plane_call(packed.list_desc, pp, 'melf_process_wide_list')
        every_plane_call(wl.changed(case.plane_desc, reserved=1), pp, 'reserved field of the wide frame descriptor')
        with pytest.raises(_hip.HipError, match='at most 1024 frames'):
            ctx.wide_list_to_bgr(wl.with_n(case.list_desc, 1025), [fp[0]] * 1025)
        empty = wl.with_n(case.list_desc, 0)
        assert len(ctx.process_wide_list(empty, [])) == 0 and len(ctx.process_wide_list_dev(empty, [])) == 0
        assert len(ctx.process_wide_plane_list(wl.with_n(case.plane_desc, 0), [])) == 0
        assert ctx.wide_list_to_bgr(empty, []).shape[0] == 0
        assert fc.launch_counts(ctx) == before
    finally:
        ctx.set_profiling(0)


@pytest.mark.gpu
def test_wide_lists_in_a_torch_process():
    """MeterReader.read_wide_frame_list / read_wide_plane_list with torch tensors on the reader's GPU -- a list of separately
    allocated frames, a x[:, y0:, x0:] view per frame, planes --, two caller streams, frames-resident mode on and off, out= a
    device tensor without synchronisation: in a fresh child process that imports torch first."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'wide_list_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch wide list path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])

