"""A frame's planes in separate allocations: melf_process_plane_list / melf_process_plane_list_dev, MeterReader.read_plane_list,
plane_list_check / plane_split of melf_stage_plan.h and the kernel k_plane_rows.

The parity bar everywhere is byte equality of the records with the family's own call on one contiguous batch holding the same
samples in list order: there is no tolerance.  In every parity test at least three quarters of the reference batch's records are
FRAME_OK (frame_cases.synth makes every ninth frame constant: 29 of 33 read; asserted on the reference records), so failure records
are not compared with failure records.  No test places a plane against unmapped memory: what is read from each plane's pointer is
the CPU sweep's subject (tests/plane_runs_main.cpp)."""
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
from tests import plane_list_cases as plc  # noqa: E402
from tests.frame_cases import env  # noqa: E402,F401

KERNEL = 'k_plane_rows'
# tests/test_frame_list.py: the substrings existing metadata tests count kernels by
COUNTED = ('k_dials', 'k_prep_lplane', 'k_needles', 'k_yneedle', 'k_lplane_yuv', 'k_match_yuv', 'k_yuv2bgr', 'k_lplane_px4', 'k_match_px4',
           'k_p422_', 'k_yp_', 'k_y16_', 'k_v210_', 'k_y210_', 'k_p32_', 'k_planar_', 'k_match_mfma', 'k_match_gen', 'k_fused_mask', 'k_jpeg_',
           'k_bgr2hls', 'k_stream_probe')
N = 33   # one 32-frame match group plus one
ERR_INVALID = -1   # MELF_ERR_INVALID


def ok_enough(want):
    assert 4 * int((want['status'] == _hip.FRAME_OK).sum()) >= 3 * len(want), want['status']


# ------------------------------------------------------------------------------------------------------------------- CPU ---
def test_plane_runs_on_the_cpu(tmp_path):
    """tests/plane_runs_main.cpp, plain and under the host sanitizers: the four families' descriptors with the plane offsets counted
    from each plane's own pointer, every plane a malloc of its own of exactly its extent, the split runs walked through the
    functions k_plane_rows calls; the staged frames equal the one-allocation walk's.  Every family saw more than 1000 cases, odd
    origins, rectangles touching the frame's edges, full and tail pieces, and rejected the descriptors the rules name."""
    import re
    from tests import test_dials_instantiations as di
    (cxx, inc) = di.rocm_clangxx()
    out = fc.build_and_run(tmp_path, cxx, os.path.join(ROOT, 'tests', 'plane_runs_main.cpp'), 'plane_runs', ['-D__HIP_PLATFORM_AMD__', '-I' + inc],
                           ['-fsanitize=address,undefined'])
    seen = {m.group(1): tuple(int(m.group(k)) for k in (2, 3, 4, 5, 6, 7))
            for m in re.finditer(r'family (\w+): cases (\d+) odd_origin (\d+) edge (\d+) rejected \d+ full_pieces (\d+) tail_pieces (\d+) rules (\d+)', out)}
    assert sorted(seen) == sorted(['yuv', 'yuv_planar', 'yuv16', 'planes']), out
    for (fam, (cases, odd, edge, full, tail, rules)) in seen.items():
        assert cases > 1000 and odd > 100 and edge > 100 and full > 0 and tail > 0 and rules > 100, (fam, out)
    assert re.search(r'one-plane and unknown families: 18 rejections', out), out


def plane_kernels(lib=None):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    return {k: d for (k, d) in kernel_meta.kernel_metadata(lib).items() if KERNEL in k}


def test_plane_kernel_metadata_and_name():
    """k_plane_rows is in the product library and in the diagnostic one, once each: wave size 64, no private segment, no spilled
    registers.  Its name contains neither `gather` (tests/test_frame_list.py wants exactly one such kernel) nor any substring the
    other metadata tests count kernels by."""
    src = open(os.path.join(ROOT, 'meterelf_amd', 'csrc', 'k_gather.hip')).read()
    assert '\n%s(' % KERNEL in src
    assert 'gather' not in KERNEL
    for sub in COUNTED:
        assert sub not in KERNEL, sub
    for lib in (None, os.path.join(ROOT, 'meterelf_amd', 'csrc', 'libmeterelf_hip_diag.so')):
        new = plane_kernels(lib)
        assert len(new) == 1, (lib, list(new))
        ((name, d),) = new.items()
        kernel_part = name.split('EPK')[0]   # the mangled name up to its argument types (which spell out RowRuns, PlaneSplit)
        assert 'gather' not in kernel_part
        for sub in COUNTED:
            assert sub not in name, (name, sub)
        assert d['wavefront_size'] == 64 and d.get('private_segment_fixed_size', 0) == 0, d
        assert d.get('vgpr_spill_count', 0) == 0 and d.get('sgpr_spill_count', 0) == 0, d


def test_exports():
    """The two entry points are exported and listed; the families keep their eight codes."""
    L = _hip.lib()
    assert hasattr(L, 'melf_process_plane_list') and hasattr(L, 'melf_process_plane_list_dev')
    assert 'melf_process_plane_list' in _hip.EXPORTS and 'melf_process_plane_list_dev' in _hip.EXPORTS
    assert sorted(_hip.LIST_FAMILIES.values()) == list(range(8))
    text = open(os.path.join(ROOT, 'include', 'meterelf_hip.h')).read()
    assert 'int melf_process_plane_list_dev(' in text and 'int melf_process_plane_list(' in text
    assert 'MELF_K_COUNT = 10' in text and _hip.K_COUNT == 10


class StandIn:
    """A context that records what read_plane_list hands to the library"""

    def __init__(self):
        self.calls = []

    def process_plane_list(self, family, desc, ptrs, nplanes):
        self.calls.append(('host', family, desc, list(ptrs), nplanes))
        return np.zeros(desc.n, _hip.RESULT_DTYPE)

    def process_plane_list_dev(self, family, desc, ptrs, nplanes, **kw):
        self.calls.append(('dev', family, desc, list(ptrs), nplanes))
        return np.zeros(desc.n, _hip.RESULT_DTYPE)


def stand_in_reader():
    from meterelf_amd import MeterReader
    r = MeterReader.__new__(MeterReader)
    r.device = 0
    r.ctx = StandIn()
    return r


def padded(rows, cols, dtype=np.uint8, pad=6):
    """a (rows, cols) view of an array whose rows are pad elements longer"""
    return np.zeros((rows, cols + pad), dtype)[:, :cols]


def test_read_plane_list_tables_and_offsets():
    """read_plane_list, with a stand-in context: the descriptor and the pointer table for nv12, nv21, i420, yv12, p010, i444 and
    'planar' with 'rgb' -- slot order (Y, U or interleaved chroma, V; B, G, R) whatever the tuple's, offsets from each plane's own
    pointer, pitches from the planes' strides."""
    (H, W) = (12, 16)
    r = stand_in_reader()

    def last():
        (kind, family, desc, ptrs, nplanes) = r.ctx.calls[-1]
        assert kind == 'host'
        return family, desc, ptrs, nplanes

    def addr(a):
        return a.ctypes.data
    # nv12: (Y, C), C as (Hc, Wc * 2) and as (Hc, Wc, 2); padded rows give the pitches
    pairs = np.zeros((H // 2, (W + 10) // 2, 2), np.uint8)[:, :W // 2]   # (Hc, Wc, 2), its rows W + 10 bytes apart
    frames = [(padded(H, W, pad=6), padded(H // 2, W, pad=10)), (padded(H, W, pad=6), pairs)]
    assert len(r.read_plane_list(frames, 'yuv', 'nv12')) == 2
    (family, d, ptrs, nplanes) = last()
    assert (family, nplanes) == ('yuv', 2) and isinstance(d, _hip.MelfYuvFrames)
    assert (d.format, d.matrix, d.n, d.H, d.W, d.y_pitch, d.c_pitch, d.u_offset, d.v_offset) == (_hip.YUV_NV12, 0, 2, H, W, W + 6, W + 10, 0, 1)
    assert ptrs == [addr(frames[0][0]), addr(frames[0][1]), addr(frames[1][0]), addr(frames[1][1])]
    # nv21 through 'yuv_planar': V is the first byte of a pair
    frames = [(np.zeros((H, W), np.uint8), np.zeros((H // 2, W), np.uint8))]
    r.read_plane_list(frames, 'yuv_planar', 'nv21', matrix='bt709')
    (family, d, ptrs, nplanes) = last()
    assert (family, nplanes) == ('yuv_planar', 2) and isinstance(d, _hip.MelfYuvPlanarFrames)
    assert (d.matrix, d.sub_x, d.sub_y, d.c_step, d.y_pitch, d.c_pitch, d.u_offset, d.v_offset) == (_hip.YUV_BT709_LIMITED, 1, 1, 2, W, W, 1, 0)
    # i420 (Y, U, V) and yv12 (Y, V, U): slot 1 is U, slot 2 is V
    (y, a, b) = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8))
    r.read_plane_list([(y, a, b)], 'yuv', 'i420')
    (family, d, ptrs, nplanes) = last()
    assert (family, nplanes, d.format, d.u_offset, d.v_offset, d.c_pitch) == ('yuv', 3, _hip.YUV_I420, 0, 0, W // 2)
    assert ptrs == [addr(y), addr(a), addr(b)]
    r.read_plane_list([(y, a, b)], 'yuv', 'yv12')
    (family, d, ptrs, nplanes) = last()
    assert (nplanes, d.format, d.u_offset, d.v_offset) == (3, _hip.YUV_I420, 0, 0)
    assert ptrs == [addr(y), addr(b), addr(a)]
    # p010: 16-bit samples, byte pitches, {0, 2}
    (y, c) = (padded(H, W, np.uint16, 3), padded(H // 2, W, np.uint16, 5))
    r.read_plane_list([(y, c)], 'yuv16', 'p010', matrix='bt709')
    (family, d, ptrs, nplanes) = last()
    assert (family, nplanes) == ('yuv16', 2) and isinstance(d, _hip.MelfYuv16Frames)
    assert (d.matrix, d.sub_y, d.c_step, d.shift, d.y_pitch, d.c_pitch, d.u_offset, d.v_offset) == (3, 1, 2, 8, 2 * (W + 3), 2 * (W + 5), 0, 2)
    assert ptrs == [addr(y), addr(c)]
    # i444: three full planes
    planes = tuple(np.zeros((H, W), np.uint8) for _ in range(3))
    r.read_plane_list([planes], 'yuv_planar', 'i444')
    (family, d, ptrs, nplanes) = last()
    assert (nplanes, d.sub_x, d.sub_y, d.c_step, d.c_pitch, d.u_offset, d.v_offset) == (3, 0, 0, 1, W, 0, 0)
    assert ptrs == [addr(p) for p in planes]
    # planar 'rgb': the tuple is (R, G, B), the slots B, G, R
    (R, G, B) = (padded(H, W, pad=4) for _ in range(3))
    r.read_plane_list([(R, G, B), (R, G, B)], 'planar', 'rgb')
    (family, d, ptrs, nplanes) = last()
    assert (family, nplanes) == ('planar', 3) and isinstance(d, _hip.MelfPlanarFrames)
    assert (d.n, d.H, d.W, d.b_offset, d.g_offset, d.r_offset, d.row_pitch) == (2, H, W, 0, 0, 0, W + 4)
    assert ptrs == [addr(B), addr(G), addr(R)] * 2
    assert len(r.read_plane_list([], 'yuv', 'nv12')) == 0


def test_read_plane_list_value_errors():
    """Every ValueError of read_plane_list names frame, plane and field (stand-in context: nothing reaches a library)."""
    (H, W) = (12, 16)
    r = stand_in_reader()
    (y, c) = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W), np.uint8))
    with pytest.raises(ValueError, match='yuv, yuv_planar, yuv16, planar'):
        r.read_plane_list([(y, c)], 'views', 'bgr')
    with pytest.raises(ValueError, match='yuv, yuv_planar, yuv16, planar'):
        r.read_plane_list([(y, c)], 'yuv422', 'yuyv')
    with pytest.raises(ValueError, match='frame 1 of the list has 3 planes'):
        r.read_plane_list([(y, c), (y, c, c)], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 0 of the list has 2 planes'):
        r.read_plane_list([(y, c)], 'yuv', 'i420')
    with pytest.raises(ValueError, match='frame 1, plane 1 of the list differs in shape'):
        r.read_plane_list([(y, c), (y, c[:, :-2])], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 0, plane 1 of the list differs in shape'):   # not the format's subsampling
        r.read_plane_list([(y, np.zeros((H, W), np.uint8))], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 1, plane 0 of the list differs in y_pitch: %d, not %d' % (W + 6, W)):
        r.read_plane_list([(y, c), (padded(H, W), c)], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 1, plane 1 of the list differs in c_pitch'):
        r.read_plane_list([(y, c), (y, padded(H // 2, W))], 'yuv', 'nv12')
    (u, v) = (np.zeros((H // 2, W // 2), np.uint8), padded(H // 2, W // 2))
    with pytest.raises(ValueError, match='frame 0, plane 2 of the list differs in c_pitch'):   # U and V share one field
        r.read_plane_list([(y, u, v)], 'yuv', 'i420')
    with pytest.raises(ValueError, match='frame 0, plane 1 of the list differs in row_pitch'):
        r.read_plane_list([(y, padded(H, W), y)], 'planar', 'rgb')
    with pytest.raises(ValueError, match='frame 0, plane 1 of the list has a layout'):   # every other byte: it would have to be copied
        r.read_plane_list([(y, np.zeros((H // 2, 2 * W), np.uint8)[:, ::2])], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 0, plane 0 of the list has a layout'):   # rows in reverse
        r.read_plane_list([(y[::-1], c)], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 0, plane 0 of the list: frames must be uint16'):
        r.read_plane_list([(y, c)], 'yuv16', 'p010', matrix='bt709')
    with pytest.raises(ValueError, match='frame 0, plane 1 of the list: a plane must be'):
        r.read_plane_list([(y, c[0])], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='odd'):
        r.read_plane_list([(np.zeros((H + 1, W), np.uint8), c)], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='matrix'):   # no default for 16-bit material
        r.read_plane_list([(y.astype(np.uint16), c.astype(np.uint16))], 'yuv16', 'p010')
    with pytest.raises(ValueError, match='takes no matrix'):
        r.read_plane_list([(y, y, y)], 'planar', 'rgb', matrix='bt601')
    with pytest.raises(ValueError, match='rgb, bgr, gbr'):
        r.read_plane_list([(y, y, y, y)], 'planar', 'rgba')
    with pytest.raises(ValueError, match='out= takes the records of device frames only'):
        r.read_plane_list([(y, c)], 'yuv', 'nv12', out=np.zeros(1))
    assert r.ctx.calls == []


class ArrayLike:
    """A plane that is neither an ndarray nor a tensor: np.asarray makes a fresh array of it at every conversion (as of a PIL image),
    which nothing but the reader then owns"""

    def __init__(self, rows, cols, made):
        (self.rows, self.cols, self.made) = (rows, cols, made)

    def __array__(self, dtype=None, copy=None):
        import weakref
        a = np.full((self.rows, self.cols), 7, np.uint8)
        self.made.append(weakref.ref(a))
        return a


def test_converted_planes_live_until_the_call():
    """Planes given as array-likes are converted by np.asarray; the table holds their addresses only.  At the library call every
    converted array of every frame is still alive, and the table's addresses are theirs."""
    (H, W) = (12, 16)
    made = []
    seen = []

    class Checking(StandIn):
        def process_plane_list(self, family, desc, ptrs, nplanes):
            arrays = [ref() for ref in made]
            seen.append((len(arrays), [a is not None for a in arrays], list(ptrs) == [a.ctypes.data for a in arrays if a is not None]))
            return StandIn.process_plane_list(self, family, desc, ptrs, nplanes)
    r = stand_in_reader()
    r.ctx = Checking()
    frames = [(ArrayLike(H, W, made), ArrayLike(H // 2, W // 2, made), ArrayLike(H // 2, W // 2, made)) for _i in range(5)]
    assert len(r.read_plane_list(frames, 'yuv', 'i420')) == 5
    assert seen == [(15, [True] * 15, True)], seen
    import gc
    gc.collect()
    assert not any(ref() is not None for ref in made)   # ... and released once the call has returned


class FakeDevice:
    def __init__(self, index):
        (self.type, self.index) = ('cuda', index)

    def __eq__(self, other):
        return isinstance(other, FakeDevice) and other.index == self.index


class FakeTensor:
    """What _hip._unwrap looks at of a torch uint8 tensor on a GPU, over a numpy array's memory: nothing here is ever read"""
    __module__ = 'torch'

    def __init__(self, a, index=0):
        (self.a, self.dtype, self.device, self.shape) = (a, 'torch.uint8', FakeDevice(index), a.shape)

    def stride(self):
        return tuple(st // self.a.itemsize for st in self.a.strides)

    def data_ptr(self):
        return self.a.ctypes.data


def test_read_plane_list_device_value_errors():
    """The ValueErrors about where the planes are, with stand-in device tensors: host and device planes mixed, a plane on another
    device (frame and plane named), and planes on another device than the reader's."""
    (H, W) = (12, 16)
    r = stand_in_reader()
    (y, c) = (np.zeros((H, W), np.uint8), np.zeros((H // 2, W), np.uint8))
    assert _hip._is_torch(FakeTensor(y)) and _hip.plane_view(FakeTensor(y, 1)).on_device and _hip.plane_view(FakeTensor(y, 1)).device == 1
    with pytest.raises(ValueError, match='frame 1, plane 0 of the list is in device memory, frame 0, plane 0 in host memory'):
        r.read_plane_list([(y, c), (FakeTensor(y), FakeTensor(c))], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 0, plane 1 of the list is in host memory, frame 0, plane 0 in device memory'):
        r.read_plane_list([(FakeTensor(y), c)], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 1, plane 1 of the list is on cuda:1, frame 0, plane 0 on cuda:0'):
        r.read_plane_list([(FakeTensor(y), FakeTensor(c)), (FakeTensor(y), FakeTensor(c, 1))], 'yuv', 'nv12')
    with pytest.raises(ValueError, match='frame 0, plane 2 of the list is on cuda:0, frame 0, plane 0 on cuda:1'):
        r.read_plane_list([(FakeTensor(y, 1), FakeTensor(y, 1), FakeTensor(y))], 'planar', 'bgr')
    with pytest.raises(ValueError, match='frames are on cuda:1, the reader on cuda:0'):
        r.read_plane_list([(FakeTensor(y, 1), FakeTensor(c, 1))], 'yuv', 'nv12')
    assert r.ctx.calls == []


# ------------------------------------------------------------------------------------------------------------------- GPU ---
@pytest.fixture(scope='module')
def src():
    s = flc.synth_source(N)
    assert set(s.bgr.shape[1:3]) == {480, 640}   # the fixtures' geometry
    return s


def dev_parity(ctx, src_, layout, fmt, is_padded):
    rng = np.random.default_rng(5)
    big = plc.batch(src_, layout, fmt, rng, N, is_padded)
    for n in (1, N):
        b = big if n == N else plc.Batch(big.ptr, type(big.desc).from_buffer_copy(big.desc), big.extent - (N - 1) * big.desc.frame_stride, big.keep)
        b.desc.n = n
        c = plc.cut(layout, b.desc)
        whole = fc.DevBuf(b.ptr, b.extent)
        planes = plc.DevPlanes(b, c, np.random.default_rng(n))
        try:
            want = flc.dev_batch(ctx, layout, whole.d.value, b.desc)
            ok_enough(want)
            if n > 1:
                for k in range(c.nplanes):
                    assert len(set(planes.spread(k))) > 1, 'the planes of slot %d lie one stride apart' % k
            got = ctx.process_plane_list_dev(layout, c.desc, planes.ptrs, c.nplanes)
            assert got.tobytes() == want.tobytes(), (layout, fmt, n, is_padded)
        finally:
            planes.free()
            whole.free()


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', plc.FORMATS, ids=['%s-%s' % lf for lf in plc.FORMATS])
def test_parity(env, src, layout, fmt):  # noqa: F811
    """Every format name of the four layouts, 1 frame and 33: every plane a device allocation of its own of exactly its extent,
    allocated in shuffled order with spacers (the addresses of no slot are one stride apart: asserted); the records of
    melf_process_plane_list_dev equal the family's _dev call on the contiguous copy."""
    dev_parity(env['sample-images1']['reader'].ctx, src, layout, fmt, False)


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', plc.SHAPES, ids=['%s-%s' % lf for lf in plc.SHAPES])
def test_parity_with_padded_pitches(env, src, layout, fmt):  # noqa: F811
    """The same with Y and chroma pitches padded differently (planar RGB: padded rows) and gaps between the planes of the
    contiguous reference, one format per shape of the row runs."""
    dev_parity(env['sample-images1']['reader'].ctx, src, layout, fmt, True)


def host_parity(ctx, src_, layout, fmt, is_padded):
    if True:
        b = plc.batch(src_, layout, fmt, np.random.default_rng(5), N, is_padded)
        c = plc.cut(layout, b.desc)
        want = flc.host_batch(ctx, layout, b.ptr, b.desc)
        ok_enough(want)
        copies = []
        table = []
        for (i, frame) in enumerate(plc.host_addresses(b, c)):
            for (k, a) in enumerate(frame):
                raw = np.empty(c.extents[k] + 64 + 16 * ((i + k) % 5), np.uint8)     # allocations of differing sizes
                copy = raw[-raw.ctypes.data % 16:][:c.extents[k]]                    # exactly the extent
                copy[...] = np.frombuffer((C.c_uint8 * c.extents[k]).from_address(a), np.uint8)
                copies.append(raw)
                table.append(copy.ctypes.data)
        got = ctx.process_plane_list(layout, c.desc, table, c.nplanes)
        assert got.tobytes() == want.tobytes(), (layout, fmt, is_padded)


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', plc.FORMATS, ids=['%s-%s' % lf for lf in plc.FORMATS])
def test_host_planes(env, src, layout, fmt):  # noqa: F811
    """Every format name of the four layouts: numpy planes, each an allocation of its own of exactly its extent, through
    melf_process_plane_list equal the family's host call on the contiguous batch."""
    host_parity(env['sample-images1']['reader'].ctx, src, layout, fmt, False)


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', plc.SHAPES, ids=['%s-%s' % lf for lf in plc.SHAPES])
def test_host_planes_with_padded_pitches(env, src, layout, fmt):  # noqa: F811
    """The same with Y and chroma pitches padded differently, one format per shape of the row runs."""
    host_parity(env['sample-images1']['reader'].ctx, src, layout, fmt, True)


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt,slots', [('yuv', 'nv12', (1,)), ('yuv', 'i420', (1, 2)), ('yuv', 'i420', (2,)), ('planar', 'rgb', (2,))],
                         ids=['nv12-chroma', 'i420-chroma', 'i420-v', 'planar-r'])
def test_the_table_is_what_is_read(env, src, layout, fmt, slots):  # noqa: F811
    """The Y planes in list order, the planes of `slots` those of the next frame: the records equal the contiguous batch assembled
    that way and differ from the unrotated batch's -- slots 1 and 2 are read from their own pointers."""
    ctx = env['sample-images1']['reader'].ctx
    b = plc.batch(src, layout, fmt, np.random.default_rng(5), N)
    c = plc.cut(layout, b.desc)
    planes = plc.DevPlanes(b, c, np.random.default_rng(3))
    bufs = []
    try:
        wants = []
        for sl in (slots, ()):
            (keep, ptr, d, extent) = plc.rotated(b, c, sl)
            whole = fc.DevBuf(ptr, extent)
            bufs.append(whole)
            wants.append(flc.dev_batch(ctx, layout, whole.d.value, d))
        (want_rot, want_plain) = wants
        ok_enough(want_plain)   # (the rotated batch pairs a frame's luma with its neighbour's chroma: fewer of its frames read)
        assert want_rot.tobytes() != want_plain.tobytes()
        table = [planes.at((i + 1) % N if k in slots else i, k) for i in range(N) for k in range(c.nplanes)]
        got = ctx.process_plane_list_dev(layout, c.desc, table, c.nplanes)
        assert got.tobytes() == want_rot.tobytes()
        assert got.tobytes() != want_plain.tobytes()
        assert ctx.process_plane_list_dev(layout, c.desc, planes.ptrs, c.nplanes).tobytes() == want_plain.tobytes()
    finally:
        planes.free()
        for w in bufs:
            w.free()


@pytest.mark.gpu
def test_repeated_and_aliased_planes(env, src):  # noqa: F811
    """Frames repeated in the list, and one Y plane's allocation serving as three frames' Y: the records repeat accordingly."""
    ctx = env['sample-images1']['reader'].ctx
    b = plc.batch(src, 'yuv', 'i420', np.random.default_rng(5), N)
    c = plc.cut('yuv', b.desc)
    whole = fc.DevBuf(b.ptr, b.extent)
    planes = plc.DevPlanes(b, c, np.random.default_rng(6))
    try:
        want = flc.dev_batch(ctx, 'yuv', whole.d.value, b.desc)
        ok_enough(want)
        assert len(set(r.tobytes() for r in want)) > N // 2   # the records tell the frames apart
        order = list(range(N))
        order[7] = order[20] = order[21] = 3
        table = [planes.at(i, k) for i in order for k in range(3)]
        assert ctx.process_plane_list_dev('yuv', c.desc, table, 3).tobytes() == want[order].tobytes()
        # planes that point into the contiguous batch itself: aliases of one mapping
        table = [whole.d.value + i * c.frame_stride + c.offsets[k] for i in order for k in range(3)]
        assert ctx.process_plane_list_dev('yuv', c.desc, table, 3).tobytes() == want[order].tobytes()
    finally:
        planes.free()
        whole.free()


@pytest.mark.gpu
def test_chunks_and_timings(env, src):  # noqa: F811
    """1025 frames made by repeating the 33 frames' pointers go through in two chunks: the records repeat accordingly, and
    melf_ctx_timings counts two k_gather launches for the call and none for a batch call."""
    ctx = env['sample-images1']['reader'].ctx
    b = plc.batch(src, 'yuv', 'nv12', np.random.default_rng(5), N)
    c = plc.cut('yuv', b.desc)
    whole = fc.DevBuf(b.ptr, b.extent)
    planes = plc.DevPlanes(b, c, np.random.default_rng(7))
    try:
        ctx.set_profiling(1)
        ctx.timings()
        want = flc.dev_batch(ctx, 'yuv', whole.d.value, b.desc)
        ok_enough(want)
        assert ctx.timings()['k_gather'][1] == 0
        long_n = 1025
        order = [i % N for i in range(long_n)]
        d = type(c.desc).from_buffer_copy(c.desc)
        d.n = long_n
        got = ctx.process_plane_list_dev('yuv', d, [planes.at(i, k) for i in order for k in range(2)], 2)
        t = ctx.timings()
        assert t['k_gather'][1] == 2 and t['k_gather'][0] > 0, t['k_gather']
        assert got.tobytes() == want[order].tobytes()
    finally:
        ctx.set_profiling(0)
        planes.free()
        whole.free()


@pytest.mark.gpu
def test_lanes_streams_and_device_results(env, src):  # noqa: F811
    """Records into a device buffer (no host copy) on two caller streams alternately, four calls with different lists, frames-
    resident mode off and on; two calls back to back on one stream; and planes written by a copy enqueued on the same stream just
    before the call.  Every call's records equal the contiguous read's.  (The form of test_frame_list.test_lanes_and_ordering.)"""
    from meterelf_amd import MeterReader
    hip = fc.hip_rt()
    rsz = _hip.RESULT_DTYPE.itemsize
    b = plc.batch(src, 'yuv', 'nv12', np.random.default_rng(5), N)
    c = plc.cut('yuv', b.desc)
    r = MeterReader(env['sample-images1']['params'])
    whole = fc.DevBuf(b.ptr, b.extent)
    planes = plc.DevPlanes(b, c, np.random.default_rng(4))
    streams = [C.c_void_p(), C.c_void_p()]
    d_res = C.c_void_p()
    late = None
    try:
        want = flc.dev_batch(r.ctx, 'yuv', whole.d.value, b.desc)
        ok_enough(want)
        orders = [list(range(N)), list(range(N))[::-1], [(7 * i) % N for i in range(N)], [(5 * i + 3) % N for i in range(N)]]
        for s in streams:
            assert hip.hipStreamCreate(C.byref(s)) == 0
        assert hip.hipMalloc(C.byref(d_res), C.c_size_t(4 * N * rsz)) == 0

        def table(order):
            return [planes.at(i, k) for i in order for k in range(2)]

        def fetch():
            got = np.zeros(4 * N, _hip.RESULT_DTYPE)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), d_res, C.c_size_t(got.nbytes), 2) == 0
            assert hip.hipMemset(d_res, 0, C.c_size_t(got.nbytes)) == 0
            return got
        for resident in (False, True):
            r.ctx.set_frames_resident(resident)
            for (i, order) in enumerate(orders):
                assert r.ctx.process_plane_list_dev('yuv', c.desc, table(order), 2, d_results_ptr=d_res.value + i * N * rsz, want_host=False,
                                                    stream=streams[i % 2].value) is None
            r.ctx.sync()
            got = fetch()
            for (i, order) in enumerate(orders):
                assert got[i * N:(i + 1) * N].tobytes() == want[order].tobytes(), (resident, i)
            # back to back on one stream: the second call's copy overwrites the staged batch the first call's kernels read
            for (i, order) in enumerate(orders[:2]):
                r.ctx.process_plane_list_dev('yuv', c.desc, table(order), 2, d_results_ptr=d_res.value + i * N * rsz, want_host=False,
                                             stream=streams[0].value)
            r.ctx.sync()
            got = fetch()
            for (i, order) in enumerate(orders[:2]):
                assert got[i * N:(i + 1) * N].tobytes() == want[order].tobytes(), (resident, 'back to back', i)
            # the resident mode on the reader's own (NULL) stream
            assert r.ctx.process_plane_list_dev('yuv', c.desc, table(orders[2]), 2).tobytes() == want[orders[2]].tobytes(), (resident, 'null stream')
            # planes written on the stream just before the call: a zeroed allocation filled by an asynchronous copy from the
            # contiguous batch; the copy kernel must see the copy's bytes
            late = fc.DevBuf(np.zeros(b.extent, np.uint8).ctypes.data, b.extent)
            assert hip.hipMemcpyAsync(late.d, whole.d, C.c_size_t(b.extent), 3, streams[1]) == 0
            got = r.ctx.process_plane_list_dev('yuv', c.desc, [late.d.value + i * c.frame_stride + c.offsets[k] for i in range(N) for k in range(2)], 2,
                                               stream=streams[1].value)
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
        planes.free()
        whole.free()


@pytest.mark.gpu
def test_argument_errors(env, src):  # noqa: F811
    """MELF_ERR_INVALID with a message that names the frame's and the plane's index, or the rule; n == 0 succeeds.  Nothing is
    launched."""
    ctx = env['sample-images1']['reader'].ctx
    L = ctx._L
    b16 = plc.batch(src, 'yuv16', 'p010', np.random.default_rng(5), 4)
    c16 = plc.cut('yuv16', b16.desc)
    good16 = [a for frame in plc.host_addresses(b16, c16) for a in frame]   # host addresses: no call below gets as far as reading them
    b = plc.batch(src, 'yuv', 'i420', np.random.default_rng(5), 4)
    c = plc.cut('yuv', b.desc)
    good = [a for frame in plc.host_addresses(b, c) for a in frame]
    out = np.zeros(4, _hip.RESULT_DTYPE)

    def call(family, d, ptrs, nplanes, host=False):
        table = flc.pointer_table(ptrs) if ptrs is not None else None
        dref = C.byref(d) if d is not None else None
        if host:
            rc = L.melf_process_plane_list(ctx._h, family, dref, table, nplanes, out.ctypes.data_as(C.c_void_p))
        else:
            rc = L.melf_process_plane_list_dev(ctx._h, family, dref, table, nplanes, None, out.ctypes.data_as(C.c_void_p), None)
        return rc, L.melf_last_error().decode()
    ctx.set_profiling(1)
    ctx.timings()
    before = fc.launch_counts(ctx)
    (YUV, YUV16) = (_hip.LIST_FAMILIES['yuv'], _hip.LIST_FAMILIES['yuv16'])
    for host in (False, True):
        (rc, msg) = call(YUV, None, good, 3, host)
        assert rc == ERR_INVALID and 'descriptor is NULL' in msg, msg
        (rc, msg) = call(YUV, c.desc, good[:7] + [None] + good[8:], 3, host)
        assert rc == ERR_INVALID and 'frame 2, plane 1 of the list' in msg and 'NULL' in msg, msg
        (rc, msg) = call(YUV16, c16.desc, good16[:3] + [good16[3] + 1] + good16[4:], 2, host)
        assert rc == ERR_INVALID and 'frame 1, plane 1 of the list' in msg and '2-byte aligned' in msg, msg
        (rc, msg) = call(YUV, c.desc, good + good, 2, host)
        assert rc == ERR_INVALID and 'nplanes' in msg, msg
        (rc, msg) = call(YUV16, c16.desc, good16 + good16, 3, host)
        assert rc == ERR_INVALID and 'nplanes' in msg, msg
        for family in ('views', 'yuv422', 'yuv422_10', 'packed32'):
            (rc, msg) = call(_hip.LIST_FAMILIES[family], c.desc, good, 3, host)
            assert rc == ERR_INVALID and 'melf_process_frame_list' in msg, msg
        for family in (-1, 8):
            (rc, msg) = call(family, c.desc, good, 3, host)
            assert rc == ERR_INVALID and 'unknown family' in msg, msg
        bad = type(c.desc).from_buffer_copy(c.desc)
        bad.u_offset = 1   # a planar layout's offsets count from the plane's own pointer: 0
        (rc, msg) = call(YUV, bad, good, 3, host)
        assert rc == ERR_INVALID and "plane's own pointer" in msg, msg
        bad = type(b.desc).from_buffer_copy(b.desc)   # the contiguous batch's descriptor: offsets from the frame's first byte
        (rc, msg) = call(YUV, bad, good, 3, host)
        assert rc == ERR_INVALID and "plane's own pointer" in msg, msg
        bad = type(c.desc).from_buffer_copy(c.desc)
        bad.W += 1   # odd
        (rc, msg) = call(YUV, bad, good, 3, host)
        assert rc == ERR_INVALID and 'even' in msg, msg
        (rc, msg) = call(YUV, c.desc, None, 3, host)
        assert rc == ERR_INVALID and 'array of plane pointers is NULL' in msg, msg
        empty = type(c.desc).from_buffer_copy(c.desc)
        empty.n = 0
        (rc, msg) = call(YUV, empty, None, 3, host)
        assert rc == 0
    assert fc.launch_counts(ctx) == before
    ctx.set_profiling(0)


@pytest.mark.gpu
def test_read_plane_list_in_a_torch_process():
    """MeterReader.read_plane_list with separately allocated torch device tensors, host planes and out=, one format per layout, in
    a child process that imports torch first (tests/frame_cases.py says why)."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'plane_list_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch plane list path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
