"""Frames, rows and planes that lie 2 GiB, 4 GiB and more from the base pointer, in every family.

Every reading kernel forms byte addresses from base + f * frame_stride + row * pitch + plane offset + x * bytes, and the descriptors
take strides and offsets of 64 bits and pitches up to INT32_MAX.  The suite's largest device buffer (test_config5_resident_full_size,
3.18 GB) crosses 2^31 but not 2^32, and the bounds programs run the shared address headers on small heap buffers.  Here:

CPU   tests/far_addr_main.cpp evaluates every function of the address headers at far arguments against the same formula in 128-bit
      arithmetic, plain and under ASan + UBSan; and the three placements' own arithmetic (what lies where, what a wrapped offset
      would meet) is checked without a GPU.
GPU   one sparse arena (far_cases.FarArena: a single allocation of 8 GiB + 1 MiB filled with 0x80, of which a test writes a few
      hundred KB) and its host twin, and three placements of frames the existing builders make:
      A  far frames: 33 frames 2^27 + 4096 bytes apart; frames 16 .. 32 (beyond 2^31; frame 32 beyond 2^32) are corner_frames(),
         frames 0 .. 15 stay filler, so that a frame offset cut to 31 or 32 bits lands in filler (asserted).
      B  far rows: one frame of 252 rows whose packed / Y rows lie 2^25 + 64 bytes apart (rows >= 128 beyond 2^32), the chroma
         planes behind them at their tight pitch (their offsets beyond 2^32); also through a frame list and a plane list.
      C  far planes: planar RGB with the planes at 0, 2^32 + 64 and 2^33 + 128, all three channel orders, two frames.
      Expected records are always read_frames of the family's BGR frames on a reader made under the same MELF_MATCH, byte for byte;
      melf_ctx_last_match and melf_ctx_last_dials are asserted after every call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import far_cases as far  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import frame_list_cases as flc  # noqa: E402
from tests import oriented_cases as oc  # noqa: E402
from tests import plane_list_cases as plc  # noqa: E402

ARENA_BYTES = far.C_OFFSETS[2] + (1 << 20)          # placement C, the largest: the third plane and two frames of it
A_SHAPE = fc.ENDS_CASES[0][0]                        # (410, 300): meter_rect (50, 160)-(300, 410) ends on the last row and column
B_RECT = (50, 0, 300, 250)                           # placements B and C: meter_rect in the frame's first rows, as first_bytes has it
B_SHAPE = (far.B_ROWS, 302)
TO_BGR = {'yuv': ('yuv_to_bgr', 'nv12'), 'yuv422': ('yuv422_to_bgr', 'uyvy'), 'yuv_planar': ('yuv_planar_to_bgr', 'nv24'),
          'yuv16': ('yuv16_to_bgr', 'p010'), 'yuv422_10': ('yuv422_10_to_bgr', 'v210'), 'packed32': ('packed32_to_bgr', 'y410')}


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_far_addr_sweep(tmp_path):
    """tests/far_addr_main.cpp, plain and under the host sanitizers: every offset and every decision of the address headers at frame
    indices to 1023, strides to 2^36, pitches to INT32_MAX and plane offsets to 2^40 equals the 128-bit formula, no int product
    overflows (UBSan ends the run), and the comparator tells an offset from its 32-bit and 31-bit truncations."""
    out = fc.build_and_run(tmp_path, os.environ.get('CXX', 'g++'), os.path.join(ROOT, 'tests', 'far_addr_main.cpp'), 'far_addr', [],
                           ['-fsanitize=address,undefined'])
    lines = out.splitlines()
    assert lines[0].startswith('comparator: 32-bit and 31-bit truncations'), lines[0]
    assert lines[-1] == 'failures 0', lines[-1]
    counts = {ln.split()[0]: int(ln.split()[-2]) for ln in lines if ln.endswith('evaluations')}
    for header in ('melf_prep_addr.h', 'melf_y16_addr.h', 'melf_p10_addr.h', 'melf_p32_addr.h', 'melf_stage_plan.h', 'melf_orient_addr.h',
                   'melf_jpeg_orient_addr.h'):
        assert counts.get(header, 0) > 0, (header, counts)


def frames_a():
    """Placement A's frames 16 .. 32: corner_frames() cut so that the crop ends on the frame's last row and column."""
    (base, _mx, _my) = fc.corner_frames()
    return np.ascontiguousarray(base[far.A_FIRST:, :A_SHAPE[0], :A_SHAPE[1]])


def frames_b(n):
    """n frames for placements B and C: corner_frames() moved up so that the meter lies in rows 0 .. 250, cut to 252 rows."""
    (base, _mx, _my) = fc.corner_frames()
    return np.ascontiguousarray(np.roll(base[:n], -160, axis=1)[:, :B_SHAPE[0], :B_SHAPE[1]])


class Recorder:
    """What a placement function would copy where, without memory (FarArena's interface)."""
    FILL = far.FILL

    def __init__(self):
        self._written = []

    def put(self, offset, host_bytes):
        self._written.append((offset, offset + np.asarray(host_bytes).nbytes))

    def put_rows(self, offset, pitch, rows):
        for (r, row) in enumerate(rows):
            self.put(offset + r * pitch, row)

    def written(self):
        return sorted(self._written)


def test_placements_without_memory():
    """The arithmetic of placements A and B for every format, on a recorder instead of memory: the descriptors pass 2^31 and 2^32
    where the module's head says, everything fits the arena, and every interval a load wrapped at 2^31 or 2^32 would read is
    filler -- so the GPU tests cannot pass on a kernel that cuts an offset.  Not vacuous: assert_wraps_find_filler fails on a
    placement that has frame 0 written."""
    assert ARENA_BYTES <= far.ARENA_MAX
    assert far.A_FIRST * far.A_STRIDE >= 1 << 31 and (far.A_FRAMES - 1) * far.A_STRIDE >= 1 << 32 and far.A_STRIDE % 16 == 0
    assert 64 * far.B_PITCH >= 1 << 31 and 128 * far.B_PITCH >= 1 << 32 and 192 * far.B_PITCH >= 3 << 31 and far.B_PITCH % 16 == 0
    rng = np.random.default_rng(1)
    (src_a, src_b) = (flc.Source(frames_a()[:, :32, :36]), flc.Source(frames_b(1)))
    for layout in far.LAYOUTS:
        for fmt in far.FORMATS[layout]:
            # A, on frames cut small (the intervals' starts are what matters; the GPU test asserts the same on the frames it reads)
            (buf, d) = far.tight_batch(src_a, layout, fmt, rng)
            rec = Recorder()
            iv = far.put_far_frames(rec, buf, d)
            assert far.assert_wraps_find_filler(rec.written(), iv) == (far.A_FRAMES - far.A_FIRST) + 1
            if layout == 'planar':
                continue
            (buf, d) = far.tight_batch(src_b, layout, fmt, rng)
            (desc, c_tight, c_far) = far.far_rows_desc(layout, d)
            rec = Recorder()
            iv = far.put_far_rows(rec, layout, buf, d, c_tight, c_far)
            assert far.assert_wraps_find_filler(rec.written(), iv) >= (far.B_ROWS - 64) + (far.B_ROWS - 128)
            assert rec.written()[-1][1] == far.frame_extent(layout, desc) <= desc.frame_stride <= ARENA_BYTES
            if c_far is not None:
                assert min(desc.u_offset, desc.v_offset) == c_far >= 1 << 32
    rec = Recorder()
    rec.put(0, np.zeros(200000, np.uint8))
    rec.put(far.A_FIRST * far.A_STRIDE, np.zeros(200000, np.uint8))
    with pytest.raises(AssertionError):
        far.assert_wraps_find_filler(rec.written(), rec.written()[1:])


# ------------------------------------------------------------------------------------------------------------- GPU ---------
class State:
    """The module's arena, its host twin, and three readers (MELF_MATCH fast, gen, dot4) per meter_rect, all made on first use."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.arena = None
        self.twin = None
        self._readers = {}
        self.kernels = set()

    def memory(self):
        if self.arena is None:
            self.arena = far.FarArena(ARENA_BYTES)
            self.twin = far.HostTwin(ARENA_BYTES)
        return self.arena, self.twin

    def readers(self, key):
        """[(reader, the kernel melf_ctx_last_match names)] for key 'frames' (the fixture's meter_rect) or 'rows' (B_RECT)."""
        from meterelf_amd import MeterReader, _params
        if key not in self._readers:
            params = (_params.load(os.path.join(fc.GOLDEN, 'sample-images1', 'params.yml')) if key == 'frames'
                      else fc.params_with_rect(self.tmp, 'sample-images1', B_RECT, 'rows'))
            made = self._readers[key] = []
            mp = pytest.MonkeyPatch()
            try:
                for (kind, kernel) in fc.MATCH_KINDS:
                    mp.setenv('MELF_MATCH', kind)
                    r = MeterReader(params)
                    r.ctx.set_profiling(True)
                    made.append((r, kernel))
            finally:
                mp.undo()
        return self._readers[key]

    def close(self):
        try:
            for made in self._readers.values():
                for (r, _k) in made:
                    self.kernels |= {k for (k, (_ms, cnt)) in r.ctx.timings().items() if cnt}
                    r.close()
            print('kernels the far placements reached: ' + ' '.join(sorted(self.kernels)))
        finally:
            if self.arena is not None:
                self.arena.free()
                self.twin.free()


@pytest.fixture(scope='module')
def state(tmp_path_factory):
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    st = State(tmp_path_factory.mktemp('far'))
    try:
        yield st
    finally:
        st.close()


def ran(ctx, kernel, family, tag):
    assert ctx.last_match()['kernel'] == kernel, tag
    assert ctx.last_dials()['family'] == family, (tag, ctx.last_dials())


def same_records(got, want, tag):
    assert got.tobytes() == want.tobytes(), (tag, 'frames that differ', [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()])


@pytest.mark.gpu
@pytest.mark.parametrize('layout', far.LAYOUTS)
def test_far_frames(state, layout):
    """Placement A, every format of the family, the device entry point on the arena and the host entry point on its twin, under
    the three match kernels: 33 records equal to read_frames of the BGR frames -- sixteen frames of filler and the seventeen far
    frames, which all read FRAME_OK."""
    (arena, twin) = state.memory()
    src = flc.Source(frames_a())
    rng = np.random.default_rng(16)
    for fmt in far.FORMATS[layout]:
        (buf, d) = far.tight_batch(src, layout, fmt, rng)
        desc = far.far_frames_desc(d)
        assert far.A_FIRST * desc.frame_stride >= 1 << 31 and (desc.n - 1) * desc.frame_stride >= 1 << 32
        assert (desc.n - 1) * desc.frame_stride + d.frame_stride <= arena.nbytes <= far.ARENA_MAX
        for mem in (arena, twin):
            mem.reset()
            iv = far.put_far_frames(mem, buf, d)
            assert mem.written() == iv and len(iv) == 17
            assert far.assert_wraps_find_filler(mem.written(), iv) == 18   # frames 16 .. 32 at 2^31, frame 32 at 2^32
        ref = flc.reference_bgr(src, layout, fmt)
        for (r, kernel) in state.readers('frames'):
            for (mem, entry, where) in ((arena, flc.dev_batch, 'device'), (twin, flc.host_batch, 'host')):
                fill = far.filler_bgr(layout, fmt, d.H, d.W, mem.FILL)
                want = r.read_frames(np.concatenate([np.repeat(fill, far.A_FIRST, axis=0), ref]))
                assert r.ctx.last_match()['kernel'] == kernel
                assert (want['status'][far.A_FIRST:] == _hip.FRAME_OK).all(), (fmt, kernel)
                assert (want['status'][:far.A_FIRST] != _hip.FRAME_OK).all(), (fmt, kernel)
                got = entry(r.ctx, layout, mem.ptr, desc)
                ran(r.ctx, kernel, far.dial_family(layout, fmt), (fmt, where))
                same_records(got, want, (layout, fmt, kernel, where))


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['views', 'yuv'])
def test_far_frames_oriented(state, layout):
    """melf_process_oriented_dev on placement A's stored arena at codes 3 and 6: k_orient_tiles forms f * frame_stride itself.  The
    records equal read_frames of the oriented frames, and those of the far frames differ from a filler frame's."""
    (arena, _twin) = state.memory()
    src = flc.Source(frames_a())
    rng = np.random.default_rng(36)
    (H, W) = A_SHAPE
    for fmt in far.FORMATS[layout]:
        (buf, d) = far.tight_batch(src, layout, fmt, rng)
        desc = far.far_frames_desc(d)
        arena.reset()
        iv = far.put_far_frames(arena, buf, d)
        assert far.assert_wraps_find_filler(arena.written(), iv) == 18
        if layout == 'views':
            stored = np.concatenate([np.full((far.A_FIRST, H, W, 3), far.FILL, np.uint8), src.bgr])
        else:
            planes = [np.concatenate([np.full((far.A_FIRST,) + p.shape[1:], far.FILL, np.uint8), p]) for p in src.yuv(1, 1)]
        for code in (3, 6):
            if layout == 'views':
                upright = np.ascontiguousarray(oc.orient(stored, code, axes=(1, 2)))
            else:
                upright = fc.yuv_to_bgr(*[np.ascontiguousarray(oc.orient(p, code, axes=(1, 2))) for p in planes], 1, 1, 0)
            for (r, kernel) in state.readers('frames'):
                want = r.read_frames(upright)
                assert all(want[i].tobytes() != want[0].tobytes() for i in range(far.A_FIRST, far.A_FRAMES)), (fmt, code, kernel)
                got = r.ctx.process_oriented_dev(layout, desc, code, arena.ptr)
                ran(r.ctx, kernel, far.dial_family(layout, fmt), (fmt, code))
                same_records(got, want, (layout, fmt, code, kernel))


def place_far_rows(mems, src, layout, fmt, rng):
    """Placement B of src's one frame in format fmt on every memory of mems (the arena, its twin), with its preconditions.
    Returns the far descriptor."""
    (buf, d) = far.tight_batch(src, layout, fmt, rng)
    (desc, c_tight, c_far) = far.far_rows_desc(layout, d)
    pitch = desc.y_pitch if hasattr(desc, 'y_pitch') else desc.row_pitch
    assert 64 * pitch >= 1 << 31 and 128 * pitch >= 1 << 32 and 192 * pitch >= 3 << 31
    if c_far is not None:
        assert min(desc.u_offset, desc.v_offset) >= 1 << 32
    for mem in mems:
        assert far.frame_extent(layout, desc) <= mem.nbytes <= far.ARENA_MAX
        mem.reset()
        iv = far.put_far_rows(mem, layout, buf, d, c_tight, c_far)
        assert far.assert_wraps_find_filler(mem.written(), iv) >= (far.B_ROWS - 64) + (far.B_ROWS - 128)
    return desc


def far_rows_decide(r, ref, want, tag):
    """The rows beyond 2^32, and those beyond 2^31, decide the record: with them replaced by filler the frame reads differently."""
    assert (want['status'] == _hip.FRAME_OK).all(), tag
    for cut in (128, 64):
        near = ref.copy()
        near[:, cut:] = far.FILL
        assert r.read_frames(near).tobytes() != want.tobytes(), (tag, cut)


@pytest.mark.gpu
@pytest.mark.parametrize('layout', [la for la in far.LAYOUTS if la != 'planar'])
def test_far_rows(state, layout):
    """Placement B, every format of the family, under the three match kernels: the device entry point on the arena, and the host
    entry point on its twin (the host packer walks the same far rows)."""
    (arena, twin) = state.memory()
    src = flc.Source(frames_b(1))
    rng = np.random.default_rng(25)
    for fmt in far.FORMATS[layout]:
        desc = place_far_rows((arena, twin), src, layout, fmt, rng)
        ref = flc.reference_bgr(src, layout, fmt)
        for (r, kernel) in state.readers('rows'):
            want = r.read_frames(ref)
            assert r.ctx.last_match()['kernel'] == kernel
            far_rows_decide(r, ref, want, (fmt, kernel))
            for (mem, entry, where) in ((arena, flc.dev_batch, 'device'), (twin, flc.host_batch, 'host')):
                got = entry(r.ctx, layout, mem.ptr, desc)
                ran(r.ctx, kernel, far.dial_family(layout, fmt), (fmt, where))
                same_records(got, want, (layout, fmt, kernel, where))


@pytest.mark.gpu
@pytest.mark.parametrize('layout,fmt', [('views', 'bgr'), ('views', 'rgba'), ('yuv', 'nv12'), ('yuv', 'i420')])
def test_far_rows_lists(state, layout, fmt):
    """Placement B read through the pointer lists: melf_process_frame_list_dev with the frame's pointer (k_gather_rows computes
    row * src_pitch) and, for the 4:2:0 frames, melf_process_plane_list_dev with one pointer per plane into the arena (k_plane_rows;
    the Y plane has the far rows)."""
    (arena, _twin) = state.memory()
    src = flc.Source(frames_b(1))
    desc = place_far_rows((arena,), src, layout, fmt, np.random.default_rng(52))
    ref = flc.reference_bgr(src, layout, fmt)
    for (r, kernel) in state.readers('rows'):
        want = r.read_frames(ref)
        far_rows_decide(r, ref, want, (fmt, kernel))
        got = r.ctx.process_frame_list_dev(layout, desc, [arena.ptr])
        ran(r.ctx, kernel, far.dial_family(layout, fmt), (fmt, 'frame list'))
        same_records(got, want, (layout, fmt, kernel, 'frame list'))
        if layout == 'yuv':
            c = plc.cut(layout, desc)
            assert c.offsets[0] == 0 and min(c.offsets[1:]) >= 1 << 32
            got = r.ctx.process_plane_list_dev(layout, c.desc, [[arena.ptr + off for off in c.offsets]], c.nplanes)
            ran(r.ctx, kernel, far.dial_family(layout, fmt), (fmt, 'plane list'))
            same_records(got, want, (layout, fmt, kernel, 'plane list'))


@pytest.mark.gpu
def test_far_planes(state):
    """Placement C: planar RGB with the planes at 0, 2^32 + 64 and 2^33 + 128 at a tight pitch, in all three channel orders, the
    device entry point on the arena and the host entry point on its twin.  Two frames whose planes interleave: frame k's base is k
    planes (rounded up to 64 bytes) behind the arena's, each read by a one-frame call -- melf_planar_frames wants a frame_stride
    of at least one frame's span, so one descriptor cannot hold both.
    A plane offset cut to 32 bits does not find filler here: 2^32 + 64 modulo 2^32 lies inside the first plane, whatever the
    frame's size.  What is asserted instead is what that precondition is for: the frame read with the second and / or the third
    plane fetched at the wrapped offset (bytes of the first plane, 64 / 128 bytes on) gives another record."""
    (arena, twin) = state.memory()
    src = flc.Source(frames_b(2))
    rng = np.random.default_rng(33)
    (H, W) = B_SHAPE
    span = H * W
    step = (span + 63) // 64 * 64
    for order in far.FORMATS['planar']:
        (buf, d) = far.tight_batch(src, 'planar', order, rng)
        assert d.frame_stride == 3 * span and d.row_pitch == W
        desc = oc.copy_desc(d)
        desc.n = 1
        for (k, ch) in enumerate(order):
            setattr(desc, ch + '_offset', far.C_OFFSETS[k])
        desc.frame_stride = (far.C_OFFSETS[2] + span + 15) // 16 * 16
        assert sorted((desc.b_offset, desc.g_offset, desc.r_offset)) == [0, (1 << 32) + 64, (1 << 33) + 128]
        assert step + far.frame_extent('planar', desc) <= arena.nbytes <= far.ARENA_MAX
        for mem in (arena, twin):
            mem.reset()
            for f in range(2):
                for k in range(3):
                    mem.put(f * step + far.C_OFFSETS[k], buf[f * d.frame_stride + k * span:f * d.frame_stride + (k + 1) * span])
        # the first 2^32 bytes hold the two first planes and filler: what a wrapped plane offset reads
        low = np.full(2 * step + span + 256, far.FILL, np.uint8)
        for f in range(2):
            low[f * step:f * step + span] = buf[f * d.frame_stride:f * d.frame_stride + span]
        for (r, kernel) in state.readers('rows'):
            want = r.read_frames(src.bgr)
            assert r.ctx.last_match()['kernel'] == kernel
            assert (want['status'] == _hip.FRAME_OK).all() and want[0].tobytes() != want[1].tobytes()
            for f in range(2):
                for wrapped in ((1,), (2,), (1, 2)):
                    bad = src.bgr[f:f + 1].copy()
                    for k in wrapped:
                        at = f * step + far.C_OFFSETS[k] % (1 << 32)
                        bad[0, :, :, 'bgr'.index(order[k])] = low[at:at + span].reshape(H, W)
                    assert r.read_frames(bad).tobytes() != want[f:f + 1].tobytes(), (order, f, wrapped, kernel)
                for (mem, entry, where) in ((arena, flc.dev_batch, 'device'), (twin, flc.host_batch, 'host')):
                    got = entry(r.ctx, 'planar', mem.ptr + f * step, desc)
                    ran(r.ctx, kernel, 'planar', (order, f, where))
                    same_records(got, want[f:f + 1], ('planar', order, f, kernel, where))


@pytest.mark.gpu
@pytest.mark.parametrize('layout', list(TO_BGR))
def test_far_frames_to_bgr(state, layout):
    """The conversion kernels on placement A.  Every *_to_bgr entry point takes host memory, so the frames come from the host twin:
    one call on all 33 frames (12 MB of output; the kernel forms f * frame_stride for frames beyond 2^31 and 2^32 of the uploaded
    batch) and three one-frame calls with the base moved to frames 0, 16 and 32, against frame_cases.yuv_to_bgr of the samples."""
    from meterelf_amd import MeterReader, _params
    (_arena, twin) = state.memory()
    (method, fmt) = TO_BGR[layout]
    src = flc.Source(frames_a())
    (buf, d) = far.tight_batch(src, layout, fmt, np.random.default_rng(7))
    desc = far.far_frames_desc(d)
    assert far.A_FIRST * desc.frame_stride >= 1 << 31 and (desc.n - 1) * desc.frame_stride >= 1 << 32
    twin.reset()
    iv = far.put_far_frames(twin, buf, d)
    assert far.assert_wraps_find_filler(twin.written(), iv) == 18
    want = np.concatenate([np.repeat(far.filler_bgr(layout, fmt, d.H, d.W, twin.FILL), far.A_FIRST, axis=0), flc.reference_bgr(src, layout, fmt)])
    assert want.nbytes <= 64 << 20
    r = MeterReader(_params.load(os.path.join(fc.GOLDEN, 'sample-images1', 'params.yml')))
    try:
        r.ctx.set_profiling(True)
        got = getattr(r.ctx, method)(twin.ptr, desc)
        differ = [i for i in range(far.A_FRAMES) if not np.array_equal(got[i], want[i])]
        assert not differ, (layout, fmt, differ)
        one = oc.copy_desc(desc)
        one.n = 1
        for f in (0, far.A_FIRST, far.A_FRAMES - 1):
            assert np.array_equal(getattr(r.ctx, method)(twin.ptr + f * desc.frame_stride, one)[0], want[f]), (layout, fmt, f)
        state.kernels |= {k for (k, (_ms, cnt)) in r.ctx.timings().items() if cnt}
    finally:
        r.close()
