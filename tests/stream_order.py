"""Support for tests/test_stream_order.py and tests/stream_order_torch_child.py: the stream-order contract of the *_dev entry points
(include/meterelf_hip.h; DESIGN.md section 3, "Stream order").  No test functions here.

The gate.  A Gate holds a HIP stream still until the test opens it, with no GPU code of its own: hipLaunchHostFunc(stream, fn, NULL)
on the runtime instance helpers.hip_runtime() returns, fn a ctypes callback that waits on a threading.Event.  Work enqueued on the
stream behind the gate -- and whatever the library orders behind that work with events -- cannot start before Gate.release(); work
that was wrongly left unordered runs at once, 50 ms ahead of its producers, and the records show it.  The callback calls no HIP
function; its wait has a ceiling of 20 s, after which it returns by itself and sets Gate.expired, so nothing can hang; the callback
object lives as long as the Gate, which `gated` keeps until the stream has been synchronised.  Every test asserts at its end that no
gate expired (Gate.check): an expired gate is a failure, never a pass.  Gate.release() first asserts hipStreamQuery(stream) ==
hipErrorNotReady -- the gate really held -- and sleeps 50 ms with the gate closed: two hundred times the 0.24 - 0.26 ms of a 1024-frame
step; the steps of this module's 48-frame shapes have not been measured.

Rules for a gated section (between Gate() and release()); breaking one blocks the host until the ceiling:
- allocate and free all device memory outside it;
- make an ungated warm-up call of the same shape and mode first ON EACH LANE (the buffers are the lane's: a warm-up that ran on the
  other lane leaves the gated call to grow its own), so that no grow(), table build or gen_entry eviction synchronises the device
  while the gate is closed;
- never pass want_host=True or out_host, never call hipDeviceSynchronize or ctx.sync();
- at most one list call per lane: the next one waits on the host for the previous pointer-table upload (ev_list_tab);
- gated streams are created hipStreamNonBlocking.

What a pass does not show: streams share the process's few hardware queues, and a stream that shares one with the held stream is
held with it.  Work that the library wrongly leaves unordered on such a stream cannot run ahead, and that run does not see the
mistake.  The tests here keep to one or two caller streams; with the library's ordering calls removed one at a time (the ev_join and
ev_call waits of the resident batch and list flows, the ev_fork waits, claim_lane's ev_order wait) each targeted test failed.  A
scenario with the unordered work on a further caller stream passed with claim_lane's wait removed -- its event stayed unready while
the gate was closed, which a shared queue would explain; the cause was not looked into further -- and is not here.

The scene all cases share: R, 48 synthetic sample-images1 frames (test_gpu_parity.synth_frames), and D, the decoy: R rolled by one
frame.  A Case expresses both in one entry point's input format with the existing *_cases modules, as the bytes of one or more device
allocations, and knows the device call and the host call of that entry point; references() takes the records of R and of D from the
host path and asserts that every frame of both reads with status OK and that the two records of every slot differ bytewise.  FILL
(0xEE) is the byte the tests pre-fill results with: no valid record and no mask value."""
import contextlib
import ctypes as C
import functools
import glob
import os
import sys
import threading
import time
from typing import Callable, NamedTuple, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402

HIP_ERROR_NOT_READY = 600
STREAM_NON_BLOCKING = 1
(H2D, D2H, D2D) = (1, 2, 3)
CEILING = 20.0       # seconds a closed gate holds at the most
HEAD_START = 0.05    # seconds a gate stays closed after the last enqueue
FILL = 0xEE
N = 48               # frames of the scene
N_LIST = 12          # elements of a list
SEED = 62
RSZ = _hip.RESULT_DTYPE.itemsize
HOST_FN = C.CFUNCTYPE(None, C.c_void_p)


# ------------------------------------------------------------------------------------------------------------ the runtime ---
class Hip:
    """The few runtime calls the tests make themselves, checked; device addresses and streams are ints."""

    def __init__(self):
        from tests.helpers import hip_runtime
        self.rt = hip_runtime()

    @staticmethod
    def _ok(rc, what):
        assert rc == 0, '%s failed with HIP error %d' % (what, rc)

    def malloc(self, nbytes):
        p = C.c_void_p()
        self._ok(self.rt.hipMalloc(C.byref(p), C.c_size_t(max(int(nbytes), 1))), 'hipMalloc')
        return p.value

    def free(self, p):
        self.rt.hipFree(C.c_void_p(p))

    def upload(self, p, arr):
        """blocking; outside gated sections only"""
        arr = np.ascontiguousarray(arr)
        self._ok(self.rt.hipMemcpy(C.c_void_p(p), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), H2D), 'hipMemcpy')

    def download(self, p, nbytes):
        """blocking; outside gated sections only"""
        out = np.empty(nbytes, np.uint8)
        self._ok(self.rt.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(nbytes), D2H), 'hipMemcpy')
        return out

    def fill(self, p, byte, nbytes):
        """blocking"""
        self._ok(self.rt.hipMemset(C.c_void_p(p), byte, C.c_size_t(nbytes)), 'hipMemset')
        self._ok(self.rt.hipDeviceSynchronize(), 'hipDeviceSynchronize')

    def copy_async(self, dst, src, nbytes, stream):
        self._ok(self.rt.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), D2D, C.c_void_p(stream)), 'hipMemcpyAsync')

    def fill_async(self, p, byte, nbytes, stream):
        self._ok(self.rt.hipMemsetAsync(C.c_void_p(p), byte, C.c_size_t(nbytes), C.c_void_p(stream)), 'hipMemsetAsync')

    def stream(self):
        s = C.c_void_p()
        self._ok(self.rt.hipStreamCreateWithFlags(C.byref(s), STREAM_NON_BLOCKING), 'hipStreamCreateWithFlags')
        return s.value

    def stream_destroy(self, s):
        self.rt.hipStreamDestroy(C.c_void_p(s))

    def stream_sync(self, s):
        self._ok(self.rt.hipStreamSynchronize(C.c_void_p(s)), 'hipStreamSynchronize')

    def stream_query(self, s):
        return self.rt.hipStreamQuery(C.c_void_p(s))

    def event(self):
        e = C.c_void_p()
        self._ok(self.rt.hipEventCreateWithFlags(C.byref(e), 2), 'hipEventCreateWithFlags')   # hipEventDisableTiming
        return e.value

    def event_destroy(self, e):
        self.rt.hipEventDestroy(C.c_void_p(e))

    def event_record(self, e, s):
        self._ok(self.rt.hipEventRecord(C.c_void_p(e), C.c_void_p(s)), 'hipEventRecord')

    def event_query(self, e):
        return self.rt.hipEventQuery(C.c_void_p(e))

    def device_sync(self):
        self._ok(self.rt.hipDeviceSynchronize(), 'hipDeviceSynchronize')


# --------------------------------------------------------------------------------------------------------------- the gate ---
class Gate:
    """Closes `stream` (an int) at the point of construction; release() opens it.  The module docstring has the rules."""

    def __init__(self, hip, stream, ceiling=CEILING):
        self.hip = hip
        self.stream = stream
        self.expired = False
        self._open = threading.Event()

        def wait(_user):
            if not self._open.wait(ceiling):
                self.expired = True
        self._fn = HOST_FN(wait)   # alive as long as the gate
        hip._ok(hip.rt.hipLaunchHostFunc(C.c_void_p(stream), self._fn, None), 'hipLaunchHostFunc')

    def holds(self):
        return not self.expired and self.hip.stream_query(self.stream) == HIP_ERROR_NOT_READY

    def open(self):
        self._open.set()

    def release(self):
        """The gate really held; whatever was wrongly left unordered gets its head start; open."""
        assert self.holds(), 'the gate did not hold its stream (expired: %s)' % self.expired
        time.sleep(HEAD_START)
        assert self.holds(), 'the gate did not hold its stream for the head start (expired: %s)' % self.expired
        self.open()

    def check(self):
        assert not self.expired, 'a gate ran into its ceiling: something waited on the host for gated work'


@contextlib.contextmanager
def gated(hip, stream, ceiling=CEILING):
    """A Gate on `stream`; whatever happens inside, the gate is opened and the stream synchronised before the caller frees anything,
    and the callback outlives that."""
    gate = Gate(hip, stream, ceiling)
    try:
        yield gate
    finally:
        gate.open()
        hip.rt.hipStreamSynchronize(C.c_void_p(stream))


# -------------------------------------------------------------------------------------------------------------- the scene ---
@functools.lru_cache(maxsize=None)
def scene():
    """(R, D): the real frames and the decoys, (48, H, W, 3) BGR each, read-only"""
    from tests.test_gpu_parity import GOLDEN, _good, synth_frames
    files = _good(sorted(glob.glob(os.path.join(GOLDEN, 'sample-images1', '*.jpg'))))
    R = synth_frames(files, N, SEED)
    D = np.roll(R, 1, axis=0)
    R.setflags(write=False)
    D.setflags(write=False)
    return R, D


class Case(NamedTuple):
    real: list                # uint8 arrays, one per input allocation of the call (Arena): R in the entry point's format
    decoy: list               # D the same way: same count and sizes
    dev: Callable             # dev(ctx, ptrs, d_out, stream): enqueues the call on the allocations at ptrs (ints), results to d_out
    host: Optional[Callable]  # host(ctx, arrays) -> the records of the host path of the same entry point (None: no host reference)
    promised: bool            # a contiguous batch through batch_dev: complete at the call in frames-resident mode
    out_bytes: int            # bytes the call writes
    pick: Optional[list] = None   # result slot -> frame of the scene (None: slot i = frame i)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


@functools.lru_cache(maxsize=None)
def _scene_bytes():
    return [[_bytes(x)] for x in scene()]


def _view_bytes(v):
    return np.frombuffer((C.c_uint8 * v.extent).from_address(v.ptr), np.uint8).copy()


def _both(make):
    """make(bgr frames) -> (list of arrays, anything the calls need) for R and for D; the second parts must agree in what matters"""
    (R, D) = scene()
    (real, aux) = make(R)
    (decoy, _aux) = make(D)
    assert [len(a) for a in real] == [len(a) for a in decoy]
    return real, decoy, aux


def _batch_case():
    (R, D) = scene()
    (n, H, W) = R.shape[:3]
    return Case(*_scene_bytes(),
                lambda ctx, p, out, st: ctx.process_batch_dev(p[0], n, H, W, d_results_ptr=out, want_host=False, stream=st),
                lambda ctx, a: ctx.process_batch(a[0].reshape(R.shape)), True, n * RSZ)


def _stream_case():
    """melf_process_stream_dev's overlapped branch: 3 batches of 32 over the 48 frames, 8 frames apart"""
    (R, D) = scene()
    (n, H, W) = R.shape[:3]
    (nb, m, step) = (3, 32, 8)
    assert (nb - 1) * step + m == n
    return Case(*_scene_bytes(),
                lambda ctx, p, out, st: ctx.process_stream_dev(p[0], nb, step * H * W * 3, m, H, W, out, m, stream=st),
                lambda ctx, a: ctx.process_batch(a[0].reshape(R.shape)), False, nb * m * RSZ, [b * step + j for b in range(nb) for j in range(m)])


def _hls_case():
    (R, D) = scene()
    (n, H, W) = R.shape[:3]
    return Case(*_scene_bytes(), lambda ctx, p, out, st: ctx.hls_inrange_close_dev(p[0], n, H, W, out, stream=st), None, False, n * H * W)


def _family_batch_case(layout, fmt):
    """one contiguous batch of a descriptor family through its melf_process_*_dev (batch_dev, as melf_process_batch_dev)"""
    from tests import frame_list_cases as flc

    def make(bgr):
        (arr, view, _kw) = flc.make(flc.Source(bgr.copy()), layout, fmt, np.random.default_rng(1))
        v = view(arr)
        assert not v.copied and v.n == N
        return [_view_bytes(v)], flc.descriptor(v)
    (real, decoy, desc) = _both(make)
    return Case(real, decoy, lambda ctx, p, out, st: flc.dev_batch(ctx, layout, p[0], desc, d_results_ptr=out, want_host=False, stream=st),
                lambda ctx, a: flc.host_batch(ctx, layout, a[0].ctypes.data, desc), True, N * RSZ)


def _cut(bgr, n=N):
    """the frames' top-left part that holds meter_rect, as tests/test_wide_list.py cuts them"""
    return np.ascontiguousarray(bgr[:n, :412, :302])


def _wide_case():
    """melf_process_wide_dev: float16, planar"""
    from tests import wide_cases as wc
    from tests import wide_list_cases as wl

    def make(bgr):
        case = wl.fixture_case(_cut(bgr), wc.F16, 0, True)
        return [_bytes(case.buf)], case.desc
    (real, decoy, desc) = _both(make)
    return Case(real, decoy, lambda ctx, p, out, st: ctx.process_wide_dev(p[0], desc, d_results_ptr=out, want_host=False, stream=st),
                lambda ctx, a: ctx.process_wide(a[0].ctypes.data, desc), False, N * RSZ)


def _oriented_case(code=6):
    """melf_process_oriented_dev: packed BGR stored so that rot90cw (a transposing orientation) makes it upright"""
    from tests import frame_list_cases as flc
    from tests import oriented_cases as oc

    def make(bgr):
        (arr, view, _kw) = flc.make(flc.Source(bgr.copy()), 'views', 'bgr', np.random.default_rng(1))
        v = view(arr)
        (d, buf) = oc.stored_batch('views', flc.descriptor(v), oc.as_buffer(v), code)
        return [_bytes(buf)], d
    (real, decoy, d) = _both(make)
    return Case(real, decoy, lambda ctx, p, out, st: ctx.process_oriented_dev('views', d, code, p[0], d_results_ptr=out, want_host=False, stream=st),
                lambda ctx, a: ctx.process_oriented('views', d, code, a[0].ctypes.data), False, N * RSZ)


def _frame_list_case(layout, fmt):
    """melf_process_frame_list_dev: 12 frames, each with a pointer of its own"""
    from tests import frame_list_cases as flc

    def make(bgr):
        (arr, view, _kw) = flc.make(flc.Source(bgr[:N_LIST].copy()), layout, fmt, np.random.default_rng(1))
        v = view(arr)
        assert not v.copied and v.n == N_LIST
        ext = flc.frame_extent(v)
        whole = _view_bytes(v)
        return [whole[i * v.frame_stride:i * v.frame_stride + ext].copy() for i in range(N_LIST)], flc.descriptor(v)
    (real, decoy, desc) = _both(make)
    return Case(real, decoy, lambda ctx, p, out, st: ctx.process_frame_list_dev(layout, desc, p, d_results_ptr=out, want_host=False, stream=st),
                lambda ctx, a: ctx.process_frame_list(layout, desc, [x.ctypes.data for x in a]), False, N_LIST * RSZ)


def _plane_list_case(layout, fmt):
    """melf_process_plane_list_dev: 12 frames, every plane with a pointer of its own"""
    from tests import frame_list_cases as flc
    from tests import plane_list_cases as plc

    def make(bgr):
        b = plc.batch(flc.Source(bgr[:N_LIST].copy()), layout, fmt, np.random.default_rng(1))
        c = plc.cut(layout, b.desc)
        planes = [np.frombuffer((C.c_uint8 * c.extents[k]).from_address(addr), np.uint8).copy()
                  for row in plc.host_addresses(b, c) for (k, addr) in enumerate(row)]
        return planes, (c.desc, c.nplanes)
    (real, decoy, (desc, nplanes)) = _both(make)
    return Case(real, decoy,
                lambda ctx, p, out, st: ctx.process_plane_list_dev(layout, desc, p, nplanes, d_results_ptr=out, want_host=False, stream=st),
                lambda ctx, a: ctx.process_plane_list(layout, desc, [x.ctypes.data for x in a], nplanes), False, N_LIST * RSZ)


def _wide_list_case(planes):
    """melf_process_wide_list_dev (float16, packed) / melf_process_wide_plane_list_dev (float16, planar): 12 frames"""
    from tests import wide_cases as wc
    from tests import wide_list_cases as wl

    def make(bgr):
        case = wl.fixture_case(_cut(bgr, N_LIST), wc.F16, 0, planes)
        if planes:
            return [_bytes(p) for fr in case.host_planes for p in fr], case.plane_desc
        return [_bytes(f) for f in case.host_frames], case.list_desc
    (real, decoy, desc) = _both(make)
    if planes:
        return Case(real, decoy, lambda ctx, p, out, st: ctx.process_wide_plane_list_dev(desc, p, d_results_ptr=out, want_host=False, stream=st),
                    lambda ctx, a: ctx.process_wide_plane_list(desc, [x.ctypes.data for x in a]), False, N_LIST * RSZ)
    return Case(real, decoy, lambda ctx, p, out, st: ctx.process_wide_list_dev(desc, p, d_results_ptr=out, want_host=False, stream=st),
                lambda ctx, a: ctx.process_wide_list(desc, [x.ctypes.data for x in a]), False, N_LIST * RSZ)


CASES = {
    'batch': _batch_case,
    'yuv-nv12': lambda: _family_batch_case('yuv', 'nv12'),
    'wide-f16-planar': _wide_case,
    'oriented-rot90cw': _oriented_case,
    'frame-list-views': lambda: _frame_list_case('views', 'bgr'),
    'frame-list-nv12': lambda: _frame_list_case('yuv', 'nv12'),
    'plane-list-nv12': lambda: _plane_list_case('yuv', 'nv12'),
    'wide-list': lambda: _wide_list_case(False),
    'wide-plane-list': lambda: _wide_list_case(True),
    'stream': _stream_case,
    'hls-mask': _hls_case,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def references(ctx, c):
    """(ref_R, ref_D) as bytes, from the host path of the case's entry point: every frame of both sets reads with status OK, and
    the two records of every result slot differ bytewise"""
    out = []
    for arrays in (c.real, c.decoy):
        recs = c.host(ctx, arrays)
        assert (recs['status'] == _hip.FRAME_OK).all(), recs['status']
        out.append(recs[c.pick] if c.pick is not None else recs)
    (ref_R, ref_D) = out
    assert len(ref_R) * RSZ == c.out_bytes
    assert all(ref_R[i].tobytes() != ref_D[i].tobytes() for i in range(len(ref_R)))
    assert bytes([FILL]) * RSZ not in (ref_R.tobytes(), ref_D.tobytes())
    return ref_R.tobytes(), ref_D.tobytes()


# --------------------------------------------------------------------------------------------------- the device side ---
class Arena:
    """The input allocations of a call, side by side in one device allocation, 256-byte aligned and a varying number of bytes apart,
    so that one runtime copy fills all of them and one memset clears them: a gated section is the same handful of commands whatever
    the number of elements.  ptrs: their addresses."""

    def __init__(self, hip, arrays):
        self.hip = hip
        offs = []
        at = 0
        for (k, a) in enumerate(arrays):
            offs.append(at)
            at += (len(a) + 255) // 256 * 256 + 256 * (k % 3)
        self.nbytes = max(at, 1)
        self.base = hip.malloc(self.nbytes)
        hip.fill(self.base, 0, self.nbytes)
        self.ptrs = [self.base + o for o in offs]
        self.set(arrays)

    def set(self, arrays):
        """blocking: outside gated sections"""
        for (p, a) in zip(self.ptrs, arrays):
            self.hip.upload(p, a)
        self.hip.device_sync()

    def copy_from(self, src, stream):
        assert src.nbytes == self.nbytes
        self.hip.copy_async(self.base, src.base, self.nbytes, stream)

    def zero(self, stream):
        self.hip.fill_async(self.base, 0, self.nbytes, stream)


class Rig:
    """The device memory of one case, all of it allocated before and freed after the gated section: `frames`, the Arena of the
    call's input, holding D; `real`, one holding R; `decoy`, one holding D (on request); d_out, the call's results, zeros; d_keep, as
    large, zeros.  extra_out: more result / keep pairs."""

    def __init__(self, hip, c, with_decoy=False, extra_out=0):
        self.hip = hip
        self.c = c
        self.frames = Arena(hip, c.decoy)
        self.real = Arena(hip, c.real)
        self.decoy = Arena(hip, c.decoy) if with_decoy else None
        self.outs = [self._zeros(c.out_bytes) for _ in range(1 + extra_out)]
        self.keeps = [self._zeros(c.out_bytes) for _ in range(1 + extra_out)]
        (self.d_out, self.d_keep) = (self.outs[0], self.keeps[0])
        hip.device_sync()

    def _zeros(self, nbytes):
        p = self.hip.malloc(nbytes)
        self.hip.fill(p, 0, nbytes)
        return p

    def kept(self, k=0):
        return self.hip.download(self.keeps[k], self.c.out_bytes).tobytes()

    def free(self):
        for a in (self.frames, self.real, self.decoy):
            if a is not None:
                self.hip.free(a.base)
        for p in self.outs + self.keeps:
            self.hip.free(p)
        (self.frames, self.real, self.decoy, self.outs, self.keeps) = (None, None, None, [], [])
