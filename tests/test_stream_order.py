"""The stream-order contract of the *_dev entry points (include/meterelf_hip.h; DESIGN.md section 3, "Stream order"): what a call
waits for and what the caller's stream waits for afterwards, per entry point, without and with melf_ctx_set_frames_resident.

Every other test of these paths drains the device before and after each call and so cannot see a missing event wait.  Here the
caller's stream is held by a gate (tests/stream_order.py: a host function that waits for the test) while the producer of the frames,
the library call and the consumers of the records are enqueued behind it; anything the library leaves unordered runs 50 ms early,
on decoy frames or into results that are then overwritten.  The base sequence on the gated stream S (`frames` hold the decoys D,
d_out zeros):

    gate | d_out <- 0xEE | frames <- R | the call (d_out) | d_keep <- d_out | frames <- 0 | d_out <- 0xEE | release, synchronise S

and d_keep must hold the records of R: read-after-write on the frames, write-after-write and read-after-write on the records,
write-after-read on both.  For a contiguous batch in frames-resident mode the frames are promised complete at the call: `frames`
hold R from the start and there is no producer copy; list-flow calls keep it in both modes (the promise covers batches only).

The self-tests at the end make the mistake on the test's side -- the call or the consumer on another stream -- and must see the
decoys' records, or the fill."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import stream_order as so

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def rt():
    """One reader of sample-images1 and the runtime; the cases' host arrays are dropped with the module"""
    from meterelf_amd import MeterReader, _hip, _params
    from tests.test_gpu_parity import GOLDEN
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    reader = MeterReader(_params.load(os.path.join(GOLDEN, 'sample-images1', 'params.yml')))
    yield reader.ctx, so.Hip()
    reader.close()
    for f in (so.case, so.scene, so._scene_bytes):
        f.cache_clear()


class Session:
    """A test's streams and rigs: freed in the order that is safe whatever failed (mode back, context drained, then streams, then
    memory), as the existing lane tests do in their finally."""

    def __init__(self, rt):
        (self.ctx, self.hip) = rt
        self.streams = []
        self.rigs = []
        self.events = []
        self.gates = []
        self._spare = None

    def __enter__(self):
        self.ctx.sync()   # the lanes forget earlier tests' streams: the first caller stream gets lane 0, the second lane 1
        return self

    def stream(self):
        self.streams.append(self.hip.stream())
        return self.streams[-1]

    def spare(self):
        """a stream for the warm-up of the second lane"""
        if self._spare is None:
            self._spare = self.stream()
        return self._spare

    def rig(self, c, **kw):
        self.rigs.append(so.Rig(self.hip, c, **kw))
        return self.rigs[-1]

    def event(self):
        self.events.append(self.hip.event())
        return self.events[-1]

    def gate(self, stream, ceiling=so.CEILING):
        cm = so.gated(self.hip, stream, ceiling)
        g = cm.__enter__()
        self.gates.append((cm, g))
        return g

    def __exit__(self, *exc):
        for (cm, _g) in self.gates:
            cm.__exit__(None, None, None)   # opens and synchronises the stream
        try:
            self.ctx.set_frames_resident(False)
            self.ctx.sync()
            self.hip.device_sync()
        finally:
            for s in self.streams:
                self.hip.stream_destroy(s)
            for e in self.events:
                self.hip.event_destroy(e)
            for r in self.rigs:
                r.free()
        if exc[0] is None:
            for (_cm, g) in self.gates:
                g.check()
        return False


def warm_up(s, c, rig, stream, forget=True):
    """Two ungated calls of the case's shape in the current mode, one per lane, drained: the lanes forget their streams, `stream`
    gets lane 0 and a spare stream lane 1 (in frames-resident mode consecutive calls alternate between the lanes whatever their
    stream).  Returns what the second call wrote.  forget: the lanes forget the streams again afterwards (melf_ctx_sync)"""
    s.ctx.sync()
    for st in (stream, s.spare()):
        c.dev(s.ctx, rig.frames.ptrs, rig.d_out, st)
        s.hip.stream_sync(st)
    if forget:
        s.ctx.sync()
    s.hip.device_sync()
    got = s.hip.download(rig.d_out, c.out_bytes).tobytes()
    s.hip.fill(rig.d_out, 0, c.out_bytes)
    return got


def refs(s, c, rig):
    """(ref_R, ref_D): from the host path; for the mask, which has none, from the ungated call"""
    if c.host is not None:
        return so.references(s.ctx, c)
    S = s.streams[0]
    c.dev(s.ctx, rig.real.ptrs, rig.d_out, S)
    s.hip.stream_sync(S)
    ref_R = s.hip.download(rig.d_out, c.out_bytes).tobytes()
    c.dev(s.ctx, rig.frames.ptrs, rig.d_out, S)
    s.hip.stream_sync(S)
    ref_D = s.hip.download(rig.d_out, c.out_bytes).tobytes()
    s.hip.fill(rig.d_out, 0, c.out_bytes)
    assert ref_R != ref_D and so.FILL not in np.unique(np.frombuffer(ref_R + ref_D, np.uint8))
    return ref_R, ref_D


def where(got, want, ref_D):
    """for the assertion message: how many result bytes differ, and whether the decoys' records or the fill came out"""
    n = int((np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8)).sum())
    return '%d of %d bytes differ; decoy records: %s; all fill: %s; all zero: %s' % (
        n, len(want), got == ref_D, got == bytes([so.FILL]) * len(got), got == bytes(len(got)))


# ------------------------------------------------------------------------------------------------ every entry point ---------
@pytest.mark.parametrize('resident', [False, True], ids=['ordered', 'resident'])
@pytest.mark.parametrize('name', list(so.CASES))
def test_call_is_ordered_on_its_stream(rt, name, resident):
    """The base sequence over every asynchronous entry point, in both modes."""
    c = so.case(name)
    promised = resident and c.promised
    with Session(rt) as s:
        S = s.stream()
        rig = s.rig(c)
        (ref_R, ref_D) = refs(s, c, rig)
        s.ctx.set_frames_resident(resident)
        assert warm_up(s, c, rig, S) == ref_D   # the device call on the decoys, drained: the entry point itself is right
        if promised:
            rig.frames.set(c.real)
        gate = s.gate(S)
        s.hip.fill_async(rig.d_out, so.FILL, c.out_bytes, S)
        if not promised:
            rig.frames.copy_from(rig.real, S)
        c.dev(s.ctx, rig.frames.ptrs, rig.d_out, S)
        s.hip.copy_async(rig.d_keep, rig.d_out, c.out_bytes, S)
        rig.frames.zero(S)
        s.hip.fill_async(rig.d_out, so.FILL, c.out_bytes, S)
        gate.release()
        s.hip.stream_sync(S)
        got = rig.kept()
        assert got == ref_R, where(got, ref_R, ref_D)
        assert s.hip.download(rig.d_out, c.out_bytes).tobytes() == bytes([so.FILL]) * c.out_bytes   # the call wrote nothing late


# ---------------------------------------------------------------------------------------------------- three scenarios ---------
def test_third_stream_takes_a_lane_over_behind_its_pending_call(rt):
    """S_a is gated with a call pending (lane 0); S_b makes a call (lane 1) that completes with the gate still closed; S_c makes a
    call and gets the least recently used lane, S_a's: an event recorded on S_c behind that call is not ready while the gate is
    closed, so the take-over waited for S_a's work.  All three record sets are right."""
    c = so.case('batch')
    with Session(rt) as s:
        (Sa, Sb, Sc) = (s.stream(), s.stream(), s.stream())
        rig = s.rig(c, with_decoy=True, extra_out=2)
        (ref_R, ref_D) = so.references(s.ctx, c)
        s.ctx.sync()   # (the host path took a lane for the context's own stream)
        ev = s.event()
        for st in (Sa, Sb):   # one warm-up per lane; Sa keeps lane 0 and Sb lane 1
            c.dev(s.ctx, rig.frames.ptrs, rig.d_out, st)
            s.hip.stream_sync(st)
        gate = s.gate(Sa)
        s.hip.fill_async(rig.outs[0], so.FILL, c.out_bytes, Sa)
        rig.frames.copy_from(rig.real, Sa)
        c.dev(s.ctx, rig.frames.ptrs, rig.outs[0], Sa)
        s.hip.copy_async(rig.keeps[0], rig.outs[0], c.out_bytes, Sa)
        rig.frames.zero(Sa)
        # S_b: the other lane, not held by anything
        c.dev(s.ctx, rig.real.ptrs, rig.outs[1], Sb)
        s.hip.copy_async(rig.keeps[1], rig.outs[1], c.out_bytes, Sb)
        s.hip.stream_sync(Sb)
        assert gate.holds()
        # S_c: no lane of its own and none free
        c.dev(s.ctx, rig.decoy.ptrs, rig.outs[2], Sc)
        s.hip.copy_async(rig.keeps[2], rig.outs[2], c.out_bytes, Sc)
        s.hip.event_record(ev, Sc)
        time.sleep(so.HEAD_START)
        assert s.hip.event_query(ev) == so.HIP_ERROR_NOT_READY, 'the third stream did not wait for the lane\'s pending call'
        gate.release()
        s.hip.stream_sync(Sa)
        s.hip.stream_sync(Sc)
        (a, b, d) = (rig.kept(0), rig.kept(1), rig.kept(2))
        assert b == ref_R, where(b, ref_R, ref_D)
        assert a == ref_R, where(a, ref_R, ref_D)
        assert d == ref_D, where(d, ref_D, ref_R)


def test_two_resident_calls_back_to_back_write_the_same_records(rt):
    """Frames-resident mode, one gated stream, two calls (one per lane) into the same d_out with a keep-copy behind each: the second
    call's dials kernel has to wait for the first call's join and keep-copy."""
    c = so.case('batch')
    with Session(rt) as s:
        S = s.stream()
        rig = s.rig(c, with_decoy=True, extra_out=1)
        (ref_R, ref_D) = so.references(s.ctx, c)
        s.ctx.set_frames_resident(True)
        warm_up(s, c, rig, S)
        gate = s.gate(S)
        s.hip.fill_async(rig.d_out, so.FILL, c.out_bytes, S)
        c.dev(s.ctx, rig.real.ptrs, rig.d_out, S)
        s.hip.copy_async(rig.keeps[0], rig.d_out, c.out_bytes, S)
        c.dev(s.ctx, rig.decoy.ptrs, rig.d_out, S)
        s.hip.copy_async(rig.keeps[1], rig.d_out, c.out_bytes, S)
        rig.real.zero(S)
        rig.decoy.zero(S)
        s.hip.fill_async(rig.d_out, so.FILL, c.out_bytes, S)
        gate.release()
        s.hip.stream_sync(S)
        (first, second) = (rig.kept(0), rig.kept(1))
        assert first == ref_R, where(first, ref_R, ref_D)
        assert second == ref_D, where(second, ref_D, ref_R)


def test_mode_switch_behind_one_gate(rt):
    """A frames-resident call, melf_ctx_set_frames_resident(0), then an ordered call on the same gated stream whose frames are
    produced behind the gate.  Both lanes belong to their own streams when the ordered call arrives, so it takes one over
    (claim_lane: from a lane's own stream to the caller's)."""
    c = so.case('batch')
    with Session(rt) as s:
        S = s.stream()
        rig = s.rig(c, with_decoy=True, extra_out=1)
        (ref_R, ref_D) = so.references(s.ctx, c)
        warm_up(s, c, rig, S)
        s.ctx.set_frames_resident(True)
        warm_up(s, c, rig, S, forget=False)   # one call per lane: each lane now belongs to its own stream
        rig.frames.set(c.real)    # `frames` hold R; the second call is to see D in them
        gate = s.gate(S)
        s.hip.fill_async(rig.d_out, so.FILL, c.out_bytes, S)
        c.dev(s.ctx, rig.real.ptrs, rig.d_out, S)
        s.hip.copy_async(rig.keeps[0], rig.d_out, c.out_bytes, S)
        s.ctx.set_frames_resident(False)
        rig.frames.copy_from(rig.decoy, S)
        c.dev(s.ctx, rig.frames.ptrs, rig.d_out, S)
        s.hip.copy_async(rig.keeps[1], rig.d_out, c.out_bytes, S)
        rig.frames.zero(S)
        rig.real.zero(S)
        s.hip.fill_async(rig.d_out, so.FILL, c.out_bytes, S)
        gate.release()
        s.hip.stream_sync(S)
        (first, second) = (rig.kept(0), rig.kept(1))
        assert first == ref_R, where(first, ref_R, ref_D)
        assert second == ref_D, where(second, ref_D, ref_R)


# ------------------------------------------------------------------------------------------- the harness can fail ---------
def test_selftest_call_on_another_stream_reads_the_decoys(rt):
    """(a) The producer copy is gated on S, the library call goes to S2: the kept records are the decoys'."""
    c = so.case('batch')
    with Session(rt) as s:
        (S, S2) = (s.stream(), s.stream())
        rig = s.rig(c)
        (ref_R, ref_D) = so.references(s.ctx, c)
        assert warm_up(s, c, rig, S2) == ref_D   # (and the context knows no stream: the call below is ordered behind nothing of S)
        gate = s.gate(S)
        rig.frames.copy_from(rig.real, S)
        c.dev(s.ctx, rig.frames.ptrs, rig.d_out, S2)
        s.hip.copy_async(rig.d_keep, rig.d_out, c.out_bytes, S2)
        s.hip.stream_sync(S2)
        gate.release()
        s.hip.stream_sync(S)
        got = rig.kept()
        assert got == ref_D, where(got, ref_D, ref_R)


def test_selftest_consumer_on_another_stream_keeps_the_fill(rt):
    """(b) The library call is behind the gate on S, the keep-copy goes to S2: the kept bytes are the fill."""
    c = so.case('batch')
    with Session(rt) as s:
        (S, S2) = (s.stream(), s.stream())
        rig = s.rig(c)
        warm_up(s, c, rig, S)
        s.hip.fill(rig.d_out, so.FILL, c.out_bytes)
        gate = s.gate(S)
        rig.frames.copy_from(rig.real, S)
        c.dev(s.ctx, rig.frames.ptrs, rig.d_out, S)
        s.hip.copy_async(rig.d_keep, rig.d_out, c.out_bytes, S2)
        s.hip.stream_sync(S2)
        gate.release()
        s.hip.stream_sync(S)
        assert rig.kept() == bytes([so.FILL]) * c.out_bytes


def test_selftest_a_gate_nobody_opens_expires(rt):
    """(c) A gate with a ceiling of 0.2 s that is never opened lets its stream go and says so."""
    hip = rt[1]
    S = hip.stream()
    try:
        gate = so.Gate(hip, S, ceiling=0.2)
        assert gate.holds()
        t0 = time.monotonic()
        hip.stream_sync(S)
        assert gate.expired and time.monotonic() - t0 < 5.0
        assert not gate.holds()
        with pytest.raises(AssertionError, match='ceiling'):
            gate.check()
    finally:
        hip.stream_sync(S)
        hip.stream_destroy(S)


# ------------------------------------------------------------------------------------------------------- through torch ---------
def test_stream_order_in_a_torch_process():
    """MeterReader's device path on a gated torch side stream (tests/stream_order_torch_child.py), in a child process that imports
    torch first (tests/frame_cases.py says why)."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'stream_order_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch stream order ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
