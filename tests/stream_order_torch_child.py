"""The stream order of MeterReader's device path under torch, run by tests/test_stream_order.py in a fresh process that imports torch
before the package loads the library (tests/frame_cases.py says why).  _engine.MeterReader._read_view enqueues on
torch.cuda.current_stream; here that is a side stream held by the gate of tests/stream_order.py (launched on side.cuda_stream), with
the producer of the frames, the read into out= and the consumer of the records enqueued behind it:

    gate | dec <- real | read(dec, out=out) | keep = out.clone() | dec.zero_() | release | side.synchronize()

and keep must hold the records of the real frames.  Three reads: read_frame_views of a tensor read in place, read_frame_list whose
twelve elements are filled behind the gate, and read_frame_views of a channels-first tensor's permuted view, which frames_view copies
to a packed tensor (`copied`) that _read_view protects with record_stream -- the test drops its references to the source before it
opens the gate.  Each sequence runs once without a gate first: the warm-up the gate's rules ask for (no allocation or buffer growth
behind a closed gate), and the check that the sequence itself is right."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from meterelf_amd import MeterReader, _hip, _params
    from tests import stream_order as so
    from tests.test_gpu_parity import GOLDEN

    reader = MeterReader(_params.load(os.path.join(GOLDEN, 'sample-images1', 'params.yml')), device=0)
    dev = torch.device('cuda', 0)
    hip = so.Hip()
    side = torch.cuda.Stream(dev)
    (R, D) = (np.ascontiguousarray(x[..., ::-1]) for x in so.scene())   # RGB
    refs = []
    for x in so.scene():
        recs = reader.read_frames(x)
        assert (recs['status'] == _hip.FRAME_OK).all()
        refs.append(recs)
    (ref_R, ref_D) = refs
    assert all(ref_R[i].tobytes() != ref_D[i].tobytes() for i in range(so.N))

    def records(n):
        return torch.zeros((n, so.RSZ), dtype=torch.uint8, device=dev)

    def sequence(make, produce, read, consume, want, gate_it, tag):
        """make() -> the decoy tensors; produce(dec): dec <- real; read(dec, out); consume(dec): dec <- 0 and the references go"""
        dec = make()
        out = records(len(want))
        torch.cuda.synchronize()
        gate = None
        try:
            with torch.cuda.stream(side):
                if gate_it:
                    gate = so.Gate(hip, side.cuda_stream)
                produce(dec)
                read(dec, out)
                keep = out.clone()
                consume(dec)
                del dec
                out.fill_(so.FILL)
            if gate_it:
                gate.release()
        finally:
            if gate_it and gate is not None:
                gate.open()
            side.synchronize()
        if gate_it:
            gate.check()
        got = keep.cpu().numpy().tobytes()
        assert got == want.tobytes(), (tag, 'gated' if gate_it else 'ungated', 'decoy records: %s' % (got == ref_D[:len(want)].tobytes()))
        torch.cuda.synchronize()

    # 1. read_frame_views, in place
    real = torch.from_numpy(R).to(dev)
    decoy = torch.from_numpy(D).to(dev)
    assert not _hip.frames_view(decoy, 'rgb').copied
    for gate_it in (False, True):
        sequence(lambda: [decoy.clone()], lambda d: d[0].copy_(real, non_blocking=True),
                 lambda d, out: reader.read_frame_views(d[0], 'rgb', out=out), lambda d: d[0].zero_(), ref_R, gate_it, 'views')

    # 2. read_frame_list: the elements are filled behind the gate
    # (the elements are frames 0, 3, 6 .. of one tensor three times as long, so that one copy_ fills them and one zero_ clears them)
    n = so.N_LIST

    def make_list():
        pool = torch.zeros((3 * n,) + tuple(decoy.shape[1:]), dtype=torch.uint8, device=dev)
        pool[::3].copy_(decoy[:n])
        return [pool] + [pool[3 * i] for i in range(n)]
    for gate_it in (False, True):
        sequence(make_list, lambda d: d[0][::3].copy_(real[:n], non_blocking=True),
                 lambda d, out: reader.read_frame_list(d[1:], 'views', 'rgb', out=out), lambda d: d[0].zero_(), ref_R[:n], gate_it, 'list')

    # 3. a layout frames_view has to copy: the permuted view of channels-first frames
    real_cf = real.permute(0, 3, 1, 2).contiguous()
    decoy_cf = decoy.permute(0, 3, 1, 2).contiguous()
    assert _hip.frames_view(decoy_cf.permute(0, 2, 3, 1), 'rgb').copied
    for gate_it in (False, True):
        sequence(lambda: [decoy_cf.clone()], lambda d: d[0].copy_(real_cf, non_blocking=True),
                 lambda d, out: reader.read_frame_views(d[0].permute(0, 2, 3, 1), 'rgb', out=out), lambda d: d[0].zero_(), ref_R, gate_it, 'copied')

    reader.ctx.sync()
    reader.close()
    print('torch stream order ok')


if __name__ == '__main__':
    main()
