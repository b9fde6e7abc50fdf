"""The torch checks of MeterReader.read_oriented_frames, run by tests/test_oriented.py in a fresh process that imports torch before
the package loads the library (tests/frame_cases.py says why)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import pytest
    from tests import frame_cases as fc
    from tests import frame_list_cases as flc
    from tests import oriented_cases as oc
    from meterelf_amd import _hip
    n = 33
    T = fc._Torch(n, 21)
    (torch, reader, dev) = (T.torch, T.reader, T.dev)
    # a CUDA tensor batch stored on its side: what the issue's caller holds
    upright = torch.from_numpy(T.bgr).to(dev)
    want = reader.read_frame_views(upright)
    assert 4 * int((want['status'] == _hip.FRAME_OK).sum()) >= 3 * n
    stored = torch.rot90(upright, 1, (1, 2)).contiguous()   # rot90ccw: shown upright by rot90cw
    assert reader.read_frame_views(torch.rot90(stored, -1, (1, 2)).contiguous()).tobytes() == want.tobytes()
    T.three_ways(lambda f, out=None: reader.read_oriented_frames(f, 'views', 'bgr', 'rot90cw', out=out), stored, lambda: stored.cpu(), want, 'bgr rot90cw')
    assert reader.read_oriented_frames(stored, 'views', 'bgr', 6).tobytes() == want.tobytes()
    assert reader.read_oriented_frames(upright.flip(1, 2).contiguous(), 'views', 'bgr', 'rot180').tobytes() == want.tobytes()
    assert reader.read_oriented_frames(upright, 'views', 'bgr', 'normal').tobytes() == want.tobytes()
    # a view with padded rows is read in place
    wide = torch.zeros((n, stored.shape[1], stored.shape[2] + 5, 3), dtype=torch.uint8, device=dev)
    wide[:, :, :stored.shape[2]] = stored
    assert reader.read_oriented_frames(wide[:, :, :stored.shape[2]], 'views', 'bgr', 'rot90cw').tobytes() == want.tobytes()
    # the other families, one format each, device and host, from the stored batch oriented_cases makes
    src = flc.Source(T.bgr)
    rng = np.random.default_rng(1)
    bits = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
    for (layout, fmt) in flc.ONE_PER_FAMILY:
        if layout not in oc.FAMILIES:
            continue
        (arr, view, kw) = flc.make(src, layout, fmt, rng)
        kw = {k: v for (k, v) in kw.items() if k == 'matrix'}
        want = getattr(reader, flc.METHOD[layout])(arr, fmt, **kw)
        v = view(arr)
        (d, buf) = oc.stored_batch(layout, flc.descriptor(v), oc.as_buffer(v), 8)
        # the stored batch in the shape the layout's batch method documents: the upright array's with H and W exchanged
        (H, W) = (d.H, d.W)
        shape = {'views': lambda: (n, H, W, arr.shape[3]), 'planar': lambda: (n, arr.shape[1], H, W),
                 'packed32': lambda: (n, H, W) + arr.shape[3:]}.get(layout, lambda: (n, arr.shape[1] * arr.shape[2] // W, W))()
        st = np.ascontiguousarray(buf[:n * d.frame_stride].view(arr.dtype).reshape(shape)) if layout != 'planar' else None
        if st is None:   # (N, C, H, W): the three planes the descriptor names, in the array's channel order
            st = oc.orient(arr, oc.inverse(8), axes=(2, 3)).copy()
        t = torch.from_numpy(st.view(bits.get(st.dtype, st.dtype))).to(dev)
        assert reader.read_oriented_frames(t, layout, fmt, 'rot90ccw', **kw).tobytes() == want.tobytes(), (layout, fmt, 'device')
        assert reader.read_oriented_frames(st, layout, fmt, 8, **kw).tobytes() == want.tobytes(), (layout, fmt, 'host')
    with pytest.raises(ValueError, match='out must be'):
        reader.read_oriented_frames(stored, 'views', 'bgr', 6, out=T.records(n - 1))
    with pytest.raises(ValueError, match='orientation'):
        reader.read_oriented_frames(stored, 'views', 'bgr', 'sideways')
    reader.ctx.sync()
    reader.close()
    print('torch oriented path ok')


if __name__ == '__main__':
    main()
