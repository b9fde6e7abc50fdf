"""The torch checks of MeterReader.read_frame_list, run by tests/test_frame_list.py in a fresh process that imports torch before the
package loads the library (tests/frame_cases.py says why)."""
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
    from meterelf_amd import _hip
    n = 33
    T = fc._Torch(n, 21)
    (torch, reader, dev) = (T.torch, T.reader, T.dev)
    src = flc.Source(T.bgr)
    rng = np.random.default_rng(1)

    def to_torch(a):
        """a torch tensor of the array's bits (int16 / int32 where torch has no unsigned type of that size)"""
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view({np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)))

    for (layout, fmt) in flc.ONE_PER_FAMILY:
        (arr, _view, kw) = flc.make(src, layout, fmt, rng)
        want = getattr(reader, flc.METHOD[layout])(arr, fmt, **kw)   # the batch method on the one array
        assert 4 * int((want['status'] == _hip.FRAME_OK).sum()) >= 3 * n, (layout, fmt)

        def read(frames, **more):
            return reader.read_frame_list(frames, layout, fmt, **dict(kw, **more))
        # separately allocated device tensors
        ts = [to_torch(arr[i]).to(dev) for i in range(n)]
        assert len({b.data_ptr() - a.data_ptr() for (a, b) in zip(ts, ts[1:])}) > 0
        assert read(ts).tobytes() == want.tobytes(), (layout, fmt, 'device list')
        out = T.records(n)
        assert read(ts, out=out) is out
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), (layout, fmt, 'out=')
        # views into one big tensor, in reverse order
        big = to_torch(arr).to(dev)
        assert read([big[i] for i in reversed(range(n))]).tobytes() == want[::-1].tobytes(), (layout, fmt, 'views reversed')
        # host lists: numpy arrays, torch CPU tensors
        assert read([np.array(arr[i]) for i in range(n)]).tobytes() == want.tobytes(), (layout, fmt, 'numpy list')
        assert read([to_torch(arr[i]).clone() for i in range(n)]).tobytes() == want.tobytes(), (layout, fmt, 'cpu tensor list')
        # the ValueErrors
        with pytest.raises(ValueError, match='frame 1 of the list is in host memory'):
            read([ts[0], to_torch(arr[1])])
        with pytest.raises(ValueError):   # an element of another shape (the view function's own message, or "differs from frame 0")
            read([ts[0], ts[1], ts[2][:-2]] if layout != 'planar' else [ts[0], ts[1], ts[2][:, :-2]])
        with pytest.raises(ValueError, match='out= takes the records of device frames only'):
            read([np.array(arr[i]) for i in range(n)], out=out)
        with pytest.raises(ValueError, match='out must be'):
            read(ts, out=T.records(n - 1))
        if torch.cuda.device_count() > 1:
            with pytest.raises(ValueError, match='differs from frame 0 in device'):
                read([ts[0], ts[1].to(torch.device('cuda', 1))])
        assert len(read([])) == 0
    # an element the view function would have to copy: BGR pixels six bytes apart
    (arr, _view, kw) = flc.make(src, 'views', 'bgr', rng)
    (H, W) = arr.shape[1:3]
    wide = torch.zeros((H, 2 * W, 3), dtype=torch.uint8, device=dev)[:, ::2]
    with pytest.raises(ValueError, match='frame 1 of the list has a layout'):
        reader.read_frame_list([torch.from_numpy(arr[0]).to(dev), wide], 'views', 'bgr')
    with pytest.raises(ValueError, match='frame 2 of the list differs from frame 0 in H: %d, not %d' % (H - 2, H)):
        reader.read_frame_list([arr[0], arr[1], arr[2][:-2]], 'views', 'bgr')
    with pytest.raises(ValueError, match='layout'):
        reader.read_frame_list([arr[0]], 'bayer', 'bgr')
    with pytest.raises(ValueError, match='takes no matrix'):
        reader.read_frame_list([arr[0]], 'views', 'bgr', matrix='bt709')
    reader.ctx.sync()
    reader.close()
    print('torch frame list path ok')


if __name__ == '__main__':
    main()
