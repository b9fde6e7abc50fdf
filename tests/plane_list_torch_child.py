"""The torch checks of MeterReader.read_plane_list, run by tests/test_plane_list.py in a fresh process that imports torch before the
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
        """a torch tensor of the array's bits (int16 where torch has no unsigned type of that size), its strides kept"""
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        return torch.from_numpy(a)

    def planes_of(arr, layout, fmt):
        """One frame-tuple per frame: the batch method's array cut at its plane boundaries (numpy views)"""
        if layout == 'planar':
            return [tuple(arr[i, k] for k in range(3)) for i in range(n)]
        if layout == 'yuv':
            (sx, sy, semi) = (1, 1, fmt == 'nv12')
        elif layout == 'yuv_planar':
            (sx, sy, step, _vf) = _hip.YUV_PLANAR_FORMATS[fmt]
            semi = step == 2
        else:
            (sy, step, _vf, _shift) = _hip.YUV16_FORMATS[fmt]
            (sx, semi) = (1, step == 2)
        (rows, W) = arr.shape[1:]
        H = rows * (1 << sx) * (1 << sy) // ((1 << sx) * (1 << sy) + 2)
        (ch, cw) = (H >> sy, W >> sx)
        out = []
        for i in range(n):
            flat = arr[i].reshape(-1)
            y = flat[:H * W].reshape(H, W)
            if semi:
                out.append((y, flat[H * W:].reshape(ch, 2 * cw)))
            else:
                out.append((y, flat[H * W:H * W + ch * cw].reshape(ch, cw), flat[H * W + ch * cw:].reshape(ch, cw)))
        return out

    for (layout, fmt) in (('yuv', 'nv12'), ('yuv', 'yv12'), ('yuv_planar', 'nv61'), ('yuv16', 'p010'), ('planar', 'gbr')):
        (arr, _view, kw) = flc.make(src, layout, fmt, rng)
        arr = np.ascontiguousarray(arr)
        want = getattr(reader, flc.METHOD[layout])(arr, fmt, **kw)   # the batch method on the one array
        assert 4 * int((want['status'] == _hip.FRAME_OK).sum()) >= 3 * n, (layout, fmt)
        cuts = planes_of(arr, layout, fmt)

        def read(frames, **more):
            return reader.read_plane_list(frames, layout, fmt, **dict(kw, **more))
        # every plane a device tensor of its own
        ts = [tuple(to_torch(np.ascontiguousarray(p)).to(dev) for p in frame) for frame in cuts]
        assert read(ts).tobytes() == want.tobytes(), (layout, fmt, 'device planes')
        out = T.records(n)
        assert read(ts, out=out) is out
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), (layout, fmt, 'out=')
        # the list reversed
        assert read(ts[::-1]).tobytes() == want[::-1].tobytes(), (layout, fmt, 'reversed')
        # host planes: numpy views into the one array, torch CPU tensors of their own
        assert read(cuts).tobytes() == want.tobytes(), (layout, fmt, 'numpy planes')
        assert read([tuple(to_torch(np.ascontiguousarray(p)).clone() for p in frame) for frame in cuts]).tobytes() == want.tobytes(), (layout, fmt, 'cpu tensors')
        # the ValueErrors that need a device
        with pytest.raises(ValueError, match='frame 1, plane [01] of the list is in host memory'):   # (slot order: 'gbr' meets its B, plane 1, first)
            read([ts[0], tuple(to_torch(np.ascontiguousarray(p)) for p in cuts[1])])
        with pytest.raises(ValueError, match=r'frame 0, plane \d of the list is in (host|device) memory, frame 0, plane \d in'):   # (in slot order)
            read([(ts[0][0],) + tuple(to_torch(np.ascontiguousarray(p)) for p in cuts[0][1:])])
        with pytest.raises(ValueError, match='out must be'):
            read(ts, out=T.records(n - 1))
        if torch.cuda.device_count() > 1:
            with pytest.raises(ValueError, match=r'frame 1, plane \d of the list is on cuda:1'):
                read([ts[0], tuple(t.to(torch.device('cuda', 1)) for t in ts[1])])
    reader.ctx.sync()
    reader.close()
    print('torch plane list path ok')


if __name__ == '__main__':
    main()
