"""The torch checks of read_yuv16_frames, run by tests/test_yuv16_frames.py in a fresh process that imports torch before the package
loads the library (tests/frame_cases.py says why)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import pytest
    from tests import frame_cases as fc
    from tests import yuv16_cases as yc
    from meterelf_amd import _hip
    T = fc._Torch(64, 9)
    (torch, reader, dev, bgr) = (T.torch, T.reader, T.dev, T.bgr)
    rng = np.random.default_rng(1)
    W = bgr.shape[2]
    for fmt in ('p010', 'i010', 'p210', 'yuv422p12le'):
        step = yc.FORMATS[fmt][1]
        src8 = yc.planes_of(bgr, fmt, 3)
        want = reader.read_frames(yc.bgr_of(src8, fmt, 3))
        assert (want['status'] == _hip.FRAME_OK).sum() > 32

        def read(x, **kw):
            return reader.read_yuv16_frames(x, fmt, 'bt709', **kw)
        src16 = yc.widen_planes(src8, fmt, rng)
        for pad in ((0, 12) if step == 2 else (0,)):
            arr = yc.conventional16(*src16, fmt, pad, rng)
            whole = arr.base if pad else arr
            # torch.int16 holding the same bits, and torch.uint16 where the installed torch has it
            makers = [lambda a: torch.from_numpy(a.view(np.int16))]
            if hasattr(torch, 'uint16'):
                makers.append(torch.from_numpy)
            for make in makers:
                t = make(whole).to(dev)[:, :, :W]
                assert not _hip.yuv16_frames_view(t, fmt, 'bt709').copied
                T.three_ways(read, t, lambda: make(np.ascontiguousarray(arr)), want, (fmt, pad))
        # every other frame in place
        t = torch.from_numpy(yc.conventional16(*src16, fmt).view(np.int16)).to(dev)
        assert not _hip.yuv16_frames_view(t[::2], fmt, 3).copied
        assert read(t[::2]).tobytes() == want[::2].tobytes()
        if step == 1:
            # padded rows of a planar layout (its chroma rows are half rows): one packed copy, on the device, with out=
            wide = torch.zeros((t.shape[0], t.shape[1], W + 8), dtype=torch.int16, device=dev)
            wide[:, :, :W] = t
            assert _hip.yuv16_frames_view(wide[:, :, :W], fmt, 3).copied
            out = T.records(len(want))
            read(wide[:, :, :W], out=out)
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == want.tobytes()
            with pytest.raises(ValueError):
                read(t.cpu(), out=out)   # out= takes device frames only
        with pytest.raises(ValueError):
            reader.read_yuv16_frames(t.to(torch.uint8), fmt, 'bt709')
    tp = torch.from_numpy(yc.conventional16(*yc.widen_planes(yc.planes_of(bgr, 'p010', 3), 'p010', rng), 'p010').view(np.int16)).to(dev)
    T.two_streams(lambda i, o: reader.read_yuv16_frames(tp, 'p010', 'bt709', out=o), reader.read_frames(yc.bgr_of(yc.planes_of(bgr, 'p010', 3), 'p010', 3)))
    reader.ctx.sync()
    reader.close()
    print('torch yuv16 path ok')


if __name__ == '__main__':
    main()
