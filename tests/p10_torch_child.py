"""The torch checks of read_yuv422_10_frames, run by tests/test_yuv422_10_frames.py in a fresh process that imports torch before the
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
    from tests import p10_cases as pc
    from meterelf_amd import _hip
    T = fc._Torch(64, 9)
    (torch, reader, dev, bgr) = (T.torch, T.reader, T.dev, T.bgr)
    rng = np.random.default_rng(1)
    W = bgr.shape[2]
    src8 = fc.bgr_to_yuv(bgr, 1, 0, pc.MATRIX)
    want = pc.want_8bit(reader, src8)
    assert (want['status'] == _hip.FRAME_OK).sum() > 32
    for fmt in pc.FORMATS:
        signed = np.int32 if fmt == 'v210' else np.int16
        width = W if fmt == 'v210' else None

        def read(x, **kw):
            return reader.read_yuv422_10_frames(x, fmt, 'bt709', width=width, **kw)
        for pad in (0, 2):
            arr = np.asarray(pc.conventional10(*src8, fmt, pad, rng))
            whole = arr.base if fmt == 'y210' else arr   # (y210: the [:, :, :W] view of rows `pad` macropixels longer)
            # torch.int32 / torch.int16 holding the same bits: a device tensor read in place
            t = torch.from_numpy(whole.view(signed)).to(dev)
            if fmt == 'y210':
                t = t[:, :, :W]
            assert not _hip.yuv422_10_frames_view(t, fmt, 'bt709', width=width).copied
            T.three_ways(read, t, lambda: torch.from_numpy(np.ascontiguousarray(arr).view(signed)), want, (fmt, pad))
        # every other frame in place; out= under a non-default current stream
        assert not _hip.yuv422_10_frames_view(t[::2], fmt, 3, width=width).copied
        assert read(t[::2]).tobytes() == want[::2].tobytes()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            out = T.records(len(want))
            assert read(t, out=out) is out
        side.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), (fmt, 'side stream')
        # a layout the descriptor cannot express: one packed copy, on the device
        if fmt == 'v210':
            odd = torch.zeros((t.shape[0], t.shape[1], pc.v210_row_bytes(W) // 4 + 2), dtype=torch.int32, device=dev)
            odd[:, :, :pc.v210_row_bytes(W) // 4] = t[:, :, :pc.v210_row_bytes(W) // 4]
        else:
            odd = torch.zeros((t.shape[0], t.shape[1], W + 1, 2), dtype=torch.int16, device=dev)[:, :, :W]
            odd[...] = t
        assert _hip.yuv422_10_frames_view(odd, fmt, 3, width=width).copied
        out = T.records(len(want))
        read(odd, out=out)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), (fmt, 'copied')
        with pytest.raises(ValueError):
            read(t.cpu(), out=out)   # out= takes device frames only
        with pytest.raises(ValueError):
            read(t.to(torch.uint8))
    tv = torch.from_numpy(np.asarray(pc.conventional10(*src8, 'v210', 0, rng)).view(np.int32)).to(dev)
    T.two_streams(lambda i, o: reader.read_yuv422_10_frames(tv, 'v210', 'bt709', width=W, out=o), want)
    reader.ctx.sync()
    reader.close()
    print('torch yuv422_10 path ok')


if __name__ == '__main__':
    main()
