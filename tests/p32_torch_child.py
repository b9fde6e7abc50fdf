"""The torch checks of read_packed32_frames, run by tests/test_packed32_frames.py in a fresh process that imports torch before the
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
    from tests import p32_cases as pc
    from meterelf_amd import _hip
    T = fc._Torch(64, 9)
    (torch, reader, dev, bgr) = (T.torch, T.reader, T.dev, T.bgr)
    rng = np.random.default_rng(1)
    W = bgr.shape[2]
    for fmt in ('y410', 'vuya', 'x2rgb10'):
        kind = pc.kind_of(fmt)
        src = pc.F32[kind].from_bgr(bgr)
        want = pc.want_8bit(reader, src, kind)
        assert (want['status'] == _hip.FRAME_OK).sum() > 32
        matrix = pc.matrix_of(fmt, 'bt709')

        def read(x, **kw):
            return reader.read_packed32_frames(x, fmt, matrix, **kw)
        for pad in (0, 3):
            arr = pc.conventional32(*src, fmt, pad, rng)
            # torch.int32 holding the same bits: a device tensor read in place, rows `pad` words longer than W
            t = torch.from_numpy(arr.base.view(np.int32)).to(dev)[:, :, :W]
            assert not _hip.packed32_frames_view(t, fmt, matrix).copied
            assert (t.stride(1) == W + pad) and t.dtype == torch.int32
            T.three_ways(read, t, lambda: torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)), want, (fmt, pad))
        # strided views in place: every other frame, and every other frame of rows cut short by a word (odd W); out= under a
        # non-default current stream
        assert not _hip.packed32_frames_view(t[::2], fmt, matrix).copied
        assert read(t[::2]).tobytes() == want[::2].tobytes()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            out = T.records(len(want))
            assert read(t, out=out) is out
        side.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), (fmt, 'side stream')
        # a layout the descriptor cannot express (a pixel stride of two words): one packed copy, on the device
        odd = torch.zeros((t.shape[0], t.shape[1], 2 * W), dtype=torch.int32, device=dev)[:, :, ::2]
        odd[...] = t
        assert _hip.packed32_frames_view(odd, fmt, matrix).copied
        out = T.records(len(want))
        read(odd, out=out)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), (fmt, 'copied')
        with pytest.raises(ValueError):
            read(t.cpu(), out=out)   # out= takes device frames only
        with pytest.raises(ValueError):
            read(t.to(torch.int64))
        if fmt == 'vuya':            # the byte form on the device: (N, H, W, 4) uint8, the word's bytes in memory order
            t8 = t.contiguous().view(torch.uint8).view(t.shape[0], t.shape[1], W, 4)
            assert not _hip.packed32_frames_view(t8, fmt, matrix).copied
            assert read(t8).tobytes() == want.tobytes(), (fmt, 'bytes')
    src = pc.F32['yuv'].from_bgr(bgr)
    want = pc.want_8bit(reader, src, 'yuv')
    tv = torch.from_numpy(np.ascontiguousarray(pc.conventional32(*src, 'y410', 0, rng)).view(np.int32)).to(dev)
    T.two_streams(lambda i, o: reader.read_packed32_frames(tv, 'y410', 'bt709', out=o), want)
    reader.ctx.sync()
    reader.close()
    print('torch packed32 path ok')


if __name__ == '__main__':
    main()
