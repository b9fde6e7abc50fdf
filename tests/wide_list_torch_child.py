"""The torch checks of MeterReader.read_wide_frame_list / read_wide_plane_list, run by tests/test_wide_list.py in a fresh process that
imports torch before the package loads the library (tests/frame_cases.py says why): lists of separately allocated device tensors, a
x[:, y0:, x0:] view per frame, planes as separate tensors, host lists, out= a device tensor without synchronisation, two caller
streams with frames-resident mode off and on, and frames written on the stream just before the call."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import pytest
    from tests import frame_cases as fc
    from meterelf_amd import _hip
    n = 12
    T = fc._Torch(n, 41)
    (torch, reader, dev) = (T.torch, T.reader, T.dev)
    (H, W) = T.bgr.shape[1:3]
    rgb8 = np.ascontiguousarray(T.bgr[..., ::-1])
    chw = torch.from_numpy(rgb8).to(dev).permute(0, 3, 1, 2).contiguous().float() / 255.0   # (N, 3, H, W) in [0, 1], R G B
    (sa, sb) = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    rev = list(range(n))[::-1]

    for (dtype, kw) in ((torch.float16, {}), (torch.bfloat16, dict(scale=255.999, rounding='floor')), (torch.float32, dict(scale=(255.0, 254.5, 255.5)))):
        batch = chw.to(dtype).contiguous()
        want = reader.read_wide_frames(batch, 'chw', 'rgb', **kw)   # the batch method on the stacked tensor
        if dtype != torch.bfloat16:
            assert 4 * int((want['status'] == _hip.FRAME_OK).sum()) >= 3 * n, (dtype, want['status'])
        tag = (str(dtype),)

        def read(frames, layout='chw', **more):
            return reader.read_wide_frame_list(frames, layout, 'rgb', **dict(kw, **more))

        def read_planes(frames, order='rgb', **more):
            pkw = dict(kw, **more)
            if order != 'rgb' and np.ndim(pkw.get('scale', 0.0)):
                pkw['scale'] = tuple(pkw['scale']['rgb'.index(c)] for c in order)
            return reader.read_wide_plane_list(frames, order, **pkw)
        # separately allocated device tensors
        ts = [batch[i].clone() for i in range(n)]
        assert len({b.data_ptr() - a.data_ptr() for (a, b) in zip(ts, ts[1:])}) > 0
        assert read(ts).tobytes() == want.tobytes(), tag + ('device list',)
        assert read([ts[i] for i in rev]).tobytes() == want[rev].tobytes(), tag + ('reversed',)
        # views into the batch itself
        assert read([batch[i] for i in range(n)]).tobytes() == want.tobytes(), tag + ('views of one tensor',)
        # a spatial crop x[:, y0:, x0:] of a larger tensor per frame: a base and pitch with the sample's own alignment only
        bigs = [torch.full((3, H + 5, W + 7), float('nan'), dtype=dtype, device=dev) for _ in range(n)]
        crops = [b[:, 3:, 5:][:, :H, :W] for b in bigs]
        for (c, t) in zip(crops, ts):
            c.copy_(t)
        assert crops[0].data_ptr() == bigs[0].data_ptr() + (3 * (W + 7) + 5) * batch.element_size()
        assert read(crops).tobytes() == want.tobytes(), tag + ('crop per frame',)
        # channels last, one tensor per frame
        hwc = [t.permute(1, 2, 0).contiguous() for t in ts]
        assert read(hwc, 'hwc').tobytes() == want.tobytes(), tag + ('hwc list',)
        # planes as separate tensors, in r g b and in g b r order; the planes of a crop
        planes = [tuple(t[k].clone() for k in range(3)) for t in ts]
        assert read_planes(planes).tobytes() == want.tobytes(), tag + ('plane list',)
        assert read_planes([(p[1], p[2], p[0]) for p in planes], 'gbr').tobytes() == want.tobytes(), tag + ('gbr plane list',)
        assert read_planes([tuple(c[k] for k in range(3)) for c in crops]).tobytes() == want.tobytes(), tag + ('planes of crops',)
        # host lists: torch CPU tensors and, where numpy has the type, numpy arrays
        assert read([t.cpu() for t in ts]).tobytes() == want.tobytes(), tag + ('cpu tensors',)
        assert read_planes([tuple(p.cpu() for p in fr) for fr in planes]).tobytes() == want.tobytes(), tag + ('cpu planes',)
        if dtype != torch.bfloat16:
            assert read([t.cpu().numpy() for t in ts]).tobytes() == want.tobytes(), tag + ('numpy list',)

        # two caller streams, frames-resident mode off and on, out= device tensors, nothing synchronised in between; the last call's
        # frames are written on its stream just before it
        for resident in (False, True):
            reader.ctx.set_frames_resident(resident)
            torch.cuda.synchronize()
            outs = [T.records(n) for _ in range(5)]
            with torch.cuda.stream(sa):
                assert read(ts, out=outs[0]) is outs[0]
            with torch.cuda.stream(sb):
                assert read_planes([planes[i] for i in rev], out=outs[1]) is outs[1]
            with torch.cuda.stream(sa):
                read([crops[i] for i in rev], out=outs[2])
            with torch.cuda.stream(sb):
                read(hwc, 'hwc', out=outs[3])
                late = [torch.zeros_like(t) for t in ts]
                for (dst, t) in zip(late, ts):
                    dst.copy_(t, non_blocking=True)
                read(late, out=outs[4])
            torch.cuda.synchronize()
            for (k, order) in enumerate((None, rev, rev, None, None)):
                w = want if order is None else want[order]
                assert outs[k].cpu().numpy().tobytes() == w.tobytes(), tag + ('resident' if resident else 'not resident', 'call %d' % k)
        reader.ctx.set_frames_resident(False)
        with pytest.raises(ValueError, match='out must be'):
            read(ts, out=T.records(n - 1))
        with pytest.raises(ValueError, match='frame 1 of the list is in host memory'):
            read([ts[0], ts[1].cpu()])
        with pytest.raises(ValueError, match='frame 1, plane 2 of the list is in host memory'):
            read_planes([planes[0], (planes[1][0], planes[1][1], planes[1][2].cpu())])
        with pytest.raises(ValueError, match='frame 2 of the list: the strides'):
            read([ts[0], ts[1], ts[2][:, :, ::2]])
        del bigs, crops, hwc, planes, ts

    # 16-bit words: torch.int16 holding the bits (torch.uint16 where the installed torch has it), packed and as gbr planes
    words = (rgb8.astype(np.uint16) << np.uint16(8)) | np.random.default_rng(2).integers(0, 256, size=rgb8.shape, dtype=np.uint16)
    want = reader.read_frame_views(rgb8, 'rgb')
    assert reader.read_wide_frame_list([words[i] for i in range(n)], 'hwc', 'rgb', shift=8).tobytes() == want.tobytes()
    ti = [torch.from_numpy(words[i].view(np.int16)).to(dev) for i in range(n)]
    assert reader.read_wide_frame_list(ti, 'hwc', 'rgb', shift=8).tobytes() == want.tobytes()
    if hasattr(torch, 'uint16'):
        assert reader.read_wide_frame_list([t.view(torch.uint16) for t in ti], 'hwc', 'rgb', shift=8).tobytes() == want.tobytes()
    gbr = [tuple(torch.from_numpy(np.ascontiguousarray(words[i][..., k]).view(np.int16)).to(dev) for k in (1, 2, 0)) for i in range(n)]
    assert reader.read_wide_plane_list(gbr, 'gbr', shift=8).tobytes() == want.tobytes()
    assert reader.read_wide_plane_list([tuple(np.ascontiguousarray(words[i][..., k]) for k in (1, 2, 0)) for i in range(n)], 'gbr',
                                       shift=8).tobytes() == want.tobytes()
    with pytest.raises(ValueError, match='integer frames need shift'):
        reader.read_wide_frame_list(ti, 'hwc', 'rgb')
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match='differs from frame 0 in device'):
            reader.read_wide_frame_list([ti[0], ti[1].to(torch.device('cuda', 1))], 'hwc', 'rgb', shift=8)
    reader.ctx.sync()
    reader.close()
    print('torch wide list path ok')


if __name__ == '__main__':
    main()
