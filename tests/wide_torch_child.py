"""The torch checks of MeterReader.read_wide_frames, run by tests/test_wide_frames.py in a fresh process that imports torch before the
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
    from tests import wide_cases as wc
    from meterelf_amd import _hip
    n = 12
    T = fc._Torch(n, 31)
    (torch, reader, dev) = (T.torch, T.reader, T.dev)
    (H, W) = T.bgr.shape[1:3]
    rgb8 = np.ascontiguousarray(T.bgr[..., ::-1])
    chw = torch.from_numpy(rgb8).to(dev).permute(0, 3, 1, 2).contiguous().float() / 255.0   # (N, 3, H, W) in [0, 1], R G B
    side = torch.cuda.Stream(dev)
    # an ImageNet Normalize on top, undone by scale = std * 255, offset = mean * 255
    (mean, std) = (np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32))
    normed = (chw - torch.from_numpy(mean).to(dev)[None, :, None, None]) / torch.from_numpy(std).to(dev)[None, :, None, None]

    for (dtype, type_) in ((torch.float16, wc.F16), (torch.bfloat16, wc.BF16), (torch.float32, wc.F32)):
        for (src, kw) in ((chw, {}), (normed, dict(scale=std * 255.0, offset=mean * 255.0)), (chw, dict(scale=255.999, rounding='floor'))):
            t = src.to(dtype).contiguous()
            # the host path on the same samples, and (anchor) the 8-bit planar path on the numpy-narrowed frames
            want = reader.read_wide_frames(t.cpu(), 'chw', 'rgb', **kw)
            x32 = t.float().cpu().numpy()
            sc = np.asarray(kw.get('scale', 255.0), np.float32).reshape(-1, 1, 1)
            of = np.asarray(kw.get('offset', 0.0), np.float32).reshape(-1, 1, 1)
            narrowed = wc.narrow_float(x32, sc, of, kw.get('rounding', 'nearest'))
            assert want.tobytes() == reader.read_planar_frames(narrowed, 'rgb').tobytes(), (dtype, kw)
            if type_ != wc.BF16 and 'rounding' not in kw:
                assert 4 * int((want['status'] == _hip.FRAME_OK).sum()) >= 3 * n, (dtype, want['status'])

            def read(frames, layout, order='rgb', **more):
                return reader.read_wide_frames(frames, layout, order, **dict(kw, **more))
            tag = (str(dtype), sorted(kw))
            # (N, 3, H, W) on the device; on a non-default current stream with out= a device tensor
            assert read(t, 'chw').tobytes() == want.tobytes(), tag
            with torch.cuda.stream(side):
                out = T.records(n)
                assert read(t, 'chw', out=out) is out
            side.synchronize()
            assert out.cpu().numpy().tobytes() == want.tobytes(), tag + ('out=',)
            # (N, H, W, 3)
            hwc = t.permute(0, 2, 3, 1).contiguous()
            assert read(hwc, 'hwc').tobytes() == want.tobytes(), tag + ('hwc',)
            assert read(hwc.cpu(), 'hwc').tobytes() == want.tobytes(), tag + ('hwc host',)
            # a channel slice of 4 channels, both layouts, in place
            c4 = torch.full((n, 4, H, W), float('nan'), dtype=dtype, device=dev)
            c4[:, :3] = t
            v = _hip.wide_frames_view(c4[:, :3], 'chw', 'rgb')
            assert v.ptr == c4.data_ptr() and v.frame_stride == 4 * H * W * t.element_size() and v.on_device
            assert read(c4[:, :3], 'chw').tobytes() == want.tobytes(), tag + ('4 planes',)
            assert read(c4, 'chw', 'rgba').tobytes() == want.tobytes(), tag + ('rgba planes',)
            h4 = c4.permute(0, 2, 3, 1).contiguous()
            v = _hip.wide_frames_view(h4[..., :3], 'hwc', 'rgb')
            assert v.ptr == h4.data_ptr() and v.pixel_format == _hip.PIX_RGBA
            with torch.cuda.stream(side):
                out = T.records(n)
                read(h4[..., :3], 'hwc', out=out)
            side.synchronize()
            assert out.cpu().numpy().tobytes() == want.tobytes(), tag + ('4 samples',)
            # a spatial crop of larger frames: a base and pitch with the sample's own alignment only
            big = torch.full((n, 3, H + 5, W + 7), float('nan'), dtype=dtype, device=dev)
            crop = big[:, :, 3:3 + H, 5:5 + W]
            crop.copy_(t)
            v = _hip.wide_frames_view(crop, 'chw', 'rgb')
            assert v.ptr == big.data_ptr() + (3 * (W + 7) + 5) * t.element_size() and v.row_pitch == (W + 7) * t.element_size()
            assert read(crop, 'chw').tobytes() == want.tobytes(), tag + ('crop',)
            bigh = torch.full((n, H + 2, W + 3, 3), float('nan'), dtype=dtype, device=dev)
            croph = bigh[:, 1:1 + H, 3:3 + W]
            croph.copy_(hwc)
            assert read(croph, 'hwc').tobytes() == want.tobytes(), tag + ('hwc crop',)
            # strides that do not fit: ValueError before the library is called
            for (bad, layout) in ((t.permute(0, 2, 3, 1), 'hwc'), (hwc.permute(0, 3, 1, 2), 'chw'), (t[:, :, :, ::2], 'chw'), (t[:, :, ::2][:, :, :, 1::3], 'chw')):
                with pytest.raises(ValueError, match='do not fit melf_wide_frames'):
                    read(bad, layout)
            del c4, h4, big, bigh
        with pytest.raises(ValueError, match='out must be'):
            reader.read_wide_frames(t, 'chw', out=T.records(n - 1))
        with pytest.raises(ValueError, match='out= takes the records of device frames only'):
            reader.read_wide_frames(t.cpu(), 'chw', out=T.records(n))
        with pytest.raises(ValueError, match='float frames take no shift'):
            reader.read_wide_frames(t, 'chw', shift=8)

    # 16-bit words: torch.int16 holding the bits (torch.uint16 where the installed torch has it)
    words = (rgb8.astype(np.uint16) << np.uint16(8)) | np.random.default_rng(2).integers(0, 256, size=rgb8.shape, dtype=np.uint16)
    want = reader.read_frame_views(rgb8, 'rgb')
    assert reader.read_wide_frames(words, 'hwc', 'rgb', shift=8).tobytes() == want.tobytes()
    ti = torch.from_numpy(words.view(np.int16)).to(dev)
    assert reader.read_wide_frames(ti, 'hwc', 'rgb', shift=8).tobytes() == want.tobytes()
    if hasattr(torch, 'uint16'):
        assert reader.read_wide_frames(ti.view(torch.uint16), 'hwc', 'rgb', shift=8).tobytes() == want.tobytes()
    with pytest.raises(ValueError, match='integer frames need shift'):
        reader.read_wide_frames(ti, 'hwc', 'rgb')
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match='frames are on cuda:1'):
            reader.read_wide_frames(ti.to(torch.device('cuda', 1)), 'hwc', 'rgb', shift=8)
    reader.ctx.sync()
    reader.close()
    print('torch wide path ok')


if __name__ == '__main__':
    main()
