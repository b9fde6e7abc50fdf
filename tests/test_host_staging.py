"""The host-pointer entry points' staging pipeline past its second chunk (melf_process_batch, melf_process_frames,
melf_process_yuv, melf_process_yuv422, melf_process_planes).

Host frames are packed in chunks of 128 into one of two pinned staging buffers; from the third chunk on the host waits for the
copy that last read a buffer before it packs into it again.  The per-format files stop at 131 frames (two chunks), so here one
layout of each family -- BGR, BGRA, NV12, I420, YUYV, planar RGB -- is read as 257 frames: three chunks, the third packed into
staging buffer 0 again, and a last chunk of one frame.

No oracle: the per-format files tie the device path to it.  Asserted, record for record and exactly: the host entry point's 257
records equal the *_dev entry point's for the same bytes uploaded once, and records 0 .. 127 equal those of a separate 128-frame
host call.  Frames of 410 x 300, the smallest the default meter_rect (50, 160)-(300, 410) fits; frame i is one of 32 distinct
frames, chosen so that the frames at one staging slot differ from chunk to chunk.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests.frame_cases import env  # noqa: E402,F401  (the module-scoped readers + fixture frames)

N, CHUNK, H, W, NVAR = 257, 128, 410, 300, 32
CASES = ('bgr', 'bgra', 'nv12', 'i420', 'yuyv', 'planar')


@pytest.fixture(scope='module')
def staged(env):  # noqa: F811
    """32 distinct 410 x 300 BGR frames off the sample-images1 fixtures (shifted by even amounts; one constant: Dials not found)
    and which of them frame i of the 257 is; computed once, never written to."""
    e = env['sample-images1']
    base = [f for f in e['frames'] if f.shape == (640, 480, 3)]
    var = np.empty((NVAR, H, W, 3), np.uint8)
    for k in range(NVAR):
        var[k] = np.roll(base[k % len(base)], (2 * (k % 5) - 4, 2 * (k % 3) - 2), axis=(0, 1))[:H, :W]
    var[9] = 128
    pick = (7 * np.arange(N) + np.arange(N) // 32) % NVAR
    # one staging slot sees different frames in chunks 0, 1 and 2
    assert pick[0] != pick[CHUNK] and pick[0] != pick[2 * CHUNK] and pick[CHUNK] != pick[2 * CHUNK]
    var.setflags(write=False)
    return dict(reader=e['reader'], var=var, pick=pick)


def _layout(case, var, pick):
    """(array of the 257 frames, view function of a leading part of it, host call, device call) of one case."""
    ctx_calls = {
        'yuv': ('process_yuv', 'process_yuv_dev'), 'yuv422': ('process_yuv422', 'process_yuv422_dev'),
        'planes': ('process_planes', 'process_planes_dev')}
    if case == 'bgr':
        arr = var[pick]
        return arr, None, None
    if case == 'bgra':
        (arr, fmt) = fc.to_layout(var, 'bgra')
        arr = arr[pick]
        return arr, (lambda a: _hip.frames_view(a, fmt)), None
    if case in ('nv12', 'i420'):
        arr = fc.conventional420(*fc.F420.from_bgr(var), case)[pick]
        return arr, (lambda a: _hip.yuv_frames_view(a, case)), ctx_calls['yuv']
    if case == 'yuyv':
        arr = fc.conventional422(*fc.F422.from_bgr(var), case)[pick]
        return arr, (lambda a: _hip.yuv422_frames_view(a, case)), ctx_calls['yuv422']
    arr = fc.to_planes(var, 'rgb')[pick]
    return arr, (lambda a: _hip.planar_frames_view(a, 'rgb')), ctx_calls['planes']


def _host_and_dev(ctx, case, arr, view, calls):
    """Records of the host entry point and of the *_dev entry point for the same bytes."""
    hip = fc.hip_rt()
    d = C.c_void_p()
    if case == 'bgr':   # the packed-BGR entry points take no descriptor
        (ptr, extent) = (arr.ctypes.data, arr.nbytes)
        host = ctx.process_batch(arr)
    else:
        v = view(arr)
        assert not v.copied and v.n == len(arr) and (v.H, v.W) == (H, W)
        (ptr, extent) = (v.ptr, v.extent)
        if case == 'bgra':
            host = ctx.process_frames(v.ptr, v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride)
        else:
            host = getattr(ctx, calls[0])(v.ptr, v.descriptor())
    assert hip.hipMalloc(C.byref(d), C.c_size_t(extent)) == 0
    try:
        assert hip.hipMemcpy(d, C.c_void_p(ptr), C.c_size_t(extent), 1) == 0
        if case == 'bgr':
            dev = ctx.process_batch_dev(d.value, len(arr), H, W)
        elif case == 'bgra':
            dev = ctx.process_frames_dev(d.value, v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride)
        else:
            dev = getattr(ctx, calls[1])(d.value, v.descriptor())
    finally:
        hip.hipFree(d)
    return host, dev


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_three_chunks_reuse_staging_buffer_0(staged, case):
    ctx = staged['reader'].ctx
    (arr, view, calls) = _layout(case, staged['var'], staged['pick'])
    assert len(arr) == N and arr.flags.c_contiguous
    (host, dev) = _host_and_dev(ctx, case, arr, view, calls)
    assert len(host) == N and len(dev) == N
    bad = [i for i in range(N) if host[i].tobytes() != dev[i].tobytes()]
    assert not bad, (case, 'host and device records differ at frames', bad[:8])
    # the comparison is not one of rejected frames with rejected frames: most are read, the constant one is not
    ok = host['status'] == _hip.FRAME_OK
    assert ok.sum() >= N // 2 and (host['status'][staged['pick'] == 9] == _hip.FRAME_DIALS_NOT_FOUND).all(), (case, int(ok.sum()))
    if case == 'bgr':
        first = ctx.process_batch(arr[:CHUNK])
    else:
        v = view(arr[:CHUNK])
        assert not v.copied and v.n == CHUNK
        first = (ctx.process_frames(v.ptr, v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride) if case == 'bgra'
                 else getattr(ctx, calls[0])(v.ptr, v.descriptor()))
    bad = [i for i in range(CHUNK) if first[i].tobytes() != host[i].tobytes()]
    assert not bad, (case, 'the 128-frame call and the 257-frame call differ at frames', bad[:8])
