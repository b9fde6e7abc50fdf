#!/usr/bin/env python3
"""Planar and semi-planar YUV 4:2:2 / 4:4:4 frames in place (melf_process_yuv_planar_dev) against packed BGR frames and against
NV12 through the existing entry point, tools/yuv422_rate.py's method: one process, 1024-frame steps at config 3 (640 x 480,
sample-images1 params), frames resident in HBM, --nbuf (4) distinct batches in rotation, consecutive steps alternating between two
caller streams, records to a device buffer, the region between two device synchronisations on the wall clock.

    python3 tools/yuv_planar_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

Rows: BGR (melf_process_batch_dev), NV12 (melf_process_yuv_dev), I422, NV16, I444, NV24 (melf_process_yuv_planar_dev), all made
from the same synthetic pictures (float BT.601 limited range, the chroma block's mean); the BGR row reads the conversion of
include/meterelf_hip.h of the 4:4:4 planes.  Before anything is timed every YUV row's records of its first batch are compared, byte
for byte, with process_batch_dev of the header's conversion of that row's own planes, and NV12's with NV12 through the new entry
point.  The rows take turns, R rounds of K steps each after W untimed steps.  Then a few steps of each with every kernel bracketed
by events: the prep kernel's (k_lplane) and the dial reader's (k_dials) time per step.  Prints a table with each row's ratio to
the BGR row and to the NV12 row of the same run."""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch  # before the package loads the library: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from meterelf_amd import _engine, _hip, _params  # noqa: E402
from meterelf_amd._image import imread_bgr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=30)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--batch', type=int, default=1024)
ap.add_argument('--nbuf', type=int, default=4)
args = ap.parse_args()

dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
gdir = os.path.join(ROOT, 'tests', 'golden', 'sample-images1')
params = _params.load(os.path.join(gdir, 'params.yml'))
base = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(gdir, '*.jpg')))]
shapes = [b.shape for b in base]
base = torch.from_numpy(np.stack([b for b in base if b.shape == max(set(shapes), key=shapes.count)])).to(dev)
(K, H, W, _) = base.shape
(B, NB) = (args.batch, args.nbuf)
N = B * NB
rng = np.random.default_rng(3)
shifts = rng.integers(-8, 9, size=(N, 2))

# name -> (pixel_format, sub_x, sub_y); the arrays are the raw-video (N, rows, W) layout
LAYOUTS = {'NV12': ('nv12', 1, 1), 'I422': ('i422', 1, 0), 'NV16': ('nv16', 1, 0), 'I444': ('i444', 0, 0), 'NV24': ('nv24', 0, 0)}
arrays = {name: torch.empty((N, H + 2 * (H >> sy) // (1 << sx), W), dtype=torch.uint8, device=dev) for (name, (_f, sx, sy)) in LAYOUTS.items()}
bgr = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)


def q8(t):
    return torch.clamp(torch.floor(t + 0.5), 0, 255).to(torch.uint8)


def to_bgr(Y, U, V, sx, sy):
    """the conversion of include/meterelf_hip.h (BT.601 limited), in integers, nearest chroma sample"""
    yy = torch.clamp(Y.to(torch.int32) - 16, min=0) * 1220542 + (1 << 19)
    (ui, vi) = (U.to(torch.int32) - 128, V.to(torch.int32) - 128)
    if sy:
        (ui, vi) = (ui.repeat_interleave(2, dim=1), vi.repeat_interleave(2, dim=1))
    if sx:
        (ui, vi) = (ui.repeat_interleave(2, dim=2), vi.repeat_interleave(2, dim=2))
    out = torch.empty(Y.shape + (3,), dtype=torch.uint8, device=Y.device)
    out[..., 2] = torch.clamp((yy + 1673527 * vi) >> 20, 0, 255).to(torch.uint8)
    out[..., 1] = torch.clamp((yy - 852492 * vi - 409993 * ui) >> 20, 0, 255).to(torch.uint8)
    out[..., 0] = torch.clamp((yy + 2116026 * ui) >> 20, 0, 255).to(torch.uint8)
    return out


def planes_of(arr, name):
    """Y, U, V of a raw-video array of layout `name` (views / copies, for the records check)"""
    (_f, sx, sy) = LAYOUTS[name]
    m = len(arr)
    (ch, cw) = (H >> sy, W >> sx)
    Y = arr[:, :H]
    c = arr[:, H:].reshape(m, -1)
    if name.startswith('NV'):
        c = c.reshape(m, ch, cw, 2)
        return Y, c[..., 0], c[..., 1]
    return Y, c[:, :ch * cw].reshape(m, ch, cw), c[:, ch * cw:].reshape(m, ch, cw)


for i0 in range(0, N, 256):
    src = torch.stack([torch.roll(base[i % K], shifts=(int(shifts[i, 1]), int(shifts[i, 0])), dims=(0, 1)) for i in range(i0, min(i0 + 256, N))])
    f = src.to(torch.float64)
    (b, g, r) = (f[..., 0], f[..., 1], f[..., 2])
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    m = len(src)
    Y = q8(y)
    for (name, (_f, sx, sy)) in LAYOUTS.items():
        (ch, cw) = (H >> sy, W >> sx)
        (U, V) = (q8(u.reshape(m, ch, 1 << sy, cw, 1 << sx).mean(dim=(2, 4))), q8(v.reshape(m, ch, 1 << sy, cw, 1 << sx).mean(dim=(2, 4))))
        a = arrays[name][i0:i0 + m]
        a[:, :H] = Y
        c = a[:, H:].reshape(m, -1)
        if name.startswith('NV'):
            c = c.reshape(m, ch, cw, 2)
            c[..., 0] = U
            c[..., 1] = V
        else:
            c[:, :ch * cw] = U.reshape(m, -1)
            c[:, ch * cw:] = V.reshape(m, -1)
        if name == 'I444':
            bgr[i0:i0 + m] = to_bgr(Y, U, V, 0, 0)
    del src, f, b, g, r, y, u, v
torch.cuda.synchronize()

ctx = _hip.Context(_engine.make_blob(params), 0)
rsz = _hip.RESULT_DTYPE.itemsize
d_res = torch.zeros((N, rsz), dtype=torch.uint8, device=dev)
streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
descs = {}
for (name, (fmt, _sx, _sy)) in LAYOUTS.items():
    view = _hip.yuv_frames_view(arrays[name][:B], fmt) if name == 'NV12' else _hip.yuv_planar_frames_view(arrays[name][:B], fmt)
    assert not view.copied
    descs[name] = (view.descriptor(), B * view.frame_stride)


def step_bgr(i, stream):
    k = i % NB
    ctx.process_batch_dev(bgr.data_ptr() + k * B * H * W * 3, B, H, W, d_results_ptr=d_res.data_ptr() + k * B * rsz, want_host=False, stream=stream)


def step_of(name):
    (desc, batch_bytes) = descs[name]
    call = ctx.process_yuv_dev if name == 'NV12' else ctx.process_yuv_planar_dev

    def step(i, stream):
        k = i % NB
        call(arrays[name].data_ptr() + k * batch_bytes, desc, d_results_ptr=d_res.data_ptr() + k * B * rsz, want_host=False, stream=stream)
    return step


def run(fn, steps, nstreams=2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i, streams[i % nstreams].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


rows = [('BGR, melf_process_batch_dev', step_bgr), ('NV12, melf_process_yuv_dev', step_of('NV12'))]
rows += [('%s, melf_process_yuv_planar_dev' % name, step_of(name)) for name in ('I422', 'NV16', 'I444', 'NV24')]
# the records: every YUV row's first batch against process_batch_dev of the header's conversion of its own planes
for name in LAYOUTS:
    (_f, sx, sy) = LAYOUTS[name]
    own = to_bgr(*planes_of(arrays[name][:B], name), sx, sy).contiguous()
    torch.cuda.synchronize()
    want = ctx.process_batch_dev(own.data_ptr(), B, H, W)
    d_res.zero_()
    step_of(name)(0, streams[0].cuda_stream)
    torch.cuda.synchronize()
    got = d_res[:B].cpu().numpy().tobytes()
    assert got == want.tobytes(), '%s records differ from the records of its BGR conversion' % name
    if name == 'NV12':
        (fmt, _sx, _sy) = LAYOUTS[name]
        v = _hip.yuv_planar_frames_view(arrays[name][:B], fmt)
        assert ctx.process_yuv_planar_dev(v.ptr, v.descriptor()).tobytes() == got, 'NV12: the two entry points differ'
    ok = int((want['status'] == _hip.FRAME_OK).sum())
    print('%s: %d of %d frames of the first batch read; records == those of its BGR conversion' % (name, ok, B))
    del own
print('match kernel: %s' % ctx.last_match()['kernel'])

for (_name, fn) in rows:
    run(fn, args.warmup)
times = {name: [] for (name, _fn) in rows}
for r in range(args.rounds):
    for (name, fn) in (rows if r % 2 == 0 else rows[::-1]):
        run(fn, 4)   # the other row's last steps are out of the lanes
        times[name].append(run(fn, args.steps))
# per-kernel times: every kernel bracketed by events, one caller stream
kern = {}
ctx.set_profiling(1)
for (name, fn) in rows:
    run(fn, 2 * NB, 1)
    ctx.timings()
    run(fn, 2 * NB, 1)
    kern[name] = {k: (ms / max(cnt, 1)) for (k, (ms, cnt)) in ctx.timings().items() if cnt}
ctx.set_profiling(0)

med = {name: float(np.median(t)) for (name, t) in times.items()}
(t_bgr, t_nv12) = (med[rows[0][0]], med[rows[1][0]])
print('%d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps' % (B, W, H, NB, args.rounds, args.steps))
print('| %-36s | %8s | %15s | %7s | %7s | %11s | %10s |' % ('row', 'ms/step', 'spread', 'vs BGR', 'vs NV12', 'k_lplane ms', 'k_dials ms'))
print('|%s|%s|%s|%s|%s|%s|%s|' % ('-' * 38, '-' * 10, '-' * 17, '-' * 9, '-' * 9, '-' * 13, '-' * 12))
for (name, _fn) in rows:
    t = times[name]
    print('| %-36s | %8.4f | %6.4f..%6.4f | %6.3fx | %6.3fx | %11.4f | %10.4f |'
          % (name, med[name], min(t), max(t), med[name] / t_bgr, med[name] / t_nv12, kern[name].get('k_lplane', 0.0), kern[name].get('k_dials', 0.0)))
ctx.sync()
ctx.close()
