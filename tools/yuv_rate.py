#!/usr/bin/env python3
"""NV12 frames in place against packed BGR frames, bench.py's method: 1024-frame steps at config 3 (640 x 480, sample-images1
params), frames resident in HBM, --nbuf (4) distinct batches in rotation (more than the Infinity Cache holds), consecutive steps
alternating between two caller streams, records to a device buffer, the region between two device synchronisations on the wall
clock (bench.py: timed_steps).

    python3 tools/yuv_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

The NV12 frames are made from the synthetic BGR frames (float BT.601 limited range, 2 x 2 chroma mean); the BGR frames that are
timed are the conversion of include/meterelf_hip.h of those NV12 frames, so that both rows read the same pictures and their
records can be compared (they are, byte for byte, before anything is timed).  The rows take turns, R rounds of K steps each after
W untimed steps.  Then a few steps of each with every kernel bracketed by events: the prep kernel's (k_lplane) and the dial
reader's (k_dials) time per step.  Prints a table and the prep kernel's algorithmic bytes per frame."""
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

nv12 = torch.empty((N, H * 3 // 2, W), dtype=torch.uint8, device=dev)
bgr = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)


def q8(t):
    return torch.clamp(torch.floor(t + 0.5), 0, 255).to(torch.uint8)


for i0 in range(0, N, 256):
    src = torch.stack([torch.roll(base[i % K], shifts=(int(shifts[i, 1]), int(shifts[i, 0])), dims=(0, 1)) for i in range(i0, min(i0 + 256, N))])
    f = src.to(torch.float64)
    (b, g, r) = (f[..., 0], f[..., 1], f[..., 2])
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    m = len(src)
    u = u.reshape(m, H // 2, 2, W // 2, 2).mean(dim=(2, 4))
    v = v.reshape(m, H // 2, 2, W // 2, 2).mean(dim=(2, 4))
    (Y, U, V) = (q8(y), q8(u), q8(v))
    nv12[i0:i0 + m, :H] = Y
    nv12[i0:i0 + m, H:, 0::2] = U
    nv12[i0:i0 + m, H:, 1::2] = V
    # the conversion of include/meterelf_hip.h, in integers
    yy = torch.clamp(Y.to(torch.int32) - 16, min=0) * 1220542 + (1 << 19)
    ui = (U.to(torch.int32) - 128).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    vi = (V.to(torch.int32) - 128).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    bgr[i0:i0 + m, ..., 2] = torch.clamp((yy + 1673527 * vi) >> 20, 0, 255).to(torch.uint8)
    bgr[i0:i0 + m, ..., 1] = torch.clamp((yy - 852492 * vi - 409993 * ui) >> 20, 0, 255).to(torch.uint8)
    bgr[i0:i0 + m, ..., 0] = torch.clamp((yy + 2116026 * ui) >> 20, 0, 255).to(torch.uint8)
    del src, f, b, g, r, y, u, v, yy, ui, vi
torch.cuda.synchronize()

ctx = _hip.Context(_engine.make_blob(params), 0)
rsz = _hip.RESULT_DTYPE.itemsize
d_res = torch.zeros((N, rsz), dtype=torch.uint8, device=dev)
streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
view = _hip.yuv_frames_view(nv12[:B], 'nv12')
desc = view.descriptor()
yuv_batch_bytes = B * view.frame_stride
# the same frames as I420 (U plane, then V plane behind the Y rows): the planar kernels' times
i420 = nv12.clone()
i420[:, H:] = torch.cat([nv12[:, H:, 0::2].reshape(N, -1), nv12[:, H:, 1::2].reshape(N, -1)], dim=1).reshape(N, H // 2, W)
view_p = _hip.yuv_frames_view(i420[:B], 'i420')
desc_p = view_p.descriptor()


def step_bgr(i, stream):
    k = i % NB
    ctx.process_batch_dev(bgr.data_ptr() + k * B * H * W * 3, B, H, W, d_results_ptr=d_res.data_ptr() + k * B * rsz, want_host=False, stream=stream)


def step_nv12(i, stream):
    k = i % NB
    ctx.process_yuv_dev(nv12.data_ptr() + k * yuv_batch_bytes, desc, d_results_ptr=d_res.data_ptr() + k * B * rsz, want_host=False, stream=stream)


def run(fn, steps, nstreams=2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i, streams[i % nstreams].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def step_i420(i, stream):
    k = i % NB
    ctx.process_yuv_dev(i420.data_ptr() + k * B * view_p.frame_stride, desc_p, d_results_ptr=d_res.data_ptr() + k * B * rsz, want_host=False, stream=stream)


rows = [('BGR, melf_process_batch_dev', step_bgr), ('NV12, melf_process_yuv_dev', step_nv12), ('I420, melf_process_yuv_dev', step_i420)]
# the same records, byte for byte
run(step_bgr, NB)
ref = d_res.clone()
d_res.zero_()
run(step_nv12, NB)
assert torch.equal(d_res, ref), 'NV12 records differ from the BGR records'
d_res.zero_()
run(step_i420, NB)
assert torch.equal(d_res, ref), 'I420 records differ from the BGR records'
ok = int((ref.cpu().numpy().view(_hip.RESULT_DTYPE)['status'] == _hip.FRAME_OK).sum())
print('frames read: %d of %d; NV12 records == BGR records' % (ok, N))
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

P = ctx.params
(x0, x1) = (min(P.rect_x0, W), min(P.rect_x1, W))
(y0, y1) = (min(P.rect_y0, H), min(P.rect_y1, H))
(cr, cc) = (y1 - y0, x1 - x0)
crow = ((y1 - 1) >> 1) - (y0 >> 1) + 1
cbytes = (((x1 - 1) >> 1) - (x0 >> 1) + 1) * 2
alg = {'BGR': cr * cc * 3, 'NV12': cr * cc + crow * cbytes, 'I420': cr * cc + crow * cbytes}
old = float(np.median(times[rows[0][0]]))
print('%d-frame steps, %dx%d, %d batches in rotation (BGR %.2f GB, NV12 %.2f GB), two caller streams, %d rounds x %d steps'
      % (B, W, H, NB, bgr.numel() / 1e9, nv12.numel() / 1e9, args.rounds, args.steps))
print('| %-28s | %8s | %15s | %7s | %11s | %10s | %22s |' % ('row', 'ms/step', 'spread', 'vs BGR', 'k_lplane ms', 'k_dials ms', 'prep bytes read/frame'))
print('|%s|%s|%s|%s|%s|%s|%s|' % ('-' * 30, '-' * 10, '-' * 17, '-' * 9, '-' * 13, '-' * 12, '-' * 24))
for (name, _fn) in rows:
    t = times[name]
    print('| %-28s | %8.4f | %6.4f..%6.4f | %6.3fx | %11.4f | %10.4f | %22d |'
          % (name, float(np.median(t)), min(t), max(t), float(np.median(t)) / old, kern[name].get('k_lplane', 0.0), kern[name].get('k_dials', 0.0),
             alg[name.split(',')[0]]))
ctx.sync()
ctx.close()
