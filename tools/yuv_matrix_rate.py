#!/usr/bin/env python3
"""NV12 frames in place under each colour matrix, the method of tools/yuv_rate.py: 1024-frame steps at config 3 (640 x 480,
sample-images1 params), frames resident in HBM, --nbuf (4) distinct batches in rotation, consecutive steps alternating between
two caller streams, records to a device buffer, the region between two device synchronisations on the wall clock.

    python3 tools/yuv_matrix_rate.py [--matrix bt601,bt601-full,bt709,bt709-full] [--encode bt601|own] [--steps 20] [--warmup 30]
                                     [--rounds 5]

One row per matrix, all rows reading the same NV12 bytes (made from the synthetic BGR frames with the float BT.601 limited-range
conversion): the rows differ in the six scalars of the kernels' YuvMatrix argument only.  The rows take turns, R rounds of K steps
each after W untimed steps; then a few steps of each with every kernel bracketed by events: the prep kernel's (k_lplane_yuv) and
the dial reader's (k_yneedle) time per step through melf_ctx_timings.  MELF_LIB_PATH selects the library, so that
`--matrix bt601` also times a build from before the matrices existed (its only matrix) in the same session.
--encode own: every row reads NV12 frames made with its own matrix instead, i.e. the same pictures as different bytes: the dial
reader's work depends on the colours it sees (how many pixels pass its prefilter), which the same bytes under another matrix change."""
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
ap.add_argument('--matrix', default=','.join(_hip.YUV_MATRIX_CODES))
ap.add_argument('--encode', choices=('bt601', 'own'), default='bt601')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=30)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--batch', type=int, default=1024)
ap.add_argument('--nbuf', type=int, default=4)
args = ap.parse_args()
names = [m for m in args.matrix.split(',') if m]

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
# Kr, Kb, limited range of each matrix: the float conversion that makes the frames
STANDARD = {'bt601': (0.299, 0.114, True), 'bt601-full': (0.299, 0.114, False), 'bt709': (0.2126, 0.0722, True), 'bt709-full': (0.2126, 0.0722, False)}


def q8(t):
    return torch.clamp(torch.floor(t + 0.5), 0, 255).to(torch.uint8)


def make_nv12(enc):
    (kr, kb, limited) = STANDARD[enc]
    out = torch.empty((N, H * 3 // 2, W), dtype=torch.uint8, device=dev)
    for i0 in range(0, N, 256):
        src = torch.stack([torch.roll(base[i % K], shifts=(int(shifts[i, 1]), int(shifts[i, 0])), dims=(0, 1)) for i in range(i0, min(i0 + 256, N))])
        f = src.to(torch.float64)
        (b, g, r) = (f[..., 0], f[..., 1], f[..., 2])
        yl = kr * r + (1.0 - kr - kb) * g + kb * b
        (u, v) = ((b - yl) / (2.0 * (1.0 - kb)), (r - yl) / (2.0 * (1.0 - kr)))
        (y, u, v) = (16.0 + yl * 219.0 / 255.0, 128.0 + u * 224.0 / 255.0, 128.0 + v * 224.0 / 255.0) if limited else (yl, 128.0 + u, 128.0 + v)
        m = len(src)
        out[i0:i0 + m, :H] = q8(y)
        out[i0:i0 + m, H:, 0::2] = q8(u.reshape(m, H // 2, 2, W // 2, 2).mean(dim=(2, 4)))
        out[i0:i0 + m, H:, 1::2] = q8(v.reshape(m, H // 2, 2, W // 2, 2).mean(dim=(2, 4)))
        del src, f, b, g, r, yl, y, u, v
    return out


frames = {}
for name in names:
    enc = name if args.encode == 'own' else 'bt601'
    if enc not in frames:
        frames[enc] = make_nv12(enc)
    frames[name] = frames[enc]
nv12 = frames[names[0]]
torch.cuda.synchronize()

ctx = _hip.Context(_engine.make_blob(params), 0)
rsz = _hip.RESULT_DTYPE.itemsize
d_res = torch.zeros((N, rsz), dtype=torch.uint8, device=dev)
streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
descs = {m: _hip.yuv_frames_view(nv12[:B], 'nv12', m).descriptor() for m in names}
batch_bytes = B * _hip.yuv_frames_view(nv12[:B], 'nv12').frame_stride


def stepper(name):
    def step(i, stream):
        k = i % NB
        ctx.process_yuv_dev(frames[name].data_ptr() + k * batch_bytes, descs[name], d_results_ptr=d_res.data_ptr() + k * B * rsz, want_host=False,
                            stream=stream)
    return step


def run(fn, steps, nstreams=2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i, streams[i % nstreams].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


rows = [(m, stepper(m)) for m in names]
print('library: %s; frames encoded with %s' % (os.environ.get('MELF_LIB_PATH', 'the package\'s'), 'each row\'s own matrix' if args.encode == 'own' else 'bt601'))
ok = {}
for (name, fn) in rows:
    d_res.zero_()
    run(fn, NB)
    ok[name] = int((d_res.cpu().numpy().view(_hip.RESULT_DTYPE)['status'] == _hip.FRAME_OK).sum())
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

first = float(np.median(times[names[0]]))
print('%d-frame steps, %dx%d NV12, %d batches in rotation (%.2f GB), two caller streams, %d rounds x %d steps'
      % (B, W, H, NB, nv12.numel() / 1e9, args.rounds, args.steps))
print('| %-12s | %8s | %15s | %9s | %11s | %10s | %11s |' % ('matrix', 'ms/step', 'spread', 'vs %s' % names[0][:6], 'k_lplane ms', 'k_dials ms', 'frames read'))
print('|%s|%s|%s|%s|%s|%s|%s|' % ('-' * 14, '-' * 10, '-' * 17, '-' * 11, '-' * 13, '-' * 12, '-' * 13))
for (name, _fn) in rows:
    t = times[name]
    print('| %-12s | %8.4f | %6.4f..%6.4f | %8.3fx | %11.4f | %10.4f | %4d / %4d |'
          % (name, float(np.median(t)), min(t), max(t), float(np.median(t)) / first, kern[name].get('k_lplane', 0.0), kern[name].get('k_dials', 0.0),
             ok[name], N))
ctx.sync()
ctx.close()
