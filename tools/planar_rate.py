#!/usr/bin/env python3
"""Planar RGB frames (N, 3, H, W) in place against packed BGR frames and against the interleaving copy such a caller makes today,
bench.py's method: 1024-frame steps at config 3 (640 x 480, sample-images1 params), frames resident in HBM, --nbuf (4) distinct
batches in rotation (more than the Infinity Cache holds), consecutive steps alternating between two caller streams, records to a
device buffer, the region between two device synchronisations on the wall clock (bench.py: timed_steps).

    python3 tools/planar_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

Three rows read the same pictures: (1) packed BGR through melf_process_batch_dev; (2) the same frames as RGB planes through
melf_process_planes_dev; (3) what a caller with RGB planes does without it: planes.permute(0, 2, 3, 1).contiguous() on the GPU
(torch, on the step's stream, inside the timed step) and melf_process_frames_dev on the packed RGB frames that gives.  All records
are compared, byte for byte, before anything is timed.  The rows take turns, R rounds of K steps each after W untimed steps.
Then a few steps of each with every kernel bracketed by events: the prep kernel's (k_lplane) and the dial reader's (k_dials)
time per step.  Prints a table and whether row 2 beats row 3 by more than the rounds' spread."""
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

bgr = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
planes = torch.empty((N, 3, H, W), dtype=torch.uint8, device=dev)   # R, G, B
for i0 in range(0, N, 256):
    src = torch.stack([torch.roll(base[i % K], shifts=(int(shifts[i, 1]), int(shifts[i, 0])), dims=(0, 1)) for i in range(i0, min(i0 + 256, N))])
    bgr[i0:i0 + len(src)] = src
    planes[i0:i0 + len(src)] = src.flip(3).permute(0, 3, 1, 2)
    del src
torch.cuda.synchronize()

ctx = _hip.Context(_engine.make_blob(params), 0)
rsz = _hip.RESULT_DTYPE.itemsize
d_res = torch.zeros((N, rsz), dtype=torch.uint8, device=dev)
streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
view = _hip.planar_frames_view(planes[:B], 'rgb')
assert not view.copied
desc = view.descriptor()
batch_bytes = B * view.frame_stride


def step_bgr(i, stream):
    k = i % NB
    ctx.process_batch_dev(bgr.data_ptr() + k * B * H * W * 3, B, H, W, d_results_ptr=d_res.data_ptr() + k * B * rsz, want_host=False,
                          stream=stream.cuda_stream)


def step_planes(i, stream):
    k = i % NB
    ctx.process_planes_dev(planes.data_ptr() + k * batch_bytes, desc, d_results_ptr=d_res.data_ptr() + k * B * rsz, want_host=False,
                           stream=stream.cuda_stream)


def step_copy(i, stream):
    k = i % NB
    with torch.cuda.stream(stream):
        packed = planes[k * B:(k + 1) * B].permute(0, 2, 3, 1).contiguous()   # (B, H, W, 3) R G B: the copy today's route writes
        packed.record_stream(stream)
    ctx.process_frames_dev(packed.data_ptr(), _hip.PIX_RGB, B, H, W, W * 3, H * W * 3, d_results_ptr=d_res.data_ptr() + k * B * rsz,
                           want_host=False, stream=stream.cuda_stream)


def run(fn, steps, nstreams=2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i, streams[i % nstreams])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


rows = [('BGR, melf_process_batch_dev', step_bgr), ('RGB planes, melf_process_planes_dev', step_planes),
        ('RGB planes, permute().contiguous() + frames_dev', step_copy)]
# the same records, byte for byte
run(step_bgr, NB)
ref = d_res.clone()
for (name, fn) in rows[1:]:
    d_res.zero_()
    run(fn, NB)
    assert torch.equal(d_res, ref), '%s: records differ from the BGR records' % name
ok = int((ref.cpu().numpy().view(_hip.RESULT_DTYPE)['status'] == _hip.FRAME_OK).sum())
print('frames read: %d of %d; records of all three rows identical' % (ok, N))
print('match kernel: %s' % ctx.last_match()['kernel'])

for (_name, fn) in rows:
    run(fn, args.warmup)
times = {name: [] for (name, _fn) in rows}
for r in range(args.rounds):
    order = rows[r % 3:] + rows[:r % 3]
    for (name, fn) in order:
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
crop = (y1 - y0) * (x1 - x0) * 3
alg = [crop, crop, 2 * H * W * 3 + crop]   # row 3: the copy reads and writes every frame, then the kernels read the crop
old = float(np.median(times[rows[0][0]]))
print('%d-frame steps, %dx%d, %d batches in rotation (%.2f GB each layout), two caller streams, %d rounds x %d steps'
      % (B, W, H, NB, bgr.numel() / 1e9, args.rounds, args.steps))
print('| %-47s | %8s | %15s | %7s | %11s | %10s | %16s |' % ('row', 'ms/step', 'spread', 'vs BGR', 'k_lplane ms', 'k_dials ms', 'bytes read+written/frame'[:16]))
print('|%s|%s|%s|%s|%s|%s|%s|' % ('-' * 49, '-' * 10, '-' * 17, '-' * 9, '-' * 13, '-' * 12, '-' * 18))
for ((name, _fn), a) in zip(rows, alg):
    t = times[name]
    print('| %-47s | %8.4f | %6.4f..%6.4f | %6.3fx | %11.4f | %10.4f | %16d |'
          % (name, float(np.median(t)), min(t), max(t), float(np.median(t)) / old, kern[name].get('k_lplane', 0.0), kern[name].get('k_dials', 0.0), a))
(t2, t3) = (times[rows[1][0]], times[rows[2][0]])
spread = max(max(t) - min(t) for t in times.values())
gain = float(np.median(t3)) - float(np.median(t2))
print('planes in place against the copying route: %.4f ms per step shorter (median), largest spread between rounds %.4f ms: %s'
      % (gain, spread, 'beyond the spread' if gain > spread and max(t2) < min(t3) else 'NOT beyond the spread'))
ctx.sync()
ctx.close()
