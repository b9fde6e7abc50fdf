#!/usr/bin/env python3
"""One call's time by pixel layout: 1024-frame steps at config 3 (640 x 480, sample-images1 params), frames resident in HBM, one
caller stream, records to a device buffer (melf_process_batch_dev / melf_process_frames_dev), event-timed.

    python3 tools/pixel_format_rate.py [--steps K] [--rounds R] [--warmup W]

Rows: packed BGR through the old entry point; BGR, RGB, BGRA, RGBA through the new one; and, for scale, the torch pass that
converts the same batch from RGBA / RGB to packed BGR (what a caller did before the new entry point).  Every row has its own copy
of the frames, so that the timed region rotates over more than 256 MB (a 1024-frame batch is 0.94 GB in BGR, 1.26 GB in BGRA)
as bench.py's does; the rows take turns, K steps each, in an order that rotates from round to round, R rounds, after W untimed
steps of every row.  Prints a table (median ms per step over the rounds and its ratio to the old entry point's) and, for the rows
that run the library's kernels, the prep and the dial kernel's own time per launch (every kernel bracketed by events,
melf_ctx_set_profiling); a last row gives the dial kernel of melf_read_dials on the same number of HLS crops (host-fed: no step
time).  MELF_LIB_PATH selects the library, so that two builds can be compared."""
import argparse
import glob
import os
import sys

import numpy as np
import torch  # before the package loads the library: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from meterelf_amd import _engine, _hip, _params  # noqa: E402
from meterelf_amd._image import imread_bgr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--warmup', type=int, default=300)
ap.add_argument('--batch', type=int, default=1024)
args = ap.parse_args()

dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
gdir = os.path.join(ROOT, 'tests', 'golden', 'sample-images1')
params = _params.load(os.path.join(gdir, 'params.yml'))
base = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(gdir, '*.jpg')))]
shapes = [b.shape for b in base]
base = torch.from_numpy(np.stack([b for b in base if b.shape == max(set(shapes), key=shapes.count)])).to(dev)   # the fixture's frame size
(K, H, W, _) = base.shape
B = args.batch
rng = np.random.default_rng(3)
shifts = rng.integers(-8, 9, size=(B, 2))
bgr = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
for i in range(B):
    bgr[i] = torch.roll(base[i % K], shifts=(int(shifts[i, 1]), int(shifts[i, 0])), dims=(0, 1))
gen = torch.Generator(device=dev)
gen.manual_seed(4)
layouts = {'bgr': bgr.clone(), 'rgb': bgr.flip(-1).contiguous()}
for (name, order) in (('bgra', [0, 1, 2]), ('rgba', [2, 1, 0])):
    t = torch.randint(0, 256, (B, H, W, 4), dtype=torch.uint8, device=dev, generator=gen)
    t[..., :3] = bgr[..., order]
    layouts[name] = t
conv_out = torch.empty_like(bgr)

ctx = _hip.Context(_engine.make_blob(params), 0)
rsz = _hip.RESULT_DTYPE.itemsize
d_res = torch.empty((B, rsz), dtype=torch.uint8, device=dev)
stream = torch.cuda.current_stream(dev)
views = {k: _hip.frames_view(v, k) for (k, v) in layouts.items()}
old_frames = bgr.clone()


def step_old():
    ctx.process_batch_dev(old_frames.data_ptr(), B, H, W, d_results_ptr=d_res.data_ptr(), want_host=False, stream=stream.cuda_stream)


def step_new(name):
    v = views[name]
    return lambda: ctx.process_frames_dev(v.ptr, v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride, d_results_ptr=d_res.data_ptr(),
                                          want_host=False, stream=stream.cuda_stream)


rows = [('BGR, melf_process_batch_dev', step_old)] + [('%s, melf_process_frames_dev' % k.upper(), step_new(k)) for k in ('bgr', 'rgb', 'bgra', 'rgba')]
rows += [('torch RGBA -> packed BGR (conversion alone)', lambda: conv_out.copy_(layouts['rgba'][..., [2, 1, 0]])),
         ('torch RGB -> packed BGR (conversion alone)', lambda: conv_out.copy_(layouts['rgb'].flip(-1)))]

# every row's records equal the old entry point's
step_old()
ref = d_res.clone()
ok = int((torch.from_numpy(ref.cpu().numpy().view(_hip.RESULT_DTYPE)['status'].copy()) == _hip.FRAME_OK).sum())
print('frames read: %d of %d' % (ok, B))
for (name, fn) in rows[1:5]:
    d_res.zero_()
    fn()
    torch.cuda.synchronize()
    assert torch.equal(d_res, ref), name

for (name, fn) in rows:
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
times = {name: [] for (name, _fn) in rows}
for r in range(args.rounds):
    for (name, fn) in rows[r % len(rows):] + rows[:r % len(rows)]:   # the order rotates: no row always follows the conversions
        (e0, e1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e0.record(stream)
        for _ in range(args.steps):
            fn()
        e1.record(stream)
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.steps)
# per-kernel times: every kernel bracketed by events
kern = {}
ctx.set_profiling(1)
for (name, fn) in rows[:5]:
    for _ in range(4):
        fn()
    torch.cuda.synchronize()
    ctx.timings()
    for _ in range(8):
        fn()
    torch.cuda.synchronize()
    kern[name] = {k: (ms / max(cnt, 1)) for (k, (ms, cnt)) in ctx.timings().items() if cnt}
hls = np.random.default_rng(5).integers(0, 256, (B, ctx.params.th, ctx.params.tw, 3), dtype=np.uint8)
ctx.read_dials(hls)
ctx.timings()
for _ in range(4):
    ctx.read_dials(hls)
kern['HLS crops, melf_read_dials'] = {k: (ms / max(cnt, 1)) for (k, (ms, cnt)) in ctx.timings().items() if cnt}
ctx.set_profiling(0)
old = float(np.median(times[rows[0][0]]))
print('%d-frame steps, %dx%d, %d rounds x %d steps (median ms per step; spread = min..max of the rounds)' % (B, W, H, args.rounds, args.steps))
print('| %-45s | %8s | %15s | %7s |' % ('row', 'ms/step', 'spread', 'vs old'))
print('|%s|%s|%s|%s|' % ('-' * 47, '-' * 10, '-' * 17, '-' * 9))
for (name, _fn) in rows:
    t = times[name]
    print('| %-45s | %8.4f | %6.4f..%6.4f | %6.3fx |' % (name, float(np.median(t)), min(t), max(t), float(np.median(t)) / old))
print('| %-45s | %11s | %10s |' % ('row', 'k_lplane ms', 'k_dials ms'))
print('|%s|%s|%s|' % ('-' * 47, '-' * 13, '-' * 12))
for (name, k) in kern.items():
    print('| %-45s | %11.4f | %10.4f |' % (name, k.get('k_lplane', 0.0), k.get('k_dials', 0.0)))
ctx.sync()
ctx.close()
