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
import numpy as np

import frame_rates as fr

args = fr.arg_parser(steps=40, warmup=300, rounds=5, nbuf=None).parse_args()
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)
torch = fr.torch
bgr = R.empty(H, W, 3)
for (i0, src) in R.chunks():
    bgr[i0:i0 + len(src)] = src
gen = torch.Generator(device=R.dev)
gen.manual_seed(4)
layouts = {'bgr': bgr.clone(), 'rgb': bgr.flip(-1).contiguous()}
for (name, order) in (('bgra', [0, 1, 2]), ('rgba', [2, 1, 0])):
    t = torch.randint(0, 256, (B, H, W, 4), dtype=torch.uint8, device=R.dev, generator=gen)
    t[..., :3] = bgr[..., order]
    layouts[name] = t
conv_out = torch.empty_like(bgr)

ctx = R.open()
views = {k: fr._hip.frames_view(v, k) for (k, v) in layouts.items()}
old_frames = bgr.clone()


def step_new(name):
    v = views[name]
    assert v.ptr == layouts[name].data_ptr()
    return R.step(ctx.process_frames_dev, layouts[name], 0, v.pixel_format, v.n, v.H, v.W, v.row_pitch, v.frame_stride)


rows = [('BGR, melf_process_batch_dev', R.step(ctx.process_batch_dev, old_frames, 0, B, H, W))]
rows += [('%s, melf_process_frames_dev' % k.upper(), step_new(k)) for k in ('bgr', 'rgb', 'bgra', 'rgba')]
rows += [('torch RGBA -> packed BGR (conversion alone)', lambda i, stream: conv_out.copy_(layouts['rgba'][..., [2, 1, 0]])),
         ('torch RGB -> packed BGR (conversion alone)', lambda i, stream: conv_out.copy_(layouts['rgb'].flip(-1)))]

# every row's records equal the old entry point's
ok = R.check_records(rows[1:5], rows[0], lambda name: name, run=R.run_events)
print('frames read: %d of %d' % (ok, B))

for (name, fn) in rows:
    R.run_events(fn, args.warmup)
times = {name: [] for (name, _fn) in rows}
for r in range(args.rounds):
    for (name, fn) in fr.rotated(rows, r):   # the order rotates: no row always follows the conversions
        times[name].append(R.run_events(fn, args.steps))
kern = R.kernel_times(rows[:5], run=R.run_events, steps=(4, 8))
hls = np.random.default_rng(5).integers(0, 256, (B, ctx.params.th, ctx.params.tw, 3), dtype=np.uint8)
ctx.set_profiling(1)
ctx.read_dials(hls)
ctx.timings()
for _ in range(4):
    ctx.read_dials(hls)
kern['HLS crops, melf_read_dials'] = fr.per_launch(ctx.timings())
ctx.set_profiling(0)
fr.print_table('%d-frame steps, %dx%d, %d rounds x %d steps (median ms per step; spread = min..max of the rounds)' % (B, W, H, args.rounds, args.steps),
               rows, times, rows[0], name=('row', 45), vs=('vs old', 7))
fr.print_table(None, [(name, None) for name in kern], None, None, fr.kernel_columns(kern), name=('row', 45))
R.close()
