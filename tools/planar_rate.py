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
import numpy as np

import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)
torch = fr.torch
bgr = R.empty(H, W, 3)
planes = R.empty(3, H, W)   # R, G, B
for (i0, src) in R.chunks():
    bgr[i0:i0 + len(src)] = src
    fr.write_planes(planes[i0:i0 + len(src)], src)
    del src
torch.cuda.synchronize()

ctx = R.open()
view = fr._hip.planar_frames_view(planes[:B], 'rgb')
assert not view.copied


def step_copy(i, stream):
    k = i % R.NB
    with torch.cuda.stream(stream):
        packed = planes[k * B:(k + 1) * B].permute(0, 2, 3, 1).contiguous()   # (B, H, W, 3) R G B: the copy today's route writes
        packed.record_stream(stream)
    ctx.process_frames_dev(packed.data_ptr(), fr._hip.PIX_RGB, B, H, W, W * 3, H * W * 3, d_results_ptr=R.d_res.data_ptr() + k * B * R.rsz,
                           want_host=False, stream=stream.cuda_stream)


rows = [('BGR, melf_process_batch_dev', R.step(ctx.process_batch_dev, bgr, B * H * W * 3, B, H, W)),
        ('RGB planes, melf_process_planes_dev', R.step(ctx.process_planes_dev, planes, B * view.frame_stride, view.descriptor())),
        ('RGB planes, permute().contiguous() + frames_dev', step_copy)]
ok = R.check_records(rows[1:], rows[0], lambda name: '%s: records differ from the BGR records' % name)
print('frames read: %d of %d; records of all three rows identical' % (ok, R.N))
print('match kernel: %s' % ctx.last_match()['kernel'])
times = R.alternate(rows, fr.rotated)
kern = R.kernel_times(rows)

P = ctx.params
(x0, x1) = (min(P.rect_x0, W), min(P.rect_x1, W))
(y0, y1) = (min(P.rect_y0, H), min(P.rect_y1, H))
crop = (y1 - y0) * (x1 - x0) * 3
alg = dict(zip([name for (name, _fn) in rows], [crop, crop, 2 * H * W * 3 + crop]))   # row 3: the copy reads and writes every frame, then the kernels read the crop
fr.print_table('%d-frame steps, %dx%d, %d batches in rotation (%.2f GB each layout), two caller streams, %d rounds x %d steps'
               % (B, W, H, R.NB, bgr.numel() / 1e9, args.rounds, args.steps), rows, times, rows[0],
               fr.kernel_columns(kern) + [('bytes read+written/frame'[:16], 16, lambda name: '%d' % alg[name])], name=('row', 47))
(t2, t3) = (times[rows[1][0]], times[rows[2][0]])
spread = max(max(t) - min(t) for t in times.values())
gain = float(np.median(t3)) - float(np.median(t2))
print('planes in place against the copying route: %.4f ms per step shorter (median), largest spread between rounds %.4f ms: %s'
      % (gain, spread, 'beyond the spread' if gain > spread and max(t2) < min(t3) else 'NOT beyond the spread'))
R.close()
