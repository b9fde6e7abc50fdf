#!/usr/bin/env python3
"""10-bit YUV frames in place (melf_process_yuv16_dev: P010, I010) against the same pictures as NV12 / I420 through
melf_process_yuv_dev, and against what a caller does without it: a pass that reduces every P010 frame to NV12 (the high byte of each
sample, one strided device copy of the whole frame on the call's stream) followed by the NV12 read.  tools/yuv_planar_rate.py's
method: one process, 1024-frame steps at config 3 (640 x 480, sample-images1 params), frames resident in HBM, --nbuf (4) distinct
batches in rotation, consecutive steps alternating between two caller streams, records to a device buffer, the region between two
device synchronisations on the wall clock.

    python3 tools/yuv16_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

All rows are made from the same synthetic pictures (float BT.709 limited range, the chroma block's mean) and read under 'bt709'.
P010 holds the 8-bit value in the high byte (the low byte zero), I010 the value times four in the low ten bits: both reduce to the
NV12 / I420 rows' samples, so before anything is timed the 16-bit rows' records of every batch are compared, byte for byte, with
their 8-bit row's.  The rows take turns, R rounds of K steps each after W untimed steps.  Then a few steps of each with every
kernel bracketed by events: the prep kernel's (k_lplane) and the dial reader's (k_dials) time per step (the reduce pass is torch's
copy kernel, not the library's: its time is the last row's step, the pass alone).  Prints a table with each row's ratio to the NV12
row of the same run."""
import numpy as np

import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)
torch = fr.torch
rows420 = fr.yuv_rows(H, 1, 1)

nv12 = R.empty(rows420, W)
i420 = R.empty(rows420, W)
p010 = R.empty(rows420, W, 2)      # the two bytes of a little-endian sample
i010 = R.empty(rows420, W, 2)
for (i0, src) in R.chunks():
    (Y, U, V) = fr.encode(src, 1, 1, 'bt709')
    m = len(src)
    fr.write_yuv(nv12[i0:i0 + m], Y, U, V, semi=True)
    fr.write_yuv(i420[i0:i0 + m], Y, U, V, semi=False)
    p010[i0:i0 + m, ..., 1] = nv12[i0:i0 + m]                      # value << 8
    p010[i0:i0 + m, ..., 0] = 0
    i010[i0:i0 + m, ..., 1] = i420[i0:i0 + m] >> 6                 # value << 2
    i010[i0:i0 + m, ..., 0] = (i420[i0:i0 + m] << 2)
    del src, Y, U, V
torch.cuda.synchronize()
(p010s, i010s) = (p010.view(torch.int16).squeeze(-1), i010.view(torch.int16).squeeze(-1))   # (N, rows, W) samples, the same bits

ctx = R.open()
v8 = {name: fr._hip.yuv_frames_view(arr[:B], name, 'bt709') for (name, arr) in (('nv12', nv12), ('i420', i420))}
v16 = {name: fr._hip.yuv16_frames_view(arr[:B], name, 'bt709') for (name, arr) in (('p010', p010s), ('i010', i010s))}
assert not any(v.copied for v in list(v8.values()) + list(v16.values()))
step_nv12 = R.step(ctx.process_yuv_dev, nv12, B * v8['nv12'].frame_stride, v8['nv12'].descriptor())
step_i420 = R.step(ctx.process_yuv_dev, i420, B * v8['i420'].frame_stride, v8['i420'].descriptor())
step_p010 = R.step(ctx.process_yuv16_dev, p010s, B * v16['p010'].frame_stride, v16['p010'].descriptor())
step_i010 = R.step(ctx.process_yuv16_dev, i010s, B * v16['i010'].frame_stride, v16['i010'].descriptor())

# what callers do today: every P010 frame reduced to NV12 by a pass over the whole frame (its high bytes), then the NV12 read; one
# scratch batch per caller stream
scratch = [torch.empty((B, rows420, W), dtype=torch.uint8, device=R.dev) for _s in R.streams]


def step_reduce(i, stream):
    with torch.cuda.stream(stream):
        scratch[R.streams.index(stream)].copy_(p010[(i % R.NB) * B:(i % R.NB + 1) * B, ..., 1])


def step_today(i, stream):
    step_reduce(i, stream)
    # (the records go to batch i % nbuf's slice, as R.step has it; the frames are the stream's scratch batch)
    ctx.process_yuv_dev(scratch[R.streams.index(stream)].data_ptr(), v8['nv12'].descriptor(),
                        d_results_ptr=R.d_res.data_ptr() + (i % R.NB) * B * R.rsz, want_host=False, stream=stream.cuda_stream)


rows = [('NV12, melf_process_yuv_dev', step_nv12), ('I420, melf_process_yuv_dev', step_i420),
        ('P010, melf_process_yuv16_dev', step_p010), ('I010, melf_process_yuv16_dev', step_i010),
        ('P010 -> NV12 pass + melf_process_yuv_dev', step_today), ('P010 -> NV12 pass (conversion alone)', step_reduce)]
ok = R.check_records([rows[2], rows[4]], rows[0], lambda name: '%s: records differ from the NV12 row\'s' % name)
R.check_records([rows[3]], rows[1], lambda name: '%s: records differ from the I420 row\'s' % name)
print('%d of %d frames read; the 16-bit rows\' records == their 8-bit rows\'' % (ok, R.N))
print('match kernel: %s; dial kernel of the last 16-bit call: %s' % (ctx.last_match()['kernel'], ctx.last_dials()))
times = R.alternate(rows, fr.rotated)
kern = R.kernel_times(rows)

fr.print_table('%d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps' % (B, W, H, R.NB, args.rounds, args.steps),
               rows, times, rows[0], fr.kernel_columns(kern), name=('row', 42), vs=('vs NV12', 7))
frame16 = rows420 * W * 2
print('bytes per frame: NV12 %d, P010 %d; the reduce pass reads %d and writes %d of them per frame, the prep kernel reads the crop only'
      % (rows420 * W, frame16, frame16, rows420 * W))
R.close()
