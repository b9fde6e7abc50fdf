#!/usr/bin/env python3
"""YUYV (packed YUV 4:2:2) frames in place against packed BGR frames, bench.py's method: 1024-frame steps at config 3 (640 x 480, sample-images1
params), frames resident in HBM, --nbuf (4) distinct batches in rotation (more than the Infinity Cache holds), consecutive steps
alternating between two caller streams, records to a device buffer, the region between two device synchronisations on the wall
clock (bench.py: timed_steps).

    python3 tools/yuv422_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

The YUYV frames are made from the synthetic BGR frames (float BT.601 limited range, the mean of each horizontal pixel pair for
chroma); the BGR frames that are timed are the conversion of include/meterelf_hip.h of those YUYV frames, so that both rows read the same pictures and their
records can be compared (they are, byte for byte, before anything is timed).  The rows take turns, R rounds of K steps each after
W untimed steps.  Then a few steps of each with every kernel bracketed by events: the prep kernel's (k_lplane) and the dial
reader's (k_dials) time per step.  Prints a table and the prep kernel's algorithmic bytes per frame."""
import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)
yuyv = R.empty(H, W, 2)
bgr = R.empty(H, W, 3)
for (i0, src) in R.chunks():
    (Y, U, V) = fr.encode(src, 1, 0)
    fr.write_422(yuyv[i0:i0 + len(src)], Y, U, V, 'yuyv')
    bgr[i0:i0 + len(src)] = fr.to_bgr(Y, U, V, 1, 0)
    del src, Y, U, V
fr.torch.cuda.synchronize()

ctx = R.open()
view = fr._hip.yuv422_frames_view(yuyv[:B], 'yuyv')
assert not view.copied

rows = [('BGR, melf_process_batch_dev', R.step(ctx.process_batch_dev, bgr, B * H * W * 3, B, H, W)),
        ('YUYV, melf_process_yuv422_dev', R.step(ctx.process_yuv422_dev, yuyv, B * view.frame_stride, view.descriptor()))]
ok = R.check_records(rows[1:], rows[0], lambda name: '%s records differ from the BGR records' % name.split(',')[0])
print('frames read: %d of %d; YUYV records == BGR records' % (ok, R.N))
print('match kernel: %s' % ctx.last_match()['kernel'])
times = R.alternate(rows, fr.forward_reversed)
kern = R.kernel_times(rows)

P = ctx.params
(x0, x1) = (min(P.rect_x0, W), min(P.rect_x1, W))
(y0, y1) = (min(P.rect_y0, H), min(P.rect_y1, H))
(cr, cc) = (y1 - y0, x1 - x0)
mpx = ((x1 - 1) >> 1) - (x0 >> 1) + 1   # macropixels a crop row touches
alg = {'BGR': cr * cc * 3, 'YUYV': cr * mpx * 4}
fr.print_table('%d-frame steps, %dx%d, %d batches in rotation (BGR %.2f GB, YUYV %.2f GB), two caller streams, %d rounds x %d steps'
               % (B, W, H, R.NB, bgr.numel() / 1e9, yuyv.numel() / 1e9, args.rounds, args.steps), rows, times, rows[0],
               fr.kernel_columns(kern) + [('prep bytes read/frame', 22, lambda name: '%d' % alg[name.split(',')[0]])], name=('row', 30))
R.close()
