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
import numpy as np

import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)
torch = fr.torch

# name -> (pixel_format, sub_x, sub_y); the arrays are the raw-video (N, rows, W) layout
LAYOUTS = {'NV12': ('nv12', 1, 1), 'I422': ('i422', 1, 0), 'NV16': ('nv16', 1, 0), 'I444': ('i444', 0, 0), 'NV24': ('nv24', 0, 0)}
arrays = {name: R.empty(fr.yuv_rows(H, sx, sy), W) for (name, (_f, sx, sy)) in LAYOUTS.items()}
bgr = R.empty(H, W, 3)
for (i0, src) in R.chunks():
    for (name, (_f, sx, sy)) in LAYOUTS.items():
        (Y, U, V) = fr.encode(src, sx, sy)
        fr.write_yuv(arrays[name][i0:i0 + len(src)], Y, U, V, semi=name.startswith('NV'))
        if name == 'I444':
            bgr[i0:i0 + len(src)] = fr.to_bgr(Y, U, V, 0, 0)
    del src, Y, U, V
torch.cuda.synchronize()

ctx = R.open()
steps = {}
for (name, (fmt, _sx, _sy)) in LAYOUTS.items():
    view = fr._hip.yuv_frames_view(arrays[name][:B], fmt) if name == 'NV12' else fr._hip.yuv_planar_frames_view(arrays[name][:B], fmt)
    assert not view.copied
    steps[name] = R.step(ctx.process_yuv_dev if name == 'NV12' else ctx.process_yuv_planar_dev, arrays[name], B * view.frame_stride, view.descriptor())

rows = [('BGR, melf_process_batch_dev', R.step(ctx.process_batch_dev, bgr, B * H * W * 3, B, H, W)), ('NV12, melf_process_yuv_dev', steps['NV12'])]
rows += [('%s, melf_process_yuv_planar_dev' % name, steps[name]) for name in ('I422', 'NV16', 'I444', 'NV24')]
# the records: every YUV row's first batch against process_batch_dev of the header's conversion of its own planes
for (name, (fmt, sx, sy)) in LAYOUTS.items():
    own = fr.to_bgr(*fr.yuv_planes(arrays[name][:B], H, sx, sy, semi=name.startswith('NV')), sx, sy).contiguous()
    torch.cuda.synchronize()
    want = ctx.process_batch_dev(own.data_ptr(), B, H, W)
    R.d_res.zero_()
    steps[name](0, R.streams[0])
    torch.cuda.synchronize()
    got = R.d_res[:B].cpu().numpy().tobytes()
    assert got == want.tobytes(), '%s records differ from the records of its BGR conversion' % name
    if name == 'NV12':
        v = fr._hip.yuv_planar_frames_view(arrays[name][:B], fmt)
        assert ctx.process_yuv_planar_dev(v.ptr, v.descriptor()).tobytes() == got, 'NV12: the two entry points differ'
    ok = int((want['status'] == fr._hip.FRAME_OK).sum())
    print('%s: %d of %d frames of the first batch read; records == those of its BGR conversion' % (name, ok, B))
    del own
print('match kernel: %s' % ctx.last_match()['kernel'])
times = R.alternate(rows, fr.forward_reversed)
kern = R.kernel_times(rows)

t_nv12 = float(np.median(times[rows[1][0]]))
fr.print_table('%d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps' % (B, W, H, R.NB, args.rounds, args.steps),
               rows, times, rows[0], [('vs NV12', 7, lambda name: '%.3fx' % (float(np.median(times[name])) / t_nv12))] + fr.kernel_columns(kern),
               name=('row', 36))
R.close()
