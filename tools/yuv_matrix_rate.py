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
import os

import frame_rates as fr

ap = fr.arg_parser()
ap.add_argument('--matrix', default=','.join(fr._hip.YUV_MATRIX_CODES))
ap.add_argument('--encode', choices=('bt601', 'own'), default='bt601')
args = ap.parse_args()
names = [m for m in args.matrix.split(',') if m]
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)


def make_nv12(enc):
    out = R.empty(H * 3 // 2, W)
    for (i0, src) in R.chunks():
        fr.write_yuv(out[i0:i0 + len(src)], *fr.encode(src, 1, 1, enc), semi=True)
    return out


frames = {}
for name in names:
    enc = name if args.encode == 'own' else 'bt601'
    if enc not in frames:
        frames[enc] = make_nv12(enc)
    frames[name] = frames[enc]
nv12 = frames[names[0]]
fr.torch.cuda.synchronize()

ctx = R.open()
batch_bytes = B * fr._hip.yuv_frames_view(nv12[:B], 'nv12').frame_stride
rows = [(m, R.step(ctx.process_yuv_dev, frames[m], batch_bytes, fr._hip.yuv_frames_view(nv12[:B], 'nv12', m).descriptor())) for m in names]
print('library: %s; frames encoded with %s' % (os.environ.get('MELF_LIB_PATH', 'the package\'s'), 'each row\'s own matrix' if args.encode == 'own' else 'bt601'))
ok = {}
for (name, fn) in rows:
    R.d_res.zero_()
    R.run(fn, R.NB)
    ok[name] = int((R.d_res.cpu().numpy().view(fr._hip.RESULT_DTYPE)['status'] == fr._hip.FRAME_OK).sum())
print('match kernel: %s' % ctx.last_match()['kernel'])
times = R.alternate(rows, fr.forward_reversed)
kern = R.kernel_times(rows)

fr.print_table('%d-frame steps, %dx%d NV12, %d batches in rotation (%.2f GB), two caller streams, %d rounds x %d steps'
               % (B, W, H, R.NB, nv12.numel() / 1e9, args.rounds, args.steps), rows, times, rows[0],
               fr.kernel_columns(kern) + [('frames read', 11, lambda name: '%4d / %4d' % (ok[name], R.N))],
               name=('matrix', 12), vs=('vs %s' % names[0][:6], 9))
R.close()
