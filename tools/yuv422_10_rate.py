#!/usr/bin/env python3
"""Packed 10-bit YUV 4:2:2 frames in place (melf_process_yuv422_10_dev: v210, Y210) against the same pictures as 8-bit UYVY through
melf_process_yuv422_dev, and against what a caller does without it: a torch pass that unpacks every whole v210 frame to UYVY (the top
8 bits of each 10-bit field: three shift-and-mask passes over the frame's words on the call's stream; the fields of a group already
lie in UYVY order) followed by the UYVY read.  tools/yuv16_rate.py's method: one process, 1024-frame steps at config 3 (640 x 480,
sample-images1 params), frames resident in HBM, --nbuf (4) distinct batches in rotation, consecutive steps alternating between two
caller streams, records to a device buffer, the region between two device synchronisations on the wall clock.

    python3 tools/yuv422_10_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

All rows are made from the same synthetic pictures (float BT.709 limited range, the chroma pair's mean) and read under 'bt709'.  A
v210 field holds the 8-bit value times four, a Y210 word the value in its high byte: both reduce to the UYVY row's samples, so before
anything is timed the 10-bit rows' records of every batch are compared, byte for byte, with the UYVY row's.  The v210 rows have the
conventional pitch, ((W + 47) / 48) * 128 bytes.  The rows take turns, R rounds of K steps each after W untimed steps.  Then a few
steps of each with every kernel bracketed by events: the prep kernel's (k_lplane) and the dial reader's (k_dials) time per step
(the unpack pass is torch's kernels, not the library's: its time is the last row's step, the pass alone).  Prints a table with each
row's ratio to the UYVY row of the same run."""
import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)
torch = fr.torch
G = (W + 5) // 6                      # groups of a v210 row
PW = (W + 47) // 48 * 32              # words of a v210 row at the conventional pitch

uyvy = R.empty(H, W, 2)
v210 = torch.zeros((R.N, H, PW), dtype=torch.int32, device=R.dev)
y210 = R.empty(H, W, 2, 2)            # the two bytes of a little-endian word, the words Y0 U Y1 V
for (i0, src) in R.chunks():
    (Y, U, V) = fr.encode(src, 1, 0, 'bt709')
    m = len(src)
    fr.write_422(uyvy[i0:i0 + m], Y, U, V, 'uyvy')
    # the twelve fields of a group in order are U Y V Y U Y V Y U Y V Y: the UYVY bytes, times four, three to a word
    f = torch.zeros((m, H, 12 * G), dtype=torch.int32, device=R.dev)
    f[:, :, :2 * W] = uyvy[i0:i0 + m].reshape(m, H, 2 * W).to(torch.int32) << 2
    f = f.reshape(m, H, 4 * G, 3)
    v210[i0:i0 + m, :, :4 * G] = f[..., 0] | (f[..., 1] << 10) | (f[..., 2] << 20)
    y210[i0:i0 + m, :, :, 0, 1] = Y                              # value << 8
    y210[i0:i0 + m, :, 0::2, 1, 1] = U
    y210[i0:i0 + m, :, 1::2, 1, 1] = V
    y210[i0:i0 + m, ..., 0] = 0
    del src, Y, U, V, f
torch.cuda.synchronize()
y210s = y210.view(torch.int16).squeeze(-1)   # (N, H, W, 2) words, the same bits

ctx = R.open()
v8 = fr._hip.yuv422_frames_view(uyvy[:B], 'uyvy', 'bt709')
vv = fr._hip.yuv422_10_frames_view(v210[:B], 'v210', 'bt709', width=W)
vy = fr._hip.yuv422_10_frames_view(y210s[:B], 'y210', 'bt709')
assert not (v8.copied or vv.copied or vy.copied)
step_uyvy = R.step(ctx.process_yuv422_dev, uyvy, B * v8.frame_stride, v8.descriptor())
step_v210 = R.step(ctx.process_yuv422_10_dev, v210, B * vv.frame_stride, vv.descriptor())
step_y210 = R.step(ctx.process_yuv422_10_dev, y210s, B * vy.frame_stride, vy.descriptor())

# what callers do today: every v210 frame unpacked to UYVY by a pass over the whole frame, then the UYVY read; one scratch batch per
# caller stream (whole groups: the read looks at the first 2 W bytes of a row)
scratch = [torch.empty((B, H, 12 * G), dtype=torch.uint8, device=R.dev) for _s in R.streams]
d_today = fr._hip.MelfYuv422Frames(fr._hip.YUV422_UYVY, fr._hip.YUV_BT709_LIMITED, B, H, W, 0, 12 * G, H * 12 * G)
assert (12 * G) % 4 == 0


def step_unpack(i, stream):
    with torch.cuda.stream(stream):
        words = v210[(i % R.NB) * B:(i % R.NB + 1) * B, :, :4 * G]
        out = scratch[R.streams.index(stream)].view(B, H, 4 * G, 3)
        for k in range(3):
            out[..., k] = (words >> (10 * k + 2)) & 255


def step_today(i, stream):
    step_unpack(i, stream)
    # (the records go to batch i % nbuf's slice, as R.step has it; the frames are the stream's scratch batch)
    ctx.process_yuv422_dev(scratch[R.streams.index(stream)].data_ptr(), d_today,
                           d_results_ptr=R.d_res.data_ptr() + (i % R.NB) * B * R.rsz, want_host=False, stream=stream.cuda_stream)


rows = [('UYVY, melf_process_yuv422_dev', step_uyvy), ('v210, melf_process_yuv422_10_dev', step_v210),
        ('Y210, melf_process_yuv422_10_dev', step_y210), ('v210 -> UYVY pass + melf_process_yuv422_dev', step_today),
        ('v210 -> UYVY pass (unpacking alone)', step_unpack)]
ok = R.check_records([rows[3], rows[1], rows[2]], rows[0], lambda name: '%s: records differ from the UYVY row\'s' % name)
print('%d of %d frames read; the 10-bit rows\' records == the UYVY row\'s' % (ok, R.N))
print('match kernel: %s; dial kernel of the last 10-bit call: %s' % (ctx.last_match()['kernel'], ctx.last_dials()))
times = R.alternate(rows, fr.rotated)
kern = R.kernel_times(rows)

fr.print_table('%d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps' % (B, W, H, R.NB, args.rounds, args.steps),
               rows, times, rows[0], fr.kernel_columns(kern), name=('row', 44), vs=('vs UYVY', 7))
print('bytes per frame: UYVY %d, v210 %d (pitch %d), Y210 %d; the unpack pass reads %d and writes %d of them per frame, the prep kernel reads the crop only'
      % (H * W * 2, H * PW * 4, PW * 4, H * W * 4, H * G * 16, H * G * 12))
R.close()
