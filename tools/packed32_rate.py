#!/usr/bin/env python3
"""4:4:4 frames of one 32-bit word per pixel in place (melf_process_packed32_dev: VUYA, Y410, X2RGB10) against BGRA through
melf_process_frames_dev -- the same bytes per pixel, the yardstick -- and against what a caller does without it: a torch pass that
unpacks every whole Y410 frame to three 8-bit planes (the top 8 bits of each 10-bit field: three shift-and-mask passes over the
frame's words on the call's stream) followed by the planar 4:4:4 read (melf_process_yuv_planar_dev on i444).  tools/yuv422_10_rate.py's
method: one process, 1024-frame steps at config 3 (640 x 480, sample-images1 params), frames resident in HBM, --nbuf (4) distinct
batches in rotation -- 4 x 1024 x 1.2 MB, well beyond the 256 MB cache --, consecutive steps alternating between two caller streams,
records to a device buffer, the region between two device synchronisations on the wall clock.

    python3 tools/packed32_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

All rows are made from the same synthetic pictures: encoded to 4:4:4 (float BT.709 limited range) and read under 'bt709'; the RGB
rows (BGRA, X2RGB10) hold the BGR frames the header's integer conversion makes of those samples, so that every row's records are the
same records.  A 10-bit field holds the 8-bit value times four.  Before anything is timed -- the check's own steps are the first
the device sees -- the records of every row of every batch are compared, byte for byte, with the i444 row's (the unpack-and-read
row: its read is melf_process_yuv_planar_dev on the i444 frames of the samples).  The rows take turns, R rounds of K steps each after
W untimed steps of each.  Then a few steps of each with every kernel bracketed by events: the prep kernel's (k_lplane) and the dial
reader's (k_dials) time per step (the unpack pass is torch's kernels, not the library's: its time is the last row's step, the pass
alone).  Prints a table with each row's ratio to the BGRA row of the same run, and the in-place rows' ratio to the unpack-and-read
row."""
import numpy as np

import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)
torch = fr.torch

bgra = R.empty(H, W, 4)
words = {fmt: torch.empty((R.N, H, W), dtype=torch.int32, device=R.dev) for fmt in ('vuya', 'y410', 'x2rgb10')}
for (i0, src) in R.chunks():
    (Y, U, V) = fr.encode(src, 0, 0, 'bt709')
    m = len(src)
    bgr = fr.to_bgr(Y, U, V, 0, 0, 3).to(torch.int32)
    (y, u, v) = (Y.to(torch.int32), U.to(torch.int32), V.to(torch.int32))
    bgra[i0:i0 + m, ..., :3] = bgr.to(torch.uint8)
    bgra[i0:i0 + m, ..., 3] = 255
    words['vuya'][i0:i0 + m] = v | (u << 8) | (y << 16) | (0x7f << 24)                    # bytes V U Y A
    words['y410'][i0:i0 + m] = (u << 2) | (y << 12) | (v << 22) | (1 << 30)               # U bits 0-9, Y 10-19, V 20-29, A 30-31
    words['x2rgb10'][i0:i0 + m] = (bgr[..., 0] << 2) | (bgr[..., 1] << 12) | (bgr[..., 2] << 22) | (1 << 30)   # B bits 0-9, G 10-19, R 20-29
    del src, Y, U, V, y, u, v, bgr
torch.cuda.synchronize()

ctx = R.open()
v4 = fr._hip.frames_view(bgra[:B], 'bgra')
views = {fmt: fr._hip.packed32_frames_view(words[fmt][:B], fmt, 'bt709' if fmt != 'x2rgb10' else None) for fmt in words}
assert not v4.copied and not any(v.copied for v in views.values())


def step_bgra(i, stream):
    k = i % R.NB
    ctx.process_frames_dev(bgra.data_ptr() + k * B * v4.frame_stride, v4.pixel_format, B, H, W, v4.row_pitch, v4.frame_stride,
                           d_results_ptr=R.d_res.data_ptr() + k * B * R.rsz, want_host=False, stream=stream.cuda_stream)


steps32 = {fmt: R.step(ctx.process_packed32_dev, words[fmt], B * views[fmt].frame_stride, views[fmt].descriptor()) for fmt in words}

# what callers do today: every Y410 frame unpacked to the three planes of an i444 frame by a pass over the whole frame, then the
# planar 4:4:4 read; one scratch batch per caller stream
scratch = [torch.empty((B, 3 * H, W), dtype=torch.uint8, device=R.dev) for _s in R.streams]
d_today = fr._hip.yuv_planar_frames_view(scratch[0], 'i444', 'bt709').descriptor()


def step_unpack(i, stream):
    with torch.cuda.stream(stream):
        w = words['y410'][(i % R.NB) * B:(i % R.NB + 1) * B]
        out = scratch[R.streams.index(stream)].view(B, 3, H, W)
        for (k, pos) in enumerate((12, 2, 22)):
            out[:, k] = (w >> pos) & 255


def step_today(i, stream):
    step_unpack(i, stream)
    # (the records go to batch i % nbuf's slice, as R.step has it; the frames are the stream's scratch batch)
    ctx.process_yuv_planar_dev(scratch[R.streams.index(stream)].data_ptr(), d_today,
                               d_results_ptr=R.d_res.data_ptr() + (i % R.NB) * B * R.rsz, want_host=False, stream=stream.cuda_stream)


rows = [('BGRA, melf_process_frames_dev', step_bgra), ('VUYA, melf_process_packed32_dev', steps32['vuya']),
        ('Y410, melf_process_packed32_dev', steps32['y410']), ('X2RGB10, melf_process_packed32_dev', steps32['x2rgb10']),
        ('Y410 -> i444 pass + melf_process_yuv_planar_dev', step_today), ('Y410 -> i444 pass (unpacking alone)', step_unpack)]
ok = R.check_records(rows[:4], rows[4], lambda name: '%s: records differ from the i444 row\'s' % name)
print('%d of %d frames read; the in-place rows\' records == the i444 row\'s' % (ok, R.N))
print('match kernel: %s; dial kernel of the last call: %s' % (ctx.last_match()['kernel'], ctx.last_dials()))
times = R.alternate(rows, fr.rotated)
kern = R.kernel_times(rows)

fr.print_table('%d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps' % (B, W, H, R.NB, args.rounds, args.steps),
               rows, times, rows[0], fr.kernel_columns(kern), name=('row', 48), vs=('vs BGRA', 7))
today = float(np.median(times[rows[4][0]]))
print('the unpack-and-read row takes %s times the VUYA, Y410 and X2RGB10 rows' % ', '.join('%.2f' % (today / float(np.median(times[rows[k][0]]))) for k in (1, 2, 3)))
print('bytes per frame: every layout %d; the unpack pass reads them and writes %d per frame, the prep kernel reads the crop only' % (H * W * 4, H * W * 3))
R.close()
