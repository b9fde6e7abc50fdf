#!/usr/bin/env python3
"""RGB frames of wide samples in place (melf_process_wide_dev: 16-bit words, float16, float32; packed (N, H, W, 3) and planar
(N, 3, H, W)) against the 8-bit frames of the same samples through melf_process_frames_dev / melf_process_planes_dev -- the yardstick
-- and against what a caller does without it: torch's conversion of every whole frame to uint8 (x.mul(255).round().clamp(0, 255) to
uint8, or >> 8 for 16-bit words, on the call's stream) followed by the 8-bit read.  tools/packed32_rate.py's method: one process,
1024-frame steps at config 3 (640 x 480, sample-images1 params), frames resident in HBM, --nbuf (4) distinct batches in rotation --
well beyond the 256 MB cache --, consecutive steps alternating between two caller streams, records to a device buffer, the region
between two device synchronisations on the wall clock.

    python3 tools/wide_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

All rows are made from the same synthetic pictures.  A 16-bit word holds the 8-bit value in its high byte (shift 8), a float the
value / 255 rounded to its type: all three narrow back to the 8-bit frames' own samples.  One group of four rows per sample type and
layout, each measured on its own (the wide frames of one group are freed before the next is made):
    (a) the 8-bit batch in place    (b) the wide batch, melf_process_wide_dev    (c) torch's conversion + (a)    and the conversion alone
Before anything of a group is timed -- the check's own steps are the first the device sees of it -- the records of (b) and (c) of
every batch are compared, byte for byte, with (a)'s.  The rows take turns, R rounds of K steps each after W untimed steps of each.
Then a few steps of each with every kernel bracketed by events: the narrowing kernel's (k_narrow_rows, timed as k_gather), the prep
kernel's (k_lplane) and the dial reader's (k_dials) time per step.  Prints a table per group with each row's ratio to (a), and at
the end (b) / (a) and (c) / (b) of every group."""
import numpy as np

import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W) = (R.B, R.H, R.W)
torch = fr.torch

packed8 = R.empty(H, W, 3)      # R G B
planar8 = R.empty(3, H, W)
for (i0, src) in R.chunks():
    m = len(src)
    packed8[i0:i0 + m] = src.flip(3)
    fr.write_planes(planar8[i0:i0 + m], src)
    del src
torch.cuda.synchronize()

ctx = R.open()
v_packed = fr._hip.frames_view(packed8[:B], 'rgb')
v_planar = fr._hip.planar_frames_view(planar8[:B], 'rgb')
assert not v_packed.copied and not v_planar.copied


def step_packed8_from(frames, batch_bytes):
    """fn(i, stream): the 8-bit packed read of batch i % nbuf of `frames` (batch_bytes 0: of the one scratch batch)"""
    return R.step(ctx.process_frames_dev, frames, batch_bytes, v_packed.pixel_format, B, H, W, v_packed.row_pitch, v_packed.frame_stride)


def step_planar8_from(frames, batch_bytes):
    return R.step(ctx.process_planes_dev, frames, batch_bytes, v_planar.descriptor())


def widen(frames8, kind):
    """the 8-bit frames as wide samples of `kind`, on the device, chunk by chunk"""
    if kind == 'u16':
        out = torch.zeros(frames8.shape + (2,), dtype=torch.uint8, device=R.dev)   # the two bytes of a little-endian word: value << 8
        for i0 in range(0, R.N, 256):
            out[i0:i0 + 256, ..., 1] = frames8[i0:i0 + 256]
        return out.view(torch.int16).squeeze(-1)
    out = torch.empty(frames8.shape, dtype=torch.float16 if kind == 'f16' else torch.float32, device=R.dev)
    for i0 in range(0, R.N, 256):
        out[i0:i0 + 256] = frames8[i0:i0 + 256].to(torch.float32) / 255.0
    return out


summary = []
kern_cols = [(title, len(title), None) for title in ('k_gather ms', 'k_lplane ms', 'k_dials ms')]
for kind in ('u16', 'f16', 'f32'):
    for (layout, frames8, step8_from) in (('hwc', packed8, step_packed8_from), ('chw', planar8, step_planar8_from)):
        wide = widen(frames8, kind)
        torch.cuda.synchronize()
        shift = dict(shift=8) if kind == 'u16' else {}
        v = fr._hip.wide_frames_view(wide[:B], layout, 'rgb', **shift)
        step_a = step8_from(frames8, B * (v_packed if layout == 'hwc' else v_planar).frame_stride)
        step_b = R.step(ctx.process_wide_dev, wide, B * v.frame_stride, v.descriptor())
        # what callers do today: every whole frame converted to uint8 by torch on the call's stream, then the 8-bit read; one scratch
        # batch per caller stream
        scratch = [torch.empty((B,) + tuple(frames8.shape[1:]), dtype=torch.uint8, device=R.dev) for _s in R.streams]
        reads = [step8_from(s, 0) for s in scratch]

        def step_convert(i, stream):
            with torch.cuda.stream(stream):
                w = wide[(i % R.NB) * B:(i % R.NB + 1) * B]
                out = scratch[R.streams.index(stream)]
                if kind == 'u16':
                    out.copy_(w >> 8)                 # (an int16 holding the word: the cast to uint8 keeps the high byte)
                else:
                    out.copy_(w.mul(255).round_().clamp_(0, 255))

        def step_c(i, stream):
            step_convert(i, stream)
            reads[R.streams.index(stream)](i, stream)

        name8 = 'melf_process_frames_dev' if layout == 'hwc' else 'melf_process_planes_dev'
        tag = '%s %s' % (kind, layout)
        rows = [('(a) %s uint8, %s' % (tag, name8), step_a), ('(b) %s, melf_process_wide_dev' % tag, step_b),
                ('(c) %s -> uint8 pass + %s' % (tag, name8), step_c), ('    %s -> uint8 pass (conversion alone)' % tag, step_convert)]
        ok = R.check_records(rows[1:3], rows[0], lambda name: '%s: records differ from row (a)\'s' % name)
        assert 4 * ok >= 3 * R.N, '%s: only %d of %d frames read' % (tag, ok, R.N)
        print('%s: %d of %d frames read; the wide rows\' records == the 8-bit row\'s' % (tag, ok, R.N))
        R.run(step_b, 1)
        print('%s: match kernel: %s; dial kernel of the last wide call: %s' % (tag, ctx.last_match()['kernel'], ctx.last_dials()))
        times = R.alternate(rows, fr.rotated)
        kern = R.kernel_times(rows)
        cols = [(t, w, lambda name, k=k: '%.4f' % kern[name].get(k, 0.0)) for ((t, w, _f), k) in zip(kern_cols, ('k_gather', 'k_lplane', 'k_dials'))]
        fr.print_table('%s: %d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps'
                       % (tag, B, W, H, R.NB, args.rounds, args.steps), rows, times, rows[0], cols, name=('row', 50), vs=('vs (a)', 7))
        (a, b, c) = (float(np.median(times[rows[k][0]])) for k in range(3))
        summary.append((tag, b / a, c / b, wide.element_size()))
        del wide, scratch, reads, rows, step_a, step_b, step_c, step_convert, v   # (the steps hold the frames)
        torch.cuda.empty_cache()

print('(b) / (a) and (c) / (b), medians:')
for (tag, ba, cb, ss) in summary:
    print('  %-8s (b) takes %.3f times (a); (c) takes %.3f times (b)%s' % (tag, ba, cb, '' if cb > 1.0 else '  -- the wide read does NOT beat convert-and-read here'))
print('bytes per frame: uint8 %d, 16-bit %d, float32 %d; the conversion pass reads a whole frame and writes %d, the narrowing kernel reads the crop only'
      % (H * W * 3, H * W * 6, H * W * 12, H * W * 3))
R.close()
