#!/usr/bin/env python3
"""RGB frames of wide samples in separate allocations (melf_process_wide_list_dev: k_narrow_list_rows takes every frame's address from
a table) and wide planar frames whose planes are (melf_process_wide_plane_list_dev: k_narrow_plane_rows) against the wide batch read
in place (melf_process_wide_dev, k_narrow_rows) and against what a caller with such a list does without them: torch.stack of the
frames -- or of the planes -- into one batch on the call's stream, then the batch read.  16-bit words, float16 and float32; packed
(H, W, 3) and planar (3, H, W) frames.
tools/wide_rate.py's method: one process, 1024-frame steps at config 3 (640 x 480, sample-images1 params), everything resident in
HBM, --nbuf (4) distinct batches in rotation -- well beyond the 256 MB cache --, consecutive steps alternating between two caller
streams, records to a device buffer, the region between two device synchronisations on the wall clock.

    python3 tools/wide_list_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

One group of rows per sample type and layout, each measured on its own (its frames are freed before the next group's are made):
    (a) the wide batch in place, melf_process_wide_dev
    (b) the same frames as a list of one-allocation frames (each a tensor of its own, cloned in shuffled order), melf_process_wide_list_dev
    (c) planar only: the same samples as a list of planes (every plane a tensor of its own), melf_process_wide_plane_list_dev
    (d) torch.stack of the listed frames into one batch per caller stream, then (a) on it
    (e) planar only: torch.stack of the listed planes into one batch per caller stream, then (a) on it
Before anything of a group is timed the records of every other row, of every batch, are compared byte for byte with (a)'s.  The
rows take turns, R rounds of K steps each after W untimed steps of each.  Then a few steps of each with every kernel bracketed by
events: the narrowing kernel's time per launch (entry k_gather of melf_ctx_timings), the prep kernel's and the dial reader's.  The
closing lines give (b)/(a), (c)/(b), (d)/(b) and (e)/(c) of every group, with the spread of (a)'s own turns."""
import ctypes as C

import numpy as np

import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W, NB) = (R.B, R.H, R.W, R.NB)
torch = fr.torch
_hip = fr._hip

packed8 = R.empty(H, W, 3)      # R G B
planar8 = R.empty(3, H, W)
for (i0, src) in R.chunks():
    m = len(src)
    packed8[i0:i0 + m] = src.flip(3)
    fr.write_planes(planar8[i0:i0 + m], src)
    del src
torch.cuda.synchronize()
ctx = R.open()


def widen(frames8, kind):
    """the 8-bit frames as wide samples of `kind`, on the device, chunk by chunk (tools/wide_rate.py's)"""
    if kind == 'u16':
        out = torch.zeros(frames8.shape + (2,), dtype=torch.uint8, device=R.dev)   # the two bytes of a little-endian word: value << 8
        for i0 in range(0, R.N, 256):
            out[i0:i0 + 256, ..., 1] = frames8[i0:i0 + 256]
        return out.view(torch.int16).squeeze(-1)
    out = torch.empty(frames8.shape, dtype=torch.float16 if kind == 'f16' else torch.float32, device=R.dev)
    for i0 in range(0, R.N, 256):
        out[i0:i0 + 256] = frames8[i0:i0 + 256].to(torch.float32) / 255.0
    return out


def results(k):
    return R.d_res.data_ptr() + k * B * R.rsz


order = np.random.default_rng(5).permutation(R.N)
summary = []
for kind in ('u16', 'f16', 'f32'):
    for (layout, frames8) in (('hwc', packed8), ('chw', planar8)):
        planar = layout == 'chw'
        wide = widen(frames8, kind)
        torch.cuda.synchronize()
        shift = dict(shift=8) if kind == 'u16' else {}
        v = _hip.wide_frames_view(wide[:B], layout, 'rgb', **shift)
        desc = v.descriptor()
        batch_bytes = B * v.frame_stride
        ldesc = _hip.MelfWideFrames.from_buffer_copy(desc)
        ldesc.frame_stride = 0
        pdesc = _hip.MelfWideFrames.from_buffer_copy(ldesc)
        (pdesc.b_offset, pdesc.g_offset, pdesc.r_offset) = (0, 0, 0)
        # the frame list: every frame a tensor of its own; the plane list: every plane one; both allocated in shuffled order
        singles = [None] * R.N
        planes = [None] * R.N
        for i in order:
            singles[int(i)] = wide[int(i)].clone()
            if planar:
                planes[int(i)] = tuple(wide[int(i)][k].clone() for k in range(3))   # R, G, B: the array's order
        assert len({b.data_ptr() - a.data_ptr() for (a, b) in zip(singles, singles[1:])}) > 1, 'the frames lie one stride apart'
        frame_tables = [(C.c_void_p * B)(*[t.data_ptr() for t in singles[k * B:(k + 1) * B]]) for k in range(NB)]
        # plane slots 0 / 1 / 2 = B / G / R
        plane_tables = [(C.c_void_p * (3 * B))(*[t[s].data_ptr() for t in planes[k * B:(k + 1) * B] for s in (2, 1, 0)]) for k in range(NB)] if planar else None
        scratch = [torch.empty((B,) + tuple(wide.shape[1:]), dtype=wide.dtype, device=R.dev) for _s in R.streams]
        step_a = R.step(ctx.process_wide_dev, wide, batch_bytes, desc)

        def step_b(i, stream):
            k = i % NB
            ctx.process_wide_list_dev(ldesc, frame_tables[k], d_results_ptr=results(k), want_host=False, stream=stream.cuda_stream)

        def step_c(i, stream):
            k = i % NB
            ctx.process_wide_plane_list_dev(pdesc, plane_tables[k], 3, d_results_ptr=results(k), want_host=False, stream=stream.cuda_stream)

        def step_d(i, stream):
            k = i % NB
            s = R.streams.index(stream)
            with torch.cuda.stream(stream):
                torch.stack(singles[k * B:(k + 1) * B], out=scratch[s])
            ctx.process_wide_dev(scratch[s].data_ptr(), desc, d_results_ptr=results(k), want_host=False, stream=stream.cuda_stream)

        def step_e(i, stream):
            k = i % NB
            s = R.streams.index(stream)
            with torch.cuda.stream(stream):
                torch.stack([p for t in planes[k * B:(k + 1) * B] for p in t], out=scratch[s].view(3 * B, H, W))
            ctx.process_wide_dev(scratch[s].data_ptr(), desc, d_results_ptr=results(k), want_host=False, stream=stream.cuda_stream)

        tag = '%s %s' % (kind, layout)
        rows = [('(a) %s batch, melf_process_wide_dev' % tag, step_a), ('(b) %s frame list, melf_process_wide_list_dev' % tag, step_b)]
        if planar:
            rows.append(('(c) %s plane list, melf_process_wide_plane_list_dev' % tag, step_c))
        rows.append(('(d) %s torch.stack of the frames + (a)' % tag, step_d))
        if planar:
            rows.append(('(e) %s torch.stack of the planes + (a)' % tag, step_e))
        ok = R.check_records(rows[1:], rows[0], lambda name: '%s: records differ from row (a)\'s' % name)
        assert 4 * ok >= 3 * R.N, '%s: only %d of %d frames read' % (tag, ok, R.N)
        print('%s: %d of %d frames read; the records of the other rows == row (a)\'s' % (tag, ok, R.N))
        times = R.alternate(rows, fr.rotated)
        kern = R.kernel_times(rows)
        cols = [('k_gather ms', 11, lambda name: '%.4f' % kern[name].get('k_gather', 0.0))] + fr.kernel_columns(kern)
        fr.print_table('%s: %d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps'
                       % (tag, B, W, H, NB, args.rounds, args.steps), rows, times, rows[0], cols, name=('row', 62), vs=('vs (a)', 7))
        med = {name[:3]: float(np.median(times[name])) for (name, _fn) in rows}
        ta = times[rows[0][0]]
        summary.append((tag, med, min(ta), max(ta)))
        del wide, singles, planes, scratch, frame_tables, plane_tables, rows, step_a, step_b, step_c, step_d, step_e, v   # (the steps hold the frames)
        torch.cuda.empty_cache()

print('ratios of the medians:')
for (tag, med, lo, hi) in summary:
    line = '  %-8s (b)/(a) %.3f   (d)/(b) %.2f' % (tag, med['(b)'] / med['(a)'], med['(d)'] / med['(b)'])
    if '(c)' in med:
        line += '   (c)/(b) %.3f   (e)/(c) %.2f' % (med['(c)'] / med['(b)'], med['(e)'] / med['(c)'])
    line += '   (a) %.4f ms, its turns %.4f..%.4f' % (med['(a)'], lo, hi)
    if med['(d)'] < med['(b)'] or med.get('(e)', med.get('(c)', 0.0)) < med.get('(c)', 0.0):
        line += '  -- the list read does NOT beat stack-and-read here'
    print(line)
R.close()
