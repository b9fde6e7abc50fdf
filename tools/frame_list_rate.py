#!/usr/bin/env python3
"""Frames in separate allocations (melf_process_frame_list_dev: one gather of the meter crop's rows, then the unchanged kernels)
against the contiguous batch read in place -- the floor, unchanged code -- and against what callers do today: torch.stack of the
list into one array, then the batch read.  BGR (melf_frames), NV12 (melf_yuv_frames) and P010 (melf_yuv16_frames).
tools/packed32_rate.py's method: one process, 1024-frame steps at config 3 (640 x 480, sample-images1 params), frames resident in
HBM, --nbuf (4) distinct batches in rotation -- 4 x 1024 frames twice over (the contiguous array and the list's own allocations),
well beyond the 256 MB cache --, consecutive steps alternating between two caller streams, records to a device buffer, the region
between two device synchronisations on the wall clock.

    python3 tools/frame_list_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

Rows, per format:
    (a) the contiguous batch read in place (melf_process_*_dev)
    (b) the same frames as a list of separate allocations (each frame a tensor of its own, cloned in shuffled order) through
        melf_process_frame_list_dev
    (c) torch.stack of that list into a scratch batch on the call's stream, then (a) on the scratch batch
    (d) the gather kernel of (b) alone (melf_gather_frame_list_dev of the diagnostic build: the pointer table goes up, k_gather_rows
        runs, nothing is read)
Before anything is timed the list row's records of every batch are compared, byte for byte, with the contiguous row's.  The rows
take turns, R rounds of K steps each after W untimed steps of each.  Then a few steps of each with every kernel bracketed by events:
the gather kernel's (k_gather), the prep kernel's (k_lplane) and the dial reader's (k_dials) time per launch; the gather's bytes --
the crop's rows read once and written once -- over its time, beside the bare 3:1 stream of melf_stream_probe_dev in the same run.
The table's ratio column is against the first row, BGR (a); the closing lines give each format's own (b)/(a), (c)/(b) and (b) - (a).
Runs on the diagnostic build (the product's code + the two measurement entry points): MELF_LIB_PATH names another."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault('MELF_LIB_PATH', os.path.join(ROOT, 'meterelf_amd', 'csrc', 'libmeterelf_hip_diag.so'))

import numpy as np  # noqa: E402

import frame_rates as fr  # noqa: E402

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W, NB) = (R.B, R.H, R.W, R.NB)
torch = fr.torch
rows420 = fr.yuv_rows(H, 1, 1)

bgr = R.empty(H, W, 3)
nv12 = R.empty(rows420, W)
p010 = R.empty(rows420, W, 2)      # the two bytes of a little-endian sample
for (i0, src) in R.chunks():
    (Y, U, V) = fr.encode(src, 1, 1, 'bt709')
    m = len(src)
    bgr[i0:i0 + m] = src
    fr.write_yuv(nv12[i0:i0 + m], Y, U, V, semi=True)
    p010[i0:i0 + m, ..., 1] = nv12[i0:i0 + m]                      # value << 8
    p010[i0:i0 + m, ..., 0] = 0
    del src, Y, U, V
torch.cuda.synchronize()
p010s = p010.view(torch.int16).squeeze(-1)                         # (N, rows, W) samples, the same bits

ctx = R.open()
assert hasattr(fr._hip.lib(), 'melf_gather_frame_list_dev'), 'frame_list_rate.py needs the diagnostic build (make -C meterelf_amd/csrc diag; MELF_LIB_PATH)'
vb = fr._hip.frames_view(bgr[:B], 'bgr')
formats = {
    'BGR': ('views', bgr, vb, fr._hip.MelfFrames(vb.pixel_format, B, H, W, vb.row_pitch, vb.frame_stride), ctx._L.melf_process_frames_dev),
    'NV12': ('yuv', nv12) + (lambda v: (v, v.descriptor()))(fr._hip.yuv_frames_view(nv12[:B], 'nv12', 'bt709')) + (ctx._L.melf_process_yuv_dev,),
    'P010': ('yuv16', p010s) + (lambda v: (v, v.descriptor()))(fr._hip.yuv16_frames_view(p010s[:B], 'p010', 'bt709')) + (ctx._L.melf_process_yuv16_dev,),
}
order = np.random.default_rng(5).permutation(R.N)
rows = []
keep = []
moved = {}
for (name, (layout, arr, v, desc, entry)) in formats.items():
    assert not v.copied
    # the list: every frame a tensor of its own, allocated in shuffled order; one pointer table per batch
    singles = [None] * R.N
    for i in order:
        singles[int(i)] = arr[int(i)].clone()
    tables = [(C.c_void_p * B)(*[t.data_ptr() for t in singles[k * B:(k + 1) * B]]) for k in range(NB)]
    assert len({b.data_ptr() - a.data_ptr() for (a, b) in zip(singles, singles[1:])}) > 1, 'the frames lie one stride apart'
    scratch = [torch.empty_like(arr[:B]) for _s in R.streams]
    keep.append((singles, tables, scratch))
    batch_bytes = B * v.frame_stride

    def step_a(i, stream, arr=arr, desc=desc, entry=entry, batch_bytes=batch_bytes):
        k = i % NB
        ctx._dev(entry, arr.data_ptr() + k * batch_bytes, desc, R.d_res.data_ptr() + k * B * R.rsz, False, stream.cuda_stream)

    def step_b(i, stream, layout=layout, desc=desc, tables=tables):
        k = i % NB
        ctx.process_frame_list_dev(layout, desc, tables[k], d_results_ptr=R.d_res.data_ptr() + k * B * R.rsz, want_host=False, stream=stream.cuda_stream)

    def step_c(i, stream, singles=singles, scratch=scratch, desc=desc, entry=entry):
        k = i % NB
        out = scratch[R.streams.index(stream)]
        with torch.cuda.stream(stream):
            torch.stack(singles[k * B:(k + 1) * B], out=out)
        ctx._dev(entry, out.data_ptr(), desc, R.d_res.data_ptr() + k * B * R.rsz, False, stream.cuda_stream)

    def step_d(i, stream, name=name, layout=layout, desc=desc, tables=tables):
        moved[name] = ctx.gather_frame_list_dev(layout, desc, tables[i % NB], stream=stream.cuda_stream)

    rows += [('%s (a) contiguous, %s' % (name, entry.__name__), step_a), ('%s (b) list, melf_process_frame_list_dev' % name, step_b),
             ('%s (c) torch.stack + %s' % (name, entry.__name__), step_c), ('%s (d) gather kernel alone' % name, step_d)]

ok = 0
for f in range(len(formats)):
    ok = R.check_records([rows[4 * f + 1], rows[4 * f + 2]], rows[4 * f], lambda name: '%s: records differ from the contiguous row\'s' % name)
    print('%s: %d of %d frames read; the list row\'s and the stack row\'s records == the contiguous row\'s' % (rows[4 * f][0].split()[0], ok, R.N))
print('match kernel: %s; dial kernel of the last call: %s' % (ctx.last_match()['kernel'], ctx.last_dials()))
times = R.alternate(rows, fr.rotated)
kern = R.kernel_times(rows)

# the bare 3:1 stream of the diagnostic build over the first BGR batch, in the same run
probe_out = torch.empty(B * H * W, dtype=torch.uint8, device=R.dev)
in_bytes = B * H * W * 3
ctx.set_profiling(1)
for i in range(12):
    if i == 4:
        torch.cuda.synchronize()
        ctx.timings()
    ctx.stream_probe_dev(bgr.data_ptr() + (i % NB) * in_bytes, in_bytes, probe_out.data_ptr(), 0, stream=R.streams[0].cuda_stream)
torch.cuda.synchronize()
(pms, pn) = ctx.timings()['k_stream_probe']
ctx.set_profiling(0)
probe_gbps = (in_bytes // (48 * 1024)) * 64 * 1024 / (pms / max(pn, 1) * 1e-3) / 1e9


def gather_gbps(name):
    fmt = name.split()[0]
    ms = kern[name].get('k_gather', 0.0)
    return '%.0f' % (moved[fmt] / (ms * 1e-3) / 1e9) if ms and '(d)' in name else ''


cols = [('k_gather ms', 11, lambda name: '%.4f' % kern[name].get('k_gather', 0.0))] + fr.kernel_columns(kern) + [('gather GB/s', 11, gather_gbps)]
fr.print_table('%d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps' % (B, W, H, NB, args.rounds, args.steps),
               rows, times, rows[0], cols, name=('row', 50), vs=('vs (a)', 7))
med = {name: float(np.median(t)) for (name, t) in times.items()}
for f in range(len(formats)):
    (a, b, c, d) = (med[rows[4 * f + k][0]] for k in range(4))
    fmt = rows[4 * f][0].split()[0]
    g = kern[rows[4 * f + 3][0]].get('k_gather', 0.0)
    print('%s: (b)/(a) %.3f   (c)/(b) %.2f   (b)-(a) %.4f ms, (d) %.4f ms a step, its kernel %.4f ms; the gather moves %.1f MB a step (read + write), '
          'the stack %.1f MB; gather %.0f GB/s = %.2f of the bare stream\'s %.0f GB/s'
          % (fmt, b / a, c / b, b - a, d, g, moved[fmt] / 1e6, 2 * B * formats[fmt][2].frame_stride / 1e6,
             moved[fmt] / (g * 1e-3) / 1e9 if g else 0.0, (moved[fmt] / (g * 1e-3) / 1e9 / probe_gbps) if g else 0.0, probe_gbps))
R.close()
