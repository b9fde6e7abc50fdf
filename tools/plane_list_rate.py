#!/usr/bin/env python3
"""A frame's planes in separate allocations (melf_process_plane_list_dev: one copy kernel, k_plane_rows, takes run k of every
frame from the frame's k-th pointer, then the unchanged kernels) against the frame list of one-allocation frames
(melf_process_frame_list_dev), against the contiguous batch read in place, and against what a caller with separate planes does
today: concatenate every frame's planes into one allocation, then the frame list.  NV12 and I420 (melf_yuv_frames), P010
(melf_yuv16_frames) and planar RGB (melf_planar_frames).
tools/frame_list_rate.py's method: one process, 1024-frame steps at config 3 (640 x 480, sample-images1 params), everything
resident in HBM, --nbuf (4) distinct batches in rotation -- 4 x 1024 frames three times over (the contiguous array, the frames'
own allocations, the planes' own allocations), well beyond the 256 MB cache --, consecutive steps alternating between two caller
streams, records to a device buffer, the region between two device synchronisations on the wall clock.

    python3 tools/plane_list_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

Rows, per format:
    (a) the contiguous batch read in place (melf_process_*_dev)
    (b) the same frames as a list of one-allocation frames (each a tensor of its own, cloned in shuffled order) through
        melf_process_frame_list_dev
    (c) the same samples as a list of planes (every plane a tensor of its own, cloned in shuffled order) through
        melf_process_plane_list_dev
    (d) what a caller does today: torch.cat of each frame's planes into a frame allocation of its own on the call's stream, then (b)
        on those
(A row (e), (c) as one k_gather_rows launch per plane, would need a one-plane descriptor per plane and an entry point that stages
without reading; it is not arranged.)
Before anything is timed the records of rows (b), (c) and (d) of every batch are compared, byte for byte, with the contiguous
row's.  The rows take turns, R rounds of K steps each after W untimed steps of each.  Then a few steps of each with every kernel
bracketed by events: the copy kernel's time per launch (entry k_gather of melf_ctx_timings: k_gather_rows in (b) and (d),
k_plane_rows in (c)), the prep kernel's and the dial reader's.  The table's ratio column is against each format's own (a); the
closing lines give each format's (c)/(b) with the spread of (b), (d)/(c) and (b)/(a)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import frame_rates as fr  # noqa: E402

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W, NB) = (R.B, R.H, R.W, R.NB)
torch = fr.torch
_hip = fr._hip
rows420 = fr.yuv_rows(H, 1, 1)

nv12 = R.empty(rows420, W)
i420 = R.empty(rows420, W)
p010 = R.empty(rows420, W, 2)      # the two bytes of a little-endian sample
rgb = R.empty(3, H, W)
for (i0, src) in R.chunks():
    (Y, U, V) = fr.encode(src, 1, 1, 'bt709')
    m = len(src)
    fr.write_yuv(nv12[i0:i0 + m], Y, U, V, semi=True)
    fr.write_yuv(i420[i0:i0 + m], Y, U, V, semi=False)
    p010[i0:i0 + m, ..., 1] = nv12[i0:i0 + m]                      # value << 8
    p010[i0:i0 + m, ..., 0] = 0
    fr.write_planes(rgb[i0:i0 + m], src)
    del src, Y, U, V
torch.cuda.synchronize()
p010s = p010.view(torch.int16).squeeze(-1)                         # (N, rows, W) samples, the same bits


def planes420(frame, semi):
    """the plane slots (Y, interleaved chroma) / (Y, U, V) of one raw-video 4:2:0 frame (rows, W): views"""
    if semi:
        return (frame[:H], frame[H:])
    c = frame[H:].reshape(-1)
    q = (H // 2) * (W // 2)
    return (frame[:H], c[:q].reshape(H // 2, W // 2), c[q:].reshape(H // 2, W // 2))


def plane_descriptor(desc, offsets):
    d = type(desc).from_buffer_copy(desc)
    d.frame_stride = 0
    for (name, value) in offsets.items():
        setattr(d, name, value)
    return d


ctx = R.open()
L = ctx._L
formats = {
    # name: (layout, the contiguous array, its view, the batch entry point, frame -> plane slots, the plane offsets of the plane list)
    'NV12': ('yuv', nv12, _hip.yuv_frames_view(nv12[:B], 'nv12', 'bt709'), L.melf_process_yuv_dev, lambda f: planes420(f, True),
             {'u_offset': 0, 'v_offset': 1}),
    'I420': ('yuv', i420, _hip.yuv_frames_view(i420[:B], 'i420', 'bt709'), L.melf_process_yuv_dev, lambda f: planes420(f, False),
             {'u_offset': 0, 'v_offset': 0}),
    'P010': ('yuv16', p010s, _hip.yuv16_frames_view(p010s[:B], 'p010', 'bt709'), L.melf_process_yuv16_dev, lambda f: planes420(f, True),
             {'u_offset': 0, 'v_offset': 2}),
    'RGB planes': ('planar', rgb, _hip.planar_frames_view(rgb[:B], 'rgb'), L.melf_process_planes_dev, lambda f: (f[2], f[1], f[0]),
                   {'b_offset': 0, 'g_offset': 0, 'r_offset': 0}),
}
order = np.random.default_rng(5).permutation(R.N)
rows = []
keep = []
for (name, (layout, arr, v, entry, slots, offsets)) in formats.items():
    assert not v.copied
    desc = v.descriptor()
    pdesc = plane_descriptor(desc, offsets)
    # the frame list: every frame a tensor of its own; the plane list: every plane one; both allocated in shuffled order
    singles = [None] * R.N
    planes = [None] * R.N
    for i in order:
        singles[int(i)] = arr[int(i)].clone()
        planes[int(i)] = tuple(p.clone() for p in slots(arr[int(i)]))
    np_ = len(planes[0])
    frame_tables = [(C.c_void_p * B)(*[t.data_ptr() for t in singles[k * B:(k + 1) * B]]) for k in range(NB)]
    plane_tables = [(C.c_void_p * (B * np_))(*[p.data_ptr() for t in planes[k * B:(k + 1) * B] for p in t]) for k in range(NB)]
    assert len({b.data_ptr() - a.data_ptr() for (a, b) in zip(singles, singles[1:])}) > 1, 'the frames lie one stride apart'
    assert len({b[1].data_ptr() - a[1].data_ptr() for (a, b) in zip(planes, planes[1:])}) > 1, 'the planes lie one stride apart'
    # row (d): per caller stream B frame allocations to concatenate into, and their pointer table.  The concatenation lays the
    # planes in raw-video order (for RGB planes: R, G, B, the array's), which is the contiguous descriptor's
    cat_order = (lambda t: (t[2], t[1], t[0])) if layout == 'planar' else (lambda t: t)
    scratch = [[torch.empty(arr[0].numel(), dtype=arr.dtype, device=R.dev) for _i in range(B)] for _s in R.streams]
    scratch_tables = [(C.c_void_p * B)(*[t.data_ptr() for t in s]) for s in scratch]
    keep.append((singles, planes, frame_tables, plane_tables, scratch, scratch_tables))
    batch_bytes = B * v.frame_stride

    def step_a(i, stream, arr=arr, desc=desc, entry=entry, batch_bytes=batch_bytes):
        k = i % NB
        ctx._dev(entry, arr.data_ptr() + k * batch_bytes, desc, R.d_res.data_ptr() + k * B * R.rsz, False, stream.cuda_stream)

    def step_b(i, stream, layout=layout, desc=desc, tables=frame_tables):
        k = i % NB
        ctx.process_frame_list_dev(layout, desc, tables[k], d_results_ptr=R.d_res.data_ptr() + k * B * R.rsz, want_host=False, stream=stream.cuda_stream)

    def step_c(i, stream, layout=layout, pdesc=pdesc, tables=plane_tables, np_=np_):
        k = i % NB
        ctx.process_plane_list_dev(layout, pdesc, tables[k], np_, d_results_ptr=R.d_res.data_ptr() + k * B * R.rsz, want_host=False, stream=stream.cuda_stream)

    def step_d(i, stream, layout=layout, desc=desc, planes=planes, scratch=scratch, scratch_tables=scratch_tables, cat_order=cat_order):
        k = i % NB
        s = R.streams.index(stream)
        with torch.cuda.stream(stream):
            for (j, t) in enumerate(planes[k * B:(k + 1) * B]):
                torch.cat([p.reshape(-1) for p in cat_order(t)], out=scratch[s][j])
        ctx.process_frame_list_dev(layout, desc, scratch_tables[s], d_results_ptr=R.d_res.data_ptr() + k * B * R.rsz, want_host=False, stream=stream.cuda_stream)

    rows += [('%s (a) contiguous, %s' % (name, entry.__name__), step_a), ('%s (b) frame list, melf_process_frame_list_dev' % name, step_b),
             ('%s (c) plane list, melf_process_plane_list_dev' % name, step_c), ('%s (d) torch.cat per frame + frame list' % name, step_d)]

for f in range(len(formats)):
    ok = R.check_records(rows[4 * f + 1:4 * f + 4], rows[4 * f], lambda name: '%s: records differ from the contiguous row\'s' % name)
    print('%s: %d of %d frames read; the records of rows (b), (c) and (d) == the contiguous row\'s' % (rows[4 * f][0].split(' (')[0], ok, R.N))
print('match kernel: %s; dial kernel of the last call: %s' % (ctx.last_match()['kernel'], ctx.last_dials()))
times = R.alternate(rows, fr.rotated)
kern = R.kernel_times(rows)

cols = [('copy kernel ms', 14, lambda name: '%.4f' % kern[name].get('k_gather', 0.0))] + fr.kernel_columns(kern)
for f in range(len(formats)):
    block = rows[4 * f:4 * f + 4]
    fr.print_table('%s: %d-frame steps, %dx%d, %d batches in rotation, two caller streams, %d rounds x %d steps'
                   % (block[0][0].split(' (')[0], B, W, H, NB, args.rounds, args.steps),
                   block, times, block[0], cols, name=('row', 52), vs=('vs (a)', 7))
med = {name: float(np.median(t)) for (name, t) in times.items()}
for f in range(len(formats)):
    (a, b, c, d) = (med[rows[4 * f + k][0]] for k in range(4))
    tb = times[rows[4 * f + 1][0]]
    fmt = rows[4 * f][0].split(' (')[0]
    inside = min(tb) <= c <= max(tb)
    print('%s: (c)/(b) %.3f   (d)/(c) %.2f   (b)/(a) %.3f   (c) %.4f ms against (b) %.4f ms, spread of (b) %.4f..%.4f: (c) lies %s it'
          % (fmt, c / b, d / c, b / a, c, b, min(tb), max(tb), 'inside' if inside else 'outside'))
R.close()
