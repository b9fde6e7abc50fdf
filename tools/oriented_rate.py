#!/usr/bin/env python3
"""Frames stored rotated or mirrored (melf_process_oriented_dev: one kernel, k_orient_tiles, writes the meter crop of every frame
upright into a staged batch, then the unchanged kernels) against the upright batch read in place -- the floor, unchanged code --
and against what callers do today: torch.rot90 / torch.flip of every whole stored frame into an upright batch, then the batch read.
BGR under orientations 3 (rot180) and 6 (rot90cw), BGRA, NV12 and P010 under 6.
tools/frame_list_rate.py's method: one process, 1024-frame steps at config 3 (640 x 480, sample-images1 params), frames resident in
HBM, --nbuf (4) distinct batches in rotation -- 4 x 1024 frames twice over (the upright array and the stored one), well beyond the
256 MB cache --, consecutive steps alternating between two caller streams, records to a device buffer, the region between two device
synchronisations on the wall clock.

    python3 tools/oriented_rate.py [--steps 20] [--warmup 30] [--rounds 5] [--batch 1024] [--nbuf 4]

Rows, per format and orientation (the stored batch is the upright one under the inverse orientation, plane by plane):
    (a) the upright batch read in place (melf_process_*_dev)
    (b) the stored batch through melf_process_oriented_dev
    (c) torch.rot90 / torch.flip of the whole stored frames, every plane, copied into an upright scratch batch on the call's stream
        (what .contiguous() does), then (a) on the scratch batch
    (d) a frame list of the upright frames through melf_process_frame_list_dev: its k_gather time is the plain-copy kernel
        (k_gather_rows) moving the same bytes in the same run
Before anything is timed the records of (b), (c) and (d) of every batch are compared, byte for byte, with (a)'s.  The rows take
turns, R rounds of K steps each after W untimed steps of each.  Then a few steps of each with every kernel bracketed by events: the
k_gather column is k_orient_tiles in rows (b) and k_gather_rows in rows (d), per launch.  The table's ratio column is against the
first row; the closing lines give each case's own (b)/(a), (c)/(b), (b) - (a) and the kernels' ratio orient / gather."""
import ctypes as C

import numpy as np

import frame_rates as fr

args = fr.arg_parser().parse_args()
R = fr.Rates(args)
(B, H, W, NB) = (R.B, R.H, R.W, R.NB)
torch = fr.torch
rows420 = fr.yuv_rows(H, 1, 1)
INVERSE = {6: 8, 8: 6}   # every other code is its own inverse


def orient(a, code):
    """the oriented frames of stored frames a (N, rows, cols, ...): the table of include/meterelf_hip.h, as views"""
    return {1: lambda: a, 2: lambda: a.flip(2), 3: lambda: a.flip(1, 2), 4: lambda: a.flip(1), 5: lambda: a.transpose(1, 2),
            6: lambda: torch.rot90(a, -1, (1, 2)), 7: lambda: a.flip(1, 2).transpose(1, 2), 8: lambda: torch.rot90(a, 1, (1, 2))}[code]()


def planes420(a, h):
    """(Y, the interleaved chroma plane as (N, h / 2, w / 2, 2)) of a raw-video (N, h * 3 / 2, w) array: views"""
    return a[:, :h], a[:, h:].unflatten(2, (a.shape[2] // 2, 2))


bgr = R.empty(H, W, 3)
bgra = R.empty(H, W, 4)
nv12 = R.empty(rows420, W)
p010 = R.empty(rows420, W, 2)      # the two bytes of a little-endian sample
for (i0, src) in R.chunks():
    (Y, U, V) = fr.encode(src, 1, 1, 'bt709')
    m = len(src)
    bgr[i0:i0 + m] = src
    bgra[i0:i0 + m, ..., :3] = src
    bgra[i0:i0 + m, ..., 3] = 255
    fr.write_yuv(nv12[i0:i0 + m], Y, U, V, semi=True)
    p010[i0:i0 + m, ..., 1] = nv12[i0:i0 + m]                      # value << 8
    p010[i0:i0 + m, ..., 0] = 0
    del src, Y, U, V
torch.cuda.synchronize()
p010s = p010.view(torch.int16).squeeze(-1)                         # (N, rows, W) samples, the same bits


def store_packed(up, code):
    return orient(up, INVERSE.get(code, code)).contiguous()


def store420(up, code):
    (hs, ws) = (W, H) if code >= 5 else (H, W)
    out = torch.empty((R.N, hs * 3 // 2, ws), dtype=up.dtype, device=R.dev)
    for (dst, src) in zip(planes420(out, hs), planes420(up, H)):
        dst.copy_(orient(src, INVERSE.get(code, code)))
    return out


def upright_packed(stored, code, out):
    out.copy_(orient(stored, code))


def upright420(stored, code, out):
    hs = stored.shape[1] * 2 // 3
    for (dst, src) in zip(planes420(out, H), planes420(stored, hs)):
        dst.copy_(orient(src, code))


ctx = R.open()
hip = fr._hip
L = ctx._L


def packed_desc(arr, fmt):
    v = hip.frames_view(arr[:B], fmt)
    return v, hip.MelfFrames(v.pixel_format, B, v.H, v.W, v.row_pitch, v.frame_stride)


def view_desc(v):
    return v, v.descriptor()


# name: (layout, upright array, (view, descriptor) of an array's first batch, the family's _dev entry, store, upright)
cases = [
    ('BGR rot180', 3, 'views', bgr, lambda a: packed_desc(a, 'bgr'), L.melf_process_frames_dev, store_packed, upright_packed),
    ('BGR rot90cw', 6, 'views', bgr, lambda a: packed_desc(a, 'bgr'), L.melf_process_frames_dev, store_packed, upright_packed),
    ('BGRA rot90cw', 6, 'views', bgra, lambda a: packed_desc(a, 'bgra'), L.melf_process_frames_dev, store_packed, upright_packed),
    ('NV12 rot90cw', 6, 'yuv', nv12, lambda a: view_desc(hip.yuv_frames_view(a[:B], 'nv12', 'bt709')), L.melf_process_yuv_dev, store420, upright420),
    ('P010 rot90cw', 6, 'yuv16', p010s, lambda a: view_desc(hip.yuv16_frames_view(a[:B], 'p010', 'bt709')), L.melf_process_yuv16_dev, store420, upright420),
]
rows = []
keep = []
for (name, code, layout, up, describe, entry, store, upright) in cases:
    (v_up, d_up) = describe(up)
    stored = store(up, code)
    (v_st, d_st) = describe(stored)
    assert not v_up.copied and not v_st.copied
    scratch = [torch.empty_like(up[:B]) for _s in R.streams]
    tables = [(C.c_void_p * B)(*[up.data_ptr() + (k * B + i) * v_up.frame_stride for i in range(B)]) for k in range(NB)]
    keep.append((stored, scratch, tables))
    (up_bytes, st_bytes) = (B * v_up.frame_stride, B * v_st.frame_stride)

    def step_a(i, stream, up=up, d_up=d_up, entry=entry, up_bytes=up_bytes):
        k = i % NB
        ctx._dev(entry, up.data_ptr() + k * up_bytes, d_up, R.d_res.data_ptr() + k * B * R.rsz, False, stream.cuda_stream)

    def step_b(i, stream, layout=layout, d_st=d_st, code=code, stored=stored, st_bytes=st_bytes):
        k = i % NB
        ctx.process_oriented_dev(layout, d_st, code, stored.data_ptr() + k * st_bytes, d_results_ptr=R.d_res.data_ptr() + k * B * R.rsz, want_host=False,
                                 stream=stream.cuda_stream)

    def step_c(i, stream, stored=stored, scratch=scratch, code=code, upright=upright, d_up=d_up, entry=entry):
        k = i % NB
        out = scratch[R.streams.index(stream)]
        with torch.cuda.stream(stream):
            upright(stored[k * B:(k + 1) * B], code, out)
        ctx._dev(entry, out.data_ptr(), d_up, R.d_res.data_ptr() + k * B * R.rsz, False, stream.cuda_stream)

    def step_d(i, stream, layout=layout, d_up=d_up, tables=tables):
        k = i % NB
        ctx.process_frame_list_dev(layout, d_up, tables[k], d_results_ptr=R.d_res.data_ptr() + k * B * R.rsz, want_host=False, stream=stream.cuda_stream)

    rows += [('%s (a) upright, %s' % (name, entry.__name__), step_a), ('%s (b) stored, melf_process_oriented_dev' % name, step_b),
             ('%s (c) torch rot90/flip + %s' % (name, entry.__name__), step_c), ('%s (d) upright list, melf_process_frame_list_dev' % name, step_d)]

for f in range(len(cases)):
    ok = R.check_records(rows[4 * f + 1:4 * f + 4], rows[4 * f], lambda name: '%s: records differ from the upright row\'s' % name)
    print('%s: %d of %d frames read; the records of (b), (c) and (d) == the upright row\'s' % (cases[f][0], ok, R.N))
print('match kernel: %s; dial kernel of the last call: %s' % (ctx.last_match()['kernel'], ctx.last_dials()))
times = R.alternate(rows, fr.rotated)
kern = R.kernel_times(rows)

cols = [('k_gather ms', 11, lambda name: '%.4f' % kern[name].get('k_gather', 0.0))] + fr.kernel_columns(kern)
fr.print_table('%d-frame steps, %dx%d upright, %d batches in rotation, two caller streams, %d rounds x %d steps' % (B, W, H, NB, args.rounds, args.steps),
               rows, times, rows[0], cols, name=('row', 58), vs=('vs (a)', 7))
med = {name: float(np.median(t)) for (name, t) in times.items()}
for f in range(len(cases)):
    (a, b, c, d) = (med[rows[4 * f + k][0]] for k in range(4))
    (ko, kg) = (kern[rows[4 * f + 1][0]].get('k_gather', 0.0), kern[rows[4 * f + 3][0]].get('k_gather', 0.0))
    print('%s: (b)/(a) %.3f   (c)/(b) %.2f   (b)-(a) %.4f ms   (d)/(a) %.3f; k_orient_tiles %.4f ms, k_gather_rows %.4f ms a launch: orient / gather %.2f'
          % (cases[f][0], b / a, c / b, b - a, d / a, ko, kg, ko / kg if kg else 0.0))
R.close()
