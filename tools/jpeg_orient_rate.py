#!/usr/bin/env python3
"""JPEG files that carry an EXIF orientation, decoded and read on the GPU (melf_ctx_set_jpeg_orientation: the entropy decoder and the
IDCT as ever, k_jpeg_color_exif writes each pixel where the upright frame has it) against upright files through the same call --
the floor -- and against what such files cost before: the host branch of get_meter_values, Pillow decode + exif_transpose on the
default METERELF_DECODE_THREADS, then MeterReader.read_many on the rotated frames.
One process, 1024-file calls at config 3 (sample-images1 params, upright 640 x 480), file bytes in host memory, the pointer table
built once (what a compiled host pays per call).  The files: --distinct (256) frames per kind -- fixture frame i % K rolled by its
shift, as the frame-format tools make theirs --, the stored frame un-oriented in numpy and encoded at quality 95 with the tag; a
call's 1024 files are a window of that ring, --nbuf (4) windows in rotation.  Every call decodes 1024 x 921 600 bytes of frames, far
beyond the 256 MB cache.

    python3 tools/jpeg_orient_rate.py [--steps 8] [--warmup 4] [--rounds 5] [--batch 1024] [--nbuf 4] [--distinct 256] [--host-steps 2]

Rows:
    (a)  upright files (no tag), melf_jpeg_process_batch, the switch on (what get_meter_values runs)
    (a0) the same files, the switch off: the call as it was before the switch existed
    (b6) the same content stored under orientation 6 (rot90cw), the switch on        (b3) under orientation 3 (rot180)
    (c6) / (c3) the host branch for the files of (b6) / (b3): imread_bgr on a thread pool, then read_many
Before anything is timed the records of (b6), (b3) and (a) are compared, byte for byte, with the host branch's for the SAME files
(the re-encoded frames differ from kind to kind, so each kind has its own reference), and (a)'s with (a0)'s.
The GPU rows take turns, R rounds of K calls each; the host rows run --host-steps calls once.  Then a few calls of each GPU row with
every kernel bracketed by events: the colour stage's time per call (k_jpeg_color: k_jpeg_color420 for upright files,
k_jpeg_color_exif for the others), beside the Huffman and IDCT stages'."""
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import frame_rates as fr

sys.path.insert(0, os.path.join(fr.ROOT, 'tests'))
import jpeg_orient_cases as jc  # noqa: E402  (the files and the orientation table the tests use)

ap = fr.arg_parser(steps=8, warmup=4, rounds=5, batch=1024, nbuf=4)
ap.add_argument('--distinct', type=int, default=256)
ap.add_argument('--host-steps', type=int, default=2)
args = ap.parse_args()
(B, NB, D) = (args.batch, args.nbuf, args.distinct)
_hip = fr._hip
tmp = __import__('tempfile').mkdtemp(prefix='jpeg_orient_rate_')

params = fr._params.load(os.path.join(jc.GOLDEN, 'sample-images1', 'params.yml'))
base = [fr.imread_bgr(f) for f in jc.golden_files()]
shapes = [b.shape for b in base]
base = [b for b in base if b.shape == max(set(shapes), key=shapes.count)]
(H, W) = base[0].shape[:2]
shifts = np.random.default_rng(3).integers(-8, 9, size=(D, 2))
KINDS = {'a': None, 'b6': 6, 'b3': 3}
files = {k: [] for k in KINDS}
paths = {k: [] for k in KINDS}
t0 = time.perf_counter()
for i in range(D):
    rgb = np.ascontiguousarray(np.roll(base[i % len(base)], (int(shifts[i, 1]), int(shifts[i, 0])), axis=(0, 1))[:, :, ::-1])
    for (k, code) in KINDS.items():
        data = jc.stored_under(rgb, code, quality=95)
        files[k].append(data)
        p = os.path.join(tmp, '%s_%04d.jpg' % (k, i))
        with open(p, 'wb') as fh:
            fh.write(data)
        paths[k].append(p)
print('%d distinct files per kind encoded in %.1f s; mean size upright %.0f, under 6 %.0f, under 3 %.0f bytes' % (
    D, time.perf_counter() - t0, *(np.mean([len(f) for f in files[k]]) for k in KINDS)))

reader = fr._engine.MeterReader(params, jpeg_orientation=True)
ctx = reader.ctx
L = ctx._L


def window(k, kind):
    return [(kind[(k * 97 + i) % D]) for i in range(B)]     # call k's 1024 files: a window of the ring


tables = {k: [_hip._file_table(window(j, files[k])) for j in range(NB)] for k in KINDS}
out = np.zeros(B, _hip.RESULT_DTYPE)
status = np.zeros(B, np.int32)


def gpu_row(kind, switch):
    def fn(i):
        ctx.set_jpeg_orientation(switch)
        (ptrs, sizes, _keep) = tables[kind][i % NB]
        _hip.check(L.melf_jpeg_process_batch(ctx._h, ptrs, sizes, B, H, W, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        assert (status == 0).all(), (kind, switch, np.flatnonzero(status)[:8], status[status != 0][:8])
    return fn


nthreads = max(1, int(os.getenv('METERELF_DECODE_THREADS', str(min(8, os.cpu_count() or 1)))))
pool = ThreadPoolExecutor(max_workers=nthreads)


def host_row(kind):
    def fn(i):
        frames = list(pool.map(fr.imread_bgr, window(i % NB, paths[kind])))
        out[:] = np.array(reader.read_many(frames), dtype=_hip.RESULT_DTYPE)
    return fn


gpu_rows = [('(a)  upright files, switch on', gpu_row('a', True)), ('(a0) upright files, switch off', gpu_row('a', False)),
            ('(b6) stored under 6 (rot90cw), switch on', gpu_row('b6', True)), ('(b3) stored under 3 (rot180), switch on', gpu_row('b3', True))]
host_rows = [('(c6) host branch for the files of (b6), %d threads' % nthreads, host_row('b6')),
             ('(c3) host branch for the files of (b3), %d threads' % nthreads, host_row('b3'))]

# ---- the records first: every GPU row against the host branch of the same files (and (a0) against (a)) ----
def records(fn, k):
    fn(k)
    return out.copy()


for (g, h) in ((gpu_rows[2], host_rows[0]), (gpu_rows[3], host_rows[1])):
    (r_g, r_h) = (records(g[1], 1), records(h[1], 1))
    assert r_g.tobytes() == r_h.tobytes(), '%s: records differ from the host branch\'s' % g[0]
    print('%s: %d of %d files read; the records == the host branch\'s' % (g[0][:4], int((r_g['status'] == _hip.FRAME_OK).sum()), B))
(r_a, r_a0) = (records(gpu_rows[0][1], 1), records(gpu_rows[1][1], 1))
assert r_a.tobytes() == r_a0.tobytes(), '(a): records differ between the switch on and off'
frames_a = list(pool.map(fr.imread_bgr, window(1, paths['a'])))
assert r_a.tobytes() == np.array(reader.read_many(frames_a), dtype=_hip.RESULT_DTYPE).tobytes(), '(a): records differ from the host branch\'s'
print('(a) : %d of %d files read; the records == the host branch\'s and (a0)\'s' % (int((r_a['status'] == _hip.FRAME_OK).sum()), B))
del frames_a


def run(fn, steps):
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    return (time.perf_counter() - t0) / steps * 1e3


for (_n, fn) in gpu_rows:
    run(fn, args.warmup)
times = {n: [] for (n, _f) in gpu_rows + host_rows}
for r in range(args.rounds):
    for (n, fn) in fr.rotated(gpu_rows, r):
        run(fn, 1)
        times[n].append(run(fn, args.steps))
for (n, fn) in host_rows:
    times[n] = [run(fn, 1) for _ in range(args.host_steps)]

# ---- the stages of a call, every kernel bracketed by events ----
kern = {}
ctx.set_profiling(1)
for (n, fn) in gpu_rows:
    run(fn, 2)
    ctx.timings()
    calls = 2 * NB
    run(fn, calls)
    kern[n] = {k: ms / calls for (k, (ms, cnt)) in ctx.timings().items() if cnt}     # per CALL (a call launches a stage once per chunk)
ctx.set_profiling(0)
for (n, _f) in host_rows:
    kern[n] = {}
cols = [('%s ms' % k, len(k) + 3, lambda name, k=k: '%.4f' % kern[name].get(k, 0.0)) for k in ('k_jpeg_huff', 'k_jpeg_idct', 'k_jpeg_color')]
fr.print_table('%d-file calls, upright %dx%d, %d windows of %d distinct files in rotation, %d rounds x %d calls; kernel columns: ms per call'
               % (B, W, H, NB, D, args.rounds, args.steps), gpu_rows + host_rows, times, gpu_rows[0], cols, name=('row', 52), vs=('vs (a)', 8))
med = {n: float(np.median(t)) for (n, t) in times.items()}
(a, a0, b6, b3) = (med[n] for (n, _f) in gpu_rows)
(c6, c3) = (med[n] for (n, _f) in host_rows)
print('(a) %.4f ms a call = %.0f files/s; (a)/(a0) %.3f' % (a, B / a * 1e3, a / a0))
for (tag, b, c, n) in (('6', b6, c6, gpu_rows[2][0]), ('3', b3, c3, gpu_rows[3][0])):
    print('orientation %s: (b) %.4f ms a call = %.0f files/s; (b)/(a) %.3f; host branch (c) %.1f ms a call = %.0f files/s; (c)/(b) %.1f; colour stage %.4f ms a call against %.4f for upright files'
          % (tag, b, B / b * 1e3, b / a, c, B / c * 1e3, c / b, kern[n].get('k_jpeg_color', 0.0), kern[gpu_rows[0][0]].get('k_jpeg_color', 0.0)))
pool.shutdown()
reader.close()
for k in paths:
    for p in paths[k]:
        os.remove(p)
os.rmdir(tmp)
