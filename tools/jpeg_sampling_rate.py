#!/usr/bin/env python3
"""YCbCr 4:4:0 and 4:1:1 JPEG files decoded and read on the GPU (melf_ctx_set_jpeg_samplings: the entropy decoder and the IDCT as
ever, the general colour kernel k_jpeg_color with the two new upsamplers) against 4:2:2 files of the same content -- the nearest
sibling, it takes the same colour kernel -- and against what such files cost before: the host branch of get_meter_values, Pillow
on the default METERELF_DECODE_THREADS, then MeterReader.read_many on the decoded frames.
One process, 1024-file calls at config 3 (sample-images1 params, 640 x 480), file bytes in host memory, the pointer table built
once.  The files: --distinct (8) fixture frames re-encoded by tests/jpeg_writer.py in each layout with the same flat quantisation
tables and the Annex K Huffman tables (tests/jpeg_sampling_cases.reencode), repeated to the call's 1024 pointers.

    python3 tools/jpeg_sampling_rate.py [--steps 8] [--warmup 4] [--rounds 5] [--batch 1024] [--distinct 8] [--host-steps 2]
                                        [--parent-root DIR [--parent-turns 2]]

Rows:
    (a)  4:2:2 files, melf_jpeg_process_batch            (b) the same frames as 4:4:0 files        (c) as 4:1:1 files
    (db) / (dc) the host branch for the files of (b) / (c): imread_bgr on a thread pool, then read_many
    (e)  the fixture's own upright 4:2:0 files (k_jpeg_color420), the switch on like every row
Before anything is timed the records of (a), (b) and (c) are compared, byte for byte, with the host branch's for the same files.
The GPU rows take turns, R rounds of K calls each; the host rows run --host-steps calls once.  Then a few calls of each GPU row
with every kernel bracketed by events: the Huffman, IDCT and colour stages' time per call.
--parent-root DIR: a built checkout of the parent commit.  Row (e) is then run again in fresh child processes that import the
package from DIR and from this checkout, taking turns (this, parent, parent, this ...): the fixture's files on both libraries in
one lease, medians and spread of each turn."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNELS = ('k_jpeg_huff', 'k_jpeg_idct', 'k_jpeg_color')
GPU_ROWS = ['(a)  4:2:2 files', '(b)  4:4:0 files', '(c)  4:1:1 files', '(e)  fixture 4:2:0 files (k_jpeg_color420)']
HOST_ROWS = ['(db) host branch for the files of (b), %d threads', '(dc) host branch for the files of (c), %d threads']


def report(header, gpu_names, host_names, times, kern, batch):
    """The table and the closing lines.  times: name -> ms per call of each round; kern: name -> {kernel: ms per call}."""
    import frame_rates as fr
    rows = [(n, None) for n in gpu_names + host_names]
    cols = [('%s ms' % k, len(k) + 3, lambda name, k=k: '%.4f' % kern.get(name, {}).get(k, 0.0)) for k in KERNELS]
    fr.print_table(header, rows, times, rows[0], cols, name=('row', 52), vs=('vs (a)', 8))
    med = {n: float(np.median(t)) for (n, t) in times.items()}
    spread = {n: (max(t) - min(t)) / float(np.median(t)) for (n, t) in times.items()}
    (a, b, c, e) = (med[n] for n in gpu_names)
    print('(a) %.4f ms a call = %.0f files/s (spread of its rounds %.1f %%); (e) %.4f ms a call = %.0f files/s' % (a, batch / a * 1e3, 100 * spread[gpu_names[0]], e, batch / e * 1e3))
    for (tag, x, name, host) in (('4:4:0', b, gpu_names[1], host_names[0]), ('4:1:1', c, gpu_names[2], host_names[1])):
        h = med[host]
        print('%s: %.4f ms a call = %.0f files/s; vs (a) %.3f; host branch %.1f ms a call = %.0f files/s, %.0f times as long; colour stage %.4f ms a call against %.4f for 4:2:2'
              % (tag, x, batch / x * 1e3, x / a, h, batch / h * 1e3, h / x, kern.get(name, {}).get('k_jpeg_color', 0.0), kern.get(gpu_names[0], {}).get('k_jpeg_color', 0.0)))


def fixture_only(args):
    """Child process: row (e) alone with the package of args.package_root (this checkout's or the parent commit's: only calls both
    have).  Prints 'E_MS v v v ...', the ms per call of each round."""
    sys.path.insert(0, args.package_root)
    sys.path.insert(1, os.path.join(ROOT, 'tests'))
    from meterelf_amd import _engine, _hip, _params
    import jpeg_sampling_cases as sc
    assert os.path.dirname(os.path.dirname(os.path.abspath(_hip.__file__))) == os.path.abspath(args.package_root)
    (files, frames) = sc.fixture_frames(args.distinct)
    (H, W) = frames[0].shape[:2]
    blobs = [open(f, 'rb').read() for f in files]
    reader = _engine.MeterReader(_params.load(os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml')))
    B = args.batch
    (ptrs, sizes, _keep) = _hip._file_table([blobs[i % len(blobs)] for i in range(B)])
    out = np.zeros(B, _hip.RESULT_DTYPE)
    status = np.zeros(B, np.int32)
    L = reader.ctx._L

    def call():
        _hip.check(L.melf_jpeg_process_batch(reader.ctx._h, ptrs, sizes, B, H, W, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
        assert (status == 0).all()
    for _ in range(args.warmup):
        call()
    ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _k in range(args.steps):
            call()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    print('E_MS ' + ' '.join('%.4f' % v for v in ms))
    reader.close()


def both_libraries(args):
    """Row (e) in child processes, this checkout and the parent's taking turns."""
    turns = {'this commit': [], 'parent commit': []}
    for t in range(2 * args.parent_turns):
        (who, root) = ('this commit', ROOT) if t % 4 in (0, 3) else ('parent commit', os.path.abspath(args.parent_root))   # this, parent, parent, this, ...
        env = {k: v for (k, v) in os.environ.items() if k != 'MELF_LIB_PATH'}
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--fixture-only', '--package-root', root, '--batch', str(args.batch), '--steps', str(args.steps),
                            '--warmup', str(args.warmup), '--rounds', str(args.rounds), '--distinct', str(args.distinct)], env=env, stdout=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, (who, p.returncode, p.stdout[-2000:])
        ms = [float(v) for ln in p.stdout.decode().splitlines() if ln.startswith('E_MS ') for v in ln.split()[1:]]
        turns[who].append(ms)
        print('(e) %-13s turn %d: median %.4f ms a call, rounds %.4f..%.4f' % (who, len(turns[who]), float(np.median(ms)), min(ms), max(ms)))
    for (who, runs) in turns.items():
        allms = [v for r in runs for v in r]
        print('(e) %-13s: medians of the turns %s ms; all rounds %.4f..%.4f, spread %.1f %% of the median %.4f' % (
            who, ' / '.join('%.4f' % float(np.median(r)) for r in runs), min(allms), max(allms), 100 * (max(allms) - min(allms)) / float(np.median(allms)), float(np.median(allms))))
    (m_this, m_par) = (float(np.median([v for r in turns[w] for v in r])) for w in ('this commit', 'parent commit'))
    print('(e) this commit / parent commit: %.3f' % (m_this / m_par))


def main():
    ap = argparse.ArgumentParser()
    for (name, default) in (('steps', 8), ('warmup', 4), ('rounds', 5), ('batch', 1024), ('distinct', 8), ('host-steps', 2), ('parent-turns', 2)):
        ap.add_argument('--' + name, type=int, default=default)
    ap.add_argument('--parent-root')
    ap.add_argument('--fixture-only', action='store_true')
    ap.add_argument('--package-root', default=ROOT)
    args = ap.parse_args()
    if args.fixture_only:
        return fixture_only(args)
    from concurrent.futures import ThreadPoolExecutor

    import frame_rates as fr
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import jpeg_sampling_cases as sc
    _hip = fr._hip
    (B, D) = (args.batch, args.distinct)
    tmp = __import__('tempfile').mkdtemp(prefix='jpeg_sampling_rate_')
    params = fr._params.load(os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml'))
    (fixture, frames) = sc.fixture_frames(D)
    (H, W) = frames[0].shape[:2]
    kinds = {'a': '422', 'b': '440', 'c': '411'}
    (files, paths) = ({k: [] for k in kinds}, {k: [] for k in kinds})
    t0 = time.perf_counter()
    for (i, rgb) in enumerate(frames):
        for (k, sampling) in kinds.items():
            files[k].append(sc.reencode(rgb, sampling))
            paths[k].append(os.path.join(tmp, '%s_%02d.jpg' % (k, i)))
            with open(paths[k][-1], 'wb') as fh:
                fh.write(files[k][-1])
    files['e'] = [open(f, 'rb').read() for f in fixture]
    print('%d distinct frames per layout encoded in %.1f s; mean size 4:2:2 %.0f, 4:4:0 %.0f, 4:1:1 %.0f, fixture 4:2:0 %.0f bytes' % (
        D, time.perf_counter() - t0, *(np.mean([len(f) for f in files[k]]) for k in ('a', 'b', 'c', 'e'))))
    reader = fr._engine.MeterReader(params, jpeg_samplings=True)
    ctx = reader.ctx
    L = ctx._L
    tables = {k: _hip._file_table([files[k][i % D] for i in range(B)]) for k in files}
    out = np.zeros(B, _hip.RESULT_DTYPE)
    status = np.zeros(B, np.int32)

    def gpu_row(kind):
        def fn(i):
            (ptrs, sizes, _keep) = tables[kind]
            _hip.check(L.melf_jpeg_process_batch(ctx._h, ptrs, sizes, B, H, W, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
            assert (status == 0).all(), (kind, np.flatnonzero(status)[:8], status[status != 0][:8])
        return fn
    nthreads = max(1, int(os.getenv('METERELF_DECODE_THREADS', str(min(8, os.cpu_count() or 1)))))
    pool = ThreadPoolExecutor(max_workers=nthreads)

    def host_row(kind):
        def fn(i):
            frames_h = list(pool.map(fr.imread_bgr, [paths[kind][k % D] for k in range(B)]))
            out[:] = np.array(reader.read_many(frames_h), dtype=_hip.RESULT_DTYPE)
        return fn
    gpu_rows = list(zip(GPU_ROWS, (gpu_row('a'), gpu_row('b'), gpu_row('c'), gpu_row('e'))))
    host_rows = [(HOST_ROWS[0] % nthreads, host_row('b')), (HOST_ROWS[1] % nthreads, host_row('c'))]

    def records(fn):
        fn(0)
        return out.copy()
    for ((name, g), h) in ((gpu_rows[0], host_row('a')), (gpu_rows[1], host_rows[0][1]), (gpu_rows[2], host_rows[1][1])):
        (r_g, r_h) = (records(g), records(h))
        assert r_g.tobytes() == r_h.tobytes(), '%s: records differ from the host branch\'s' % name
        print('%s: %d of %d files read; the records == the host branch\'s' % (name[:4], int((r_g['status'] == _hip.FRAME_OK).sum()), B))

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
    kern = {}
    ctx.set_profiling(1)
    for (n, fn) in gpu_rows:
        run(fn, 2)
        ctx.timings()
        run(fn, 4)
        kern[n] = {k: ms / 4 for (k, (ms, cnt)) in ctx.timings().items() if cnt}     # per CALL (a call launches a stage once per chunk)
    ctx.set_profiling(0)
    report('%d-file calls, %dx%d, %d distinct files per row repeated, %d rounds x %d calls; kernel columns: ms per call' % (B, W, H, D, args.rounds, args.steps),
           [n for (n, _f) in gpu_rows], [n for (n, _f) in host_rows], times, kern, B)
    pool.shutdown()
    reader.close()
    for k in paths:
        for p in paths[k]:
            os.remove(p)
    os.rmdir(tmp)
    if args.parent_root:
        both_libraries(args)


if __name__ == '__main__':
    sys.path.insert(0, HERE)
    main()
