#!/usr/bin/env python3
"""Baseline JPEG files that end inside their scan (melf_ctx_set_jpeg_truncated: the Huffman kernels report such a file, k_jpeg_cut_tail
finishes the cut MCU from the state they leave) -- what the switch costs the files that are whole, what it gains the files that are cut,
and what the new kernel takes.  Config 3 (sample-images1 params, 640 x 480 pixels), file bytes in host memory, pointer tables built once.

    python3 tools/jpeg_cut_rate.py [--steps 8] [--warmup 4] [--rounds 5] [--batch 1024] [--distinct 8] [--mix 256]
                                   [--parent-lib PATH [--parent-turns 2]]

(a)  --parent-lib PATH: the library built from the parent commit.  The fixture's own files in --batch (1024) file calls of
     melf_jpeg_process_batch, in fresh child processes that load this checkout's library and the parent's (through MELF_LIB_PATH),
     taking turns in one lease (this, parent, parent, this ...): both medians, and the spread between one library's own turns.
(b)  --mix (256) file calls of fixture files of which 1 / 32 / all are cut inside the meter_rect window, the switch on, against the same
     call with those files through the host branch (the call without them, then imread_bgr on the default METERELF_DECODE_THREADS and
     read_many for them).  Before anything is timed the records of every GPU row are compared, byte for byte, with the host branch's.
     get_meter_values turns the switch on by default only if the 1-file row takes no longer on the GPU.
(c)  The Huffman stage's time per call (melf_ctx_timings, MELF_K_JPEG_HUFF: k_jpeg_clean, the Huffman kernels and k_jpeg_cut_tail) of the
     rows of (b) with the switch on and with it off (the cut files then come back corrupt after the same Huffman kernels): the
     difference is what k_jpeg_cut_tail and the clearing of its records take."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def fixture_only(args):
    """Child process: --batch file calls of the fixture's own files with the library MELF_LIB_PATH names (or the checkout's).  Prints
    'E_MS v v v ...', the ms per call of each round."""
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, 'tests'))
    from meterelf_amd import _engine, _hip, _params
    import jpeg_sampling_cases as sc
    (files, frames) = sc.fixture_frames(args.distinct)
    (H, W) = frames[0].shape[:2]
    blobs = [open(f, 'rb').read() for f in files]
    reader = _engine.MeterReader(_params.load(os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml')))
    if args.switch_on:
        reader.set_jpeg_truncated(True)
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
    turns = {'this commit': [], 'parent commit': [], 'this commit, switch on': []}
    plan = []
    for t in range(2 * args.parent_turns):
        plan.append('this commit' if t % 4 in (0, 3) else 'parent commit')   # this, parent, parent, this, ...
    plan += ['this commit, switch on'] * args.parent_turns
    for who in plan:
        env = {k: v for (k, v) in os.environ.items() if k != 'MELF_LIB_PATH'}
        if who == 'parent commit':
            env['MELF_LIB_PATH'] = os.path.abspath(args.parent_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--fixture-only', '--batch', str(args.batch), '--steps', str(args.steps), '--warmup', str(args.warmup),
               '--rounds', str(args.rounds), '--distinct', str(args.distinct)] + (['--switch-on'] if who.endswith('switch on') else [])
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, (who, p.returncode, p.stdout[-2000:])
        ms = [float(v) for ln in p.stdout.decode().splitlines() if ln.startswith('E_MS ') for v in ln.split()[1:]]
        turns[who].append(ms)
        print('(a) %-22s turn %d: median %.4f ms a call, rounds %.4f..%.4f' % (who, len(turns[who]), float(np.median(ms)), min(ms), max(ms)), flush=True)
    med = {}
    for (who, runs) in turns.items():
        allms = [v for r in runs for v in r]
        tm = [float(np.median(r)) for r in runs]
        med[who] = float(np.median(allms))
        print('(a) %-22s: medians of the turns %s ms (%.1f %% between its own turns); all rounds %.4f..%.4f, median %.4f' % (
            who, ' / '.join('%.4f' % v for v in tm), 100 * (max(tm) - min(tm)) / med[who], min(allms), max(allms), med[who]))
    print('(a) this commit / parent commit: %.3f on the medians; this commit with the switch on / parent commit: %.3f' % (
        med['this commit'] / med['parent commit'], med['this commit, switch on'] / med['parent commit']))


def main():
    ap = argparse.ArgumentParser()
    for (name, default) in (('steps', 8), ('warmup', 4), ('rounds', 5), ('batch', 1024), ('distinct', 8), ('parent-turns', 2), ('mix', 256)):
        ap.add_argument('--' + name, type=int, default=default)
    ap.add_argument('--parent-lib')
    ap.add_argument('--fixture-only', action='store_true')
    ap.add_argument('--switch-on', action='store_true')
    args = ap.parse_args()
    if args.fixture_only:
        return fixture_only(args)
    from concurrent.futures import ThreadPoolExecutor

    import frame_rates as fr
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import jpeg_cut_cases as cc
    import jpeg_sampling_cases as sc
    _hip = fr._hip
    (D, M) = (args.distinct, args.mix)
    tmp = __import__('tempfile').mkdtemp(prefix='jpeg_cut_rate_')
    params = fr._params.load(os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml'))
    (fixture, frames) = sc.fixture_frames(D)
    (H, W) = frames[0].shape[:2]
    whole = [open(f, 'rb').read() for f in fixture]
    ((_x0, y0), (_x1, y1)) = params.meter_rect
    (cut_files, cut_paths) = ([], [])
    for (i, data) in enumerate(whole):   # each file cut where about (y0 + y1) / 2 of its rows are decoded: inside the window
        p = cc.parse(data)
        d = cc.decode(p)
        at = p.scan_begin + int((p.scan_end - p.scan_begin) * ((y0 + y1) / 2.0 + 8 * (i % 5)) / H)
        while not cc.in_range(p, cc.rule(p, d, at)[0]):   # (outside libjpeg's plain-clamp range the cut MCU's pixels are unspecified)
            at += 1
        cut_files.append(data[:at])
        cut_paths.append(os.path.join(tmp, 'cut_%02d.jpg' % i))
        with open(cut_paths[-1], 'wb') as fh:
            fh.write(cut_files[-1])
    reader = fr._engine.MeterReader(params, jpeg_truncated=True)
    ctx = reader.ctx
    L = ctx._L
    out = np.zeros(M, _hip.RESULT_DTYPE)
    status = np.zeros(M, np.int32)
    nthreads = max(1, int(os.getenv('METERELF_DECODE_THREADS', str(min(8, os.cpu_count() or 1)))))
    pool = ThreadPoolExecutor(max_workers=nthreads)
    rows = []
    tables = {}
    for k in (1, 32, M):
        where = set(int(v) for v in np.linspace(0, M - 1, k).astype(int)) if k < M else set(range(M))
        mixed = [cut_files[i % D] if i in where else whole[i % D] for i in range(M)]
        rest = [whole[i % D] for i in range(M) if i not in where]
        paths = [cut_paths[i % D] for i in sorted(where)]
        tables[k] = (_hip._file_table(mixed), _hip._file_table(rest) if rest else None, len(rest), paths, sorted(where))

    def gpu_row(k, expect_ok=True):
        def fn(i):
            ((ptrs, sizes, _keep), _r, _n, _p, _w) = tables[k]
            _hip.check(L.melf_jpeg_process_batch(ctx._h, ptrs, sizes, M, H, W, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
            if expect_ok:
                assert (status == 0).all(), (k, np.flatnonzero(status)[:8])
        return fn

    def host_row(k):
        def fn(i):
            (_m, rest, n, paths, where) = tables[k]
            if n:
                (ptrs, sizes, _keep) = rest
                _hip.check(L.melf_jpeg_process_batch(ctx._h, ptrs, sizes, n, H, W, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
                assert (status[:n] == 0).all()
            got = np.array(reader.read_many(list(pool.map(fr.imread_bgr, paths))), dtype=_hip.RESULT_DTYPE)
            merged = np.zeros(M, _hip.RESULT_DTYPE)
            keep = np.ones(M, bool)
            keep[where] = False
            merged[keep] = out[:n]
            merged[where] = got
            out[:] = merged
        return fn
    for k in (1, 32, M):
        rows.append(('(b) %3d of %d files cut, on the GPU' % (k, M), gpu_row(k)))
        rows.append(('(b) %3d of %d files cut, those through the host branch' % (k, M), host_row(k)))
    for q in range(0, len(rows), 2):
        ctx.jpeg_truncated_files(reset=True)
        rows[q][1](0)
        (got, counted) = (out.copy(), ctx.jpeg_truncated_files(reset=True))
        rows[q + 1][1](0)
        assert got.tobytes() == out.tobytes(), '%s: records differ from the host branch\'s' % rows[q][0]
        print('%s: %d files completed under the rule, %d of %d read; the records == the host branch\'s' % (
            rows[q][0], counted, int((got['status'] == _hip.FRAME_OK).sum()), M), flush=True)

    def run(fn, steps):
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        return (time.perf_counter() - t0) / steps * 1e3
    for (_n, fn) in rows:
        run(fn, args.warmup)
    times = {n: [] for (n, _f) in rows}
    for r in range(args.rounds):
        for (n, fn) in fr.rotated(rows, r):
            run(fn, 1)
            times[n].append(run(fn, args.steps))
    fr.print_table('%d-file calls, %dx%d, %d distinct files repeated, %d rounds x %d calls, host branch on %d threads' % (M, W, H, D, args.rounds, args.steps, nthreads),
                   rows, times, rows[0], name=('row', 60), vs=('vs first', 8))
    med = {n: float(np.median(t)) for (n, t) in times.items()}
    for q in range(0, len(rows), 2):
        (g, h) = (med[rows[q][0]], med[rows[q + 1][0]])
        print('%s: %.4f ms against %.4f ms through the host branch, %.2f times as long there' % (rows[q][0][:24], g, h, h / g))
    one = med[rows[0][0]] <= med[rows[1][0]]
    print('one cut file in a call: %s on the GPU: %s' % ('no longer' if one else 'LONGER', 'the switch may be on by default' if one else 'the switch stays opt-in'))
    # (c) the Huffman stage with the switch on and off
    ctx.set_profiling(1)
    for k in (1, 32, M):
        stage = {}
        for on in (True, False):
            reader.set_jpeg_truncated(on)
            fn = gpu_row(k, expect_ok=on)
            run(fn, 2)
            ctx.timings()
            run(fn, 8)
            stage[on] = {name: v / 8 for (name, (v, cnt)) in ctx.timings().items() if cnt}
        reader.set_jpeg_truncated(True)
        (a, b) = (stage[True].get('k_jpeg_huff', 0.0), stage[False].get('k_jpeg_huff', 0.0))
        print('(c) %3d of %d files cut: Huffman stage %.4f ms a call with the switch on, %.4f with it off: k_jpeg_cut_tail and its records %.4f ms a call (IDCT %.4f, colour %.4f with it on)' % (
            k, M, a, b, a - b, stage[True].get('k_jpeg_idct', 0.0), stage[True].get('k_jpeg_color', 0.0)))
    ctx.set_profiling(0)
    pool.shutdown()
    reader.close()
    for p in cut_paths:
        os.remove(p)
    os.rmdir(tmp)
    if args.parent_lib:
        both_libraries(args)


if __name__ == '__main__':
    sys.path.insert(0, HERE)
    main()
