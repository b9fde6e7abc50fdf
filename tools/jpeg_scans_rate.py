#!/usr/bin/env python3
"""Multi-scan sequential JPEG files (melf_ctx_set_jpeg_multiscan: every scan a one-component record of its own through the entropy
decoders as they stand, the IDCT reading planar coefficient areas) and files without their Huffman tables
(melf_ctx_set_jpeg_default_tables: host code only) against their interleaved twins, and against what such files cost before: the host
branch of get_meter_values, Pillow on the default METERELF_DECODE_THREADS, then MeterReader.read_many on the decoded frames.
One process, 1024-file calls at config 3 (sample-images1 params, 640 x 480), file bytes in host memory, the pointer table built
once (the calls' inputs are host memory: there is no device buffer to rotate; the 8 distinct files of a row repeat).  The files:
--distinct (8) fixture frames re-encoded by tests/jpeg_writer.py with the same flat quantisation tables and the Annex K Huffman
tables, as 4:2:0 and as 4:2:2, interleaved (the twins), multi-scan (tests/jpeg_scans_cases.write_multiscan) and without DHT segments.

    python3 tools/jpeg_scans_rate.py [--steps 8] [--warmup 4] [--rounds 5] [--batch 1024] [--distinct 8] [--host-steps 2] [--mix 256]
                                     [--parent-root DIR [--parent-turns 2]]

Rows:
    (a0) / (a2)  interleaved 4:2:0 / 4:2:2 files, melf_jpeg_process_batch
    (b0) / (b2)  the same frames as multi-scan files          (c0) / (c2)  the twins without their DHT segments
    (e)          the fixture's own 4:2:0 files, both switches on like every row
    (hb) / (hc)  the host branch for the files of (b0) / (c0): imread_bgr on a thread pool, then read_many
    (m1)         a --mix (256) file call of fixture files with ONE multi-scan file among them, on the GPU
    (m0)         the same call with that file through the host branch: the call without it, then imread_bgr and read_many for it
Before anything is timed the records of every GPU row are compared, byte for byte, with the host branch's for the same files.
The GPU rows take turns, R rounds of K calls each; the host rows run --host-steps calls once.  Then a few calls of each GPU row
with every kernel bracketed by events: the Huffman, IDCT and colour stages' time per call.  The closing lines hold the one decision
that rests on a measurement: get_meter_values turns the multi-scan switch on by default only if (m1) takes no longer than (m0).
--parent-root DIR: a built checkout of the parent commit.  Row (e) is then run again in fresh child processes that import the
package from DIR and from this checkout, taking turns (this, parent, parent, this ...): the fixture's files on both libraries in
one lease, medians and spread of each turn."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNELS = ('k_jpeg_huff', 'k_jpeg_idct', 'k_jpeg_color')
GPU_ROWS = ['(a0) interleaved 4:2:0 files', '(a2) interleaved 4:2:2 files', '(b0) multi-scan 4:2:0 files', '(b2) multi-scan 4:2:2 files',
            '(c0) 4:2:0 files without DHT', '(c2) 4:2:2 files without DHT', '(e)  fixture 4:2:0 files']
HOST_ROWS = ['(hb) host branch for the files of (b0), %d threads', '(hc) host branch for the files of (c0), %d threads']
MIX_ROWS = ['(m1) %d fixture files, one of them multi-scan, on the GPU', '(m0) the same, that file through the host branch']


def report(header, gpu_names, host_names, mix_names, times, kern, batch):
    """The table and the closing lines.  times: name -> ms per call of each round; kern: name -> {kernel: ms per call}."""
    import frame_rates as fr
    rows = [(n, None) for n in gpu_names + host_names + mix_names]
    cols = [('%s ms' % k, len(k) + 3, lambda name, k=k: '%.4f' % kern.get(name, {}).get(k, 0.0)) for k in KERNELS]
    fr.print_table(header, rows, times, rows[0], cols, name=('row', 60), vs=('vs (a0)', 8))
    med = {n: float(np.median(t)) for (n, t) in times.items()}
    spread = {n: (max(t) - min(t)) / float(np.median(t)) for (n, t) in times.items()}
    (a0, a2, b0, b2, c0, c2, e) = (med[n] for n in gpu_names)
    print('(a0) %.4f ms a call = %.0f files/s (spread of its rounds %.1f %%); (a2) %.4f; (e) %.4f ms a call = %.0f files/s' % (
        a0, batch / a0 * 1e3, 100 * spread[gpu_names[0]], a2, e, batch / e * 1e3))
    for (tag, x0, x2, host) in (('multi-scan', b0, b2, host_names[0]), ('without DHT', c0, c2, host_names[1])):
        h = med[host]
        print('%s: 4:2:0 %.4f ms a call = %.0f files/s, %.3f of its twin; 4:2:2 %.4f ms, %.3f of its twin; host branch %.1f ms a call = %.0f files/s, %.0f times as long'
              % (tag, x0, batch / x0 * 1e3, x0 / a0, x2, x2 / a2, h, batch / h * 1e3, h / x0))
    (m1, m0) = (med[n] for n in mix_names)
    print('one multi-scan file in a call: %.4f ms on the GPU (rounds %.4f..%.4f) against %.4f ms through the host branch (rounds %.4f..%.4f): %s'
          % (m1, min(times[mix_names[0]]), max(times[mix_names[0]]), m0, min(times[mix_names[1]]), max(times[mix_names[1]]),
             'no longer, the switch may be on by default' if m1 <= m0 else 'longer, the switch stays opt-in'))


def main():
    ap = argparse.ArgumentParser()
    for (name, default) in (('steps', 8), ('warmup', 4), ('rounds', 5), ('batch', 1024), ('distinct', 8), ('host-steps', 2), ('parent-turns', 2), ('mix', 256)):
        ap.add_argument('--' + name, type=int, default=default)
    ap.add_argument('--parent-root')
    ap.add_argument('--fixture-only', action='store_true')
    ap.add_argument('--package-root', default=ROOT)
    args = ap.parse_args()
    import jpeg_sampling_rate as sr
    if args.fixture_only:
        return sr.fixture_only(args)
    from concurrent.futures import ThreadPoolExecutor

    import frame_rates as fr
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import jpeg_sampling_cases as sc
    import jpeg_scans_cases as ms
    _hip = fr._hip
    (B, D, M) = (args.batch, args.distinct, args.mix)
    tmp = __import__('tempfile').mkdtemp(prefix='jpeg_scans_rate_')
    params = fr._params.load(os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml'))
    (fixture, frames) = sc.fixture_frames(D)
    (H, W) = frames[0].shape[:2]
    qt = {0: ([sc.FLAT_Q[0]] * 64, False), 1: ([sc.FLAT_Q[1]] * 64, False)}
    files = {k: [] for k in ('a0', 'a2', 'b0', 'b2', 'c0', 'c2')}
    paths = {k: [] for k in ('b0', 'c0')}
    t0 = time.perf_counter()
    for (i, rgb) in enumerate(frames):
        for (tag, sampling) in (('0', '420'), ('2', '422')):
            grids = sc.image_coefs(rgb, sampling, qt)
            twin = sc.write(grids, (H, W), sampling, qt)
            segs = ms.segments(twin)
            files['a' + tag].append(twin)
            files['b' + tag].append(ms.write_multiscan(grids, (H, W), sampling, qt))
            files['c' + tag].append(twin[:2] + b''.join(twin[a:b] for (m, a, b) in segs if m != 0xC4) + twin[segs[-1][2]:])
        for k in paths:
            paths[k].append(os.path.join(tmp, '%s_%02d.jpg' % (k, i)))
            with open(paths[k][-1], 'wb') as fh:
                fh.write(files[k][-1])
    files['e'] = [open(f, 'rb').read() for f in fixture]
    print('%d distinct frames encoded in %.1f s; mean size interleaved 4:2:0 %.0f, multi-scan %.0f, without DHT %.0f, fixture %.0f bytes' % (
        D, time.perf_counter() - t0, *(np.mean([len(f) for f in files[k]]) for k in ('a0', 'b0', 'c0', 'e'))))
    reader = fr._engine.MeterReader(params, jpeg_multiscan=True, jpeg_default_tables=True)
    ctx = reader.ctx
    L = ctx._L
    tables = {k: _hip._file_table([files[k][i % D] for i in range(B)]) for k in files}
    mixed = [files['e'][i % D] for i in range(M)]
    mixed[M // 2] = files['b0'][0]
    tables['m1'] = _hip._file_table(mixed)
    tables['m0'] = _hip._file_table(mixed[:M // 2] + mixed[M // 2 + 1:])
    out = np.zeros(B, _hip.RESULT_DTYPE)
    status = np.zeros(B, np.int32)

    def gpu_row(kind, n=B):
        def fn(i):
            (ptrs, sizes, _keep) = tables[kind]
            _hip.check(L.melf_jpeg_process_batch(ctx._h, ptrs, sizes, n, H, W, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
            assert (status[:n] == 0).all(), (kind, np.flatnonzero(status[:n])[:8], status[:n][status[:n] != 0][:8])
        return fn
    nthreads = max(1, int(os.getenv('METERELF_DECODE_THREADS', str(min(8, os.cpu_count() or 1)))))
    pool = ThreadPoolExecutor(max_workers=nthreads)

    def host_row(kind):
        def fn(i):
            frames_h = list(pool.map(fr.imread_bgr, [paths[kind][k % D] for k in range(B)]))
            out[:] = np.array(reader.read_many(frames_h), dtype=_hip.RESULT_DTYPE)
        return fn
    rest = gpu_row('m0', M - 1)

    def mix_host(i):
        rest(i)
        one = list(pool.map(fr.imread_bgr, [paths['b0'][0]]))
        out[M - 1:M] = np.array(reader.read_many(one), dtype=_hip.RESULT_DTYPE)
    gpu_rows = list(zip(GPU_ROWS, (gpu_row(k) for k in ('a0', 'a2', 'b0', 'b2', 'c0', 'c2', 'e'))))
    host_rows = [(HOST_ROWS[0] % nthreads, host_row('b0')), (HOST_ROWS[1] % nthreads, host_row('c0'))]
    mix_rows = [(MIX_ROWS[0] % M, gpu_row('m1', M)), (MIX_ROWS[1], mix_host)]

    def records(fn):
        fn(0)
        return out.copy()
    want = records(host_rows[0][1])
    for (name, g) in gpu_rows[:6]:
        got = records(g)
        if name[2] == '0':
            assert got.tobytes() == want.tobytes(), '%s: records differ from the host branch\'s' % name
        else:
            assert got.tobytes() == records(gpu_rows[1][1]).tobytes(), '%s: records differ from the twin\'s' % name
        print('%s: %d of %d files read; the records == %s' % (name[:4], int((got['status'] == _hip.FRAME_OK).sum()), B, 'the host branch\'s' if name[2] == '0' else 'the twin\'s'))

    def run(fn, steps):
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        return (time.perf_counter() - t0) / steps * 1e3
    for (_n, fn) in gpu_rows + mix_rows:
        run(fn, args.warmup)
    times = {n: [] for (n, _f) in gpu_rows + host_rows + mix_rows}
    for r in range(args.rounds):
        for (n, fn) in fr.rotated(gpu_rows + mix_rows, r):
            run(fn, 1)
            times[n].append(run(fn, args.steps))
    for (n, fn) in host_rows:
        times[n] = [run(fn, 1) for _ in range(args.host_steps)]
    kern = {}
    ctx.set_profiling(1)
    for (n, fn) in gpu_rows + mix_rows[:1]:
        run(fn, 2)
        ctx.timings()
        run(fn, 4)
        kern[n] = {k: v / 4 for (k, (v, cnt)) in ctx.timings().items() if cnt}     # per CALL (a call launches a stage once per chunk)
    ctx.set_profiling(0)
    report('%d-file calls, %dx%d, %d distinct files per row repeated, %d rounds x %d calls; kernel columns: ms per call' % (B, W, H, D, args.rounds, args.steps),
           [n for (n, _f) in gpu_rows], [n for (n, _f) in host_rows], [n for (n, _f) in mix_rows], times, kern, B)
    pool.shutdown()
    reader.close()
    for k in paths:
        for p in paths[k]:
            os.remove(p)
    os.rmdir(tmp)
    if args.parent_root:
        sr.both_libraries(args)


if __name__ == '__main__':
    sys.path.insert(0, HERE)
    main()
