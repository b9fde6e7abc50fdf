#!/usr/bin/env python3
"""Baseline JPEG files whose scan exceeds 4 MB (melf_ctx_set_jpeg_long_scans: k_jpeg_chapters takes the scan chapter by chapter)
against what such files cost before: the host branch of get_meter_values, Pillow on the default METERELF_DECODE_THREADS, then
MeterReader.read_many on the decoded frames.  One process, sample-images1 params.  The long files are noise at quality 100, 4:4:4:
1000 x 1200 (4.9 MB, two chapters) and 1500 x 1700 (10.5 MB, three chapters), --distinct (2) of each.

    python3 tools/jpeg_long_rate.py [--steps 3] [--warmup 1] [--counts 64,256] [--mix 256] [--mix-long 1,8,32] [--distinct 2]
                                    [--parent-root DIR [--parent-turns 2] [--batch 1024] [--rounds 5] [--fixture-steps 8]]

Rows:
    (f)  a melf_jpeg_process_batch call of N files of one long size, N of --counts: the best of --steps calls on the GPU, the per-kernel
         times of one profiled call, and the host branch for the same files (imread_bgr on a thread pool, then read_many), once
    (m)  a --mix (256) name list of fixture files with 1, 8 and 32 long 4.9 MB files among them through MeterReader.read_jpeg_paths: with
         the switch on, and with it off plus the host branch for the files that come back undecoded -- what get_meter_values does
         under METERELF_JPEG_LONG=gpu and =host
Before anything is timed the records of the GPU rows are compared, byte for byte, with the host branch's for the same files.
The closing line holds the one decision that rests on a measurement: get_meter_values turns the switch on by default exactly if the
1-file row of (m) is faster on the GPU than through the host branch.
--parent-root DIR: a built checkout of the parent commit.  A --batch (1024) file call of the fixture's own files is then run in fresh
child processes that import the package from DIR and from this checkout, taking turns (this, parent, parent, this ...): medians and
spread of each turn (tools/jpeg_sampling_rate.py: both_libraries)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNELS = ('k_jpeg_huff', 'k_jpeg_idct', 'k_jpeg_color')
SIZES = (((1000, 1200), '4.9 MB'), ((1500, 1700), '10.5 MB'))
FULL_ROW = '(f) %3d files of %s'
MIX_ROW = '%2d long file%s of %d'


def report(header, full, mix, nthreads):
    """The two tables and the closing line.  full: [(name, gpu ms of each call, {kernel: ms}, host ms of each call)];
    mix: [(long files, files, gpu ms of each call, host-branch ms of each call)]."""
    print(header)
    cols = ['gpu ms', 'gpu calls'] + ['%s ms' % k for k in KERNELS] + ['host branch ms, %d threads' % nthreads, 'host / gpu']
    width = [60, 9, 21] + [len(k) + 3 for k in KERNELS] + [len(cols[-2]), 10]
    print('| %s |' % ' | '.join('%-*s' % (width[0], 'row') if i == 0 else '%*s' % (width[i], c) for (i, c) in enumerate(['row'] + cols)))
    print('|%s|' % '|'.join('-' * (w + 2) for w in width))
    for (name, gpu, kern, host) in full:
        cells = ['%.3f' % min(gpu), '%.3f..%.3f' % (min(gpu), max(gpu))] + ['%.3f' % kern.get(k, 0.0) for k in KERNELS] + ['%.1f' % min(host), '%.1fx' % (min(host) / min(gpu))]
        print('| %-*s | %s |' % (width[0], name, ' | '.join('%*s' % (w, c) for (w, c) in zip(width[1:], cells))))
    print('name lists through read_jpeg_paths, best of the calls (all calls in brackets):')
    for (nlong, n, gpu, host) in mix:
        print('%s : gpu %.3f ms  host branch %.3f ms  (gpu %s; host branch %s)' % (
            MIX_ROW % (nlong, '' if nlong == 1 else 's', n), min(gpu), min(host), ' '.join('%.3f' % v for v in gpu), ' '.join('%.3f' % v for v in host)))
    one = [m for m in mix if m[0] == 1]
    if one:
        (_l, _n, gpu, host) = one[0]
        print('one long file in a list: %.3f ms on the GPU against %.3f ms through the host branch: %s' % (
            min(gpu), min(host), "faster, METERELF_JPEG_LONG defaults to 'gpu'" if min(gpu) < min(host) else "not faster, METERELF_JPEG_LONG defaults to 'host'"))
        if not min(gpu) < min(host):
            pays = [m[0] for m in mix if min(m[2]) < min(m[3])]
            print('the switch pays from %s long files in a list on' % (str(min(pays)) if pays else 'more than %d' % max(m[0] for m in mix)))


def main():
    ap = argparse.ArgumentParser()
    for (name, default) in (('steps', 3), ('warmup', 1), ('mix', 256), ('distinct', 2), ('parent-turns', 2), ('batch', 1024), ('rounds', 5), ('fixture-steps', 8)):
        ap.add_argument('--' + name, type=int, default=default)
    ap.add_argument('--counts', default='64,256')
    ap.add_argument('--mix-long', default='1,8,32')
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
    import jpeg_long_cases as lc
    import jpeg_sampling_cases as sc
    _hip = fr._hip
    tmp = __import__('tempfile').mkdtemp(prefix='jpeg_long_rate_')
    params = fr._params.load(os.path.join(sc.GOLDEN, 'sample-images1', 'params.yml'))
    nthreads = max(1, int(os.getenv('METERELF_DECODE_THREADS', str(min(8, os.cpu_count() or 1)))))
    pool = ThreadPoolExecutor(max_workers=nthreads)
    reader = fr._engine.MeterReader(params, jpeg_long_scans=True)
    plain = fr._engine.MeterReader(params)
    ctx = reader.ctx
    L = ctx._L
    rng = np.random.default_rng(77)
    (files, paths) = ({}, {})
    for ((H, W), tag) in SIZES:
        files[tag] = [lc.encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=100, subsampling='4:4:4') for _ in range(args.distinct)]
        paths[tag] = []
        for (i, d) in enumerate(files[tag]):
            paths[tag].append(os.path.join(tmp, '%dx%d_%d.jpg' % (H, W, i)))
            with open(paths[tag][-1], 'wb') as fh:
                fh.write(d)
        print('%s: %d x %d, %s bytes, clean scans of %s bytes = %s chapters of %d' % (
            tag, H, W, [len(d) for d in files[tag]], [lc.scan_lengths(d)[1] for d in files[tag]], [lc.chapters(d, lc.PRODUCTION) for d in files[tag]], lc.PRODUCTION))

    def run(fn, steps):
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms
    full = []
    for ((H, W), tag) in SIZES:
        for n in [int(v) for v in args.counts.split(',')]:
            (ptrs, sizes, _keep) = _hip._file_table([files[tag][i % args.distinct] for i in range(n)])
            out = np.zeros(n, _hip.RESULT_DTYPE)
            status = np.zeros(n, np.int32)

            def gpu():
                _hip.check(L.melf_jpeg_process_batch(ctx._h, ptrs, sizes, n, H, W, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)))
                assert (status == 0).all(), status[status != 0][:8]
            host_out = []

            def host():
                frames_h = list(pool.map(fr.imread_bgr, [paths[tag][k % args.distinct] for k in range(n)]))
                host_out[:] = [np.array(reader.read_many(frames_h), dtype=_hip.RESULT_DTYPE)]
            run(gpu, args.warmup)
            host_ms = run(host, 1)
            assert out.tobytes() == host_out[0].tobytes(), '%s: records differ from the host branch\'s' % tag
            gpu_ms = run(gpu, args.steps)
            ctx.set_profiling(1)
            ctx.timings()
            gpu()
            kern = {k: v for (k, (v, cnt)) in ctx.timings().items() if cnt}
            ctx.set_profiling(0)
            full.append((FULL_ROW % (n, tag), gpu_ms, kern, host_ms))
            print('%s: gpu %s ms, host branch %s ms; the records == the host branch\'s' % (full[-1][0], ' '.join('%.3f' % v for v in gpu_ms), ' '.join('%.1f' % v for v in host_ms)), flush=True)
    # name lists: fixture files with long files among them
    (fixture, _frames) = sc.fixture_frames(8)
    tag = SIZES[0][1]
    mix = []
    for nlong in [int(v) for v in args.mix_long.split(',')]:
        names = [fixture[i % len(fixture)] for i in range(args.mix)]
        for j in range(nlong):
            names[(2 * j + 1) * args.mix // (2 * nlong)] = paths[tag][j % args.distinct]
        got = {}

        def gpu_list():
            got['gpu'] = reader.read_jpeg_paths(names)
            assert all(g is not None for g in got['gpu'])

        def host_list():
            recs = plain.read_jpeg_paths(names)
            todo = [i for (i, r) in enumerate(recs) if r is None]
            assert len(todo) == nlong
            frames_h = list(pool.map(fr.imread_bgr, [names[i] for i in todo]))
            for (i, r) in zip(todo, reader.read_many(frames_h)):
                recs[i] = r
            got['host'] = recs
        run(gpu_list, args.warmup)
        run(host_list, args.warmup)
        assert all(np.array(a, dtype=_hip.RESULT_DTYPE).tobytes() == np.array(b, dtype=_hip.RESULT_DTYPE).tobytes() for (a, b) in zip(got['gpu'], got['host'])), 'records differ'
        (g, h) = ([], [])
        for _ in range(args.steps):
            g += run(gpu_list, 1)
            h += run(host_list, 1)
        mix.append((nlong, args.mix, g, h))
        print('%s: gpu %s, host branch %s' % (MIX_ROW % (nlong, '' if nlong == 1 else 's', args.mix), ' '.join('%.3f' % v for v in g), ' '.join('%.3f' % v for v in h)), flush=True)
    report('long files at the production chapter length (%d bytes); kernel columns: ms of one profiled call' % lc.PRODUCTION, full, mix, nthreads)
    pool.shutdown()
    reader.close()
    plain.close()
    for t in paths:
        for p in paths[t]:
            os.remove(p)
    os.rmdir(tmp)
    if args.parent_root:
        args.steps = args.fixture_steps
        args.warmup = 4
        args.distinct = 8
        sr.both_libraries(args)


if __name__ == '__main__':
    sys.path.insert(0, HERE)
    main()
