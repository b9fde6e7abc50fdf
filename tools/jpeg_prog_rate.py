#!/usr/bin/env python3
"""Progressive JPEG files decoded and read on the GPU (melf_ctx_set_jpeg_progressive, k_jpeg_prog_scan): ms a call and files/s of
melf_jpeg_process_batch on the sample-images1 frames of the common size -- as they are (baseline), re-saved progressive at quality
95 without restart markers and with a restart interval of one MCU row, 256 and 1024 files a call, and half baseline / half
progressive -- best of three calls, then one profiled call's per-kernel times (the scans are timed under k_jpeg_huff).  Also the
host's header parse of 256 progressive files (it walks their entropy-coded bytes once).  Last, what decides get_meter_values'
default: 256-file calls of which k = 0, 1, 8, 32, 128, 256 files are progressive (no restart markers) and the rest baseline, against
the host branch's way with the same list -- the k files decoded by Pillow on 8 threads, the others through the GPU call.

    python3 tools/jpeg_prog_rate.py          (profiles/jpeg_prog/jpeg_prog_rate.txt)
"""
import sys, io, os, time, glob
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from PIL import Image
from meterelf_amd import MeterReader, _hip, _params
G = os.path.join(ROOT, 'tests', 'golden', 'sample-images1')
reader = MeterReader(_params.load(os.path.join(G, 'params.yml')), jpeg_progressive=True)
ctx = reader.ctx
src = sorted(glob.glob(os.path.join(G, '*.jpg')))
sizes = [Image.open(f).size for f in src]
size = max(set(sizes), key=sizes.count)
src = [f for (f, s) in zip(src, sizes) if s == size][:64]
prog, progr, base = [], [], []
for f in src:
    b = io.BytesIO(); Image.open(f).save(b, 'JPEG', quality=95, progressive=True); prog.append(b.getvalue())
    b = io.BytesIO(); Image.open(f).save(b, 'JPEG', quality=95, progressive=True, restart_marker_rows=1); progr.append(b.getvalue())
    base.append(open(f, 'rb').read())
(W, H) = size
print('bytes per file', len(base[0]), len(prog[0]), len(progr[0]))
t0 = time.perf_counter(); _hip.jpeg_probe_flags_batch(prog * 4, 2); print('host parse of 256 progressive files: %.2f ms' % ((time.perf_counter() - t0) * 1e3))
for (name, lst) in (('baseline', base * 4), ('progressive', prog * 4), ('progressive+rst rows', progr * 4), ('progressive x1024', prog * 16), ('progressive+rst x1024', progr * 16), ('mixed half', (base + prog) * 8)):
    best = 1e9
    for rep in range(3):
        t0 = time.perf_counter()
        (recs, st) = ctx.jpeg_process_batch(lst, H, W)
        best = min(best, time.perf_counter() - t0)
    ctx.set_profiling(1)
    ctx.jpeg_process_batch(lst, H, W)
    tm = ctx.timings()
    ctx.set_profiling(0)
    print(name, len(lst), 'files', 'status0', int((st == 0).sum()), '%.2f ms' % (best * 1e3), '%.0f files/s' % (len(lst) / best),
          {k: v for (k, v) in tm.items() if 'jpeg' in k.lower()}, flush=True)
# few progressive files among baseline ones: the GPU call as a whole, against Pillow for the k files + the GPU call for the rest
from concurrent.futures import ThreadPoolExecutor
pool = ThreadPoolExecutor(8)


def pillow(d):
    with Image.open(io.BytesIO(d)) as im:
        return np.asarray(im.convert('RGB'))[:, :, ::-1]


for k in (0, 1, 8, 32, 128, 256):
    lst = (base * 4)[:256 - k] + (prog * 4)[:k]
    (gpu, host) = (1e9, 1e9)
    for rep in range(3):
        t0 = time.perf_counter()
        (recs, st) = ctx.jpeg_process_batch(lst, H, W)
        gpu = min(gpu, time.perf_counter() - t0)
        assert (st == 0).all()
        t0 = time.perf_counter()
        frames = list(pool.map(pillow, lst[256 - k:]))
        if k < 256:
            ctx.jpeg_process_batch(lst[:256 - k], H, W)
        if k:
            reader.read_frames(np.stack(frames))
        host = min(host, time.perf_counter() - t0)
    print('256-file call, %3d progressive: GPU decode of all %.2f ms; host branch for the progressive ones %.2f ms' % (k, gpu * 1e3, host * 1e3), flush=True)
reader.close()
