"""What the frame-format rate tools share (pixel_format_rate, yuv_rate, yuv422_rate, yuv_matrix_rate, planar_rate, yuv_planar_rate,
yuv16_rate): the arguments, the fixture and the synthetic frames, the encoding of those frames as YUV and the header's integer conversion back,
the layout writers, and the measuring method.  A tool keeps its docstring, its rows, its own columns and its closing lines.

The method is bench.py's (timed_steps): frames resident in HBM, --nbuf distinct batches in rotation (more than the Infinity Cache
holds), consecutive steps alternating between two caller streams, records to a device buffer, the region between two device
synchronisations on the wall clock (Rates.run).  pixel_format_rate.py times differently -- one caller stream, events around the
steps (Rates.run_events) -- and shares the rest.

Importing this module creates no context and touches no device; the encoding functions work on CPU tensors as well
(tests/test_rate_tools.py compares them with tests/frame_cases.py, which the tools do not import: it pulls in pytest)."""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch  # before the package loads the library: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from meterelf_amd import _engine, _hip, _params  # noqa: E402
from meterelf_amd._image import imread_bgr  # noqa: E402

# matrix code: (YOFF, CY, CRV, CGV, CGU, CBU), YuvMatrix of meterelf_amd/csrc/melf_frame_layout.h
MATRIX = {
    0: (16, 1220542, 1673527, -852492, -409993, 2116026),
    2: (0, 1048576, 1470104, -748826, -360853, 1858077),
    3: (16, 1220945, 1879825, -558796, -223607, 2215014),
    4: (0, 1048576, 1651297, -490864, -196424, 1945738),
}
# Kr, Kb, limited range of each matrix name: the float conversion that makes frames of that standard
STANDARD = {'bt601': (0.299, 0.114, True), 'bt601-full': (0.299, 0.114, False), 'bt709': (0.2126, 0.0722, True), 'bt709-full': (0.2126, 0.0722, False)}


def arg_parser(steps=20, warmup=30, rounds=5, batch=1024, nbuf=4):
    """--steps --warmup --rounds --batch --nbuf with the tool's defaults; nbuf None: no --nbuf (one batch)."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=steps)
    ap.add_argument('--warmup', type=int, default=warmup)
    ap.add_argument('--rounds', type=int, default=rounds)
    ap.add_argument('--batch', type=int, default=batch)
    if nbuf is not None:
        ap.add_argument('--nbuf', type=int, default=nbuf)
    return ap


# ------------------------------------------------------------------------------------------------------------- encoding ---
def q8(t):
    return torch.clamp(torch.floor(t + 0.5), 0, 255).to(torch.uint8)


def encode(src, sub_x, sub_y, standard=None):
    """(m, H, W, 3) BGR -> Y (m, H, W), U and V (m, H >> sub_y, W >> sub_x) uint8: float64, the chroma block's mean, round half
    up.  standard None: BT.601 limited range from the three-decimal constants; a name of STANDARD: from its Kr and Kb."""
    f = src.to(torch.float64)
    (b, g, r) = (f[..., 0], f[..., 1], f[..., 2])
    if standard is None:
        y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
        u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
        v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    else:
        (kr, kb, limited) = STANDARD[standard]
        yl = kr * r + (1.0 - kr - kb) * g + kb * b
        (u, v) = ((b - yl) / (2.0 * (1.0 - kb)), (r - yl) / (2.0 * (1.0 - kr)))
        (y, u, v) = (16.0 + yl * 219.0 / 255.0, 128.0 + u * 224.0 / 255.0, 128.0 + v * 224.0 / 255.0) if limited else (yl, 128.0 + u, 128.0 + v)
    (m, H, W, _) = src.shape
    (ch, cw) = (H >> sub_y, W >> sub_x)
    return (q8(y), q8(u.reshape(m, ch, 1 << sub_y, cw, 1 << sub_x).mean(dim=(2, 4))),
            q8(v.reshape(m, ch, 1 << sub_y, cw, 1 << sub_x).mean(dim=(2, 4))))


def to_bgr(Y, U, V, sub_x, sub_y, matrix=0):
    """the conversion of include/meterelf_hip.h under matrix code `matrix`, in integers, nearest chroma sample"""
    (yoff, cy, crv, cgv, cgu, cbu) = MATRIX[matrix]
    yy = torch.clamp(Y.to(torch.int32) - yoff, min=0) * cy + (1 << 19)
    (ui, vi) = (U.to(torch.int32) - 128, V.to(torch.int32) - 128)
    if sub_y:
        (ui, vi) = (ui.repeat_interleave(2, dim=1), vi.repeat_interleave(2, dim=1))
    if sub_x:
        (ui, vi) = (ui.repeat_interleave(2, dim=2), vi.repeat_interleave(2, dim=2))
    out = torch.empty(Y.shape + (3,), dtype=torch.uint8, device=Y.device)
    out[..., 2] = torch.clamp((yy + crv * vi) >> 20, 0, 255).to(torch.uint8)
    out[..., 1] = torch.clamp((yy + cgv * vi + cgu * ui) >> 20, 0, 255).to(torch.uint8)
    out[..., 0] = torch.clamp((yy + cbu * ui) >> 20, 0, 255).to(torch.uint8)
    return out


def yuv_rows(H, sub_x, sub_y):
    """rows of the raw-video (N, rows, W) array of H-row frames"""
    return H + 2 * (H >> sub_y) // (1 << sub_x)


def write_yuv(out, Y, U, V, semi):
    """Y, U, V into out, the raw-video (m, rows, W) layout: the Y rows, then interleaved U V pairs (semi: NV12, NV16, NV24) or
    the U plane and the V plane (I420, I422, I444)."""
    (m, H, _W) = Y.shape
    (ch, cw) = U.shape[1:]
    out[:, :H] = Y
    c = out[:, H:].reshape(m, -1)
    if semi:
        c = c.reshape(m, ch, cw, 2)
        c[..., 0] = U
        c[..., 1] = V
    else:
        c[:, :ch * cw] = U.reshape(m, -1)
        c[:, ch * cw:] = V.reshape(m, -1)


def yuv_planes(arr, H, sub_x, sub_y, semi):
    """Y, U, V of a raw-video array that write_yuv made (views)"""
    (m, _rows, W) = arr.shape
    (ch, cw) = (H >> sub_y, W >> sub_x)
    c = arr[:, H:].reshape(m, -1)
    if semi:
        c = c.reshape(m, ch, cw, 2)
        return arr[:, :H], c[..., 0], c[..., 1]
    return arr[:, :H], c[:, :ch * cw].reshape(m, ch, cw), c[:, ch * cw:].reshape(m, ch, cw)


def write_422(out, Y, U, V, fmt):
    """Y, U, V (4:2:2) into out (m, H, W, 2), packed.  Bytes of a macropixel: yuyv: Y0 U Y1 V    uyvy: U Y0 V Y1    yvyu: Y0 V Y1 U"""
    (yb, cb) = (1, 0) if fmt == 'uyvy' else (0, 1)
    (first, second) = (V, U) if fmt == 'yvyu' else (U, V)
    out[..., yb] = Y
    out[:, :, 0::2, cb] = first
    out[:, :, 1::2, cb] = second


def write_planes(out, src):
    """(m, H, W, 3) BGR into out (m, 3, H, W): R, G, B planes"""
    out[...] = src.flip(3).permute(0, 3, 1, 2)


# -------------------------------------------------------------------------------------------------------------- harness ---
def forward_reversed(rows, r):
    return rows if r % 2 == 0 else rows[::-1]


def rotated(rows, r):
    return rows[r % len(rows):] + rows[:r % len(rows)]


class Rates:
    """The fixture (sample-images1: its params and the JPEGs of its commonest shape), the synthetic frames of args.batch x args.nbuf
    steps, and, after open(), a context, a record buffer for all N frames and two caller streams."""

    def __init__(self, args):
        self.args = args
        self.dev = torch.device('cuda', 0)
        torch.cuda.set_device(self.dev)
        gdir = os.path.join(ROOT, 'tests', 'golden', 'sample-images1')
        self.params = _params.load(os.path.join(gdir, 'params.yml'))
        base = [imread_bgr(f) for f in sorted(glob.glob(os.path.join(gdir, '*.jpg')))]
        shapes = [b.shape for b in base]
        self.base = torch.from_numpy(np.stack([b for b in base if b.shape == max(set(shapes), key=shapes.count)])).to(self.dev)   # the fixture's frame size
        (self.K, self.H, self.W, _) = self.base.shape
        (self.B, self.NB) = (args.batch, getattr(args, 'nbuf', 1))
        self.N = self.B * self.NB
        self.shifts = np.random.default_rng(3).integers(-8, 9, size=(self.N, 2))

    def chunks(self):
        """(i0, frames i0 .. i0 + 255) of the N synthetic BGR frames: fixture frame i % K rolled by its shift"""
        for i0 in range(0, self.N, 256):
            yield i0, torch.stack([torch.roll(self.base[i % self.K], shifts=(int(self.shifts[i, 1]), int(self.shifts[i, 0])), dims=(0, 1))
                                   for i in range(i0, min(i0 + 256, self.N))])

    def empty(self, *shape):
        """an uninitialised (N,) + shape byte array on the device, for the frames of all batches in one layout"""
        return torch.empty((self.N,) + shape, dtype=torch.uint8, device=self.dev)

    def open(self):
        self.ctx = _hip.Context(_engine.make_blob(self.params), 0)
        self.rsz = _hip.RESULT_DTYPE.itemsize
        self.d_res = torch.zeros((self.N, self.rsz), dtype=torch.uint8, device=self.dev)
        self.streams = [torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)]
        return self.ctx

    def close(self):
        self.ctx.sync()
        self.ctx.close()

    def step(self, call, frames, batch_bytes, *args):
        """fn(i, stream): call(batch i % nbuf of frames, *args) with that batch's records to its slice of the record buffer"""
        def fn(i, stream):
            k = i % self.NB
            call(frames.data_ptr() + k * batch_bytes, *args, d_results_ptr=self.d_res.data_ptr() + k * self.B * self.rsz, want_host=False,
                 stream=stream.cuda_stream)
        return fn

    def run(self, fn, steps, nstreams=2):
        """ms per step: wall clock between two device synchronisations, the steps alternating between the caller streams"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i, self.streams[i % nstreams])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    def run_events(self, fn, steps):
        """ms per step: events around the steps on one caller stream, the current one"""
        stream = torch.cuda.current_stream(self.dev)
        (e0, e1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e0.record(stream)
        for i in range(steps):
            fn(i, stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    def check_records(self, rows, ref_row, message, run=None):
        """Every row's records of all nbuf batches equal ref_row's, byte for byte (message(name) otherwise); the frames read."""
        run = run or self.run
        run(ref_row[1], self.NB)
        ref = self.d_res.clone()
        for (name, fn) in rows:
            self.d_res.zero_()
            run(fn, self.NB)
            assert torch.equal(self.d_res, ref), message(name)
        return int((ref.cpu().numpy().view(_hip.RESULT_DTYPE)['status'] == _hip.FRAME_OK).sum())

    def alternate(self, rows, order):
        """name: ms per step of each round.  The rows take turns, args.rounds rounds of args.steps steps in the order
        order(rows, round), after args.warmup untimed steps of each."""
        for (_name, fn) in rows:
            self.run(fn, self.args.warmup)
        times = {name: [] for (name, _fn) in rows}
        for r in range(self.args.rounds):
            for (name, fn) in order(rows, r):
                self.run(fn, 4)   # the other row's last steps are out of the lanes
                times[name].append(self.run(fn, self.args.steps))
        return times

    def kernel_times(self, rows, run=None, steps=None):
        """name: {kernel: ms per launch}: every kernel bracketed by events (melf_ctx_set_profiling), one caller stream"""
        run = run or (lambda fn, n: self.run(fn, n, 1))
        (first, second) = steps or (2 * self.NB, 2 * self.NB)
        kern = {}
        self.ctx.set_profiling(1)
        for (name, fn) in rows:
            run(fn, first)
            self.ctx.timings()
            run(fn, second)
            kern[name] = per_launch(self.ctx.timings())
        self.ctx.set_profiling(0)
        return kern


def per_launch(timings):
    return {k: (ms / max(cnt, 1)) for (k, (ms, cnt)) in timings.items() if cnt}


def kernel_columns(kern):
    return [(title, len(title), lambda name, k=k: '%.4f' % kern[name].get(k, 0.0)) for (title, k) in (('k_lplane ms', 'k_lplane'), ('k_dials ms', 'k_dials'))]


def print_table(header, rows, times, base_row, extra_columns=(), name=('row', 28), vs=('vs BGR', 7)):
    """header (if any), then one line per row: its name (name: the column's title and width), the median ms per step of its rounds, their
    min..max and the median's ratio to base_row's (vs: title and width) -- no times: none of these three -- then extra_columns:
    (title, width, name -> text)."""
    cols = list(extra_columns)
    if times is not None:
        base = float(np.median(times[base_row[0]]))
        cols = [('ms/step', 8, lambda n: '%.4f' % float(np.median(times[n]))),
                ('spread', 15, None),
                vs + (lambda n: '%.3fx' % (float(np.median(times[n])) / base),)] + cols
    if header:
        print(header)
    print('| %-*s | %s |' % (name[1], name[0], ' | '.join('%*s' % (w, t) for (t, w, _f) in cols)))
    print('|%s|' % '|'.join('-' * (w + 2) for w in [name[1]] + [w for (_t, w, _f) in cols]))
    for (n, _fn) in rows:
        # the spread is one character narrower than its title, as the tables under profiles/ have it
        cells = ['%6.4f..%6.4f' % (min(times[n]), max(times[n])) if f is None else '%*s' % (w, f(n)) for (_t, w, f) in cols]
        print('| %-*s | %s |' % (name[1], n, ' | '.join(cells)))
