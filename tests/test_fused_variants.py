"""Every kernel body of the fused full-frame mask (k_hls.hip: k_fused_mask_lut variants 0 / 1 / 2 / 3 / 4 / 6 / 7 / 8 and
the float-path kernel k_fused_mask), launched, ASSERTED to be the body that ran (melf_ctx_fused_variant) and compared with
the CPU oracle: on all 2^24 BGR triples and on structured frames whose blobs are in range for the bounds under test.
Further: melf_hls_inrange_close_dev on caller streams, the static split a context's 65th stream gets, and melf_bgr2hls on
all 2^24 triples.

Which body the default dispatch must pick is not copied from the product: it comes from tests/fused_census.py, a numpy
restatement over the oracle's H, L, S of every triple (tests/test_fused_census.py pins it on the CPU)."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

from tests import fused_census as fc
from tests.helpers import hip_runtime

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FLOAT = -1   # last_body of the float-path kernel k_fused_mask

# (id, bounds, environment that forces a body, the body that must run)
CASES = [
    ('red', 'red', {}, 6),
    ('green', 'green', {}, 7),
    ('blue', 'blue', {}, 8),
    ('red-bits', 'red', {'MELF_FUSED_VARIANT': 'bits'}, 0),
    ('green-bits', 'green', {'MELF_FUSED_VARIANT': 'bits'}, 1),
    ('blue-bits', 'blue', {'MELF_FUSED_VARIANT': 'bits'}, 2),
    ('several', 'several', {}, 3),
    ('seam', 'seam', {}, 3),
    ('oddshift', 'oddshift', {}, 3),
    ('red-generic', 'red', {'MELF_FUSED_VARIANT': 'generic'}, 3),
    ('several-ties', 'several', {'MELF_FUSED_VARIANT': 'ties'}, 4),
    ('red-float', 'red', {'MELF_FORCE_GENERIC_MASK': '1'}, FLOAT),
]
CASE_IDS = [c[0] for c in CASES]
QUEUE_BODIES = (0, 1, 2, 3, 6, 7, 8)   # launch shapes that can take their segments from a work queue (k_hls.hip, launch_lut_v)
# A launch of long runs for both launch shapes (256 and 512 workgroups): 640 frames of 240 x 320 take the work queue.
# (600 frames do so only with 512 workgroups, i.e. for the interval variants.)
BIG = (640, 240, 320)


@functools.lru_cache(maxsize=None)
def census(bounds):
    b = fc.BOUNDS[bounds]
    return fc.selection(b['needle']['shift'], b['lo'], b['hi'])


def _params_file(dirname, needle):
    src = os.path.join(GOLDEN, 'sample-images1')
    text = open(os.path.join(src, 'params.yml')).read()
    new = text.replace('hue_shift: 128', 'hue_shift: %d' % needle['shift'])
    new = new.replace('needle_color: {h: 125, l: 80, s: 130}', 'needle_color: {h: %(h)d, l: %(l)d, s: %(s)d}' % needle)
    new = new.replace('needle_color_range: {h: 9, l: 45, s: 35}', 'needle_color_range: {h: %(rh)d, l: %(rl)d, s: %(rs)d}' % needle)
    assert 'hue_shift: %d' % needle['shift'] in new and 'needle_color: {h: %(h)d,' % needle in new
    os.makedirs(dirname, exist_ok=True)
    with open(os.path.join(dirname, 'params.yml'), 'w') as fp:
        fp.write(new)
    shutil.copy(os.path.join(src, 'dials_gray.png'), os.path.join(dirname, 'dials_gray.png'))
    return os.path.join(dirname, 'params.yml')


class _Readers:
    """One reader per case, made on first use with the case's environment in force while the context is created and its
    tables are built (both switches are read then, never later)."""

    def __init__(self, base):
        self.base = base
        self.made = {}
        self.extra = []

    def new(self, bounds, environ):
        from meterelf_amd import MeterReader, _params
        pfile = _params_file(os.path.join(self.base, '%s-%d' % (bounds, len(self.extra) + len(self.made))), fc.BOUNDS[bounds]['needle'])
        old = {k: os.environ.get(k) for k in ('MELF_FUSED_VARIANT', 'MELF_FORCE_GENERIC_MASK')}
        try:
            for k in old:
                os.environ.pop(k, None)
            os.environ.update(environ)
            reader = MeterReader(_params.load(pfile))
            reader.ctx.fused_variant()   # builds the tables now
        finally:
            for (k, v) in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        p = reader.ctx.params
        assert (tuple(p.needle_lo), tuple(p.needle_hi), p.hue_shift) == (fc.BOUNDS[bounds]['lo'], fc.BOUNDS[bounds]['hi'],
                                                                         fc.BOUNDS[bounds]['needle']['shift'])
        return reader

    def get(self, case_id):
        if case_id not in self.made:
            (_id, bounds, environ, _body) = CASES[CASE_IDS.index(case_id)]
            self.made[case_id] = self.new(bounds, environ)
        return self.made[case_id]

    def fresh(self, bounds):
        self.extra.append(self.new(bounds, {}))
        return self.extra[-1]

    def close(self):
        for r in list(self.made.values()) + self.extra:
            r.close()


@pytest.fixture(scope='module')
def env(tmp_path_factory):
    from meterelf_amd import _hip
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    readers = _Readers(str(tmp_path_factory.mktemp('fused_variants')))
    yield readers
    readers.close()


def expected_body(body, H, W, aligned=True):
    """The body a launch of H x W frames must run: the float path for shapes and pointers the table kernel does not take."""
    return body if (body != FLOAT and aligned and W % 16 == 0 and 16 <= W <= 8192) else FLOAT


# ------------------------------------------------------------------ inputs ----

def background(in_range):
    """A colour that is out of range for the bounds (the all-triples construction and the holes in the blobs need one)."""
    for bgr in ((0, 0, 0), (255, 255, 255), (128, 128, 128), (0, 0, 255), (0, 255, 0), (255, 0, 0)):
        if not in_range[bgr[0] | bgr[1] << 8 | bgr[2] << 16]:
            return np.array(bgr, np.uint8)
    raise AssertionError('no out-of-range background among the candidates')


def blob_colour(in_range, rng):
    """(colour, noise amplitude): an in-range triple, chosen with the oracle's in-range bits, around which at least 70 % of
    the noisy neighbours are in range too -- with the largest of the amplitudes 25, 8, 2, 0 that allows it."""
    cand = rng.choice(np.flatnonzero(in_range), 256)
    cand = np.stack([cand & 255, (cand >> 8) & 255, cand >> 16], axis=-1)
    for amp in (25, 8, 2, 0):
        offs = rng.integers(-amp, amp + 1, size=(500, 3))
        px = np.clip(cand[:, None, :] + offs[None, :, :], 0, 255)
        frac = in_range[px[..., 0] | px[..., 1] << 8 | px[..., 2] << 16].mean(axis=1)
        if frac.max() >= 0.7:
            return (cand[int(frac.argmax())].astype(np.uint8), amp)
    raise AssertionError('unreachable: amplitude 0 keeps every neighbour in range')


def blobby(rng, n, H, W, colour, amp, hole):
    """Random frames with 8 x 8-blocked blobs of `colour` +- amp; a tenth of the blob pixels are holes of an out-of-range
    colour, so that the 3 x 3 closing has something to close."""
    base = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    small = rng.random((n, H // 8 + 1, W // 8 + 1)) < 0.35
    big = np.kron(small, np.ones((8, 8), bool))[:, :H, :W]
    noise = rng.integers(-amp, amp + 1, size=(n, H, W, 3), dtype=np.int16)
    blob = np.clip(colour[None, None, None, :].astype(np.int16) + noise, 0, 255).astype(np.uint8)
    blob[rng.random((n, H, W)) < 0.1] = hole
    base[big] = blob[big]
    return base


def structured_frames(bounds, n, H, W, seed):
    sel = census(bounds)
    rng = np.random.default_rng(seed)
    (colour, amp) = blob_colour(sel['in_range'], rng)
    hole = background(sel['in_range'])
    frames = blobby(rng, n, H, W, colour, amp, hole)
    # every frame, however small (W >= 16), starts with a closable hole: seven pixels of the in-range colour in row 0 with
    # an out-of-range pixel in the middle, which the closing fills even in a frame of one row
    frames[:, 0, 4:11] = colour
    frames[:, 0, 7] = hole
    return frames


def big_frames(bounds):
    (n, H, W) = BIG
    rng = np.random.default_rng(99)
    tiles = structured_frames(bounds, 8, H, W, 98)
    pick = rng.integers(0, 8, n)
    frames = tiles[pick]
    for i in range(n):
        frames[i] = np.roll(frames[i], (i * 13) % H, axis=0)
    return (frames, pick)


def oracle_mask(bounds, frame):
    """(closed mask, plain in-range bit) of one frame by the oracle."""
    from oracle import pyoracle as po
    b = fc.BOUNDS[bounds]
    shift = b['needle']['shift']
    exp = po.hls_inrange_close(frame, shift, list(b['lo']), list(b['hi']))
    hls = po.bgr2hls(frame, shift).astype(np.int32)
    plain = np.all((hls >= np.array(b['lo'])) & (hls <= np.array(b['hi'])), axis=-1)
    return (exp, plain)


# --------------------------------------------------------------- dispatch ----

@pytest.mark.parametrize('case', CASE_IDS)
def test_dispatch(env, case):
    """The context picks (or is forced to) the expected body, from the numbers the CPU census predicts, and a launch reports
    that body."""
    (_id, bounds, environ, body) = CASES[CASE_IDS.index(case)]
    ctx = env.get(case).ctx
    fv = ctx.fused_variant()
    sel = census(bounds)
    print(case, fv)
    # the three numbers do not depend on the switches
    assert (ctx.fused_table_ties(), fv['active_sectors'], fv['noniv']) == (sel['ties'], sel['active'], sel['noniv'])
    if not environ:
        assert fv['variant'] == sel['variant'] == body        # default dispatch: the census' prediction
    elif body != FLOAT:
        assert fv['variant'] == body
    else:
        assert fv['variant'] == sel['variant']                # the table variant is still chosen; it is just never launched
    frames = structured_frames(bounds, 2, 16, 32, 1)
    got = ctx.hls_inrange_close(frames)
    fv = ctx.fused_variant()
    # How the float path is known: the context records the kernel its last launch ran (melf_ctx_timings files both
    # kernels under k_fused_mask, so it cannot tell them apart).
    assert fv['last_body'] == body
    assert fv['last_queue_slot'] == -1                        # 2 frames: static split
    for f in range(2):
        assert np.array_equal(got[f], oracle_mask(bounds, frames[f])[0])


# ------------------------------------------------------------ all triples ----

SIDE = 512
PER = SIDE * SIDE
NCHUNKS = fc.N_TRIPLES // PER   # 64 chunks; chunk c holds r = 4c .. 4c + 3 with every (b, g)


# The isolated pixels keep 2 pixels away from the image border: the closing's border is neutral (nothing outside the image ever
# loses the erosion), so a pixel whose dilated 3 x 3 block touched the border would come out as 2 or 4 set pixels.
AT = (slice(2, 2 + 4 * SIDE, 4), slice(2, 2 + 4 * SIDE, 4))


def spaced_image(chunk, bg):
    """Chunk `chunk` of the 2^24 triples as isolated pixels, spacing 4, on the background: 2052 x 2064."""
    t = np.arange(chunk * PER, (chunk + 1) * PER, dtype=np.uint32)
    tri = np.stack([t & 255, (t >> 8) & 255, (t >> 16) & 255], axis=-1).astype(np.uint8).reshape(SIDE, SIDE, 3)
    img = np.empty((SIDE * 4 + 4, SIDE * 4 + 16, 3), np.uint8)
    img[:] = bg
    img[AT] = tri
    return img


@pytest.mark.parametrize('case', CASE_IDS)
def test_all_2_24_triples(env, case):
    """Every BGR triple as an isolated pixel on an out-of-range background, 64 images.  Each image is compared with the
    oracle's whole stage (HLS, inRange, dilate, erode) on the same image, and before that with the oracle's dense in-range bits
    of the 2^24 triples (its bgr2hls + the bounds), which names the triple and its table entries when a lookup is wrong."""
    from oracle import pyoracle as po
    (_id, bounds, _environ, body) = CASES[CASE_IDS.index(case)]
    ctx = env.get(case).ctx
    b = fc.BOUNDS[bounds]
    in_range = census(bounds)['in_range']
    total = int(in_range.sum())
    print(case, 'in-range triples:', total)
    assert total > 0
    bg = background(in_range)
    for chunk in range(NCHUNKS):
        img = spaced_image(chunk, bg)
        got = ctx.hls_inrange_close(img[None])[0]
        want = in_range[chunk * PER:(chunk + 1) * PER].reshape(SIDE, SIDE)
        diff = np.argwhere((got[AT] > 0) != want)
        if len(diff):
            t = chunk * PER + int(diff[0][0]) * SIDE + int(diff[0][1])
            raise AssertionError('chunk %d: triple b=%d g=%d r=%d (hue entry %d, L/S entry %d): got %d, oracle in range %s'
                                 % (chunk, t & 255, (t >> 8) & 255, t >> 16, fc.table_index()[0][t], fc.table_index()[1][t],
                                    got[AT][tuple(diff[0])], bool(want[tuple(diff[0])])))
        assert set(np.unique(got).tolist()) <= {0, 255}, chunk
        assert int(np.count_nonzero(got)) == int(want.sum()), chunk   # the isolated pixels are the only set pixels
        exp = po.hls_inrange_close(img, b['needle']['shift'], list(b['lo']), list(b['hi']))
        assert np.array_equal(got, exp), chunk
    assert ctx.fused_variant()['last_body'] == body


# ------------------------------------------------------ structured frames ----

SHAPES = [(3, 640, 480), (2, 37, 48), (5, 3, 16), (1, 1, 32), (2, 70, 1920), (1, 2, 16),
          (2, 37, 53), (1, 33, 100)]   # the last two: W % 16 != 0, the float path whatever the case


@pytest.mark.parametrize('case', CASE_IDS)
def test_structured_frames(env, case):
    """Blobs in range for the bounds under test, with holes: against the oracle, against the same frames one at a time, and
    in every frame of every shape the oracle's mask has set pixels and differs from the plain in-range bit (the closing
    changed something)."""
    (_id, bounds, _environ, body) = CASES[CASE_IDS.index(case)]
    ctx = env.get(case).ctx
    for (n, H, W) in SHAPES:
        frames = structured_frames(bounds, n, H, W, H * W + n)
        got = ctx.hls_inrange_close(frames)
        assert ctx.fused_variant()['last_body'] == expected_body(body, H, W), (n, H, W)
        for f in range(n):
            (exp, plain) = oracle_mask(bounds, frames[f])
            assert np.array_equal(got[f], exp), ((n, H, W), f, np.argwhere(got[f] != exp)[:5])
            assert (exp > 0).any() and ((exp > 0) != plain).any(), ((n, H, W), f)
            if n > 1:
                assert np.array_equal(ctx.hls_inrange_close(frames[f:f + 1])[0], got[f]), ((n, H, W), f)


@pytest.mark.parametrize('case', CASE_IDS)
def test_work_queue_launch(env, case):
    """One launch of long runs: the bodies that have a queue-fed launch shape take a work-queue slot, variant 4 and the float
    path do not; the masks equal those of the same frames in pieces (static split) and the oracle's."""
    (_id, bounds, _environ, body) = CASES[CASE_IDS.index(case)]
    ctx = env.get(case).ctx
    (frames, pick) = big_frames(bounds)
    n = len(frames)
    whole = ctx.hls_inrange_close(frames)
    fv = ctx.fused_variant()
    assert fv['last_body'] == body
    assert (fv['last_queue_slot'] >= 0) == (body in QUEUE_BODIES), fv
    parts = []
    for a in range(0, n, 40):
        parts.append(ctx.hls_inrange_close(frames[a:a + 40]))
        assert ctx.fused_variant()['last_queue_slot'] == -1
    assert np.array_equal(np.concatenate(parts), whole)
    # the oracle on the first frame made of each of the 8 tiles, and on the last frame
    sample = sorted({int(np.flatnonzero(pick == k)[0]) for k in range(8)} | {n - 1})
    assert len(sample) >= 8
    for f in sample:
        (exp, plain) = oracle_mask(bounds, frames[f])
        assert np.array_equal(whole[f], exp), (f, np.argwhere(whole[f] != exp)[:5])
        assert (exp > 0).any() and ((exp > 0) != plain).any(), f
    # a second launch right behind the first finds its queue slot zeroed again
    assert np.array_equal(ctx.hls_inrange_close(frames), whole)
    assert ctx.fused_variant()['last_queue_slot'] == fv['last_queue_slot']


# ------------------------------------------------- the device entry point ----

class _Dev:
    """Device buffers and streams from the HIP runtime the library is bound to; everything is released in close()."""

    def __init__(self):
        self.hip = hip_runtime()
        self.bufs = []
        self.streams = []

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        self.bufs.append(p)
        return p.value

    def stream(self):
        s = C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0   # hipStreamNonBlocking
        self.streams.append(s)
        return s.value

    def upload(self, dptr, a):
        a = np.ascontiguousarray(a)
        assert self.hip.hipMemcpy(C.c_void_p(dptr), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0

    def download(self, dptr, shape):
        out = np.empty(shape, np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), C.c_size_t(out.nbytes), 2) == 0
        return out

    def fill(self, dptr, value, nbytes):
        assert self.hip.hipMemset(C.c_void_p(dptr), value, C.c_size_t(nbytes)) == 0

    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0

    def close(self):
        self.hip.hipDeviceSynchronize()
        for s in self.streams:
            self.hip.hipStreamDestroy(s)
        for p in self.bufs:
            self.hip.hipFree(p)


@pytest.mark.parametrize('case', ['red', 'green-bits', 'several', 'several-ties'])
@pytest.mark.parametrize('off_frames,off_masks', [(4, 0), (0, 4), (4, 4)])
def test_dev_entry_misaligned_pointers_take_the_float_path(env, case, off_frames, off_masks):
    """Device pointers off by 4 bytes: the table kernel's 16-byte loads and stores do not apply, the float-path kernel runs
    (on a shape the table kernel would take) and gives the oracle's masks."""
    (_id, bounds, _environ, body) = CASES[CASE_IDS.index(case)]
    ctx = env.get(case).ctx
    (n, H, W) = (2, 37, 48)
    frames = structured_frames(bounds, n, H, W, 5)
    dev = _Dev()
    try:
        d_in = dev.malloc(frames.nbytes + 16)
        d_out = dev.malloc(n * H * W + 32)
        dev.fill(d_out, 0x55, n * H * W + 32)
        dev.upload(d_in + off_frames, frames)
        ctx.hls_inrange_close_dev(d_in + off_frames, n, H, W, d_out + off_masks, stream=None)
        assert ctx.fused_variant()['last_body'] == FLOAT
        dev.sync()
        raw = dev.download(d_out, (n * H * W + 32,))
        got = raw[off_masks:off_masks + n * H * W].reshape(n, H, W)
        assert (raw[:off_masks] == 0x55).all() and (raw[off_masks + n * H * W:] == 0x55).all()   # nothing written outside
        for f in range(n):
            assert np.array_equal(got[f], oracle_mask(bounds, frames[f])[0]), f
        # the same buffers, aligned: the table kernel again
        dev.upload(d_in, frames)
        ctx.hls_inrange_close_dev(d_in, n, H, W, d_out, stream=None)
        assert ctx.fused_variant()['last_body'] == body
        dev.sync()
        assert np.array_equal(dev.download(d_out, (n, H, W)), got)
    finally:
        dev.close()


def test_dev_entry_on_caller_streams(env):
    """melf_hls_inrange_close_dev on the null stream and on two caller streams, enqueued back to back: the masks of the host
    entry (which runs on the context's own stream)."""
    ctx = env.get('red').ctx
    (n, H, W) = (6, 96, 160)
    frames = structured_frames('red', n, H, W, 6)
    ref = ctx.hls_inrange_close(frames)
    for f in range(n):
        assert np.array_equal(ref[f], oracle_mask('red', frames[f])[0])
    dev = _Dev()
    try:
        d_in = dev.malloc(frames.nbytes)
        d_out = [dev.malloc(n * H * W) for _ in range(3)]
        dev.upload(d_in, frames)
        for d in d_out:
            dev.fill(d, 0x55, n * H * W)
        dev.sync()
        streams = [None, dev.stream(), dev.stream()]
        for rep in range(2):
            for (s, d) in zip(streams, d_out):
                ctx.hls_inrange_close_dev(d_in, n, H, W, d, stream=s)
                assert ctx.fused_variant()['last_body'] == 6
        dev.sync()
        for d in d_out:
            assert np.array_equal(dev.download(d, (n, H, W)), ref)
    finally:
        ctx.sync()
        dev.close()


def test_65th_stream_of_a_context_takes_the_static_split(env):
    """A work-queue slot belongs to one (context, stream); a context has 64.  Queue-sized launches on 65 distinct caller
    streams: the first 64 get slots 0 .. 63, the 65th launch runs with the static split -- and gives the same masks, the
    oracle's.  (A slot is claimed only by a launch that takes the queue, hence the 640-frame batch; the frames are small,
    they are uploaded once and every launch reads the same device buffer.)"""
    reader = env.fresh('red')
    ctx = reader.ctx
    (n, H, W) = BIG
    (frames, _pick) = big_frames('red')
    dev = _Dev()
    try:
        d_in = dev.malloc(frames.nbytes)
        d_out = dev.malloc(n * H * W)
        dev.upload(d_in, frames)
        first = None
        for k in range(65):
            dev.fill(d_out, 0x55, n * H * W)
            dev.sync()
            ctx.hls_inrange_close_dev(d_in, n, H, W, d_out, stream=dev.stream())
            fv = ctx.fused_variant()
            assert (fv['last_body'], fv['last_queue_slot']) == (6, k if k < 64 else -1), (k, fv)
            dev.sync()
            if k in (0, 63):
                got = dev.download(d_out, (n, H, W))
                if first is None:
                    first = got
                assert np.array_equal(got, first), k
        static = dev.download(d_out, (n, H, W))
        assert np.array_equal(static, first)
        for f in (0, 1, 320, n - 2, n - 1):
            exp = oracle_mask('red', frames[f])[0]
            assert np.array_equal(static[f], exp), (f, np.argwhere(static[f] != exp)[:5])
        assert (static > 0).any()
        # a stream that has its slot keeps it
        ctx.hls_inrange_close_dev(d_in, n, H, W, d_out, stream=dev.streams[3].value)
        assert ctx.fused_variant()['last_queue_slot'] == 3
        dev.sync()
        assert np.array_equal(dev.download(d_out, (n, H, W)), first)
    finally:
        ctx.sync()
        dev.close()


# ----------------------------------------------------------------- bgr2hls ----

@pytest.mark.parametrize('case,shift', [('green', 0), ('red', 128)])
def test_bgr2hls_all_2_24_triples(env, case, shift):
    """The GPU's hls_pixel against the oracle for every BGR triple (the CPU census of tests/test_fused_census.py rests on the
    oracle's values; this carries it over to the float path the table builder evaluates)."""
    ctx = env.get(case).ctx
    assert ctx.params.hue_shift == shift
    got = ctx.bgr2hls(fc.all_triples_image()).reshape(-1, 3)
    exp = np.stack(fc.hls_of_all_triples(shift), axis=-1)
    diff = np.flatnonzero((got != exp).any(axis=1))
    assert len(diff) == 0, [(int(t) & 255, (int(t) >> 8) & 255, int(t) >> 16, got[t].tolist(), exp[t].tolist()) for t in diff[:5]]
