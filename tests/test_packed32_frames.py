"""melf_process_packed32* / melf_packed32_to_bgr: 4:4:4 frames of one 32-bit word per pixel -- AYUV / VUYA (8-bit), Y410 / XV30 and
V30X (10-bit YUV) as hardware 4:4:4 decoders deliver them, X2RGB10 / X2BGR10 (10-bit RGB) as scan-out, desktop duplication and camera
ISPs do -- read in place.

The contract (include/meterelf_hip.h): a word holds three 8-bit reads s8_k = (word >> pos[k]) & 255, every other bit ignored.  YUV:
the records are byte-identical to melf_process_yuv_planar(_dev) on the 8-bit i444 frame of the s8, and so to melf_process_batch on
the BGR frame the header's integer conversion makes of it; RGB: to melf_process_batch on the BGR frame of the s8.  tests/p32_cases.py
restates the layout in numpy; the GPU tests compare all records, as bytes, with the EXISTING paths' records of the unpacked frames
(p32_cases.want_8bit).

The dial kernels' instantiations: tests/test_packed32_dials.py.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import p32_cases as pc  # noqa: E402
from tests.frame_cases import DevBuf, env  # noqa: E402,F401

FIELDS = ('colour', 'matrix', 'n', 'H', 'W', 'pos', 'row_pitch', 'frame_stride', 'reserved', 'reserved2')
MATRICES = (0, 2, 3, 4)
FORBIDDEN = ('k_dials', 'k_needles', 'k_prep_lplane', 'k_match_mfma', 'k_match_gen', 'k_v210_', 'k_y210_', 'k_y16_', 'k_yp_')


def aligned_zeros(shape, dtype, lead=0):
    """A zeroed array whose first byte lies `lead` bytes behind a multiple of 64."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(nbytes + 128, np.uint8)
    at = -raw.ctypes.data % 64 + lead
    return raw[at:at + nbytes].view(dtype).reshape(shape)


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_struct_and_constants(tmp_path):
    src = tmp_path / 'p32.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(melf_packed32_frames));\n'
                   + ''.join('printf(" %%zu", offsetof(melf_packed32_frames, %s));\n' % f for f in FIELDS)
                   + 'printf(" %zu", sizeof(((melf_packed32_frames*)0)->pos));\n'
                   + 'printf(" %d %d %d %d %d %d %d %d\\n", MELF_ABI_VERSION, MELF_DIALS_FAMILIES, MELF_DIALS10_V210, MELF_DIALS10_Y210,'
                     ' MELF_DIALS32_YUV, MELF_DIALS32_RGB, MELF_P32_YUV, MELF_P32_RGB);return 0;}\n')
    exe = tmp_path / 'p32'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfPacked32Frames
    assert tuple(f[0] for f in F._fields_) == FIELDS
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in FIELDS] + [12, 3, 12, 14, 15, 16, 17, 0, 1]
    assert _hip.ABI_VERSION == 3 and (_hip.P32_YUV, _hip.P32_RGB) == (0, 1)
    for name in ('melf_process_packed32', 'melf_process_packed32_dev', 'melf_packed32_to_bgr'):
        assert name in _hip.EXPORTS
    assert _hip.DIALS32_FAMILIES == ('p32yuv', 'p32rgb')
    assert _hip.DIALS10_FAMILIES == ('v210', 'y210') and len(_hip.DIALS_FAMILIES) == 12 and len(_hip.DIALS16_FAMILIES) == 2
    with open(os.path.join(ROOT, 'include', 'meterelf_hip.h')) as fp:
        text = fp.read()
    assert {m.group(1): int(m.group(2)) for m in re.finditer(r'\bMELF_DIALS32_([A-Z0-9_]+) = (\d+)', text)} == {'YUV': 16, 'RGB': 17}


def test_format_table_is_the_header_table():
    """_hip.PACKED32_FORMATS == the table restated in p32_cases == the rows of the header's comment, aliases included; the reads of
    every format are 8 bits apart or more, inside the word."""
    kinds = {'yuv': _hip.P32_YUV, 'rgb': _hip.P32_RGB}
    want = {name: (kinds[k], pos) for (name, (k, pos)) in pc.TABLE.items()}
    want.update({alias: want[name] for (alias, name) in pc.ALIASES.items()})
    assert _hip.PACKED32_FORMATS == want
    with open(os.path.join(ROOT, 'include', 'meterelf_hip.h')) as fp:
        text = fp.read()
    rows = {}
    for m in re.finditer(r'^ \*     (\S.*?)\s+(YUV|RGB)\s+(\d+),\s+(\d+),\s+(\d+)  ', text, re.M):
        names = [x.lower() for x in re.findall(r'[A-Za-z][A-Za-z0-9]*', m.group(1))]
        for name in names:
            if name in _hip.PACKED32_FORMATS:
                rows[name] = (kinds[m.group(2).lower()], tuple(int(m.group(k)) for k in (3, 4, 5)))
    assert rows == _hip.PACKED32_FORMATS, sorted(set(_hip.PACKED32_FORMATS) ^ set(rows))
    for (name, (_c, pos)) in _hip.PACKED32_FORMATS.items():
        assert all(0 <= p <= 24 for p in pos) and all(abs(a - b) >= 8 for (a, b) in ((pos[0], pos[1]), (pos[0], pos[2]), (pos[1], pos[2]))), name
    # what the positions mean: a byte b is read from bit 8 b, a 10-bit field at bit o from o + 2
    assert pc.pos_of('vuya') == (8 * 2, 8 * 1, 8 * 0) and pc.pos_of('ayuv') == (8 * 1, 8 * 2, 8 * 3) and pc.pos_of('uyva') == (8 * 1, 8 * 0, 8 * 2)
    assert pc.pos_of('y410') == (10 + 2, 0 + 2, 20 + 2) and pc.pos_of('v30x') == (12 + 2, 2 + 2, 22 + 2)
    assert pc.pos_of('x2rgb10') == (20 + 2, 10 + 2, 0 + 2) and pc.pos_of('x2bgr10') == (0 + 2, 10 + 2, 20 + 2)


def test_reader_method_matrix_rules():
    import inspect
    from meterelf_amd import MeterReader
    sig = inspect.signature(MeterReader.read_packed32_frames)
    assert sig.parameters['pixel_format'].default is inspect.Parameter.empty
    assert sig.parameters['matrix'].default is None and sig.parameters['out'].default is None
    assert list(sig.parameters)[1:] == ['frames', 'pixel_format', 'matrix', 'out']
    assert inspect.signature(_hip.packed32_frames_view).parameters['matrix'].default is None
    z = aligned_zeros((1, 4, 8), np.uint32)
    for fmt in pc.YUV_FORMATS + ('vuyx', 'xv30'):
        with pytest.raises(ValueError):
            _hip.packed32_frames_view(z, fmt)                      # no default: the wrong matrix raises no error
        with pytest.raises(ValueError):
            _hip.packed32_frames_view(z, fmt, None)
        assert _hip.packed32_frames_view(z, fmt, 'bt709').matrix == 3
    for fmt in pc.RGB_FORMATS + ('xrgb2101010', 'xbgr2101010', 'r10g10b10a2'):
        for m in ('bt709', 0, 3):
            with pytest.raises(ValueError):
                _hip.packed32_frames_view(z, fmt, m)               # RGB: nothing is converted
        assert _hip.packed32_frames_view(z, fmt).matrix == 0 and _hip.packed32_frames_view(z, fmt, None).colour == _hip.P32_RGB


@pytest.mark.parametrize('W', [1, 2, 3, 5, 50])
def test_packers_round_trip(W):
    rng = np.random.default_rng(W)
    (n, H) = (2, 3)
    reads = tuple(rng.integers(0, 256, (n, H, W), dtype=np.uint8) for _k in range(3))
    for fmt in pc.FORMATS:
        words = pc.pack32(reads, pc.pos_of(fmt), rng)
        assert words.shape == (n, H, W) and words.dtype == np.uint32
        for (a, b) in zip(pc.unpack32(words, pc.pos_of(fmt)), reads):
            assert np.array_equal(a, b), (fmt, W)
    # the ignored bits are random, and they do not come back
    big = pc.pack32(tuple(np.full((1, 8, 64), 200, np.uint8) for _k in range(3)), pc.pos_of('y410'), rng)
    assert len(np.unique(big & 3)) == 4 and len(np.unique(big >> 30)) == 4 and len(np.unique((big >> 10) & 3)) == 4
    assert (pc.unpack32(big, pc.pos_of('y410'))[0] == 200).all()
    # the byte formats, as bytes in memory: vuya is V U Y A, ayuv A Y U V, uyva U Y V A
    for (fmt, order) in (('vuya', (2, 1, 0)), ('ayuv', (1, 2, 3)), ('uyva', (1, 0, 2))):
        b = np.ascontiguousarray(pc.pack32(reads, pc.pos_of(fmt), rng)).view(np.uint8).reshape(n, H, W, 4)
        for (k, at) in enumerate(order):
            assert np.array_equal(b[..., at], reads[k]), (fmt, k)


def test_every_position_at_every_value():
    """Each of the three reads at every legal position 0 .. 24 and every value 0 .. 255, the other two placed so that they do not
    overlap, every other bit random: unpack32 gives the value, by a shift and a mask written out here, and the other reads are those
    of the random bits."""
    rng = np.random.default_rng(32)
    values = np.arange(256, dtype=np.uint32)
    cases = 0
    for (k, pos) in position_cases():
        w = rng.integers(0, 2 ** 32, size=(1, 1, 256), dtype=np.uint32)
        w[0, 0] = (w[0, 0] & ~np.uint32(255 << pos[k])) | (values << np.uint32(pos[k]))
        got = pc.unpack32(w, pos)
        assert np.array_equal(got[k][0, 0], values.astype(np.uint8)), (k, pos)
        for j in range(3):
            if j != k:
                assert np.array_equal(got[j][0, 0], ((w[0, 0] >> np.uint32(pos[j])) % 256).astype(np.uint8)), (k, j, pos)
        cases += 1
    assert cases == 75


def position_cases():
    """(k, pos): read k at each of 0 .. 24, the two others non-overlapping: 75 descriptors."""
    for k in range(3):
        for p in range(25):
            # two slots of 8 bits that keep clear of [p, p + 8): below it where there is room, else above
            others = [q for q in (0, 8, 16, 24) if abs(q - p) >= 8][:2] if p % 8 == 0 else \
                [q for q in (p - 16, p - 8, p + 8, p + 16) if 0 <= q <= 24][:2]
            assert len(others) == 2 and all(abs(q - p) >= 8 for q in others) and abs(others[0] - others[1]) >= 8, (p, others)
            pos = [0, 0, 0]
            pos[k] = p
            (pos[(k + 1) % 3], pos[(k + 2) % 3]) = others
            yield k, tuple(pos)


def _makers32():
    yield lambda a: a
    try:
        import torch
    except ImportError:
        return
    yield lambda a: torch.from_numpy(a.view(np.int32))   # the same bits


def test_view_layouts():
    (n, H, W) = (3, 4, 10)
    view = _hip.packed32_frames_view
    for make in _makers32():
        base = aligned_zeros((n, H, W), np.uint32)
        v = view(make(base), 'y410', 'bt709')
        assert not v.copied and v.ptr == base.ctypes.data and not v.on_device and v.matrix == 3 and v.colour == 0 and v.pos == (12, 2, 22)
        assert (v.n, v.H, v.W, v.row_pitch, v.frame_stride, v.extent) == (n, H, W, 4 * W, 4 * W * H, n * H * 4 * W)
        d = v.descriptor()
        assert (d.colour, d.matrix, d.n, d.H, d.W, tuple(d.pos), d.row_pitch, d.frame_stride, d.reserved, d.reserved2) == \
            (0, 3, n, H, W, (12, 2, 22), 4 * W, 4 * W * H, 0, 0)
        assert v.extent == pc.extent32(d)
        r = view(make(base), 'X2RGB10')
        assert not r.copied and r.colour == 1 and r.matrix == 0 and r.pos == (22, 12, 2) and r.extent == v.extent
        # every other frame, a slice of frames, rows cut to w words, every other row: in place
        v2 = view(make(base)[::2], 'vuya', 4)
        assert not v2.copied and v2.n == 2 and v2.frame_stride == 8 * W * H and v2.extent == 3 * H * 4 * W and v2.matrix == 4
        v3 = view(make(base)[1:], 'ayuv', 0)
        assert not v3.copied and v3.ptr == base.ctypes.data + 4 * W * H and v3.n == 2
        for w in (7, 1):
            vw = view(make(base)[:, :, :w], 'v30x', 'bt709')
            assert not vw.copied and vw.ptr == base.ctypes.data and (vw.W, vw.row_pitch, vw.frame_stride) == (w, 4 * W, 4 * W * H)
            assert vw.extent == (n - 1) * 4 * W * H + (H - 1) * 4 * W + 4 * w
        vx = view(make(base)[:, :, 3:], 'uyva', 2)
        assert not vx.copied and vx.ptr == base.ctypes.data + 12 and vx.W == W - 3   # a base at 12 modulo 16
        vr = view(make(base)[:, ::2], 'x2bgr10')
        assert not vr.copied and (vr.H, vr.row_pitch) == (2, 8 * W)
        # a pixel stride of two words: copied
        ve = view(make(aligned_zeros((n, H, 2 * W), np.uint32))[:, :, ::2], 'y410', 'bt709')
        assert ve.copied and (ve.row_pitch, ve.frame_stride) == (4 * W, 4 * W * H) and ve.ptr % 4 == 0
        assert view(make(base)[:0], 'y410', 'bt709').extent == 0
    # the byte formats as (N, H, W, 4) uint8, numpy and torch; a 10-bit format has no such form
    def makers8():
        yield lambda a: a
        try:
            import torch
        except ImportError:
            return
        yield torch.from_numpy
    for make in makers8():
        b8 = aligned_zeros((n, H, W, 4), np.uint8)
        for fmt in ('vuya', 'ayuv', 'uyva', 'vuyx'):
            v = view(make(b8), fmt, 'bt601')
            assert not v.copied and v.ptr == b8.ctypes.data and (v.n, v.H, v.W, v.row_pitch, v.frame_stride) == (n, H, W, 4 * W, 4 * W * H) and v.matrix == 0
            vw = view(make(b8)[::2, :, :5], fmt, 'bt601')
            assert not vw.copied and (vw.n, vw.W, vw.row_pitch, vw.frame_stride) == (2, 5, 4 * W, 8 * W * H)
        assert view(make(aligned_zeros((n, H, W, 8), np.uint8))[..., ::2], 'vuya', 0).copied    # a byte stride of 2
        for fmt in ('y410', 'x2rgb10'):
            with pytest.raises(ValueError):
                view(make(b8), fmt, pc.matrix_of(fmt))


def test_view_errors():
    view = _hip.packed32_frames_view
    z = aligned_zeros
    for name in ('yuyv', 'v210', 'p010', 'nv12', 'i444', 'rgb', 'bgra', 'y416', 'r210'):
        with pytest.raises(ValueError):
            view(z((1, 4, 8), np.uint32), name, 'bt709')                   # names of the other families, unknown names
    for m in ('bt2020', 1, 5):
        with pytest.raises(ValueError):
            view(z((1, 4, 8), np.uint32), 'y410', m)                       # unknown matrix (code 1 is never assigned)
    for dt in (np.uint16, np.int32, np.float32, np.uint64):
        with pytest.raises(ValueError):
            view(z((1, 4, 8), dt), 'y410', 'bt709')                        # not 32-bit words (numpy int32: view it as uint32)
    with pytest.raises(ValueError):
        view(z((4, 8), np.uint32), 'y410', 'bt709')                        # rank
    with pytest.raises(ValueError):
        view(z((1, 4, 8, 4), np.uint32), 'vuya', 'bt709')                  # four dimensions are bytes
    with pytest.raises(ValueError):
        view(z((1, 4, 8, 3), np.uint8), 'vuya', 'bt709')                   # ... four of them a pixel
    with pytest.raises(ValueError):
        view(z((1, 0, 8), np.uint32), 'y410', 'bt709')
    for lead in (1, 2, 3):
        with pytest.raises(ValueError):
            view(z((1, 4, 8, 4), np.uint8, lead), 'vuya', 'bt709')         # a base that is not 4-byte aligned
    with pytest.raises(ValueError):
        view(z((1, 4, 9, 4), np.uint8).reshape(-1)[2:2 + 128].view(np.uint8).reshape(1, 4, 8, 4), 'ayuv', 'bt709')
    for lead in (4, 8, 12):
        assert not view(z((1, 4, 8), np.uint32, lead), 'y410', 'bt709').copied


def test_checks_and_load_bounds(tmp_path):
    """tests/p32_bounds_main.cpp, plain and under the host sanitizers: check_packed32 over accepted and rejected descriptors,
    DialWord32<true | false> of melf_frame_src.h on exact-extent heap buffers against plain indexing, and the prep arm's functions
    of melf_prep_addr.h.  Built with the ROCm tree's clang++ as a plain C++ compiler, as tests/p10_bounds_main.cpp is."""
    from tests import test_dials_instantiations as di
    (cxx, inc) = di.rocm_clangxx()
    out = fc.build_and_run(tmp_path, cxx, os.path.join(ROOT, 'tests', 'p32_bounds_main.cpp'), 'p32_bounds', ['-D__HIP_PLATFORM_AMD__', '-I' + inc],
                           ['-fsanitize=address,undefined'])
    assert 'window loads at base + 0, 4, 8, 12 mod 16' in out and 'word by word' in out, out


def test_kernels_metadata():
    """The kernels that read these frames are in the library: 12 needle, 2 lplane, 2 match and 2 to_bgr kernels, wave size 64, no
    private segment, no spilled vector registers; the dial readers within the dial kernels' register budget (128)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    new = {k: d for (k, d) in meta.items() if 'k_p32_' in k}
    counts = [sum(('k_p32_%s' % s) in k for k in new) for s in ('needle', 'lplane', 'match', 'to_bgr')]
    assert counts == [12, 2, 2, 2], counts
    assert len(new) == 18
    for (k, d) in new.items():
        assert d.get('private_segment_fixed_size', 0) == 0 and d.get('vgpr_spill_count', 0) == 0 and d['wavefront_size'] == 64, (k, d)
        if 'needle' in k:
            assert d['vgpr_count'] <= 128, (k, d)
        for other in FORBIDDEN:   # what existing tests count kernels by
            assert other not in k, (k, other)


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _restated_bgr(words, colour, pos, matrix):
    reads = pc.unpack32(words, pos)
    if colour == _hip.P32_YUV:
        return fc.yuv_to_bgr(*reads, 0, 0, matrix)
    return np.stack([reads[2], reads[1], reads[0]], axis=-1)


@pytest.mark.gpu
@pytest.mark.parametrize('matrix', MATRICES)
@pytest.mark.parametrize('fmt', pc.FORMATS)
def test_to_bgr(env, fmt, matrix):
    """The stage kernel == the layout restated + the conversion restated (RGB: the reads themselves), byte for byte: a 256 x 256
    frame whose first read (Y / R) takes all 256 values against 65 536 random others, every ignored bit random; and one 75 x 256
    frame given by raw descriptors, each of the three reads at each position 0 .. 24 (the two others placed non-overlapping) taking
    every value."""
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(100 + matrix)
    (colour, pos) = _hip.PACKED32_FORMATS[fmt]
    reads = ((np.arange(65536, dtype=np.uint32) & 255).astype(np.uint8).reshape(1, 256, 256),
             rng.integers(0, 256, (1, 256, 256), dtype=np.uint8), rng.integers(0, 256, (1, 256, 256), dtype=np.uint8))
    src = reads if colour == _hip.P32_YUV else (np.stack([reads[2], reads[1], reads[0]], axis=-1),)
    (buf, desc) = pc.pitched32(*src, fmt, row_pad=16, rng=rng, matrix=matrix)
    got = ctx.packed32_to_bgr(buf.ctypes.data, desc)
    want = _restated_bgr(pc.pack32(reads, pos, rng), colour, pos, matrix)
    bad = np.flatnonzero((got != want).any(axis=-1).ravel())
    assert bad.size == 0, (fmt, matrix, bad.size, bad[:8])
    # every position: row r of the 75-row frame belongs to descriptor r, read on its own as a one-row frame
    values = np.arange(256, dtype=np.uint32)
    cases = list(position_cases())
    words = rng.integers(0, 2 ** 32, size=(len(cases), 256), dtype=np.uint32)
    assert words.shape == (75, 256)
    for (r, (k, p)) in enumerate(cases):
        words[r] = (words[r] & ~np.uint32(255 << p[k])) | (values << np.uint32(p[k]))
    for (r, (k, p)) in enumerate(cases):
        d = pc.descriptor(fmt, matrix, 1, 1, 256, 4 * 256, 4 * 256, pos=p)
        got = ctx.packed32_to_bgr(words[r].ctypes.data, d)
        want = _restated_bgr(words[r].reshape(1, 1, 256), colour, p, matrix)
        assert np.array_equal(got, want), (fmt, matrix, k, p)
    # ... and the frame as a whole under its last descriptor: 75 rows
    d = pc.descriptor(fmt, matrix, 1, 75, 256, 4 * 256, 75 * 4 * 256, pos=cases[-1][1])
    assert np.array_equal(ctx.packed32_to_bgr(words.ctypes.data, d), _restated_bgr(words.reshape(1, 75, 256), colour, cases[-1][1], matrix))


IDENTITY_SET = ('sample-images1', 81)
IDENTITY_MIN_OK = (3 * IDENTITY_SET[1] + 3) // 4   # three quarters of the set: the floor tests/test_yuv_planar_frames.py puts on the same frames and seed for 4:4:4


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', pc.FORMATS)
def test_identity_on_fixture_pictures(env, fmt):
    """Every fixture frame of sample-images1 (frame_cases.fixture_frames, the seed of the planar 4:4:4 test) through
    frame_cases.check_formats on the family: the reader, the host and the device entry point, the caller's array and a pitched
    buffer of exact extent.  The expected records come from the existing paths -- read_yuv_planar_frames of the i444 frames of the
    same samples, read_frames for RGB --, both asserted equal to read_frames of bgr_of; the cap on unread frames is a condition on
    THOSE records."""
    (sd, count) = IDENTITY_SET
    matrix = 0   # BT.601 limited: the matrix of the planar 4:4:4 test on these frames
    fam = pc.family(pc.kind_of(fmt), matrix)

    def check(reader, src, tag, rng):
        want = pc.want_8bit(reader, src, pc.kind_of(fmt), matrix)
        assert reader.read_frames(fam.bgr_of(*src)).tobytes() == want.tobytes(), tag
        return fc.check_formats(fam, pc.BoundReader(reader, matrix), src, tag, rng, (fmt,), want=want)
    fc.fixture_frames(fam, env[sd], sd, count, IDENTITY_MIN_OK, check)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', fc.MATCH_KINDS)
def test_each_match_kernel(env, monkeypatch, kind, kernel):  # noqa: F811
    """Each match kernel forced (MELF_MATCH), asserted through melf_ctx_last_match after every call (frame_cases' body): the
    matrix-core kernels behind k_p32_lplane, the dot4 matcher as k_p32_match."""
    groups = [(pc.F32[k], fmts, fc.as_pitched(pc.F32[k], lambda i: dict(row_pad=4 * i, stride_pad=8)))
              for (k, fmts) in (('yuv', ('y410', 'vuya')), ('rgb', ('x2rgb10',)))]
    fc.each_match_kernel(env['sample-images1'], monkeypatch, kind, kernel, groups, 64, 5, 7, 7, 32)


@pytest.mark.gpu
@pytest.mark.parametrize('colour', ('yuv', 'rgb'))
def test_buffer_ends(env, monkeypatch, tmp_path, colour):  # noqa: F811
    """frame_cases.buffer_ends with this family: device buffers that end where their allocation ends, rows pitched and tight, no
    stride padding, at every base phase the check accepts.  A buffer of s bytes that ends on a page's end starts at -s modulo 16:
    rows padded by 0, 4 and 8 bytes make s = n ((H - 1) pitch + 4 W) take all four residues over the two frame sizes of
    buffer_ends -- (410, 300): 0, 4, 8; (412, 302): 0, 12, 8 --, so the base lies at 0, 4, 8 and 12 modulo 16 (asserted)."""
    fam = pc.F32[colour]
    args = fc.family_ends(fam, ('y410',) if colour == 'yuv' else ('x2rgb10',))
    args['layouts'] = lambda src, k, fmt, rng: [fam.pitched(*src, fmt, rng=rng, row_pad=p, stride_pad=0) for p in (0, 4, 8)]
    seen = set()
    read_dev = args['read_dev']

    def read(ctx, d, desc):
        seen.add(d % 16)
        return read_dev(ctx, d, desc)
    args['read_dev'] = read
    fc.buffer_ends(monkeypatch, tmp_path, phases_of=lambda fmt: (0,), **args)
    assert seen == {0, 4, 8, 12}, seen


@pytest.mark.gpu
def test_host_staging_three_chunks(env, tmp_path):
    """257 host frames in three staging chunks of 128 frames, the crop's x origin odd and the frame's width odd."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    r = MeterReader(fc.params_with_rect(tmp_path, 'sample-images1', (53, 160, 303, 410), 'staging'))
    try:
        rng = np.random.default_rng(257)
        bgr = np.ascontiguousarray(np.roll(fc.synth(e['frames'], 257, 4), 3, axis=2)[:, :410, :305])
        for (kind, fmt) in (('yuv', 'y410'), ('yuv', 'ayuv'), ('rgb', 'x2bgr10')):
            fam = pc.F32[kind]
            src = fam.from_bgr(bgr)
            want = pc.want_8bit(r, src, kind)
            assert (want['status'] == _hip.FRAME_OK).sum() > 128
            arr = pc.conventional32(*src, fmt, 0, rng)
            assert r.read_packed32_frames(arr, fmt, pc.matrix_of(fmt)).tobytes() == want.tobytes(), fmt
    finally:
        r.close()


@pytest.mark.gpu
def test_resident_lanes_two_streams(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1) and two caller streams on one context, the format and the colour kind changing from call to
    call, a BGRA call among them: every call's records equal a synchronous call's."""
    from meterelf_amd import MeterReader
    e = env['sample-images2']
    bgr = fc.synth(e['frames'], 64, 21)
    r = MeterReader(e['params'])
    bufs = []
    keep = []
    try:
        calls = []
        for (k, fmt) in enumerate(('y410', 'x2rgb10', 'bgra', 'vuya')):
            rng = np.random.default_rng(k)
            if fmt == 'bgra':
                (raw, args) = fc.pitched_packed(bgr, 'bgra', 8, rng)
                (call, want) = (r.ctx.process_frames_dev, r.read_frames(bgr))
            else:
                kind = pc.kind_of(fmt)
                src = pc.F32[kind].from_bgr(bgr)
                want = pc.want_8bit(r, src, kind)
                (raw, desc) = pc.pitched32(*src, fmt, row_pad=4 * k, stride_pad=12 * k, rng=rng)
                (call, args) = (r.ctx.process_packed32_dev, (desc,))
            assert (want['status'] == _hip.FRAME_OK).sum() > 32
            keep.append(raw)
            bufs.append(DevBuf(raw.ctypes.data, raw.nbytes))
            assert call(bufs[-1].d.value, *args).tobytes() == want.tobytes(), fmt
            calls.append((functools.partial(call, bufs[-1].d.value, *args), want.tobytes()))
        fc.resident_calls(r, len(bgr), calls, 2 * len(calls), lambda i: (3 * i) % len(calls))
    finally:
        r.close()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_argument_errors_launch_nothing(env):
    """One descriptor (or more) per message of the check's table, through the three entry points: MELF_ERR_INVALID, the message,
    and fc.launch_counts unchanged."""
    e = env['sample-images1']
    ctx = e['reader'].ctx
    L = _hip.lib()
    bgr = np.stack(e['frames'][2:6])
    (n, H, W) = bgr.shape[:3]
    F = _hip.MelfPacked32Frames
    for fmt in ('y410', 'x2rgb10'):
        kind = pc.kind_of(fmt)
        src = pc.F32[kind].from_bgr(bgr)
        (arr, good) = pc.pitched32(*src, fmt, row_pad=16, stride_pad=32, rng=np.random.default_rng(2))
        (colour, rp, fs, pos) = (good.colour, good.row_pitch, good.frame_stride, tuple(good.pos))
        mgood = good.matrix
        row = 4 * W
        buf = DevBuf(arr.ctypes.data, arr.nbytes)
        try:
            ctx.set_profiling(1)
            fc.launch_counts(ctx)            # (reading the counts resets them: the other format's good call is out of them now)
            before = fc.launch_counts(ctx)
            assert not any(before.values())
            out = np.zeros(n, _hip.RESULT_DTYPE)
            bgr_out = np.zeros((n, H, W, 3), np.uint8)

            def D(colour=colour, matrix=mgood, n=n, H=H, W=W, pos=pos, rp=rp, fs=fs, reserved=0, reserved2=0):
                return F(colour, matrix, n, H, W, (C.c_int32 * 3)(*pos), rp, fs, reserved, reserved2)
            bad = [
                ('unknown colour', D(colour=2)), ('unknown colour', D(colour=-1)),
                ('reserved', D(reserved=1)), ('reserved', D(reserved2=1)),
                ('outside 0 .. 24', D(pos=(25, 2, 12))), ('outside 0 .. 24', D(pos=(12, -1, 22))), ('outside 0 .. 24', D(pos=(0, 8, 32))),
                ('overlap', D(pos=(12, 12, 22))), ('overlap', D(pos=(12, 5, 22))), ('overlap', D(pos=(0, 8, 15))),
                ('batch shape', D(H=0)), ('batch shape', D(W=0)), ('batch shape', D(W=-2)), ('batch shape', D(n=-1)),
                ('smaller than a row', D(rp=row - 4)), ('smaller than a row', D(rp=0)), ('smaller than a row', D(rp=-4)),
                ('row_pitch of 32-bit packed frames too large', D(rp=2 ** 31, fs=2 ** 31 * H)),
                ('smaller than a frame', D(fs=(H - 1) * rp + row - 4)), ('smaller than a frame', D(fs=0)),
                ('aligned row_pitch', D(rp=rp + 2, fs=fs + 4 * H)), ('aligned row_pitch', D(fs=fs + 2)), ('aligned row_pitch', D(fs=fs + 1)),
            ]
            if kind == 'yuv':
                bad += [('unknown YUV matrix', D(matrix=1)), ('unknown YUV matrix', D(matrix=5)), ('unknown YUV matrix', D(matrix=-1))]
            else:
                bad += [('RGB frames is not 0', D(matrix=3)), ('RGB frames is not 0', D(matrix=-1))]
            for (word, f) in bad:
                key = (fmt, word, f.colour, f.matrix, f.n, f.H, f.W, tuple(f.pos), f.row_pitch, f.frame_stride, f.reserved, f.reserved2)
                assert L.melf_process_packed32_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(f), None, _hip._ptr(out), None) == -1, key
                assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
                assert L.melf_process_packed32(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(out)) == -1, key
                assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
                assert L.melf_packed32_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(bgr_out)) == -1, key
                assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
            assert L.melf_process_packed32_dev(ctx._h, C.c_void_p(buf.d.value), None, None, _hip._ptr(out), None) == -1
            assert L.melf_process_packed32(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(out)) == -1
            assert 'descriptor is NULL' in L.melf_last_error().decode()
            assert L.melf_packed32_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(bgr_out)) == -1
            assert L.melf_process_packed32_dev(ctx._h, None, C.byref(good), None, _hip._ptr(out), None) == -1   # NULL frames
            assert 'frames pointer of 32-bit packed frames is NULL' in L.melf_last_error().decode()
            assert L.melf_process_packed32(ctx._h, None, C.byref(good), _hip._ptr(out)) == -1
            assert 'frames pointer of 32-bit packed frames is NULL' in L.melf_last_error().decode()
            assert L.melf_packed32_to_bgr(ctx._h, None, C.byref(good), _hip._ptr(bgr_out)) == -1
            assert 'frames pointer of 32-bit packed frames is NULL' in L.melf_last_error().decode()
            for off in (1, 2):                                                                                  # a misaligned base
                assert L.melf_process_packed32_dev(ctx._h, C.c_void_p(buf.d.value + off), C.byref(good), None, _hip._ptr(out), None) == -1
                assert 'aligned base' in L.melf_last_error().decode()
                assert L.melf_process_packed32(ctx._h, C.c_void_p(arr.ctypes.data + off), C.byref(good), _hip._ptr(out)) == -1
                assert 'aligned base' in L.melf_last_error().decode()
                assert L.melf_packed32_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data + off), C.byref(good), _hip._ptr(bgr_out)) == -1
                assert 'aligned base' in L.melf_last_error().decode()
            assert L.melf_process_packed32(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(good), None) == -1      # no place for the records
            empty = D(n=0)
            assert L.melf_process_packed32_dev(ctx._h, None, C.byref(empty), None, None, None) == 0             # n == 0 passes
            assert L.melf_process_packed32(ctx._h, None, C.byref(empty), None) == 0
            assert L.melf_packed32_to_bgr(ctx._h, None, C.byref(empty), None) == 0
            assert fc.launch_counts(ctx) == before
            # the context is usable, and a good descriptor runs
            assert L.melf_process_packed32_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
            assert fc.launch_counts(ctx) != before
            assert out.tobytes() == pc.want_8bit(e['reader'], src, kind).tobytes()
        finally:
            ctx.set_profiling(0)
            buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_packed32_frames with torch tensors (int32 holding the same bits), device tensors read in place, a strided view, out= a
    device tensor and two streams, in a child process that imports torch first (tests/frame_cases.py says why)."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'p32_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch packed32 path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
