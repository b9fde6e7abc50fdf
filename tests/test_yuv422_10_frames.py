"""melf_process_yuv422_10* / melf_yuv422_10_to_bgr: packed 10-bit YUV 4:2:2 frames -- v210 (six pixels in a 16-byte group of four
32-bit words: SDI / HDMI capture cards) and Y210 / Y212 / Y216 (MSB-aligned 16-bit words Y0 U Y1 V: hardware 4:2:2 decoders) -- read
in place.

The contract (include/meterelf_hip.h): every sample is read as its top 8 bits, truncation -- v210 s8 = (field >> 2) & 255, Y21x
s8 = s >> 8 --, and the records are byte-identical to melf_process_yuv422(_dev) on the 8-bit YUYV frame of the same n, H, W and
matrix whose samples are the s8, and so to melf_process_batch on the BGR frame the header's integer conversion makes of it.
tests/p10_cases.py restates the two layouts in numpy; the GPU tests compare all records, as bytes, with read_yuv422_frames of the
unpacked YUYV frames and with read_frames of the BGR frames frame_cases.yuv_to_bgr makes (p10_cases.want_8bit asserts the two equal).

The dial kernels' instantiations: tests/test_yuv422_10_dials.py.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meterelf_amd import _hip  # noqa: E402
from tests import frame_cases as fc  # noqa: E402
from tests import p10_cases as pc  # noqa: E402
from tests.frame_cases import DevBuf, env  # noqa: E402,F401

FIELDS = ('format', 'matrix', 'n', 'H', 'W', 'reserved', 'row_pitch', 'frame_stride')
MATRICES = (0, 2, 3, 4)


def aligned_zeros(shape, dtype, lead=0):
    """A zeroed array whose first byte lies `lead` bytes behind a multiple of 64."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(nbytes + 128, np.uint8)
    at = -raw.ctypes.data % 64 + lead
    return raw[at:at + nbytes].view(dtype).reshape(shape)


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_struct_and_constants(tmp_path):
    src = tmp_path / 'p10.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(melf_yuv422_10_frames));\n'
                   + ''.join('printf(" %%zu", offsetof(melf_yuv422_10_frames, %s));\n' % f for f in FIELDS)
                   + 'printf(" %d %d %d %d %d %d\\n", MELF_ABI_VERSION, MELF_DIALS_FAMILIES, MELF_DIALS10_V210, MELF_DIALS10_Y210,'
                     ' MELF_YUV422_10_V210, MELF_YUV422_10_Y210);return 0;}\n')
    exe = tmp_path / 'p10'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfYuv422_10Frames
    assert tuple(f[0] for f in F._fields_) == FIELDS
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in FIELDS] + [3, 12, 14, 15, 0, 1]
    assert _hip.ABI_VERSION == 3
    for name in ('melf_process_yuv422_10', 'melf_process_yuv422_10_dev', 'melf_yuv422_10_to_bgr'):
        assert name in _hip.EXPORTS
    assert _hip.DIALS10_FAMILIES == ('v210', 'y210') and len(_hip.DIALS_FAMILIES) == 12 and len(_hip.DIALS16_FAMILIES) == 2
    assert _hip.YUV422_10_FORMATS == {'v210': 0, 'y210': 1, 'y212': 1, 'y216': 1}


def test_reader_method_has_no_default_matrix():
    import inspect
    from meterelf_amd import MeterReader
    sig = inspect.signature(MeterReader.read_yuv422_10_frames)
    assert sig.parameters['matrix'].default is inspect.Parameter.empty
    assert sig.parameters['pixel_format'].default is inspect.Parameter.empty
    assert sig.parameters['width'].default is None and sig.parameters['out'].default is None
    assert inspect.signature(_hip.yuv422_10_frames_view).parameters['matrix'].default is inspect.Parameter.empty


def test_v210_table_is_the_header_table():
    """The (word, bit offset) table, literally, and what it amounts to: the twelve fields of a group in order are U Y V Y ..."""
    assert pc.V210_TABLE == {
        0: {'y0': (0, 10), 'y1': (1, 0), 'u': (0, 0), 'v': (0, 20)},
        1: {'y0': (1, 20), 'y1': (2, 10), 'u': (1, 10), 'v': (2, 0)},
        2: {'y0': (3, 0), 'y1': (3, 20), 'u': (2, 20), 'v': (3, 10)},
    }
    order = {}
    for (q, t) in pc.V210_TABLE.items():
        for (key, (w, bit)) in t.items():
            order[3 * w + bit // 10] = (key, q)
    assert [order[i] for i in range(12)] == [('u', 0), ('y0', 0), ('v', 0), ('y1', 0), ('u', 1), ('y0', 1), ('v', 1), ('y1', 1), ('u', 2), ('y0', 2),
                                             ('v', 2), ('y1', 2)]
    with open(os.path.join(ROOT, 'include', 'meterelf_hip.h')) as fp:
        text = fp.read()
    for row in ('0      w0, 10    w1, 0      w0, 0    w0, 20', '1      w1, 20    w2, 10     w1, 10   w2, 0', '2      w3, 0     w3, 20     w2, 20   w3, 10'):
        assert row in text, row


def test_every_field_position_at_every_value():
    """Each of the 12 field positions of a group, at every 10-bit value, all other bits of the group random (bits 30-31 too):
    unpack_v210 gives v >> 2 at the pixel and plane the order U Y V Y .. says, by a shift and a mask written out here."""
    rng = np.random.default_rng(12)
    values = np.arange(1024, dtype=np.uint32)
    where = [('u', 0), ('y', 0), ('v', 0), ('y', 1), ('u', 1), ('y', 2), ('v', 1), ('y', 3), ('u', 2), ('y', 4), ('v', 2), ('y', 5)]
    for (pos, (plane, index)) in enumerate(where):
        g = rng.integers(0, 2 ** 32, size=(1, 1024, 4), dtype=np.uint32)
        (w, bit) = (pos // 3, 10 * (pos % 3))
        g[0, :, w] = (g[0, :, w] & ~np.uint32(1023 << bit)) | (values << bit)
        (Y, U, V) = pc.unpack_v210(g, 6)
        got = dict(y=Y, u=U, v=V)[plane][0, :, index]
        assert np.array_equal(got, (values >> 2).astype(np.uint8)), pos
        # the other samples are those of the random bits, whatever the field under test holds
        for (p2, (plane2, index2)) in enumerate(where):
            if p2 != pos:
                want = ((g[0, :, p2 // 3] >> (10 * (p2 % 3) + 2)) & 255).astype(np.uint8)
                assert np.array_equal(dict(y=Y, u=U, v=V)[plane2][0, :, index2], want), (pos, p2)


@pytest.mark.parametrize('W', [2, 4, 6, 8, 10, 12, 14, 50])
def test_packers_round_trip(W):
    rng = np.random.default_rng(W)
    (n, H) = (2, 3)
    src = (rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H, W // 2), dtype=np.uint8),
           rng.integers(0, 256, (n, H, W // 2), dtype=np.uint8))
    for garbage in (False, True):
        words = pc.pack_v210(*src, rng, garbage)
        assert words.shape == (n, H, 4 * ((W + 5) // 6)) and words.dtype == np.uint32 and words.shape[2] * 4 == pc.v210_row_bytes(W)
        for (a, b) in zip(pc.unpack_v210(words, W), src):
            assert np.array_equal(a, b), (W, garbage)
        if garbage:
            assert W < 50 or ((words >> 30) != 0).any()
        else:
            assert ((words >> 30) == 0).all()
            if W % 6:   # the fields behind W are zero without garbage
                (Yt, _u, _v) = pc.unpack_v210(words, 6 * ((W + 5) // 6))
                assert (Yt[:, :, W:] == 0).all()
    # low bits: the packers fill them with random bits, and they do not come back
    big = pc.pack_v210(*(np.full((1, 8, 48 // k), 200, np.uint8) for k in (1, 2, 2)), rng)
    assert len(np.unique(big & 3)) == 4
    y = pc.pack_y210(*src, rng)
    assert y.shape == (n, H, W, 2) and y.dtype == np.uint16
    for (a, b) in zip(pc.unpack_y210(y), src):
        assert np.array_equal(a, b)
    assert np.array_equal(y[0, 0, 0::2, 1] >> 8, src[1][0, 0]) and np.array_equal(y[0, 0, 1::2, 1] >> 8, src[2][0, 0])   # Y0 U Y1 V
    assert pc.v210_pitch(1920) == 5120 and pc.v210_pitch(1280) == 3456 and pc.v210_row_bytes(1280) == 3424


def _makers32():
    yield lambda a: a
    try:
        import torch
    except ImportError:
        return
    yield lambda a: torch.from_numpy(a.view(np.int32))   # the same bits


def _makers16():
    yield lambda a: a
    try:
        import torch
    except ImportError:
        return
    if hasattr(torch, 'uint16'):
        yield torch.from_numpy
    yield lambda a: torch.from_numpy(a.view(np.int16))


def test_view_layouts_v210():
    (n, H, W) = (3, 4, 50)
    (row, pitch) = (144, 256)   # 9 groups; the conventional pitch of 50 pixels
    assert (pc.v210_row_bytes(W), pc.v210_pitch(W)) == (row, pitch)
    view = _hip.yuv422_10_frames_view
    for make in _makers32():
        base = aligned_zeros((n, H, pitch // 4), np.uint32)
        v = view(make(base), 'v210', 'bt709', width=W)
        assert not v.copied and v.ptr == base.ctypes.data and not v.on_device and v.matrix == 3 and v.format == 0
        assert (v.n, v.H, v.W, v.row_pitch, v.frame_stride) == (n, H, W, pitch, H * pitch)
        assert v.extent == (n - 1) * H * pitch + (H - 1) * pitch + row == pc.extent10(v.descriptor())
        d = v.descriptor()
        assert (d.format, d.matrix, d.n, d.H, d.W, d.reserved, d.row_pitch, d.frame_stride) == (0, 3, n, H, W, 0, pitch, H * pitch)
        # every other frame, and a slice of frames: in place
        v2 = view(make(base)[::2], 'v210', 4, W)
        assert not v2.copied and v2.n == 2 and v2.frame_stride == 2 * H * pitch and v2.extent == 2 * H * pitch + (H - 1) * pitch + row and v2.matrix == 4
        v3 = view(make(base)[1:], 'v210', 0, W)
        assert not v3.copied and v3.ptr == base.ctypes.data + H * pitch and v3.n == 2
        # the groups alone of padded rows, and tight rows: in place
        vw = view(make(base)[:, :, :row // 4], 'v210', 'bt709', W)
        assert not vw.copied and vw.ptr == base.ctypes.data and (vw.row_pitch, vw.frame_stride) == (pitch, H * pitch) and vw.extent == v.extent
        tight = aligned_zeros((n, H, row // 4), np.uint32)
        vt = view(make(tight), 'v210', 'bt709', W)
        assert not vt.copied and (vt.row_pitch, vt.frame_stride, vt.extent) == (row, H * row, n * H * row)
        # a narrower width of the same rows
        assert view(make(base), 'v210', 'bt709', 12).extent == (n - 1) * H * pitch + (H - 1) * pitch + 32
        # a row stride that is no multiple of 16 bytes, an element stride of two words: copied, the groups alone
        odd = aligned_zeros((n, H, row // 4 + 2), np.uint32)
        vo = view(make(odd), 'v210', 'bt709', W)
        assert vo.copied and vo.ptr != odd.ctypes.data and (vo.row_pitch, vo.frame_stride) == (row, H * row) and vo.ptr % 16 == 0
        ve = view(make(aligned_zeros((n, H, 2 * (row // 4)), np.uint32))[:, :, ::2], 'v210', 'bt709', W)
        assert ve.copied and ve.row_pitch == row
        # n == 0
        assert view(make(base)[:0], 'v210', 'bt709', W).extent == 0


@pytest.mark.parametrize('fmt', ['y210', 'y212', 'y216'])
def test_view_layouts_y21x(fmt):
    (n, H, W) = (3, 4, 10)
    view = _hip.yuv422_10_frames_view
    for make in _makers16():
        base = aligned_zeros((n, H, W, 2), np.uint16)
        v = view(make(base), fmt, 'bt709')
        assert not v.copied and v.ptr == base.ctypes.data and v.format == 1 and v.matrix == 3
        assert (v.n, v.H, v.W, v.row_pitch, v.frame_stride, v.extent) == (n, H, W, 4 * W, 4 * W * H, n * H * 4 * W)
        assert v.extent == pc.extent10(v.descriptor())
        assert view(make(base), fmt.upper(), 'bt709', width=W).extent == v.extent
        v2 = view(make(base)[::2], fmt, 2)
        assert not v2.copied and v2.n == 2 and v2.frame_stride == 8 * W * H and v2.extent == 3 * H * 4 * W
        v3 = view(make(base)[1:], fmt, 0)
        assert not v3.copied and v3.ptr == base.ctypes.data + 4 * W * H
        # rows padded by four pixels: in place (the pitch stays a multiple of 8); by three: copied
        wide = aligned_zeros((n, H, W + 4, 2), np.uint16)
        vw = view(make(wide)[:, :, :W], fmt, 'bt709')
        assert not vw.copied and vw.ptr == wide.ctypes.data and vw.row_pitch == 4 * (W + 4) and vw.frame_stride == 4 * (W + 4) * H
        assert vw.extent == (n - 1) * vw.frame_stride + (H - 1) * vw.row_pitch + 4 * W
        assert view(make(aligned_zeros((n, H, W + 3, 2), np.uint16))[:, :, :W], fmt, 'bt709').copied
        # an element stride: copied
        ve = view(make(aligned_zeros((n, H, 2 * W, 2), np.uint16))[:, :, ::2], fmt, 'bt709')
        assert ve.copied and (ve.row_pitch, ve.frame_stride) == (4 * W, 4 * W * H)
        assert view(make(base)[:0], fmt, 'bt709').extent == 0


def test_view_errors():
    view = _hip.yuv422_10_frames_view
    z = aligned_zeros
    with pytest.raises(TypeError):
        view(z((1, 4, 16), np.uint32), 'v210')                                   # matrix has no default
    with pytest.raises(ValueError):
        view(z((1, 4, 16), np.uint32), 'v210', 'bt709')                          # v210 needs width=
    for name in ('yuyv', 'uyvy', 'p010', 'p210', 'nv12', 'i422', 'rgb', 'y410', 'v216'):
        with pytest.raises(ValueError):
            view(z((1, 4, 16), np.uint32), name, 'bt709', 12)                    # names of the other families, unknown names
    for m in ('bt2020', 1, 5, None):
        with pytest.raises(ValueError):
            view(z((1, 4, 16), np.uint32), 'v210', m, 12)                        # unknown matrix (code 1 is never assigned)
    for dt in (np.uint8, np.uint16, np.int32, np.float32):
        with pytest.raises(ValueError):
            view(z((1, 4, 16), dt), 'v210', 'bt709', 12)                         # not 32-bit words (numpy int32: view it as uint32)
    for dt in (np.uint8, np.uint32, np.int16):
        with pytest.raises(ValueError):
            view(z((1, 4, 8, 2), dt), 'y210', 'bt709')
    with pytest.raises(ValueError):
        view(z((4, 16), np.uint32), 'v210', 'bt709', 12)                         # rank
    with pytest.raises(ValueError):
        view(z((1, 4, 16, 1), np.uint32), 'v210', 'bt709', 12)
    with pytest.raises(ValueError):
        view(z((1, 4, 8), np.uint16), 'y210', 'bt709')
    with pytest.raises(ValueError):
        view(z((1, 4, 8, 3), np.uint16), 'y210', 'bt709')
    for w in (11, 0, -2):
        with pytest.raises(ValueError):
            view(z((1, 4, 16), np.uint32), 'v210', 'bt709', w)                   # an odd width, no width
    with pytest.raises(ValueError):
        view(z((1, 4, 7, 2), np.uint16), 'y210', 'bt709')                        # odd W
    with pytest.raises(ValueError):
        view(z((1, 4, 8, 2), np.uint16), 'y210', 'bt709', width=6)               # a width that is not the array's
    with pytest.raises(ValueError):
        view(z((1, 4, 7), np.uint32), 'v210', 'bt709', 12)                       # rows of 28 bytes, two groups are 32
    with pytest.raises(ValueError):
        view(z((1, 4, 8), np.uint32), 'v210', 'bt709', 14)                       # 14 pixels are three groups
    assert view(z((1, 4, 8), np.uint32), 'v210', 'bt709', 12).row_pitch == 32
    for lead in (4, 8):
        with pytest.raises(ValueError):
            view(z((1, 4, 16), np.uint32, lead), 'v210', 'bt709', 12)            # a base that is not 16-byte aligned
    for lead in (2, 4):
        with pytest.raises(ValueError):
            view(z((1, 4, 8, 2), np.uint16, lead), 'y210', 'bt709')              # ... not 8-byte aligned
    assert not view(z((1, 4, 8, 2), np.uint16, 8), 'y210', 'bt709').copied       # 8 within 16 is fine for Y210


def test_checks_and_load_bounds(tmp_path):
    """tests/p10_bounds_main.cpp, plain and under the host sanitizers: check_yuv422_10 over accepted and rejected descriptors,
    DialV210 / DialY210 of melf_frame_src.h on exact-extent heap buffers against plain indexing, and the prep functions of
    melf_p10_addr.h.  Built with the ROCm tree's clang++ as a plain C++ compiler, as tests/frame_src_bounds_main.cpp is: the
    sources' header needs ext_vector_type, which g++ does not have."""
    from tests import test_dials_instantiations as di
    (cxx, inc) = di.rocm_clangxx()
    out = fc.build_and_run(tmp_path, cxx, os.path.join(ROOT, 'tests', 'p10_bounds_main.cpp'), 'p10_bounds', ['-D__HIP_PLATFORM_AMD__', '-I' + inc],
                           ['-fsanitize=address,undefined'])
    assert 'v210 quads at fx0 % 6 = 0, 2, 4' in out and 'with a seventh group' in out, out


def test_kernels_metadata():
    """The kernels that read these frames are in the library: 12 needle, 2 lplane, 2 match and 2 to_bgr kernels, wave size 64, no
    private segment, no spilled vector registers; the dial readers within the dial kernels' register budget (128)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    new = {k: d for (k, d) in meta.items() if 'k_v210_' in k or 'k_y210_' in k}
    for fam in ('v210', 'y210'):
        counts = [sum(('k_%s_%s' % (fam, s)) in k for k in new) for s in ('needle', 'lplane', 'match', 'to_bgr')]
        assert counts == [6, 1, 1, 1], (fam, counts)
    assert len(new) == 18
    for (k, d) in new.items():
        assert d.get('private_segment_fixed_size', 0) == 0 and d.get('vgpr_spill_count', 0) == 0 and d['wavefront_size'] == 64, (k, d)
        if 'needle' in k:
            assert d['vgpr_count'] <= 128, (k, d)
        for other in ('k_dials', 'k_needles', 'k_prep_lplane', 'k_match_mfma', 'k_match_gen'):   # what existing tests count kernels by
            assert other not in k


# ------------------------------------------------------------------------------------------------------------- GPU ---------
def _on_device(ctx, ptr, desc, extent):
    buf = DevBuf(ptr, extent)
    try:
        return ctx.process_yuv422_10_dev(buf.d.value, desc)
    finally:
        buf.free()


@pytest.mark.gpu
@pytest.mark.parametrize('matrix', MATRICES)
@pytest.mark.parametrize('fmt', pc.FORMATS)
def test_to_bgr(env, fmt, matrix):
    """The stage kernel == the layout restated + the conversion restated, byte for byte: a 256 x 256 frame whose Y takes all 256
    values against 65 536 random (U, V) and low bits, and for v210 a frame in which each of the 12 field positions of a group
    takes every 10-bit value, every other bit random (bits 30-31 included)."""
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(100 + matrix)
    Y = (np.arange(65536, dtype=np.uint32) & 255).astype(np.uint8).reshape(1, 256, 256)
    (U, V) = (rng.integers(0, 256, (1, 256, 128), dtype=np.uint8), rng.integers(0, 256, (1, 256, 128), dtype=np.uint8))
    (buf, desc) = pc.pitched10(Y, U, V, fmt, row_pad=16, rng=rng, matrix=matrix)
    got = ctx.yuv422_10_to_bgr(buf.ctypes.data, desc)
    want = fc.yuv_to_bgr(Y, U, V, 1, 0, matrix)
    bad = np.flatnonzero((got != want).any(axis=-1).ravel())
    assert bad.size == 0, (fmt, matrix, bad.size, bad[:8])
    if fmt == 'v210':
        words = rng.integers(0, 2 ** 32, size=(1, 12, 1024, 4), dtype=np.uint32)
        values = np.arange(1024, dtype=np.uint32)
        for pos in range(12):
            (w, bit) = (pos // 3, 10 * (pos % 3))
            words[0, pos, :, w] = (words[0, pos, :, w] & ~np.uint32(1023 << bit)) | (values << bit)
        words = np.ascontiguousarray(words.reshape(1, 12, 4096))
        v = _hip.yuv422_10_frames_view(words, 'v210', matrix, width=6144)
        assert not v.copied
        got = ctx.yuv422_10_to_bgr(v.ptr, v.descriptor())
        want = fc.yuv_to_bgr(*pc.unpack_v210(words, 6144), 1, 0, matrix)
        assert np.array_equal(got, want)


IDENTITY_MIN_OK = 24   # of 33: four of synth's frames are constant (Dials not found)


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', pc.FORMATS)
def test_identity_on_fixture_pictures(env, fmt):
    """sample-images1's pictures (frame_cases.synth of the fixture frames, as the 8-bit 4:2:2 file uses them: shifted, noisy, every
    9th a constant frame, so readable and unreadable frames both occur) encoded to 4:2:2 under each of the four matrices and packed
    with random low bits, garbage in bits 30-31 and behind W: 12 frames and 33 (the prep kernel's two frame groups), through the
    reader, the host and the device entry point, as the caller's array and as a pitched buffer of exact extent."""
    e = env['sample-images1']
    reader = e['reader']
    bgr = fc.synth(e['frames'], 33, 16)
    rng = np.random.default_rng(33)
    for matrix in MATRICES:
        src8 = fc.bgr_to_yuv(bgr, 1, 0, matrix)
        want = pc.want_8bit(reader, src8, matrix)
        assert (want['status'] == _hip.FRAME_OK).sum() >= IDENTITY_MIN_OK and (want['status'][:12] == _hip.FRAME_OK).sum() >= 8
        assert (want['status'][:12] == _hip.FRAME_DIALS_NOT_FOUND).any()
        for n in (12, 33):
            src = tuple(p[:n] for p in src8)
            arr = pc.conventional10(*src, fmt, 1, rng, garbage=True)
            width = getattr(arr, 'width', None)
            assert reader.read_yuv422_10_frames(arr, fmt, matrix, width=width).tobytes() == want[:n].tobytes(), (fmt, matrix, n, 'reader')
            v = pc.view10(arr, fmt, matrix)
            assert not v.copied
            pc.check_identity(reader.ctx, v.ptr, v.descriptor(), v.extent, want[:n], (fmt, matrix, n, 'array'))
            (buf, desc) = pc.pitched10(*src, fmt, row_pad=16 * (n % 2), stride_pad=48, rng=rng, matrix=matrix)
            pc.check_identity(reader.ctx, buf.ctypes.data, desc, buf.nbytes, want[:n], (fmt, matrix, n, 'pitched'))


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', fc.MATCH_KINDS)
def test_each_match_kernel(env, monkeypatch, kind, kernel):  # noqa: F811
    """Each match kernel forced (MELF_MATCH), asserted through melf_ctx_last_match after every call (frame_cases' body)."""
    fam = pc.F10
    fc.each_match_kernel(env['sample-images1'], monkeypatch, kind, kernel,
                         [(fam, fam.formats, fc.as_pitched(fam, lambda k: dict(row_pad=16 * k, stride_pad=16)))], 64, 5, 7, 7, 32)


@pytest.mark.gpu
def test_buffer_ends(env, monkeypatch, tmp_path):  # noqa: F811
    """frame_cases.buffer_ends with this family: device buffers that end where their allocation ends, rows pitched and tight, no
    stride padding, at every base phase the check accepts -- v210 buffers are whole groups, so their base is 0 within 16; Y210
    buffers of 8 bytes modulo 16 put the base at 8 within 16, and both occur (asserted)."""
    args = fc.family_ends(pc.F10)
    seen = {0: set(), 1: set()}
    read_dev = args['read_dev']

    def read(ctx, d, desc):
        seen[desc.format].add(d % 16)
        return read_dev(ctx, d, desc)
    args['read_dev'] = read
    fc.buffer_ends(monkeypatch, tmp_path, phases_of=lambda fmt: (0,), **args)
    assert seen == {0: {0}, 1: {0, 8}}, seen


@pytest.mark.gpu
def test_host_staging_three_chunks(env, tmp_path):
    """257 host frames in three staging chunks of 128 frames, the crop's x origin at residue 5 modulo 6 (and odd): the staged frame
    starts five pixels left of the crop (v210), one pixel (Y210)."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    assert 53 % 6 == 5
    r = MeterReader(fc.params_with_rect(tmp_path, 'sample-images1', (53, 160, 303, 410), 'staging'))
    try:
        rng = np.random.default_rng(257)
        bgr = np.ascontiguousarray(np.roll(fc.synth(e['frames'], 257, 4), 3, axis=2)[:, :410, :304])
        src8 = fc.bgr_to_yuv(bgr, 1, 0, pc.MATRIX)
        want = pc.want_8bit(r, src8)
        assert (want['status'] == _hip.FRAME_OK).sum() > 128
        for fmt in pc.FORMATS:
            arr = pc.conventional10(*src8, fmt, 0, rng)
            assert r.read_yuv422_10_frames(arr, fmt, 'bt709', width=304).tobytes() == want.tobytes(), fmt
    finally:
        r.close()


@pytest.mark.gpu
def test_resident_lanes_two_streams(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1) and two caller streams on one context, the format changing from call to call, an 8-bit
    UYVY call among them: every call's records equal a synchronous call's."""
    from meterelf_amd import MeterReader
    e = env['sample-images2']
    bgr = fc.synth(e['frames'], 64, 21)
    r = MeterReader(e['params'])
    bufs = []
    keep = []
    try:
        src8 = fc.bgr_to_yuv(bgr, 1, 0, pc.MATRIX)
        want = pc.want_8bit(r, src8)
        assert (want['status'] == _hip.FRAME_OK).sum() > 32
        calls = []
        for (k, fmt) in enumerate(('v210', 'y210', 'uyvy', 'v210')):
            rng = np.random.default_rng(k)
            if fmt == 'uyvy':
                (raw, desc) = fc.pitched422(*src8, 'uyvy', row_pad=4, stride_pad=8, rng=rng, matrix=pc.MATRIX)
                call = r.ctx.process_yuv422_dev
            else:
                (raw, desc) = pc.pitched10(*src8, fmt, row_pad=16 * k, stride_pad=16 * k, rng=rng)
                call = r.ctx.process_yuv422_10_dev
            keep.append(raw)
            bufs.append(DevBuf(raw.ctypes.data, raw.nbytes))
            assert call(bufs[-1].d.value, desc).tobytes() == want.tobytes(), fmt
            calls.append((functools.partial(call, bufs[-1].d.value, desc), want.tobytes()))
        fc.resident_calls(r, len(bgr), calls, 2 * len(calls), lambda i: (3 * i) % len(calls))
    finally:
        r.close()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_argument_errors_launch_nothing(env):
    e = env['sample-images1']
    ctx = e['reader'].ctx
    L = _hip.lib()
    src8 = fc.bgr_to_yuv(np.stack(e['frames'][2:6]), 1, 0, pc.MATRIX)
    (n, H, W) = src8[0].shape
    F = _hip.MelfYuv422_10Frames
    fields = [f[0] for f in F._fields_]
    for fmt in pc.FORMATS:
        (arr, good) = pc.pitched10(*src8, fmt, row_pad=16, stride_pad=32, rng=np.random.default_rng(2))
        (code, rp, fs, a) = (good.format, good.row_pitch, good.frame_stride, 16 if fmt == 'v210' else 8)
        row = pc.v210_row_bytes(W) if fmt == 'v210' else 4 * W
        buf = DevBuf(arr.ctypes.data, arr.nbytes)
        try:
            ctx.set_profiling(1)
            fc.launch_counts(ctx)            # (reading the counts resets them: the other format's good call is out of them now)
            before = fc.launch_counts(ctx)
            assert not any(before.values())
            out = np.zeros(n, _hip.RESULT_DTYPE)
            bgr_out = np.zeros((n, H, W, 3), np.uint8)

            def D(format=code, matrix=3, n=n, H=H, W=W, reserved=0, rp=rp, fs=fs):
                return F(format, matrix, n, H, W, reserved, rp, fs)
            bad = [
                ('unknown packed 10-bit', D(format=2)), ('unknown packed 10-bit', D(format=-1)),
                ('matrix', D(matrix=1)), ('matrix', D(matrix=5)), ('matrix', D(matrix=-1)),
                ('reserved', D(reserved=1)),
                ('batch shape', D(H=0)), ('batch shape', D(W=0)), ('batch shape', D(W=-2)), ('batch shape', D(n=-1)),
                ('even width', D(W=W - 1)),
                ('row_pitch smaller', D(rp=row - a)), ('row_pitch smaller', D(rp=0)), ('row_pitch smaller', D(rp=-a)),
                ('row_pitch too large', D(rp=2 ** 31, fs=2 ** 31 * H)),
                ('frame_stride smaller', D(fs=(H - 1) * rp + row - a)), ('frame_stride smaller', D(fs=0)),
                ('aligned row_pitch', D(rp=rp + a // 2, fs=fs + a * H)), ('aligned row_pitch', D(fs=fs + a // 2)), ('aligned row_pitch', D(fs=fs + 4)),
            ]
            for (word, f) in bad:
                key = (fmt, word) + tuple(getattr(f, k) for k in fields)
                assert L.melf_process_yuv422_10_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(f), None, _hip._ptr(out), None) == -1, key
                assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
                assert L.melf_process_yuv422_10(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(out)) == -1, key
                assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
                assert L.melf_yuv422_10_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(bgr_out)) == -1, key
                assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
            assert L.melf_process_yuv422_10_dev(ctx._h, C.c_void_p(buf.d.value), None, None, _hip._ptr(out), None) == -1
            assert L.melf_process_yuv422_10(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(out)) == -1
            assert 'descriptor is NULL' in L.melf_last_error().decode()
            assert L.melf_yuv422_10_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(bgr_out)) == -1
            assert L.melf_process_yuv422_10_dev(ctx._h, None, C.byref(good), None, _hip._ptr(out), None) == -1   # NULL frames
            assert 'frames pointer is NULL' in L.melf_last_error().decode()
            assert L.melf_process_yuv422_10(ctx._h, None, C.byref(good), _hip._ptr(out)) == -1
            assert 'frames pointer is NULL' in L.melf_last_error().decode()
            assert L.melf_yuv422_10_to_bgr(ctx._h, None, C.byref(good), _hip._ptr(bgr_out)) == -1
            assert 'frames pointer is NULL' in L.melf_last_error().decode()
            for off in (a // 2, 4):                                                                              # a misaligned base
                assert L.melf_process_yuv422_10_dev(ctx._h, C.c_void_p(buf.d.value + off), C.byref(good), None, _hip._ptr(out), None) == -1
                assert 'aligned base' in L.melf_last_error().decode()
                assert L.melf_process_yuv422_10(ctx._h, C.c_void_p(arr.ctypes.data + off), C.byref(good), _hip._ptr(out)) == -1
                assert 'aligned base' in L.melf_last_error().decode()
                assert L.melf_yuv422_10_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data + off), C.byref(good), _hip._ptr(bgr_out)) == -1
                assert 'aligned base' in L.melf_last_error().decode()
            assert L.melf_process_yuv422_10(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(good), None) == -1      # no place for the records
            empty = D(n=0)
            assert L.melf_process_yuv422_10_dev(ctx._h, None, C.byref(empty), None, None, None) == 0             # n == 0 passes
            assert L.melf_process_yuv422_10(ctx._h, None, C.byref(empty), None) == 0
            assert L.melf_yuv422_10_to_bgr(ctx._h, None, C.byref(empty), None) == 0
            assert fc.launch_counts(ctx) == before
            # the context is usable, and a good descriptor runs
            assert L.melf_process_yuv422_10_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
            assert fc.launch_counts(ctx) != before
            assert out.tobytes() == pc.want_8bit(e['reader'], src8).tobytes()
        finally:
            ctx.set_profiling(0)
            buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_yuv422_10_frames with torch tensors (int32 / int16 holding the same bits), device tensors read in place, out= a device
    tensor and a non-default current stream, in a child process that imports torch first (tests/frame_cases.py says why)."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'p10_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch yuv422_10 path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
