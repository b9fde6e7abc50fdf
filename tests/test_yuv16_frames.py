"""melf_process_yuv16* / melf_yuv16_to_bgr: planar and semi-planar YUV frames of 16-bit little-endian samples -- P010 / P012 / P016,
P210 / P216 (the value in the high bits), I010 / yuv420p10le, I210, the 12-bit and the 16-bit planar formats (the value in the low
bits) -- read in place.

The contract (include/meterelf_hip.h): a sample s is read as s8 = min(s >> shift, 255), truncation; the records are byte-identical
to melf_process_yuv_planar(_dev) on the 8-bit frame of the same geometry whose samples are s8, and so to melf_process_batch on the
BGR frame the header's integer conversion makes of that frame.  reduce16 of tests/yuv16_cases.py restates the reduction in numpy,
yuv_to_bgr of tests/frame_cases.py the conversion; the GPU tests compare against the 8-bit entry point on the reduced buffer
(yuv16_cases.want_8bit) and, where a BGR frame is at hand, against read_frames of it.
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
from tests import yuv16_cases as yc  # noqa: E402
from tests.frame_cases import DevBuf, env  # noqa: E402,F401

FORMATS = yc.FORMATS
NAMES = ('p010', 'p012', 'p016', 'p210', 'p216', 'i010', 'yuv420p10le', 'i210', 'yuv422p10le', 'i012', 'yuv420p12le', 'i212',
         'yuv422p12le', 'yuv420p16le', 'yuv422p16le')
FIELDS = ('matrix', 'n', 'H', 'W', 'sub_y', 'c_step', 'shift', 'reserved', 'y_pitch', 'c_pitch', 'u_offset', 'v_offset', 'frame_stride')


# ------------------------------------------------------------------------------------------------------------- CPU ---------
def test_struct_matches_header(tmp_path):
    src = tmp_path / 'yuv16.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "meterelf_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(melf_yuv16_frames));\n'
                   + ''.join('printf(" %%zu", offsetof(melf_yuv16_frames, %s));\n' % f for f in FIELDS)
                   + 'printf(" %d %d %d %d\\n", MELF_ABI_VERSION, MELF_DIALS_FAMILIES, MELF_DIALS16_STEP1, MELF_DIALS16_STEP2);return 0;}\n')
    exe = tmp_path / 'yuv16'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _hip.MelfYuv16Frames
    assert tuple(f[0] for f in F._fields_) == FIELDS
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in FIELDS] + [3, 12, 12, 13]
    for name in ('melf_process_yuv16', 'melf_process_yuv16_dev', 'melf_yuv16_to_bgr'):
        assert name in _hip.EXPORTS
    assert _hip.DIALS16_FAMILIES == ('yuv16_step1', 'yuv16_step2') and len(_hip.DIALS_FAMILIES) == 12


def test_format_table():
    """name: (sub_y, c_step, V first, shift), pinned."""
    assert tuple(FORMATS) == NAMES
    assert FORMATS == {
        'p010': (1, 2, False, 8), 'p012': (1, 2, False, 8), 'p016': (1, 2, False, 8), 'p210': (0, 2, False, 8), 'p216': (0, 2, False, 8),
        'i010': (1, 1, False, 2), 'yuv420p10le': (1, 1, False, 2), 'i210': (0, 1, False, 2), 'yuv422p10le': (0, 1, False, 2),
        'i012': (1, 1, False, 4), 'yuv420p12le': (1, 1, False, 4), 'i212': (0, 1, False, 4), 'yuv422p12le': (0, 1, False, 4),
        'yuv420p16le': (1, 1, False, 8), 'yuv422p16le': (0, 1, False, 8)}
    assert set(yc.DISTINCT) <= set(NAMES) and len({FORMATS[f] for f in yc.DISTINCT}) == len({v for v in FORMATS.values()}) == 8


def _makers():
    yield lambda a: a
    try:
        import torch
    except ImportError:
        return
    if hasattr(torch, 'uint16'):
        yield torch.from_numpy
    yield lambda a: torch.from_numpy(a.view(np.int16))   # the same bits


@pytest.mark.parametrize('fmt', NAMES)
def test_view_layouts(fmt):
    """The descriptor and the extent of the raw-video array, for numpy arrays and torch CPU tensors: exact values, in place."""
    (sy, step, vfirst, shift) = FORMATS[fmt]
    (n, H, W) = (3, 8, 12)
    (ch, cw) = (H >> sy, (W // 2) * step * 2)   # chroma rows, bytes of one
    rows = yc.rows_of(fmt, H)
    assert rows == (3 * H // 2 if sy else 2 * H)
    fb = rows * W * 2
    for make in _makers():
        base = np.zeros((n, rows, W), np.uint16)
        v = _hip.yuv16_frames_view(make(base), fmt, 'bt709')
        assert not v.copied and v.ptr == base.ctypes.data and not v.on_device and v.matrix == 3
        assert (v.n, v.H, v.W, v.sub_y, v.c_step, v.shift, v.y_pitch, v.frame_stride) == (n, H, W, sy, step, shift, 2 * W, fb)
        assert v.c_pitch == cw
        if step == 2:
            assert (v.u_offset, v.v_offset) == ((2 * H * W + 2, 2 * H * W) if vfirst else (2 * H * W, 2 * H * W + 2))
        else:
            (a, b) = (2 * H * W, 2 * H * W + ch * cw)
            assert (v.u_offset, v.v_offset) == ((b, a) if vfirst else (a, b))
        assert v.extent == n * fb == yc.extent16(v.descriptor())
        d = v.descriptor()
        assert (d.matrix, d.n, d.H, d.W, d.sub_y, d.c_step, d.shift, d.reserved) == (3, n, H, W, sy, step, shift, 0)
        # every other frame, and a slice of frames: in place
        v2 = _hip.yuv16_frames_view(make(base)[::2], fmt, 4)
        assert not v2.copied and v2.n == 2 and v2.frame_stride == 2 * fb and v2.extent == 3 * fb and v2.matrix == 4
        v3 = _hip.yuv16_frames_view(make(base)[1:], fmt, 0)
        assert not v3.copied and v3.ptr == base.ctypes.data + fb and v3.extent == 2 * fb
        # padded rows (an odd number of samples: the byte strides stay even): in place where a chroma row is one row of the array
        wide = np.zeros((n, rows, W + 5), np.uint16)
        vw = _hip.yuv16_frames_view(make(wide)[:, :, :W], fmt, 'bt709')
        if step == 2:
            rp = 2 * (W + 5)
            assert not vw.copied and vw.ptr == wide.ctypes.data and (vw.y_pitch, vw.c_pitch) == (rp, rp)
            assert min(vw.u_offset, vw.v_offset) == H * rp and vw.frame_stride == rows * rp
            assert vw.extent == (n - 1) * rows * rp + (rows - 1) * rp + 2 * W == yc.extent16(vw.descriptor())
        else:
            assert vw.copied and vw.ptr != wide.ctypes.data and (vw.y_pitch, vw.c_pitch, vw.frame_stride) == (2 * W, cw, fb)
        # an element stride of 2 samples: copied
        assert _hip.yuv16_frames_view(make(np.zeros((n, rows, 2 * W), np.uint16))[:, :, ::2], fmt, 'bt709').copied
        # n == 0
        assert _hip.yuv16_frames_view(make(base)[:0], fmt, 'bt709').extent == 0


def test_view_errors():
    z = np.zeros
    with pytest.raises(TypeError):
        _hip.yuv16_frames_view(z((1, 12, 8), np.uint16), 'p010')                    # matrix has no default
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 12, 8), np.uint16), 'nv12', 'bt709')           # not a name of the family
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 12, 8), np.uint16), 'p010', 'bt2020')          # unknown matrix
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 12, 8), np.uint16), 'p010', 1)                 # code 1 is never assigned
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 12, 8), np.uint8), 'p010', 'bt709')            # not 16-bit samples
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 12, 8), np.int16), 'p010', 'bt709')            # (numpy int16 is not taken: view it as uint16)
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((12, 8), np.uint16), 'p010', 'bt709')              # not three-dimensional
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 13, 8), np.uint16), 'p010', 'bt709')           # rows not 3 H / 2
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 12, 7), np.uint16), 'p010', 'bt709')           # odd W
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 10, 8), np.uint16), 'i010', 'bt709')           # rows not 3 H / 2 (an odd H cannot be written so)
    with pytest.raises(ValueError):
        _hip.yuv16_frames_view(z((1, 15, 8), np.uint16), 'p210', 'bt709')           # rows not 2 H
    # odd BYTE strides cannot be described: a uint16 view of a byte buffer at an odd row pitch is copied once
    raw = z(3 * 12 * 17 + 1, np.uint8)
    odd = np.lib.stride_tricks.as_strided(raw[:2].view(np.uint16), shape=(1, 12, 8), strides=(12 * 17, 17, 2))
    v = _hip.yuv16_frames_view(odd, 'p010', 'bt709')
    assert v.copied and v.y_pitch == 16 and v.ptr % 2 == 0
    # an odd H is fine at 4:2:2
    v = _hip.yuv16_frames_view(z((1, 14, 8), np.uint16), 'i210', 'bt709')
    assert (v.H, v.W, v.c_pitch, v.sub_y) == (7, 8, 8, 0)


def test_reader_method_has_no_default_matrix():
    import inspect
    from meterelf_amd import MeterReader
    sig = inspect.signature(MeterReader.read_yuv16_frames)
    assert sig.parameters['matrix'].default is inspect.Parameter.empty
    assert sig.parameters['pixel_format'].default is inspect.Parameter.empty
    assert inspect.signature(MeterReader.read_yuv_planar_frames).parameters['matrix'].default == 'bt601'   # the siblings keep theirs


def test_reduce16_hand_written_4x4():
    """min(s >> shift, 255) on a 4 x 4 frame, each value worked out by hand; the package's reduce16 and the tests' agree."""
    s = np.array([[0x0000, 0x00ff, 0x0100, 0x01ff],
                  [0x03ff, 0x0400, 0x07ff, 0x0fff],
                  [0x1000, 0x8000, 0x80ff, 0xff00],
                  [0xffff, 0x0203, 0x0040, 0x1234]], np.uint16)
    want = {
        8: [[0, 0, 1, 1], [3, 4, 7, 15], [16, 128, 128, 255], [255, 2, 0, 0x12]],                 # the high byte
        2: [[0, 63, 64, 127], [255, 255, 255, 255], [255, 255, 255, 255], [255, 128, 16, 255]],   # 10 bits in the low bits
        4: [[0, 15, 16, 31], [63, 64, 127, 255], [255, 255, 255, 255], [255, 32, 4, 255]],        # 12 bits in the low bits
        0: [[0, 255, 255, 255], [255, 255, 255, 255], [255, 255, 255, 255], [255, 255, 64, 255]],
    }
    for (shift, w) in want.items():
        assert yc.reduce16(s, shift).tolist() == w, shift
        assert _hip.reduce16(s, shift).tolist() == w, shift
    # in-range 10-bit data: truncation of the two low bits, never rounding: 0x1ff = 511 -> 127 (511 / 4 = 127.75)
    assert int(yc.reduce16(np.array([511], np.uint16), 2)[0]) == 127
    # widen is a right inverse for every shift, with any dropped bits
    rng = np.random.default_rng(0)
    p = np.arange(256, dtype=np.uint8)
    for shift in (0, 2, 4, 8):
        assert np.array_equal(yc.reduce16(yc.widen(p, shift, rng), shift), p)
    g = yc.widen(np.full(4096, 100, np.uint8), 2, rng, garbage=True)
    r = yc.reduce16(g, 2)
    assert set(np.unique(r)) == {100, 255} and 300 < (r == 255).sum() < 800


def test_desc8_is_the_same_geometry():
    """The 8-bit descriptor of a 16-bit one addresses sample k of the reduced buffer where the 16-bit one addresses bytes 2 k."""
    rng = np.random.default_rng(3)
    (n, H, W) = (2, 6, 8)
    for fmt in yc.DISTINCT:
        (sy, step, _vf, shift) = FORMATS[fmt]
        src = (rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H >> sy, W // 2), dtype=np.uint8),
               rng.integers(0, 256, (n, H >> sy, W // 2), dtype=np.uint8))
        (raw, desc, lead) = yc.pitched16(*yc.widen_planes(src, fmt, rng), fmt, y_pad=6, c_pad=2, gap=4, stride_pad=10, rng=rng, lead=2)
        assert raw.nbytes - lead == yc.extent16(desc)
        d8 = yc.desc8_of(desc)
        b8 = yc.reduce16(raw[lead // 2:], shift)
        assert b8.nbytes == fc.extent_yuv_planar(d8)
        for f in range(n):
            o = f * d8.frame_stride
            Y = np.lib.stride_tricks.as_strided(b8[o:], shape=(H, W), strides=(d8.y_pitch, 1))
            U = np.lib.stride_tricks.as_strided(b8[o + d8.u_offset:], shape=(H >> sy, W // 2), strides=(d8.c_pitch, step))
            V = np.lib.stride_tricks.as_strided(b8[o + d8.v_offset:], shape=(H >> sy, W // 2), strides=(d8.c_pitch, step))
            assert np.array_equal(Y, src[0][f]) and np.array_equal(U, src[1][f]) and np.array_equal(V, src[2][f]), fmt


def test_kernels_metadata():
    """The kernels that read these frames are in the library: no private segment, no spilled vector registers; the dial readers
    within the dial kernels' register budget (128: four waves per SIMD)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata()
    names = ('k_y16_lplane', 'k_y16_match', 'k_y16_needle', 'k_y16_to_bgr')
    new = {k: d for (k, d) in meta.items() if any(s in k for s in names)}
    assert [sum(s in k for k in new) for s in names] == [2, 1, 12, 1]
    for (k, d) in new.items():
        assert d.get('private_segment_fixed_size', 0) == 0 and d.get('vgpr_spill_count', 0) == 0, (k, d)
        if 'k_y16_needle' in k:
            assert d['vgpr_count'] <= 128, (k, d)


def test_load_bounds_sweep(tmp_path):
    """tests/y16_bounds_main.cpp: every load the kernels' address arithmetic (melf_y16_addr.h) produces lies inside a buffer of
    exact extent, over the sweep the program's head lists.  Built with the host compiler, plain and with the host sanitizers."""
    src = os.path.join(ROOT, 'tests', 'y16_bounds_main.cpp')
    cxx = os.environ.get('CXX', 'g++')
    for (tag, flags) in (('plain', ['-O2']), ('san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('y16_bounds_' + tag))
        subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror'] + flags + ['-o', exe, src])
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, (tag, p.stdout[-2000:], p.stderr[-4000:])
        assert b'failures 0' in p.stdout, p.stdout
        print(tag, p.stdout.decode().strip())


# ------------------------------------------------------------------------------------------------------------- GPU ---------
@pytest.mark.gpu
@pytest.mark.parametrize('step', [1, 2])
@pytest.mark.parametrize('shift', [0, 2, 4, 8])
def test_to_bgr_every_y_value(env, shift, step):
    """One 256 x 256 frame whose Y takes all 65 536 values, U and V from a seeded generator over the full 16 bits, 4:2:0: the stage
    kernel == reduction + conversion restated, byte for byte."""
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(1000 + 10 * shift + step)
    Y = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    (U, V) = (rng.integers(0, 65536, (1, 128, 128), dtype=np.uint16), rng.integers(0, 65536, (1, 128, 128), dtype=np.uint16))
    fmt = 'p010' if step == 2 else 'i010'
    (raw, desc, _lead) = yc.pitched16(Y, U, V, fmt, rng=rng, matrix=3)
    desc.shift = shift
    got = ctx.yuv16_to_bgr(raw.ctypes.data, desc)
    want = fc.yuv_to_bgr(yc.reduce16(Y, shift), yc.reduce16(U, shift), yc.reduce16(V, shift), 1, 1, 3)
    bad = np.flatnonzero((got != want).any(axis=-1).ravel())
    assert bad.size == 0, (shift, step, bad.size, bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize('fmt,matrix', [('p010', 3), ('p010', 0), ('i010', 4), ('i010', 2)])
def test_to_bgr_all_triples(env, fmt, matrix):
    """All 2^24 reduced (Y, U, V), as tests/test_yuv_planar_frames.py::test_to_bgr_all_triples lays them out for 4:2:0: 2048 x 2048
    chroma samples b = (U, V) = (b & 255, (b >> 8) & 255), the four pixels of a block carry Y = 4 (b >> 16) + position; widened with
    random dropped bits."""
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(matrix)
    b = np.arange(2048 * 2048, dtype=np.uint32).reshape(2048, 2048)
    U = (b & 255).astype(np.uint8)[None]
    V = ((b >> 8) & 255).astype(np.uint8)[None]
    k = ((b >> 16).astype(np.uint8) * 4)
    Y = np.empty((1, 4096, 4096), np.uint8)
    (Y[0, 0::2, 0::2], Y[0, 0::2, 1::2], Y[0, 1::2, 0::2], Y[0, 1::2, 1::2]) = (k, k + 1, k + 2, k + 3)
    arr = yc.conventional16(*yc.widen_planes((Y, U, V), fmt, rng), fmt)
    v = _hip.yuv16_frames_view(arr, fmt, matrix)
    assert not v.copied
    got = ctx.yuv16_to_bgr(v.ptr, v.descriptor())
    want = fc.yuv_to_bgr(Y, U, V, 1, 1, matrix)
    bad = np.flatnonzero((got != want).any(axis=-1).ravel())
    assert bad.size == 0, (fmt, bad.size, bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', NAMES)
def test_to_bgr_padded_pitches(env, fmt):
    ctx = env['sample-images1']['reader'].ctx
    rng = np.random.default_rng(5)
    (sy, _step, _vf, shift) = FORMATS[fmt]
    (n, H, W) = (3, 38, 50)
    src = (rng.integers(0, 65536, (n, H, W), dtype=np.uint16), rng.integers(0, 65536, (n, H >> sy, W // 2), dtype=np.uint16),
           rng.integers(0, 65536, (n, H >> sy, W // 2), dtype=np.uint16))
    (raw, desc, lead) = yc.pitched16(*src, fmt, y_pad=18, c_pad=6, gap=10, stride_pad=26, rng=rng, matrix=4, lead=2)
    want = fc.yuv_to_bgr(*(yc.reduce16(p, shift) for p in src), 1, sy, 4)
    assert np.array_equal(ctx.yuv16_to_bgr(raw.ctypes.data + lead, desc), want)


# OK-status floors of test_identity_with_the_8bit_path: what the CPU oracle reads of the same 33 frames after the 8-bit conversion
# (BT.709 limited, 4:2:0 and 4:2:2 alike) -- 29 of 33 in both sets, the other four being the constant frames synth puts in.
IDENTITY_MIN_OK = {'sample-images1': 29, 'sample-images2': 29}


@pytest.mark.gpu
@pytest.mark.parametrize('sd', ['sample-images1', 'sample-images2'])
def test_identity_with_the_8bit_path(env, sd):
    """Every format name, 33 synthetic frames (synth -> bgr_to_yuv -> widen; the dropped low bits random): melf_process_yuv16_dev,
    the host path and melf_process_yuv_planar_dev on the reduced frames are equal as bytes, and equal read_frames of the BGR frame
    the conversion makes.  For the LSB formats one more batch with garbage high bits in one sample of eight: the clamp."""
    e = env[sd]
    reader = e['reader']
    bgr = fc.synth(e['frames'], 33, 16)
    rng = np.random.default_rng(33)
    wants = {}
    for (k, fmt) in enumerate(NAMES):
        (sy, step, _vf, shift) = FORMATS[fmt]
        if sy not in wants:
            src8 = yc.planes_of(bgr, fmt, 3)
            wants[sy] = (src8, reader.read_frames(yc.bgr_of(src8, fmt, 3)))
            assert (wants[sy][1]['status'] == _hip.FRAME_OK).sum() >= IDENTITY_MIN_OK[sd], (sd, sy, (wants[sy][1]['status'] == _hip.FRAME_OK).sum())
        (src8, want) = wants[sy]
        src16 = yc.widen_planes(src8, fmt, rng)
        arr = yc.conventional16(*src16, fmt, 6 if step == 2 else 0, rng)
        v = _hip.yuv16_frames_view(arr, fmt, 'bt709')
        assert not v.copied
        got = yc.check_identity(reader.ctx, v.ptr, v.descriptor(), v.extent, (sd, fmt))
        assert got.tobytes() == want.tobytes(), (sd, fmt, 'BGR path')
        assert reader.read_yuv16_frames(arr, fmt, 'bt709').tobytes() == want.tobytes(), (sd, fmt, 'reader')
        (raw, desc, lead) = yc.pitched16(*src16, fmt, y_pad=14, c_pad=10, gap=6, stride_pad=22, rng=rng, matrix=3, vfirst=bool(k & 1))
        got = yc.check_identity(reader.ctx, raw.ctypes.data, desc, raw.nbytes, (sd, fmt, 'pitched'))
        assert got.tobytes() == want.tobytes(), (sd, fmt, 'pitched, BGR path')   # (V first or not: the same picture)
        if shift < 8:
            g16 = yc.widen_planes(src8, fmt, rng, garbage=True)
            (raw, desc, lead) = yc.pitched16(*g16, fmt, y_pad=2, c_pad=2, stride_pad=2, rng=rng, matrix=3)
            got = yc.check_identity(reader.ctx, raw.ctypes.data, desc, raw.nbytes, (sd, fmt, 'garbage'))
            assert got.tobytes() != want.tobytes()   # the clamped samples are 255 now: other frames, other records


@pytest.mark.gpu
@pytest.mark.parametrize('sd,count', [('sample-images1', 81), ('sample-images2', 223)])
def test_fixture_frames(env, sd, count):
    """All fixture JPEG frames of both sets converted, as P010 and as I010: the records equal the packed BGR path's on the
    conversion's frame.  At least three quarters of each set read OK on the BGR side (the floor of the sibling files)."""
    e = env[sd]
    assert len(e['frames']) == count
    rng = np.random.default_rng(count)
    shapes = {}
    for fr in e['frames']:
        shapes.setdefault(fr.shape, []).append(fr)
    ok = 0
    for (shape, group) in shapes.items():
        src8 = fc.bgr_to_yuv(np.stack(group), 1, 1, 3)
        want = e['reader'].read_frames(fc.yuv_to_bgr(*src8, 1, 1, 3))
        ok += int((want['status'] == _hip.FRAME_OK).sum())
        for fmt in ('p010', 'i010'):
            arr = yc.conventional16(*yc.widen_planes(src8, fmt, rng), fmt, 0, rng)
            v = _hip.yuv16_frames_view(arr, fmt, 'bt709')
            (dev, host, fam) = yc.read_all(e['reader'].ctx, v.ptr, v.descriptor(), v.extent)
            assert dev.tobytes() == want.tobytes() and host.tobytes() == want.tobytes(), (sd, shape, fmt)
    print('%s: %d of %d converted frames read OK' % (sd, ok, count))
    assert 4 * ok >= 3 * count, ok


@pytest.mark.gpu
@pytest.mark.parametrize('kind,kernel', [('fast', 'mfma'), ('gen', 'gen'), ('dot4', 'dot4')])
def test_each_match_kernel(env, monkeypatch, kind, kernel):  # noqa: F811
    """Each match kernel forced (MELF_MATCH), asserted through melf_ctx_last_match after every call; 256 frames as the siblings."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    bgr = fc.synth(e['frames'], 256, 5)
    monkeypatch.setenv('MELF_MATCH', kind)
    r = MeterReader(e['params'])
    try:
        rng = np.random.default_rng(7)
        for fmt in ('p010', 'i210'):
            src8 = yc.planes_of(bgr, fmt, 3)
            want = r.read_frames(yc.bgr_of(src8, fmt, 3))
            assert r.ctx.last_match()['kernel'] == kernel
            assert (want['status'] == _hip.FRAME_DIALS_NOT_FOUND).sum() >= 28 and (want['status'] == _hip.FRAME_OK).sum() >= 128
            (raw, desc, _lead) = yc.pitched16(*yc.widen_planes(src8, fmt, rng), fmt, y_pad=2, c_pad=6, gap=2, stride_pad=2, rng=rng, matrix=3)
            assert r.ctx.process_yuv16(raw.ctypes.data, desc).tobytes() == want.tobytes(), (kind, fmt, 'host')
            assert r.ctx.last_match()['kernel'] == kernel
            buf = DevBuf(raw.ctypes.data, raw.nbytes)
            try:
                assert r.ctx.process_yuv16_dev(buf.d.value, desc).tobytes() == want.tobytes(), (kind, fmt, 'device')
            finally:
                buf.free()
            assert r.ctx.last_match()['kernel'] == kernel
    finally:
        r.close()


@pytest.mark.gpu
def test_batch_sizes(env):
    """Prep works in groups of 32 frames: 1, 31, 32, 33 and 65 frames, device buffers of exactly the extent."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(11)
    bgr = fc.synth(e['frames'], 65, 3)
    for fmt in ('p010', 'i010'):
        src8 = yc.planes_of(bgr, fmt, 3)
        want = reader.read_frames(yc.bgr_of(src8, fmt, 3))
        assert (want['status'] == _hip.FRAME_OK).sum() > 32
        src16 = yc.widen_planes(src8, fmt, rng)
        for n in (1, 31, 32, 33, 65):
            (raw, desc, _lead) = yc.pitched16(*(p[:n] for p in src16), fmt, y_pad=2 * (n % 4), c_pad=2, stride_pad=6, rng=rng, matrix=3)
            yc.check_identity(reader.ctx, raw.ctypes.data, desc, raw.nbytes, (fmt, n), want=want[:n])


@pytest.mark.gpu
def test_exact_extent_buffers_and_phases(env):
    """Buffers of exactly the extent: at the start of an allocation and ending where one ends (DevBuf.at_end), the base at phase 0
    and at phase 2 of a dword, the chroma planes at both phases against Y (gap)."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(17)
    bgr = fc.synth(e['frames'], 33, 8)
    for fmt in ('p010', 'i010', 'p210', 'i212'):
        src8 = yc.planes_of(bgr, fmt, 3)
        want = reader.read_frames(yc.bgr_of(src8, fmt, 3))
        src16 = yc.widen_planes(src8, fmt, rng)
        for (gap, phase) in ((0, 0), (2, 2), (2, 0), (0, 2)):
            (raw, desc, lead) = yc.pitched16(*src16, fmt, y_pad=gap, c_pad=2, gap=gap, stride_pad=gap, rng=rng, matrix=3, lead=phase)
            ptr = raw.ctypes.data + lead
            yc.check_identity(reader.ctx, ptr, desc, raw.nbytes - lead, (fmt, gap, phase, 'at end'), want=want, devbuf=DevBuf.at_end, phase=phase,
                              host=False)
            buf = DevBuf(raw.ctypes.data, raw.nbytes)   # the frames' base is `phase` bytes into an allocation of phase + extent bytes
            try:
                assert (buf.d.value + lead) % 4 == phase
                assert reader.ctx.process_yuv16_dev(buf.d.value + lead, desc).tobytes() == want.tobytes(), (fmt, gap, phase, 'at start')
            finally:
                buf.free()


@pytest.mark.gpu
def test_crop_at_first_byte_and_right_edge(env, tmp_path):
    """meter_rect (0, 0)-(250, 250) on frames cut so that the meter lies in their top left corner, once with the frame larger than
    the crop and once with the crop filling it (its right edge and last row are the frame's: the last quad of a window row and the
    last prep window end at the plane's edge): the crop's first Y samples are the buffer's first bytes.  Base phases 0 and 2."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    rng = np.random.default_rng(23)
    src = fc.synth(e['frames'], 40, 3)
    for (k, (y1, x1)) in enumerate(((480, 640), (410, 300))):
        bgr = np.ascontiguousarray(src[:, 160:y1, 50:x1])
        r = MeterReader(fc.params_with_rect(tmp_path, 'sample-images1', (0, 0, 250, 250), 'corner%d' % k))
        try:
            for fmt in ('p010', 'i010', 'p210', 'i210'):
                src8 = yc.planes_of(bgr, fmt, 3)
                want = r.read_frames(yc.bgr_of(src8, fmt, 3))
                assert (want['status'] == _hip.FRAME_OK).sum() >= 20, (y1, x1, fmt)
                src16 = yc.widen_planes(src8, fmt, rng)
                for phase in (0, 2):
                    (raw, desc, lead) = yc.pitched16(*src16, fmt, y_pad=phase, c_pad=2, gap=phase, stride_pad=phase, rng=rng, matrix=3, lead=phase)
                    assert r.ctx.process_yuv16(raw.ctypes.data + lead, desc).tobytes() == want.tobytes(), (y1, x1, fmt, phase, 'host')
                    buf = DevBuf(raw.ctypes.data, raw.nbytes)   # the frames' base is `phase` bytes into the allocation
                    try:
                        assert (buf.d.value + lead) % 4 == phase
                        assert r.ctx.process_yuv16_dev(buf.d.value + lead, desc).tobytes() == want.tobytes(), (y1, x1, fmt, phase, 'device')
                    finally:
                        buf.free()
        finally:
            r.close()


@pytest.mark.gpu
def test_odd_geometry(env, tmp_path):
    """meter_rect (50, 160)-(300, 410) at odd origins in x, in y and in both, and at odd sizes; the frames are shifted by as much."""
    from meterelf_amd import MeterReader
    e = env['sample-images1']
    src = fc.synth(e['frames'], 24, 3)
    rng = np.random.default_rng(13)
    for (k, (dx, dy, dw, dh)) in enumerate(((1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1), (1, 1, -1, -1))):
        params = fc.params_with_rect(tmp_path, 'sample-images1', (50 + dx, 160 + dy, 300 + dx + dw, 410 + dy + dh), 'odd%d' % k)
        bgr = np.roll(src, (dy, dx), axis=(1, 2))
        r = MeterReader(params)
        try:
            for fmt in ('p010', 'i010', 'p216', 'yuv422p12le'):
                src8 = yc.planes_of(bgr, fmt, 3)
                want = r.read_frames(yc.bgr_of(src8, fmt, 3))
                assert (want['status'] == _hip.FRAME_OK).sum() > 12, (dx, dy, dw, dh)
                (raw, desc, _lead) = yc.pitched16(*yc.widen_planes(src8, fmt, rng), fmt, y_pad=6, c_pad=2, gap=2, stride_pad=10, rng=rng, matrix=3)
                yc.check_identity(r.ctx, raw.ctypes.data, desc, raw.nbytes, (fmt, dx, dy, dw, dh), want=want)
        finally:
            r.close()


@pytest.mark.gpu
def test_host_staging_three_chunks(env):
    """257 host frames of 410 x 300: three staging chunks of 128 frames."""
    e = env['sample-images1']
    reader = e['reader']
    rng = np.random.default_rng(257)
    bgr = np.ascontiguousarray(fc.synth(e['frames'], 257, 4)[:, :410, :300])
    for fmt in ('p010', 'i210'):
        src8 = yc.planes_of(bgr, fmt, 3)
        want = reader.read_frames(yc.bgr_of(src8, fmt, 3))
        assert (want['status'] == _hip.FRAME_OK).sum() > 128
        arr = yc.conventional16(*yc.widen_planes(src8, fmt, rng), fmt, 0, rng)
        assert reader.read_yuv16_frames(arr, fmt, 'bt709').tobytes() == want.tobytes(), fmt


@pytest.mark.gpu
def test_resident_lanes_two_streams(env):  # noqa: F811
    """melf_ctx_set_frames_resident(1) and two caller streams, the layout changing from call to call (an 8-bit call among them):
    every call's records equal a synchronous call's."""
    from meterelf_amd import MeterReader
    e = env['sample-images2']
    bgr = fc.synth(e['frames'], 96, 21)
    nf = len(bgr)
    r = MeterReader(e['params'])
    bufs = []
    keep = []
    try:
        calls = []
        for (k, fmt) in enumerate(('p010', 'i010', 'nv16', 'p210', 'i012')):
            if fmt == 'nv16':
                (Y, U, V) = fc.bgr_to_yuv(bgr, 1, 0, 3)
                want = r.read_frames(fc.yuv_to_bgr(Y, U, V, 1, 0, 3))
                (raw, desc, _lead) = fc.pitched_yuv_planar(Y, U, V, 'nv16', y_pad=3, c_pad=1, rng=np.random.default_rng(k), matrix=3)
                keep.append(raw)
                bufs.append(DevBuf(raw.ctypes.data, raw.nbytes))
                calls.append((functools.partial(r.ctx.process_yuv_planar_dev, bufs[-1].d.value, desc), want.tobytes()))
                continue
            src8 = yc.planes_of(bgr, fmt, 3)
            want = r.read_frames(yc.bgr_of(src8, fmt, 3))
            assert (want['status'] == _hip.FRAME_OK).sum() > 48
            rng = np.random.default_rng(k)
            (raw, desc, _lead) = yc.pitched16(*yc.widen_planes(src8, fmt, rng), fmt, y_pad=2 * k, c_pad=4 * k + 2, gap=2 * k, stride_pad=2 * k, rng=rng,
                                              matrix=3)
            keep.append(raw)
            bufs.append(DevBuf(raw.ctypes.data, raw.nbytes))
            calls.append((functools.partial(r.ctx.process_yuv16_dev, bufs[-1].d.value, desc), want.tobytes()))
        fc.resident_calls(r, nf, calls, 2 * len(calls), lambda i: (3 * i) % len(calls))
    finally:
        r.close()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_argument_errors_launch_nothing(env):
    e = env['sample-images1']
    ctx = e['reader'].ctx
    L = _hip.lib()
    src8 = fc.bgr_to_yuv(np.stack(e['frames'][2:6]), 1, 0, 3)
    (n, H, W) = src8[0].shape
    rng = np.random.default_rng(2)
    arr = yc.conventional16(*yc.widen_planes(src8, 'i210', rng), 'i210')
    buf = DevBuf(arr.ctypes.data, arr.nbytes)
    try:
        ctx.set_profiling(1)
        before = fc.launch_counts(ctx)
        out = np.zeros(n, _hip.RESULT_DTYPE)
        bgr_out = np.zeros((n, H, W, 3), np.uint8)
        F = _hip.MelfYuv16Frames
        (fs, q, uo) = (4 * H * W, H * W, 2 * H * W)   # bytes: a frame, a chroma plane, the Y plane

        def D(matrix=3, n=n, H=H, W=W, sub_y=0, c_step=1, shift=2, reserved=0, y_pitch=2 * W, c_pitch=W, u=uo, v=uo + q, fs=fs):
            return F(matrix, n, H, W, sub_y, c_step, shift, reserved, y_pitch, c_pitch, u, v, fs)
        # (what melf_last_error must name, the descriptor)
        bad = [
            ('reserved', D(reserved=1)),
            ('sub_y must be', D(sub_y=2)), ('sub_y must be', D(sub_y=-1)),
            ('c_step must be', D(c_step=0)), ('c_step must be', D(c_step=3)),
            ('shift must be', D(shift=-1)), ('shift must be', D(shift=9)),
            ('2 bytes apart', D(c_step=2, c_pitch=2 * W, u=uo, v=uo + 4)),       # semi-planar: offsets not one sample apart
            ('2 bytes apart', D(c_step=2, c_pitch=2 * W, u=uo, v=uo)),
            ('even', D(c_step=2, c_pitch=2 * W, u=uo, v=uo + 1)),                # ... 1 byte apart: an odd offset
            ('even width', D(W=W - 1, y_pitch=2 * W)),                           # odd W
            ('even height', D(sub_y=1, H=H - 1)),                                # odd H with sub_y
            ('batch shape', D(H=0)), ('batch shape', D(W=0)), ('batch shape', D(n=-1)),
            ('negative', D(u=-2)), ('negative', D(v=-2)),
            ('matrix', D(matrix=1)), ('matrix', D(matrix=5)), ('matrix', D(matrix=-1)),
            ('even', D(y_pitch=2 * W + 1)), ('even', D(c_pitch=W + 1)), ('even', D(u=uo + 1, v=uo + q + 1, fs=fs + 2)),
            ('even', D(v=uo + q + 1, fs=fs + 2)), ('even', D(fs=fs + 1)),        # an odd byte quantity, each of the five
            ('y_pitch', D(y_pitch=2 * W - 2)),
            ('c_pitch', D(c_pitch=W - 2)),
            ('c_pitch', D(c_step=2, c_pitch=2 * W - 2, u=uo, v=uo + 2)),
            ('two chroma planes', D(u=uo, v=uo + q - 2)),                        # the chroma planes' spans overlap each other
            ('two chroma planes', D(u=uo + q - 2, v=uo)),
            ("Y plane's span", D(u=uo - 2)),                                     # a chroma plane starts inside the Y plane's span
            ("Y plane's span", D(u=uo + q, v=uo - 2)),
            ("Y plane's span", D(c_step=2, c_pitch=2 * W, u=uo - 2, v=uo)),
            ('frame_stride', D(fs=fs - 2)),                                      # stride smaller than one frame's span
            ('frame_stride', D(c_step=2, c_pitch=2 * W, u=uo + 2, v=uo, fs=fs - 2)),
            ('y_pitch', D(y_pitch=2 ** 31)), ('c_pitch', D(c_pitch=2 ** 31)),
        ]
        fields = [f[0] for f in F._fields_]
        for (word, f) in bad:
            key = (word,) + tuple(getattr(f, k) for k in fields)
            assert L.melf_process_yuv16_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(f), None, _hip._ptr(out), None) == -1, key
            assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
            assert L.melf_process_yuv16(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(out)) == -1, key
            assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
            assert L.melf_yuv16_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), C.byref(f), _hip._ptr(bgr_out)) == -1, key
            assert word in L.melf_last_error().decode(), (key, L.melf_last_error().decode())
        assert L.melf_process_yuv16_dev(ctx._h, C.c_void_p(buf.d.value), None, None, _hip._ptr(out), None) == -1
        assert L.melf_process_yuv16(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(out)) == -1
        assert 'descriptor is NULL' in L.melf_last_error().decode()
        assert L.melf_yuv16_to_bgr(ctx._h, C.c_void_p(arr.ctypes.data), None, _hip._ptr(bgr_out)) == -1
        good = D()
        assert L.melf_process_yuv16_dev(ctx._h, None, C.byref(good), None, _hip._ptr(out), None) == -1   # NULL frames
        assert 'frames pointer is NULL' in L.melf_last_error().decode()
        assert L.melf_process_yuv16(ctx._h, None, C.byref(good), _hip._ptr(out)) == -1
        assert 'frames pointer is NULL' in L.melf_last_error().decode()
        assert L.melf_yuv16_to_bgr(ctx._h, None, C.byref(good), _hip._ptr(bgr_out)) == -1
        assert 'frames pointer is NULL' in L.melf_last_error().decode()
        assert L.melf_process_yuv16_dev(ctx._h, C.c_void_p(buf.d.value + 1), C.byref(good), None, _hip._ptr(out), None) == -1   # an odd base
        assert '2-byte aligned base' in L.melf_last_error().decode()
        assert L.melf_process_yuv16(ctx._h, C.c_void_p(arr.ctypes.data + 1), C.byref(good), _hip._ptr(out)) == -1
        assert '2-byte aligned base' in L.melf_last_error().decode()
        empty = D(n=0)
        assert L.melf_process_yuv16_dev(ctx._h, None, C.byref(empty), None, None, None) == 0             # n == 0 passes
        assert L.melf_process_yuv16(ctx._h, None, C.byref(empty), None) == 0
        assert fc.launch_counts(ctx) == before
        # a good descriptor runs
        assert L.melf_process_yuv16_dev(ctx._h, C.c_void_p(buf.d.value), C.byref(good), None, _hip._ptr(out), None) == 0
        assert fc.launch_counts(ctx) != before
        assert out.tobytes() == e['reader'].read_frames(fc.yuv_to_bgr(*src8, 1, 0, 3)).tobytes()
    finally:
        ctx.set_profiling(0)
        buf.free()


@pytest.mark.gpu
def test_torch_tensors_in_a_torch_process():
    """read_yuv16_frames with torch tensors (uint16 where torch has it, int16 as the same bits), a device tensor and out=, in a child
    process that imports torch first (tests/frame_cases.py says why)."""
    env_ = dict(os.environ)
    env_['PYTHONPATH'] = ROOT + os.pathsep + env_.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'yuv16_torch_child.py')], env=env_, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0 and b'torch yuv16 path ok' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
