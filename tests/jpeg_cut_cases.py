"""What tests/test_jpeg_truncated.py and tools/jpeg_cut_rate.py share: baseline JPEG files that end inside their scan
(melf_ctx_set_jpeg_truncated), the rule for them restated in Python, the cuts of a file, and the range filter with its cap.

The reference never comes from the GPU: a frame is Pillow's (libjpeg-turbo's) decode of `data[:cut] + FF D9`.  The rule here is
what a CPU test holds against Pillow at every cut; the GPU tests use it only to tell which cuts lie inside the range where the
project's exactness contract holds (tests/jpeg_writer.py, module docstring), and the host program's test to check the walk.

The rule.  The stream is the entropy-coded bytes without stuffing and markers, then zero bits for ever.  The cut MCU is the MCU
during whose decode a bit behind the real bytes is first required; it is decoded completely, from the zero bits; every block of
every later MCU is zero, DC included.  A stream that ends on an MCU boundary makes the next MCU the cut MCU.  With restart
intervals the last interval found may be short or empty; if it is complete and intervals are owing, the first MCU of the next
one, predictors reset, is the cut MCU.  A run that overshoots the block stores at natural index 63 (libjpeg's padded zig-zag
table)."""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # the tool imports this module from tools/, without the package
import jpeg_writer as jw  # noqa: E402

CAP = 16   # at most one cut in CAP of a file may lie outside the range (and so be left out of a comparison)


def pillow_bgr(data):
    from PIL import Image, ImageFile
    old = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = True
    try:
        with Image.open(io.BytesIO(data)) as im:
            rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = old
    return np.ascontiguousarray(rgb[:, :, ::-1])


def reference(data, cut):
    """The oracle: Pillow on the first `cut` bytes and an EOI."""
    return pillow_bgr(data[:cut] + b'\xff\xd9')


def pillow_file(size, subsampling, quality=90, restart=0, seed=5, grey=False):
    """A Pillow-written baseline file of a natural image (subsampling: '4:2:0', '4:2:2', '4:4:4'; restart: MCUs an interval)."""
    from PIL import Image
    (H, W) = size
    rng = np.random.default_rng(seed)
    (yy, xx) = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3), np.float64)
    for c in range(3):
        img[..., c] = 128 + 90 * np.sin(xx / (5.0 + 3 * c) + rng.uniform(0, 6)) * np.cos(yy / (7.0 + 2 * c))
    img += rng.normal(0, 10, img.shape)
    img = np.clip(img, 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    kw = {'restart_marker_blocks': restart} if restart else {}
    if grey:
        Image.fromarray(img[..., 1]).save(buf, 'JPEG', quality=quality, **kw)
    else:
        Image.fromarray(img).save(buf, 'JPEG', quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


# ------------------------------------------------------------------ parsing ----
class Parsed:
    """Headers of a baseline single-scan file: size, sampling, tables, selectors, restart interval, where the scan lies."""


def parse(data):
    p = Parsed()
    p.data = data
    p.q = {}
    p.restart = 0
    spec = {}
    i = 2
    while True:
        assert data[i] == 0xFF
        (m, L) = (data[i + 1], (data[i + 2] << 8) | data[i + 3])
        s = data[i + 4:i + 2 + L]
        if m == 0xDB:
            o = 0
            while o < len(s):
                (pq, t) = (s[o] >> 4, s[o] & 15)
                n = 128 if pq else 64
                zz = [(s[o + 1 + 2 * k] << 8) | s[o + 2 + 2 * k] for k in range(64)] if pq else list(s[o + 1:o + 65])
                nat = [0] * 64
                for k in range(64):
                    nat[int(jw.ZIGZAG[k])] = zz[k]
                p.q[t] = (nat, bool(pq))
                o += 1 + n
        elif m == 0xC4:
            o = 0
            while o < len(s):
                bits = [0] + list(s[o + 1:o + 17])
                n = sum(bits)
                spec[('ac' if s[o] >> 4 else 'dc', s[o] & 15)] = (bits, list(s[o + 17:o + 17 + n]))
                o += 17 + n
        elif m in (0xC0, 0xC1):
            p.size = ((s[1] << 8) | s[2], (s[3] << 8) | s[4])
            nc = s[5]
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(nc)]
            (hs, vs) = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
            p.sampling = [k for (k, v) in jw.SAMPLING.items() if v == (nc, hs, vs)][0]
            p.tq = [c[3] for c in comps]
        elif m == 0xDD:
            p.restart = (s[0] << 8) | s[1]
        elif m == 0xDA:
            nc = s[0]
            p.sel = [(p.tq[c], s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(nc)]
            p.scan_begin = i + 2 + L
            break
        i += 2 + L
    if not spec:   # a file without DHT segments: the Annex K tables
        std = jw.standard_tables()
        spec = {('dc', 0): std['dc'][0], ('dc', 1): std['dc'][1], ('ac', 0): std['ac'][0], ('ac', 1): std['ac'][1]}
    p.dc = {t: v for ((k, t), v) in spec.items() if k == 'dc'}
    p.ac = {t: v for ((k, t), v) in spec.items() if k == 'ac'}
    (p.clean, p.rst, _m, used) = clean(data[p.scan_begin:])
    p.scan_end = p.scan_begin + used   # the FF of the marker that ends the scan (EOI)
    # per prefix length of the scan's raw bytes: clean bytes and restart markers it holds (an FF whose second byte is missing is dropped)
    raw = data[p.scan_begin:p.scan_end]
    (p.pre_len, p.pre_rst) = ([0] * (len(raw) + 1), [0] * (len(raw) + 1))
    (i, out, nr) = (0, 0, 0)
    while i < len(raw):
        (p.pre_len[i], p.pre_rst[i]) = (out, nr)
        if raw[i] != 0xFF or (i + 1 < len(raw) and raw[i + 1] == 0xFF):
            out += raw[i] != 0xFF
            i += 1
            continue
        if i + 1 < len(raw):
            (p.pre_len[i + 1], p.pre_rst[i + 1]) = (out, nr)
            if raw[i + 1] == 0:
                out += 1
            else:
                nr += 1
        i += 2
    (p.pre_len[len(raw)], p.pre_rst[len(raw)]) = (out, nr)
    (nc, hs, vs) = jw.SAMPLING[p.sampling]
    p.layout = [(0, y, x) for y in range(vs) for x in range(hs)] + [(c, 0, 0) for c in range(1, nc)]
    ((p.my, p.mx), p.shapes) = jw.grid_shape(p.size, p.sampling)
    return p


def clean(raw):
    """k_jpeg_clean's rule on a byte string: (clean bytes, clean offsets where the restart intervals begin, the byte behind the FF
    that ended the scan or None, raw bytes up to that FF)."""
    out = bytearray()
    rst = [0]
    i = 0
    n = len(raw)
    while i < n:
        b = raw[i]
        if b != 0xFF:
            out.append(b)
            i += 1
            continue
        if i + 1 >= n:
            return (bytes(out), rst, None, i)
        nb = raw[i + 1]
        if nb == 0:
            out.append(0xFF)
            i += 2
        elif nb == 0xFF:
            i += 1
        elif 0xD0 <= nb <= 0xD7:
            rst.append(len(out))
            i += 2
        else:
            return (bytes(out), rst, nb, i)
    return (bytes(out), rst, None, n)


def cuts(p):
    """Every cut position of a file: from its first scan byte to its last."""
    return list(range(p.scan_begin, p.scan_end))


# ------------------------------------------------------------------ decoding ----
def _codes(spec):
    out = {}
    code = 0
    k = 0
    for l in range(1, 17):
        for _ in range(spec[0][l]):
            out[(l, code)] = spec[1][k]
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    """The real bits of a clean stream, then zeros."""

    def __init__(self, clean_bytes):
        self.bits = 8 * len(clean_bytes)
        self.v = int.from_bytes(clean_bytes + bytes(8), 'big')

    def window(self, p):   # 32 bits at p
        if p >= self.bits:
            return 0
        return (self.v >> (self.bits + 64 - 32 - p)) & 0xFFFFFFFF


def _symbol(codes, w):
    for l in range(1, 17):
        s = codes.get((l, w >> (32 - l)))
        if s is not None:
            return (l, s)
    raise ValueError('a code no table has')


def _block(bs, pos, k, codes_dc, codes_ac, pred, blk, trace=None):
    """Decodes on from coefficient index k of a block (zig-zag array blk, filled in place).  Returns (pos, pred)."""
    while k < 64:
        w = bs.window(pos)
        if trace is not None:
            trace.append((pos, k))
        if k == 0:
            (l, s) = _symbol(codes_dc, w)
            raw = (w << l & 0xFFFFFFFF) >> (32 - s) if s else 0
            v = raw - (1 << s) + 1 if s and 2 * raw < (1 << s) else raw
            pred += v
            blk[0] = pred
            k = 1
            pos += l + s
            continue
        (l, sym) = _symbol(codes_ac, w)
        (run, s) = (sym >> 4, sym & 15)
        raw = (w << l & 0xFFFFFFFF) >> (32 - s) if s else 0
        v = raw - (1 << s) + 1 if s and 2 * raw < (1 << s) else raw
        pos += l + s
        if s:
            at = k + run
            blk[min(at, 63)] = v
            k = at + 1
        elif run == 15:
            k += 16
        else:
            k = 64
    return (pos, pred)


class Decoded:
    """A whole file decoded once: the coefficient grids, and per MCU where it starts and the predictors there; per symbol its
    state (for the host program's cases)."""


def decode(p):
    d = Decoded()
    (cl, rst) = (p.clean, p.rst)
    d.clean = cl
    d.rst = rst
    bs = _Bits(cl)
    nc = len(p.sel)
    d.dc = {t: _codes(s) for (t, s) in p.dc.items()}
    d.ac = {t: _codes(s) for (t, s) in p.ac.items()}
    d.grids = [np.zeros((by, bx, 64), np.int16) for (by, bx) in p.shapes]
    d.mcu_start = []   # (bit position, predictors)
    d.symbols = []     # (bit position, block within the MCU, coefficient index, block in decode order, predictors)
    pos = 0
    pred = [0] * nc
    total = p.my * p.mx
    for m in range(total):
        if p.restart and m and m % p.restart == 0:
            pos = rst[m // p.restart] * 8
            pred = [0] * nc
        d.mcu_start.append((pos, tuple(pred)))
        (yy, xx) = divmod(m, p.mx)
        for (b, (c, y, x)) in enumerate(p.layout):
            (_tq, td, ta) = p.sel[c]
            zz = [0] * 64
            trace = []
            before = tuple(pred)
            (pos, pred[c]) = _block(bs, pos, 0, d.dc[td], d.ac[ta], pred[c], zz, trace)
            for (at, k) in trace:
                d.symbols.append((at, b, k, m * len(p.layout) + b, before if k == 0 else tuple(pred)))
            (h, v) = (jw.SAMPLING[p.sampling][1], jw.SAMPLING[p.sampling][2]) if c == 0 else (1, 1)
            d.grids[c][yy * v + y, xx * h + x, jw.ZIGZAG] = zz
        assert pos <= bs.bits
    d.sym_pos = np.array([s[0] for s in d.symbols], np.int64)
    return d


def truncated_stream(p, cut):
    """(clean bytes, intervals found, end marker) of the file's first `cut` bytes."""
    k = cut - p.scan_begin
    return (p.clean[:p.pre_len[k]], 1 + p.pre_rst[k], None)


def rule(p, d, cut):
    """The coefficient grids the rule gives the file cut at `cut`, the cut MCU's index (None: the file is whole), and the bits of
    its stream."""
    (cl, nint, _m) = truncated_stream(p, cut)
    bits = 8 * len(cl)
    assert d.clean[:len(cl)] == cl
    total = p.my * p.mx
    nc = len(p.sel)
    # the last MCU that starts inside the stream, in an interval that was found
    last = -1
    for m in range(total):
        if p.restart and m // p.restart >= nint:
            break
        if d.mcu_start[m][0] <= bits:
            last = m
    assert last >= 0
    bs = _Bits(cl)
    (pos, pred) = (d.mcu_start[last][0], list(d.mcu_start[last][1]))
    blocks = []
    for (c, _y, _x) in p.layout:
        (_tq, td, ta) = p.sel[c]
        zz = [0] * 64
        (pos, pred[c]) = _block(bs, pos, 0, d.dc[td], d.ac[ta], pred[c], zz)
        blocks.append(zz)
    cut_mcu = last
    if pos <= bits:   # decoded from real bits alone: the next MCU, if one is owing, from zeros (it begins an interval not found)
        if last + 1 >= total:
            return ([g.copy() for g in d.grids], None, bits)
        assert p.restart and (last + 1) % p.restart == 0, 'an MCU that starts inside the stream was passed over'
        cut_mcu = last + 1
        bs = _Bits(b'')
        (pos, pred) = (0, [0] * nc)
        blocks = []
        for (c, _y, _x) in p.layout:
            (_tq, td, ta) = p.sel[c]
            zz = [0] * 64
            (pos, pred[c]) = _block(bs, pos, 0, d.dc[td], d.ac[ta], pred[c], zz)
            blocks.append(zz)
    grids = [np.zeros_like(g) for g in d.grids]
    (nc_, hs, vs) = jw.SAMPLING[p.sampling]
    for m in range(cut_mcu + 1):
        (yy, xx) = divmod(m, p.mx)
        for (b, (c, y, x)) in enumerate(p.layout):
            (h, v) = (hs, vs) if c == 0 else (1, 1)
            if m < cut_mcu:
                grids[c][yy * v + y, xx * h + x] = d.grids[c][yy * v + y, xx * h + x]
            else:
                grids[c][yy * v + y, xx * h + x, jw.ZIGZAG] = np.array(blocks[b], np.int64).astype(np.int16)
    return (grids, cut_mcu, bits)


def in_range(p, grids):
    """The condition of tests/jpeg_writer.py's contract on the rule's grids: libjpeg's range limit is a plain clamp there."""
    try:
        jw.check_in_range(grids, p.q, p.sel)
    except AssertionError:
        return False
    return True


def in_range_cuts(p, d, positions):
    """[(cut, grids, cut MCU)] of the cuts inside the range; asserts that at most one cut in CAP was left out."""
    kept = []
    for cut in positions:
        (grids, cm, _bits) = rule(p, d, cut)
        if in_range(p, grids):
            kept.append((cut, grids, cm))
    left_out = len(positions) - len(kept)
    assert left_out * CAP <= len(positions), 'the range filter left out %d of %d cuts: more than one in %d' % (left_out, len(positions), CAP)
    return kept


def reencode(p, grids):
    """The rule's grids as a complete file with the file's own quantisation tables and the Annex K Huffman tables."""
    std = jw.standard_tables()
    nc = len(grids)
    dc = {t: std['dc'][t] for t in range(min(nc, 2))}
    ac = {t: std['ac'][t] for t in range(min(nc, 2))}
    sel = [(p.sel[c][0], min(c, 1), min(c, 1)) for c in range(nc)]
    return jw.write_jpeg(grids, p.size, p.sampling, p.q, dc, ac, sel=sel, check=False)


# ------------------------------------------------------------------ the host program's cases ----
def huff_slow(spec):
    """build_huff of melf_jpeg_parse.h: (limit[16], valoff[16], huffval[256])."""
    (limit, valoff) = ([], [])
    (code, k) = (0, 0)
    for l in range(1, 17):
        valoff.append(k - code)
        k += spec[0][l]
        code += spec[0][l]
        limit.append(code)
        code <<= 1
    return (limit, valoff, list(spec[1]) + [0] * (256 - len(spec[1])))


def program_input(p, d, positions):
    """The text tests/jpeg_cut_main.cpp reads: layout, the four tables, the whole clean stream, then one case per cut -- the stream's
    bits, a decoder state at a symbol boundary not behind them (bit position, block within the MCU, coefficient index, block in decode
    order, predictors) and the block the walk may not pass.  Returns (text, [(cut, first block, first coefficient index)])."""
    bpm = len(p.layout)
    (comp_bits, dc_bits, ac_bits) = (0, 0, 0)
    for (b, (c, _y, _x)) in enumerate(p.layout):
        comp_bits |= c << (2 * b)
        dc_bits |= p.sel[c][1] << b
        ac_bits |= p.sel[c][2] << b
    lines = ['%d %d %d %d' % (bpm, comp_bits, dc_bits, ac_bits)]
    for (kind, t) in (('dc', 0), ('dc', 1), ('ac', 0), ('ac', 1)):
        spec = (p.dc if kind == 'dc' else p.ac).get(t)
        (limit, valoff, vals) = huff_slow(spec) if spec else ([0] * 16, [0] * 16, [0] * 256)
        lines.append(' '.join(str(v) for v in limit + valoff + vals))
    lines.append('%d %s' % (len(d.clean), d.clean.hex() or '-'))
    total_blocks = p.my * p.mx * bpm
    per_interval = p.restart * bpm if p.restart else total_blocks
    cases = []
    for (n, cut) in enumerate(positions):
        (_grids, cm, bits) = rule(p, d, cut)
        (_cl, nint, _m) = truncated_stream(p, cut)
        first_owed = cm * bpm
        # a symbol boundary not behind the stream's end, inside the cut MCU's interval, a few symbols before the end
        hi = int(np.searchsorted(d.sym_pos, bits, side='right')) - 1
        while hi >= 0 and d.symbols[hi][3] // per_interval > first_owed // per_interval:
            hi -= 1
        lo = hi
        while lo > 0 and lo > hi - n % 7 and d.symbols[lo - 1][3] // per_interval == first_owed // per_interval and d.symbols[lo - 1][0] <= bits:
            lo -= 1
        if hi >= 0 and d.symbols[lo][3] // per_interval == first_owed // per_interval and d.symbols[lo][3] <= first_owed + bpm - 1 and nint > first_owed // per_interval:
            (pos, blk, k, nb, pred) = d.symbols[lo]
        else:   # the cut MCU begins an interval that was not found (or has no symbol inside the stream): from zero bits
            (pos, blk, k, nb, pred) = (bits, 0, 0, first_owed, (0,) * len(p.sel))
        pred = tuple(pred) + (0,) * (3 - len(pred))
        limit = min((nb // per_interval + 1) * per_interval, total_blocks)
        lines.append('%d %d %d %d %d %d %d %d %d' % ((bits, pos, blk, k, nb) + pred + (limit,)))
        cases.append((cut, nb, k))
    return ('\n'.join(lines) + '\n', cases)
