"""A baseline JPEG *writer* for the decoder tests, written from ITU-T T.81 (pure Python / numpy, no conftest, no fixtures).

Pillow's encoder and the fixture cameras all write one kind of stream (Annex K or optimiser tables, luma on tables 0 and
chroma on tables 1, one header layout, 8-bit quantisation tables, component ids 1 2 3).  This module starts from quantised
coefficient blocks and takes everything else as a parameter, so that a test can hand the GPU decoder the streams no encoder at
hand writes; Pillow (libjpeg-turbo) stays the reference DECODER.

Scope.  Every file written here must stay inside the range where libjpeg-turbo's C and SIMD code paths are one function; that
is a condition on the inputs and `write_jpeg` asserts it: every dequantised coefficient fits in int16, and a float64 inverse
DCT of every dequantised block, level shift included, stays within -256 ... +511 (and the unshifted value within the same
bounds), where libjpeg's range-limit step is a plain clamp.  Outside that range libjpeg-turbo's output depends on the build,
there is no reference, and such inputs are out of scope.  Progressive, arithmetic and 12-bit files are out of scope too.

Coefficient blocks: one int16 array per component of shape (blocks_y, blocks_x, 64), natural (row-major) order inside a
block, the grids padded to whole MCUs.  A Huffman spec is the pair (bits, vals) of a DHT segment: bits[l] = number of codes
of length l (bits[0] = 0, 17 entries), vals = the symbols in code order.
"""
import io

import numpy as np

# sampling mode -> (components, luma h, luma v); chroma is always 1 x 1.  '440' and '411' exist for the refusal tests.
SAMPLING = {'grey': (1, 1, 1), '444': (3, 1, 1), '422': (3, 2, 1), '420': (3, 2, 2), '440': (3, 1, 2), '411': (3, 4, 1)}

TAB_BITS = 10   # first-level table of the decoder under test: codes of at most TAB_BITS bits
LONG_N = 512    # 16-bit windows per AC table its long-code table holds (tests/test_jpeg_streams.py checks both against the kernel source)


def _zigzag():
    """Natural index of zig-zag position k (T.81 figure A.6), generated rather than typed in."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, np.int64)


ZIGZAG = _zigzag()
_u = np.arange(8)
_C = np.sqrt(0.25) * np.cos((2 * _u[None, :] + 1) * _u[:, None] * np.pi / 16)
_C[0, :] = np.sqrt(0.125)   # orthonormal 8-point DCT-II: coefficient = C x C^T, the scaling of T.81 A.3.3


def fdct(blocks):
    """Float64 forward DCT of (..., 8, 8) sample blocks (level shift already taken)."""
    return _C @ np.asarray(blocks, np.float64) @ _C.T


def idct(blocks):
    return _C.T @ np.asarray(blocks, np.float64) @ _C


def grid_shape(size, sampling):
    """(mcus_y, mcus_x) and per component (blocks_y, blocks_x) of the MCU-padded block grids."""
    (H, W) = size
    (nc, hs, vs) = SAMPLING[sampling]
    (my, mx) = (-(-H // (8 * vs)), -(-W // (8 * hs)))
    return (my, mx), [(my * vs, mx * hs)] + [(my, mx)] * (nc - 1)


def coefficients_from_image(img, sampling, qtables):
    """Quantised coefficient grids of an image: RGB -> YCbCr (JFIF), edge replication to whole MCUs, box downsampling of
    chroma, level shift, float64 forward DCT, division by the component's table (qtables: one 64-entry table in natural order
    per component) and rounding."""
    img = np.asarray(img)
    (nc, hs, vs) = SAMPLING[sampling]
    (H, W) = img.shape[:2]
    if nc == 1:
        planes = [img.astype(np.float64) if img.ndim == 2 else img[..., 0].astype(np.float64)]
    else:
        (r, g, b) = (img[..., 0].astype(np.float64), img[..., 1].astype(np.float64), img[..., 2].astype(np.float64))
        planes = [0.299 * r + 0.587 * g + 0.114 * b, 128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b]
    (_m, shapes) = grid_shape((H, W), sampling)
    out = []
    for (c, p) in enumerate(planes):
        (by, bx) = shapes[c]
        (fy, fx) = (1, 1) if c == 0 else (vs, hs)
        p = np.pad(p, ((0, shapes[0][0] * 8 - H), (0, shapes[0][1] * 8 - W)), mode='edge')
        if fy * fx > 1:
            p = p.reshape(by * 8, fy, bx * 8, fx).mean(axis=(1, 3))
        blocks = p.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128.0
        q = np.asarray(qtables[c], np.float64).reshape(8, 8)
        out.append(np.rint(fdct(blocks) / q).astype(np.int16).reshape(by, bx, 64))
    return out


# ------------------------------------------------------------------ Huffman specs ----
def tables_from_lengths(symbols_by_length):
    """{code length: [symbols in code order]} -> (bits, vals)."""
    bits = [0] * 17
    vals = []
    for l in sorted(symbols_by_length):
        assert 1 <= l <= 16
        bits[l] = len(symbols_by_length[l])
        vals += list(symbols_by_length[l])
    return (bits, vals)


def length_limited_tables(frequencies, max_len=16):
    """A Huffman spec for {symbol: frequency > 0} with no code longer than max_len and the all-ones code left free: the
    procedure of T.81 K.2 (a reserved extra symbol, figure K.3's adjustment of over-long codes) with max_len for its 16."""
    freq = {s: f for (s, f) in frequencies.items() if f > 0}
    assert freq
    nodes = [(f, [s]) for (s, f) in freq.items()] + [(0.5, [256])]   # 256: the reserved code point, rarest of all
    size = {s: 0 for (_f, ss) in nodes for s in ss}
    while len(nodes) > 1:
        nodes.sort(key=lambda n: (n[0], -max(n[1])))
        ((f1, s1), (f2, s2)) = nodes[:2]
        for s in s1 + s2:
            size[s] += 1
        nodes = nodes[2:] + [(f1 + f2, s1 + s2)]
    top = max(max(size.values()), max_len)
    bits = [0] * (top + 1)
    for s in size:
        bits[max(size[s], 1)] += 1
    for i in range(top, max_len, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = max_len
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1   # the reserved code point
    order = sorted(freq, key=lambda s: (size[s], -freq[s], s))
    out = [0] * 17
    out[1:max_len + 1] = bits[1:max_len + 1]
    assert sum(out) == len(order)
    return (out, order)


def _spec_from_dht(data):
    """{('dc' | 'ac', id): (bits, vals)} of every table in a file's DHT segments."""
    out = {}
    i = 2
    while data[i + 1] != 0xDA:
        (m, L) = (data[i + 1], (data[i + 2] << 8) | data[i + 3])
        if m == 0xC4:
            s = data[i + 4:i + 2 + L]
            o = 0
            while o < len(s):
                bits = [0] + list(s[o + 1:o + 17])
                n = sum(bits)
                out[('ac' if s[o] >> 4 else 'dc', s[o] & 15)] = (bits, list(s[o + 17:o + 17 + n]))
                o += 17 + n
        i += 2 + L
    return out


_STANDARD = []


def standard_tables():
    """The Annex K tables {'dc': [luma, chroma], 'ac': [luma, chroma]}, read out of a file Pillow writes without `optimize`."""
    if not _STANDARD:
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, 'JPEG', quality=75)
        t = _spec_from_dht(buf.getvalue())
        _STANDARD.append({'dc': [t[('dc', 0)], t[('dc', 1)]], 'ac': [t[('ac', 0)], t[('ac', 1)]]})
        assert sum(_STANDARD[0]['ac'][0][0]) == 162 and sum(_STANDARD[0]['dc'][0][0]) == 12
    return _STANDARD[0]


def _limit10(spec):
    """The canonical code counter after length TAB_BITS (one past the largest code of at most that length)."""
    code = 0
    for l in range(1, TAB_BITS + 1):
        code = (code << 1) + spec[0][l]
    return code


def table_class(spec, is_dc):
    """Which of the decoder's three ways a table's LONGEST codes take (jpeg_build_tables in k_jpeg.hip): 'short' = every code
    within the first-level table (no code longer than TAB_BITS bits; for a complete table: limit10 << 6 == 65536);
    'longtab' = an AC table whose long-code windows all fit its direct table (65536 - (limit10 << 6) <= LONG_N);
    'compare' = canonical compares (an AC table with more long-code space, and every DC table with long codes)."""
    if not any(spec[0][TAB_BITS + 1:17]):
        return 'short'
    space = 65536 - (_limit10(spec) << (16 - TAB_BITS))
    assert space > 0, 'codes longer than %d bits in a table with no room for them' % TAB_BITS
    if is_dc:
        return 'compare'
    return 'longtab' if space <= LONG_N else 'compare'


def code_paths(spec, is_dc):
    """{symbol: (code, length, path)}: the canonical codes, and per symbol the decoder's path for THAT code -- the first
    LONG_N windows of an AC table's long-code space go through the direct table even when the table's class is 'compare'."""
    out = {}
    code = 0
    k = 0
    first = _limit10(spec) << (16 - TAB_BITS)
    for l in range(1, 17):
        for _ in range(spec[0][l]):
            if l <= TAB_BITS:
                path = 'short'
            else:
                off = (((code << (16 - l)) >> (16 - TAB_BITS)) << (16 - TAB_BITS)) - first
                path = 'longtab' if (not is_dc and off + (1 << (16 - TAB_BITS)) <= LONG_N) else 'compare'
            out.setdefault(spec[1][k], (code & ((1 << l) - 1), l, path))
            code += 1
            k += 1
        code <<= 1
    return out


# ------------------------------------------------------------------ the writer ----
LAYOUT = dict(sof=0xC0,          # 0xC0 baseline, 0xC1 extended sequential
              jfif=True,         # APP0 JFIF segment
              merged=False,      # all Huffman tables in one DHT and all quantisation tables in one DQT segment
              order='QFHR',      # segment order: Q = DQT, F = SOF, H = DHT, R = DRI
              decoy=False,       # a wrong definition of every table in front of the right one (the last one wins)
              filler=(),         # any of 'com', 'app', 'app_big' (one APP5 segment of 65 533 bytes), put between the segments
              fill_ff=0,         # fill bytes (FF) in front of every header marker behind SOI
              garbage=False,     # non-FF garbage between the segments (libjpeg's next_marker steps over it)
              dri_first=None,    # a DRI segment with this value in front of the effective one
              omit=())           # tables used for coding but not written: ('dc', id), ('ac', id), ('q', id)


def _segment(marker, payload):
    assert len(payload) + 2 <= 65535
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)


def _dqt_payload(tid, table, bits16):
    zz = [int(np.asarray(table).reshape(64)[ZIGZAG[k]]) for k in range(64)]
    if bits16:
        return bytes([0x10 | tid]) + b''.join(v.to_bytes(2, 'big') for v in zz)
    assert max(zz) <= 255
    return bytes([tid]) + bytes(zz)


def _dht_payload(is_ac, tid, spec):
    return bytes([(0x10 if is_ac else 0) | tid]) + bytes(spec[0][1:17]) + bytes(spec[1])


def check_in_range(coefs, qtables, sel):
    """The condition of the module docstring on every block."""
    for (c, grid) in enumerate(coefs):
        q = np.asarray(qtables[sel[c][0]][0], np.int64).reshape(64)
        deq = grid.astype(np.int64) * q
        assert deq.min() >= -32768 and deq.max() <= 32767, 'dequantised coefficients leave int16 (component %d)' % c
        px = idct(deq.reshape(grid.shape[0], grid.shape[1], 8, 8))
        assert px.min() >= -256 and px.max() + 128 <= 511, 'inverse DCT leaves the range where libjpeg clamps plainly (component %d)' % c


def write_jpeg(coefs, size, sampling, qtables, dc, ac, sel=None, ids=None, restart=0, layout=None, eob=None, stats=None,
               check=True):
    """The bytes of a baseline JPEG file.
    coefs      per component an int16 array (blocks_y, blocks_x, 64), natural order, MCU-padded grids
    size       (H, W)
    sampling   a key of SAMPLING
    qtables    {id 0..3: (64 entries in natural order, 16-bit entries?)}
    dc, ac     {id: (bits, vals)}; nothing is validated, so that a test can write a table libjpeg refuses
    sel        per component (tq, td, ta); default luma 0 0 0, chroma 1 1 1
    ids        component ids; default 1 2 3
    restart    restart interval in MCUs (0: none); RSTn markers behind 1-bit padding
    layout     overrides of LAYOUT
    eob        symbols to use in turn where a block ends with an end of block (size-0 symbols with runs 1..14 mean the same
               to libjpeg); default 0x00
    stats      a dict that receives what the entropy coder counted: symbols, symbols per decoder path ('short', 'longtab',
               'compare'), long_symbols (codes above TAB_BITS bits), and -- for the state walker -- the clean scan bytes
               (no stuffing; only without restart markers), the bit offset of every symbol and of every block's end"""
    lay = dict(LAYOUT)
    lay.update(layout or {})
    (nc, hs, vs) = SAMPLING[sampling]
    (H, W) = size
    ((my, mx), shapes) = grid_shape(size, sampling)
    sel = list(sel) if sel else [(0, 0, 0), (1, 1, 1), (1, 1, 1)][:nc]
    ids = list(ids) if ids else [1, 2, 3][:nc]
    assert len(coefs) == nc and all(tuple(g.shape) == (s[0], s[1], 64) for (g, s) in zip(coefs, shapes)), 'grids must be MCU-padded'
    if check:
        check_in_range(coefs, qtables, sel)

    # ---- header segments ----
    groups = {'Q': [], 'F': [], 'H': [], 'R': []}
    qsegs = [_dqt_payload(t, qtables[t][0], qtables[t][1]) for t in sorted(qtables) if ('q', t) not in lay['omit']]
    hsegs = [_dht_payload(False, t, dc[t]) for t in sorted(dc) if ('dc', t) not in lay['omit']] + \
            [_dht_payload(True, t, ac[t]) for t in sorted(ac) if ('ac', t) not in lay['omit']]
    if lay['decoy']:
        # every table defined wrongly first: all-255 quantisation tables, and each Huffman id with the OTHER class's idea of
        # a code set (a flat 4-bit table), which decodes any of these files to garbage if it were to win
        flat = tables_from_lengths({4: list(range(12))})
        qsegs = [_dqt_payload(t, [255] * 64, False) for t in sorted(qtables)] + qsegs
        hsegs = [_dht_payload(False, t, flat) for t in sorted(dc)] + [_dht_payload(True, t, flat) for t in sorted(ac)] + hsegs
    if lay['merged']:
        groups['Q'] = [_segment(0xDB, b''.join(qsegs))]
        groups['H'] = [_segment(0xC4, b''.join(hsegs))]
    else:
        groups['Q'] = [_segment(0xDB, p) for p in qsegs]
        groups['H'] = [_segment(0xC4, p) for p in hsegs]
    sof = bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes([nc])
    for c in range(nc):
        (h, v) = (hs, vs) if c == 0 else (1, 1)
        sof += bytes([ids[c], (h << 4) | v, sel[c][0]])
    groups['F'] = [_segment(lay['sof'], sof)]
    if lay['dri_first'] is not None:
        groups['R'].append(_segment(0xDD, int(lay['dri_first']).to_bytes(2, 'big')))
    if restart or lay['dri_first'] is not None:
        groups['R'].append(_segment(0xDD, int(restart).to_bytes(2, 'big')))
    segs = []
    if lay['jfif']:
        segs.append(_segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'))
    fillers = {'com': _segment(0xFE, b'written from coefficient blocks'), 'app': _segment(0xE7, bytes(range(1, 200))),
               'app_big': _segment(0xE5, bytes(65533))}
    for (k, g) in enumerate(lay['order']):
        for f in lay['filler']:
            if f != 'app_big' or k == 1:
                segs.append(fillers[f])
        segs += groups[g]
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([ids[c], (sel[c][1] << 4) | sel[c][2]])
    segs.append(_segment(0xDA, sos + bytes([0, 63, 0])))
    head = bytearray(b'\xff\xd8')
    for (k, s) in enumerate(segs):
        if lay['garbage'] and k:   # not right behind SOI: Pillow identifies a JPEG file by FF D8 FF
            head += b'\x00\x12\x34\xd9\xc4'
        head += b'\xff' * lay['fill_ff'] + s

    # ---- entropy-coded segment ----
    dcc = {t: code_paths(dc[t], True) for t in dc}
    acc = {t: code_paths(ac[t], False) for t in ac}
    zz = [g.reshape(-1, 64)[:, ZIGZAG].astype(np.int64) for g in coefs]
    out = bytearray()
    clean = bytearray()
    state = {'acc': 0, 'n': 0}
    count = {'symbols': 0, 'short': 0, 'longtab': 0, 'compare': 0}
    (sym_at, blk_at) = ([], [])
    pos = [0]

    def put(code, length):
        state['acc'] = (state['acc'] << length) | code
        state['n'] += length
        pos[0] += length
        while state['n'] >= 8:
            state['n'] -= 8
            b = (state['acc'] >> state['n']) & 255
            out.append(b)
            clean.append(b)
            if b == 255:
                out.append(0)
        state['acc'] &= (1 << state['n']) - 1

    def flush():
        if state['n']:
            pad = 8 - state['n']
            put((1 << pad) - 1, pad)

    def symbol(table, s, value_bits, nbits):
        (code, length, path) = table[s]
        sym_at.append(pos[0])
        count['symbols'] += 1
        count[path] += 1
        put(code, length)
        if nbits:
            put(value_bits, nbits)

    eob = list(eob) if eob else [0x00]
    n_eob = 0
    pred = [0] * nc
    order = []   # (component, block row offset, block column offset) of an MCU's blocks
    for c in range(nc):
        (h, v) = (hs, vs) if c == 0 else (1, 1)
        order += [(c, y, x, h, v) for y in range(v) for x in range(h)]
    mcu = 0
    rst = 0
    for yy in range(my):
        for xx in range(mx):
            if restart and mcu and mcu % restart == 0:
                flush()
                out += bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) & 7
                pred = [0] * nc
            mcu += 1
            for (c, y, x, h, v) in order:
                blk = zz[c][(yy * v + y) * shapes[c][1] + xx * h + x]
                (_tq, td, ta) = sel[c]
                d = int(blk[0]) - pred[c]
                pred[c] = int(blk[0])
                s = abs(d).bit_length()
                symbol(dcc[td], s, d if d >= 0 else d + (1 << s) - 1, s)
                nz = np.flatnonzero(blk[1:]) + 1
                k = 1
                for j in nz:
                    run = int(j) - k
                    while run >= 16:
                        symbol(acc[ta], 0xF0, 0, 0)
                        run -= 16
                    a = int(blk[j])
                    s = abs(a).bit_length()
                    symbol(acc[ta], (run << 4) | s, a if a >= 0 else a + (1 << s) - 1, s)
                    k = int(j) + 1
                if k < 64:
                    symbol(acc[ta], eob[n_eob % len(eob)], 0, 0)
                    n_eob += 1
                blk_at.append(pos[0])
    flush()
    if stats is not None:
        stats.update(count)
        stats['long_symbols'] = count['longtab'] + count['compare']
        stats['sym_at'] = np.array(sym_at, np.int64)
        stats['blk_at'] = np.array(blk_at, np.int64)
        stats['scan'] = bytes(clean)
    return bytes(head) + bytes(out) + b'\xff\xd9'
