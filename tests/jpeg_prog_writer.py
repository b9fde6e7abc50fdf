"""A progressive JPEG *writer* for the decoder tests, written from ITU-T T.81 Annex G (pure Python / numpy).

Pillow writes exactly one colour scan script and one greyscale script; the scripts decoders get wrong are the others.  This module
builds on tests/jpeg_writer.py -- the same coefficient grids (one int16 array (blocks_y, blocks_x, 64) per component, natural
order, MCU-padded), `check_in_range` applied to every file, the same Huffman-spec helpers -- and takes the scan script as a
parameter: a list of (components, Ss, Se, Ah, Al).  Pillow (libjpeg-turbo) stays the reference DECODER.

What a scan visits (T.81 A.2): an interleaved scan (several components) the MCU-padded grids; a scan of one component only that
component's real blocks, ceil(ceil(W * hs / hs_max) / 8) by ceil(ceil(H * vs / vs_max) / 8), in raster order -- restart intervals
count in that order too.  Padded blocks a script never visits stay zero in a decoder: `decoded_grids` gives the grids a decoder
holds after the script (they differ from the input only in such blocks, which no pixel of the image depends on).
"""
import numpy as np

try:
    from tests import jpeg_writer as jw
except ImportError:   # run from the tests directory itself
    import jpeg_writer as jw

# the scripts libjpeg's jpeg_simple_progression writes
PILLOW_COLOUR = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                 ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
PILLOW_GREY = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


def real_blocks(size, sampling):
    """Per component (blocks_y, blocks_x) of the blocks that hold image samples."""
    (H, W) = size
    (nc, hs, vs) = jw.SAMPLING[sampling]
    out = [(-(-H // 8), -(-W // 8))]
    for _ in range(nc - 1):
        out.append((-(-(-(-H // vs)) // 8), -(-(-(-W // hs)) // 8)))
    return out


def _scan_blocks(comps, size, sampling):
    """The blocks of a scan in the order it sends them: a list of MCUs, each a list of (component, block row, block column)."""
    (nc, hs, vs) = jw.SAMPLING[sampling]
    ((my, mx), _shapes) = jw.grid_shape(size, sampling)
    if len(comps) > 1:
        out = []
        for yy in range(my):
            for xx in range(mx):
                mcu = []
                for c in comps:
                    (h, v) = (hs, vs) if c == 0 else (1, 1)
                    mcu += [(c, yy * v + y, xx * h + x) for y in range(v) for x in range(h)]
                out.append(mcu)
        return out
    c = comps[0]
    (by, bx) = real_blocks(size, sampling)[c]
    return [[(c, y, x)] for y in range(by) for x in range(bx)]


def decoded_grids(coefs, size, sampling, script):
    """The grids a decoder holds after a COMPLETE script: the input where a scan came by, zero elsewhere."""
    out = [np.zeros_like(g) for g in coefs]
    for (comps, Ss, Se, _Ah, _Al) in script:
        for mcu in _scan_blocks(comps, size, sampling):
            for (c, y, x) in mcu:
                idx = jw.ZIGZAG[Ss:Se + 1]
                out[c][y, x, idx] = coefs[c][y, x, idx]
    return out


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            pad = 8 - self.n
            self.put((1 << pad) - 1, pad)


def _scan_tokens(zz, scan, blocks, restart, tabs, stats):
    """The scan as tokens: ('s', table key, symbol), ('b', value, nbits), ('r', marker number)."""
    (comps, Ss, Se, Ah, Al) = scan
    tok = []
    pred = {c: 0 for c in comps}
    state = {'eobrun': 0, 'be': []}

    def emit_eobrun(ta):
        if state['eobrun'] > 0:
            nb = state['eobrun'].bit_length() - 1
            stats.setdefault('eob_categories', set()).add(nb)
            tok.append(('s', ('ac', ta), nb << 4))
            if nb:
                tok.append(('b', state['eobrun'] & ((1 << nb) - 1), nb))
            state['eobrun'] = 0
            tok.extend(('b', b, 1) for b in state['be'])
            state['be'] = []

    rst = 0
    for (m, mcu) in enumerate(blocks):
        if restart and m and m % restart == 0:
            if Ss > 0:
                emit_eobrun(tabs[comps[0]][1])
            tok.append(('r', rst))
            rst = (rst + 1) & 7
            pred = {c: 0 for c in comps}
        for (c, y, x) in mcu:
            blk = zz[c][y, x]
            (td, ta) = tabs[c]
            if Ss == 0:
                v = int(blk[0]) >> Al   # the point transform of DC values is an arithmetic shift
                if Ah == 0:
                    d = v - pred[c]
                    pred[c] = v
                    s = abs(d).bit_length()
                    tok.append(('s', ('dc', td), s))
                    if s:
                        tok.append(('b', d if d >= 0 else d + (1 << s) - 1, s))
                else:
                    tok.append(('b', v & 1, 1))
                continue
            if Ah == 0:   # AC first (G.1.2.2): values divided by 2^Al towards zero
                r = 0
                for k in range(Ss, Se + 1):
                    a = int(blk[k])
                    t = abs(a) >> Al
                    if t == 0:
                        r += 1
                        continue
                    emit_eobrun(ta)
                    while r > 15:
                        tok.append(('s', ('ac', ta), 0xF0))
                        stats['zrl_first'] = stats.get('zrl_first', 0) + 1
                        r -= 16
                    s = t.bit_length()
                    tok.append(('s', ('ac', ta), (r << 4) | s))
                    tok.append(('b', t if a >= 0 else (~t) & ((1 << s) - 1), s))
                    r = 0
                if r > 0:
                    state['eobrun'] += 1
                    if state['eobrun'] == 0x7FFF:
                        emit_eobrun(ta)
                continue
            # AC refinement (G.1.2.3)
            absv = [abs(int(blk[k])) >> Al for k in range(64)]
            last_new = max([k for k in range(Ss, Se + 1) if absv[k] == 1], default=-1)
            r = 0
            br = []
            for k in range(Ss, Se + 1):
                t = absv[k]
                if t == 0:
                    r += 1
                    continue
                while r > 15 and k <= last_new:
                    emit_eobrun(ta)
                    tok.append(('s', ('ac', ta), 0xF0))
                    stats['zrl_refine'] = stats.get('zrl_refine', 0) + 1
                    if br:
                        stats['zrl_over_history'] = stats.get('zrl_over_history', 0) + 1
                    r -= 16
                    tok.extend(('b', b, 1) for b in br)
                    br = []
                if t > 1:   # a coefficient with history: its correction bit waits for the symbol that passes it
                    br.append(t & 1)
                    continue
                emit_eobrun(ta)
                tok.append(('s', ('ac', ta), (r << 4) | 1))
                if r == 15:
                    stats['new_after_15'] = stats.get('new_after_15', 0) + 1
                tok.append(('b', 0 if int(blk[k]) < 0 else 1, 1))
                tok.extend(('b', b, 1) for b in br)
                br = []
                r = 0
            if r > 0 or br:
                state['eobrun'] += 1
                state['be'] += br
                if state['eobrun'] == 0x7FFF:
                    emit_eobrun(ta)
    if Ss > 0:
        emit_eobrun(tabs[comps[0]][1])
    return tok


def write_progressive(coefs, size, sampling, qtables, script, sel=None, ids=None, tabsel=None, specs=None, restart=0, sof=0xC2,
                      dqt_after_first_sos=False, check=True, stats=None):
    """The bytes of a progressive JPEG file.
    coefs, size, sampling, qtables, ids   as jpeg_writer.write_jpeg
    script     [(components, Ss, Se, Ah, Al)]: components a tuple of component indices; nothing is validated, so that a test can
               write a script a decoder must refuse (its entropy-coded data then mean nothing)
    sel        per component the quantisation table id; default luma 0, chroma 1
    tabsel     per scan {component: (DC table id, AC table id)} (ids 0..3); default luma (0, 0), chroma (1, 1)
    specs      per scan {('dc' | 'ac', id): (bits, vals)}; a table that is not given is the optimal one for the scan's symbols
               (T.81 K.2), so every scan redefines the ids it uses
    restart    restart interval in MCUs of each scan (single blocks in a scan of one component), or a list with one per scan
               (a DRI segment is written in front of a scan whenever the value changes)
    stats      a dict that receives 'eob_categories' (the set of EOBn categories written), 'zrl_first', 'zrl_refine',
               'zrl_over_history' (ZRL symbols that pass coefficients with history), 'new_after_15', 'specs' (per scan)"""
    (nc, hs, vs) = jw.SAMPLING[sampling]
    (H, W) = size
    (_m, shapes) = jw.grid_shape(size, sampling)
    sel = list(sel) if sel else [0, 1, 1][:nc]
    ids = list(ids) if ids else [1, 2, 3][:nc]
    stats = stats if stats is not None else {}
    assert len(coefs) == nc and all(tuple(g.shape) == (s[0], s[1], 64) for (g, s) in zip(coefs, shapes)), 'grids must be MCU-padded'
    if check:
        jw.check_in_range(coefs, qtables, [(q, 0, 0) for q in sel])
    head = bytearray(b'\xff\xd8')
    head += jw._segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in sorted(qtables):
        head += jw._segment(0xDB, jw._dqt_payload(t, qtables[t][0], qtables[t][1]))
    f = bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes([nc])
    for c in range(nc):
        (h, v) = (hs, vs) if c == 0 else (1, 1)
        f += bytes([ids[c], (h << 4) | v, sel[c]])
    head += jw._segment(sof, f)
    zz = [g[:, :, jw.ZIGZAG].astype(np.int64) for g in coefs]
    out = bytearray(head)
    dri = 0
    stats['specs'] = []
    for (si, scan) in enumerate(script):
        (comps, Ss, Se, Ah, Al) = scan
        tabs = {c: ((0, 0) if c == 0 else (1, 1)) for c in comps}
        if tabsel and tabsel[si]:
            tabs.update(tabsel[si])
        ri = restart[si] if isinstance(restart, (list, tuple)) else restart
        blocks = _scan_blocks(comps, size, sampling)
        tok = _scan_tokens(zz, (comps, Ss, min(Se, 63), Ah, Al), blocks, ri, tabs, stats)
        freq = {}
        for t in tok:
            if t[0] == 's':
                freq.setdefault(t[1], {})
                freq[t[1]][t[2]] = freq[t[1]].get(t[2], 0) + 1
        given = (specs[si] if specs and specs[si] else {})
        table = {}
        for key in sorted(freq):
            table[key] = given[key] if key in given else jw.length_limited_tables(freq[key])
            out += jw._segment(0xC4, jw._dht_payload(key[0] == 'ac', key[1], table[key]))
        stats['specs'].append(table)
        if ri != dri:
            out += jw._segment(0xDD, int(ri).to_bytes(2, 'big'))
            dri = ri
        if dqt_after_first_sos and si == 1:
            t0 = sorted(qtables)[0]
            out += jw._segment(0xDB, jw._dqt_payload(t0, qtables[t0][0], qtables[t0][1]))
        sos = bytes([len(comps)])
        for c in comps:
            sos += bytes([ids[c], (tabs[c][0] << 4) | tabs[c][1]])
        out += jw._segment(0xDA, sos + bytes([Ss, Se, (Ah << 4) | Al]))
        codes = {key: jw.code_paths(table[key], key[0] == 'dc') for key in table}
        bits = _Bits()
        for t in tok:
            if t[0] == 's':
                (code, length, _path) = codes[t[1]][t[2]]
                bits.put(code, length)
            elif t[0] == 'b':
                bits.put(t[1], t[2])
            else:
                bits.flush()
                bits.out += bytes([0xFF, 0xD0 + t[1]])
        bits.flush()
        out += bits.out
    return bytes(out) + b'\xff\xd9'
