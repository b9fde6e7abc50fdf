"""The GPU JPEG decoder on streams no encoder at hand writes (tests/jpeg_writer.py builds them from coefficient blocks):
Huffman tables of every class the kernel's table build distinguishes, table selectors in all combinations, header layouts,
restart intervals with custom tables, streams that do not self-synchronise, and files libjpeg refuses.  The reference is
Pillow's (libjpeg-turbo's) decode of the same bytes; the bar is every byte equal, or a status and a zero frame.

The CPU half validates the generator against the reference, so that a mismatch on the GPU can only be the decoder's:
a file written "plainly" (Annex K tables, selectors 0 / 1 / 1, one segment per table, no restarts) from the same coefficients
decodes in Pillow to the same bytes as every case file; the table classes the cases claim are the ones `table_class` derives
by jpeg_build_tables' rule (whose constants are read out of k_jpeg.hip); the long-code paths are actually walked; the header
probe agrees with Pillow about every file."""
import functools
import io
import os
import re

import numpy as np
import pytest

from tests import jpeg_writer as jw
from tests.test_jpeg import _natural_image, _pillow_bgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SIZES = {'420': [(40, 56), (72, 104), (37, 51)], '422': [(40, 56), (37, 51)], '444': [(40, 56), (37, 51)], 'grey': [(40, 56), (37, 51)]}
AC_ALL = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]   # the 162 AC symbols of 8-bit baseline


def _pillow_or_none(data):
    try:
        return _pillow_bgr(data)
    except Exception:   # libjpeg's refusal arrives as OSError / SyntaxError depending on where Pillow meets it
        return None


def _q(step, base=2):
    (i, j) = np.mgrid[0:8, 0:8]
    return np.minimum(base + step * (i + j), 255).reshape(64).tolist()


def _ac_freq(sym):
    (r, s) = (sym >> 4, sym & 15)
    return 4000.0 if sym == 0 else 20.0 if sym == 0xF0 else 3000.0 / ((1 + r) ** 2 * s ** 2)


# ------------------------------------------------------------------ the tables of the classes ----
@functools.lru_cache(None)
def _tables():
    std = jw.standard_tables()
    rare_first = sorted(AC_ALL, key=_ac_freq)
    t = {}
    t['a'] = dict(dc=jw.length_limited_tables({c: 100.0 / (1 + abs(c - 4)) for c in range(12)}, 10),
                  ac=jw.length_limited_tables({s: _ac_freq(s) for s in AC_ALL}, 10), dc_class='short', ac_class='short')
    t['b'] = dict(dc=std['dc'][0], ac=std['ac'][0], dc_class='short', ac_class='longtab', walked='longtab')
    # (c) two rare symbols on 1 and 2 bits, everything else on 12-bit codes behind the prefix 11: 16 384 windows of long-code
    # space; the 32 rarest of them fall into the direct table's 512 windows, the frequent ones take the compares
    t['c'] = dict(dc=std['dc'][0], ac=jw.tables_from_lengths({1: [rare_first[0]], 2: [rare_first[1]], 12: rare_first[2:]}),
                  dc_class='short', ac_class='compare', walked='compare')
    # (d) the DC categories a smooth image uses (0..3) on 13..16 bits
    t['d'] = dict(dc=jw.tables_from_lengths({1: [11], 2: [10], 3: [9], 11: [8], 12: [7, 6], 13: [5, 4], 14: [3], 15: [2], 16: [1, 0]}),
                  ac=std['ac'][0], dc_class='compare', ac_class='longtab', walked='compare', smooth=True)
    # (e) the only long codes are 16 bits: end of block and 0x01 (AC), categories 0..3 (DC)
    rest = [s for s in AC_ALL if s not in (0x00, 0x01)]
    (b9, v9) = jw.length_limited_tables({s: _ac_freq(s) for s in rest}, 9)
    b9[16] = 2
    t['e'] = dict(dc=jw.tables_from_lengths({2: [5, 6, 7], 3: [4], 4: [8], 5: [9], 6: [10], 7: [11], 16: [0, 1, 2, 3]}),
                  ac=(b9, v9 + [0x00, 0x01]), dc_class='compare', ac_class='longtab', walked='long')
    t['f'] = dict(dc=jw.tables_from_lengths({4: list(range(12))}), ac=jw.tables_from_lengths({8: AC_ALL}), dc_class='short', ac_class='short')
    return t


def _sparse_blocks(rng, shapes, choices, fill=0.5, span=12, dc=None):
    """Coefficient grids with a DC of `dc` (or a slow ramp) and AC values drawn from `choices` at zig-zag positions 1..span."""
    out = []
    for (by, bx) in shapes:
        zz = np.zeros((by, bx, 64), np.int16)
        zz[..., 1:1 + span] = rng.choice(choices, (by, bx, span)) * (rng.random((by, bx, span)) < fill)
        zz[..., 0] = dc if dc is not None else (np.arange(by)[:, None] * 3 + np.arange(bx)[None, :] * 5) % 40 - 20
        g = np.zeros_like(zz)
        g[..., jw.ZIGZAG] = zz
        out.append(g)
    return out


def _symbol_blocks(rng, shapes, symbols, nmax, dc=0):
    """Coefficient grids whose blocks hold up to nmax AC symbols drawn from `symbols` (run << 4 | size), values of either sign
    anywhere in the size's category."""
    out = []
    for (by, bx) in shapes:
        zz = np.zeros((by * bx, 64), np.int16)
        zz[:, 0] = dc
        for n in range(by * bx):
            k = 1
            for sym in rng.choice(symbols, int(rng.integers(0, nmax + 1))):
                (r, s) = (int(sym) >> 4, int(sym) & 15)
                if k + r > 63:
                    break
                k += r
                zz[n, k] = int(rng.integers(1 << (s - 1), 1 << s)) * (1 if rng.random() < 0.5 else -1)
                k += 1
        g = np.zeros_like(zz)
        g[:, jw.ZIGZAG] = zz
        out.append(g.reshape(by, bx, 64))
    return out


class Case:
    def __init__(self, group, name, size, sampling, coefs, q, dc, ac, claims=(), walked=None, plain=True, **kw):
        self.group, self.name, self.size, self.sampling, self.claims, self.walked = group, name, size, sampling, claims, walked
        self.stats = {}
        self.dc, self.ac, self.sel, self.restart = dc, ac, kw.get('sel'), kw.get('restart', 0)
        self.q0 = q[(kw.get('sel') or [(0, 0, 0)])[0][0]][0]
        self.data = jw.write_jpeg(coefs, size, sampling, q, dc, ac, stats=self.stats, **kw)
        self.plain = None
        if plain:   # the same coefficients, the quantisation tables numbered by component, everything else as Pillow writes it
            nc = len(coefs)
            sel = kw.get('sel') or [(0, 0, 0), (1, 1, 1), (1, 1, 1)][:nc]
            pq = {c: (q[sel[c][0]][0], max(q[sel[c][0]][0]) > 255) for c in range(nc)}
            std = jw.standard_tables()
            self.plain = jw.write_jpeg(coefs, size, sampling, pq, {0: std['dc'][0], 1: std['dc'][1]}, {0: std['ac'][0], 1: std['ac'][1]},
                                       sel=[(c, min(c, 1), min(c, 1)) for c in range(nc)])

    def __repr__(self):
        return '%s/%s' % (self.group, self.name)


def _image_coefs(rng, size, sampling, qs, smooth=False, noise=False):
    (H, W) = size
    if smooth:
        (yy, xx) = np.mgrid[0:H, 0:W]
        img = np.clip(np.dstack([100 + xx * 0.6 + yy * 0.3, 90 + yy * 0.5, 140 - xx * 0.4]), 0, 255).astype(np.uint8)
    elif noise:
        img = rng.integers(96, 160, (H, W, 3), dtype=np.uint8)
    else:
        img = _natural_image(rng, H, W)
    nc = jw.SAMPLING[sampling][0]
    return jw.coefficients_from_image(img[..., 1] if nc == 1 else img, sampling, qs[:nc])


@functools.lru_cache(None)
def _class_cases():
    rng = np.random.default_rng(2026)
    std = jw.standard_tables()
    T = _tables()
    out = []
    k = 0
    for sampling in ('grey', '444', '422', '420'):
        for (name, t) in T.items():
            size = SIZES[sampling][k % len(SIZES[sampling])]
            k += 1
            (ql, qc) = (_q(12, 24), _q(16, 30)) if t.get('smooth') else (_q(1), _q(2)) if name == 'b' else (_q(3), _q(5))
            if name == 'b':   # Annex K gives the frequent symbols the short codes: content made of the symbols it puts on long ones
                paths = [jw.code_paths(std['ac'][i], False) for i in (0, 1)]
                long_syms = [s for s in AC_ALL if 1 <= (s & 15) <= 5 and (s >> 4) <= 6 and all(p[s][2] == 'longtab' for p in paths)]
                assert len(long_syms) >= 10
                (ql, qc) = ([1] * 64, [1] * 64)
                coefs = _symbol_blocks(rng, jw.grid_shape(size, sampling)[1], long_syms + [0x01, 0x02], 9, dc=5)
            else:
                coefs = _image_coefs(rng, size, sampling, [ql, qc, qc], smooth=t.get('smooth', False))
            chroma = dict(t) if name != 'b' else dict(dc=std['dc'][1], ac=std['ac'][1])
            claims = [(t['dc'], True, t['dc_class']), (t['ac'], False, t['ac_class'])]
            out.append(Case('class', '%s-%s' % (name, sampling), size, sampling, coefs, {0: (ql, False), 1: (qc, False)},
                            {0: t['dc'], 1: chroma['dc']}, {0: t['ac'], 1: chroma['ac']}, claims=claims, walked=t.get('walked')))
        # crafted content for the tables that hold only the symbols used
        size = SIZES[sampling][k % len(SIZES[sampling])]
        k += 1
        shapes = jw.grid_shape(size, sampling)[1]
        ones = {0: ([1] * 64, False), 1: ([1] * 64, False)}
        one_dc = jw.tables_from_lengths({1: [0]})
        # (b') 'longtab' with the frequent symbols ON the long codes: nine rare symbols on a unary chain of 1..9 bits, the seven
        # symbols the content uses on 12-bit codes in the 128 windows behind the prefix 1^9
        lt = jw.tables_from_lengths(dict([(l, [0xFA - 16 * l]) for l in range(1, 10)] + [(12, [0x00, 0x01, 0x02, 0x03, 0x11, 0x12, 0x21])]))
        out.append(Case('class', 'longtab-%s' % sampling, size, sampling, _symbol_blocks(rng, shapes, [0x01, 0x01, 0x02, 0x03, 0x11, 0x12, 0x21], 10), ones,
                        {0: std['dc'][0], 1: std['dc'][1]}, {0: lt, 1: lt}, claims=[(lt, False, 'longtab')], walked='longtab'))
        # (g) a DC table with a single 1-bit code, an AC table with end of block and the two symbols used
        g_ac = jw.tables_from_lengths({1: [0x00], 2: [0x01], 3: [0x12]})
        zz = _symbol_blocks(rng, shapes, [0x01, 0x01, 0x12], 5)
        out.append(Case('class', 'g-%s' % sampling, size, sampling, zz, ones, {0: one_dc, 1: one_dc}, {0: g_ac, 1: g_ac},
                        claims=[(one_dc, True, 'short'), (g_ac, False, 'short')]))
        # (h) 1-bit DC code + 1-bit end of block: a block is two bits, five blocks sit in one window entry
        h_ac = jw.tables_from_lengths({1: [0x00]})
        flat = [np.zeros((s[0], s[1], 64), np.int16) for s in shapes]
        out.append(Case('class', 'h-%s' % sampling, size, sampling, flat, ones, {0: one_dc, 1: one_dc}, {0: h_ac, 1: h_ac}))
        # (i) a first symbol of 3 bits (0x01 on a 2-bit code) followed by a 7-bit code (ends at bit 10 of the window: taken as
        # the entry's second symbol) or by an 8-bit code (would end at bit 11: not taken)
        i_ac = jw.tables_from_lengths({2: [0x01], 3: [0x00], 5: [0x21], 7: [0x02], 8: [0x03], 9: [0xF0]})
        zz = _symbol_blocks(rng, shapes, [0x01, 0x01, 0x01, 0x21, 0x02, 0x03], 14, dc=3)
        out.append(Case('class', 'i-%s' % sampling, size, sampling, zz, ones, {0: std['dc'][0], 1: std['dc'][1]}, {0: i_ac, 1: i_ac},
                        claims=[(i_ac, False, 'short')]))
    return out


@functools.lru_cache(None)
def _symbol_cases():
    std = jw.standard_tables()
    ones = {0: ([1] * 64, False)}
    (dc, ac) = ({0: std['dc'][0]}, {0: std['ac'][0]})
    out = []
    size = (96, 128)
    (by, bx) = jw.grid_shape(size, 'grey')[1][0]
    # DC differences at both ends of every category, both signs: the DC values run 0, v, 0, -v ... ; category 11 needs the
    # black / white alternation (-1024 <-> 1016: +-2040, the largest difference 8-bit samples give, and -1024 <-> 0: +-1024)
    seq = []
    for s in range(1, 11):
        for v in ((1 << s) - 1, 1 << (s - 1)):
            seq += [min(v, 1016), 0, -v, 0]
    seq += [-1024, 1016, -1024, 1016, 0, -1024, 0]
    g = np.zeros((by * bx, 64), np.int16)
    g[:len(seq), 0] = seq
    # AC values at both ends of every category 1..10, both signs, on a zero DC
    vals = [sg * v for s in range(1, 11) for v in ((1 << s) - 1, 1 << (s - 1)) for sg in (1, -1)]
    g[len(seq):len(seq) + len(vals), 1] = vals
    g[len(seq) + len(vals):len(seq) + 2 * len(vals), 8] = vals
    assert len(seq) + 2 * len(vals) <= by * bx
    out.append(Case('symbols', 'categories', size, 'grey', [g.reshape(by, bx, 64)], ones, dc, ac))
    # runs: a last coefficient at zig-zag 63 (no end of block behind it), one / two / three ZRLs in a row, a run that ends at 63
    zz = np.zeros((by * bx, 64), np.int16)
    for (n, (first, second)) in enumerate([(10, 63), (0, 63), (62, 63), (5, 25), (5, 40), (5, 56), (0, 17), (0, 33), (0, 49), (46, 63),
                                           (30, 63), (14, 63), (1, 62)] * 4):
        if first:
            zz[n, first] = 3 - (n % 7)
            zz[n, first] = zz[n, first] or 2
        zz[n, second] = -5 + (n % 3)
        zz[n, 0] = n % 9 - 4
    g = np.zeros_like(zz)
    g[:, jw.ZIGZAG] = zz
    out.append(Case('symbols', 'runs', size, 'grey', [g.reshape(by, bx, 64)], ones, dc, ac))
    # size-0 symbols with runs 1..14 for the end of block (libjpeg: any size-0 symbol but ZRL ends the block)
    alias = [r << 4 for r in range(1, 15)]
    freq = {s: _ac_freq(s) for s in AC_ALL if (s & 15) <= 4}
    freq.update({s: 50.0 for s in alias})
    a_ac = jw.length_limited_tables(freq, 16)
    rng = np.random.default_rng(4)
    coefs = _sparse_blocks(rng, [(by, bx)], [1, -1, 2, -3, 6, -9, 0, 0], 0.4, 30)
    out.append(Case('symbols', 'eob-alias', size, 'grey', coefs, ones, dc, {0: a_ac}, eob=alias + [0x00]))
    return out


@functools.lru_cache(None)
def _selector_cases():
    """All 64 combinations of (td, ta) over three components, per sampling mode; DC 0 / AC 0 = Annex K luma, DC 1 / AC 1 =
    Annex K chroma: two distinct code sets each, so that a wrong choice decodes garbage."""
    std = jw.standard_tables()
    rng = np.random.default_rng(64)
    size = (24, 40)
    q = {0: (_q(2), False), 1: (_q(3), False)}
    out = []
    for sampling in ('444', '422', '420'):
        coefs = _image_coefs(rng, size, sampling, [q[0][0], q[1][0], q[1][0]])
        for n in range(64):
            sel = [(min(c, 1), (n >> (2 * c)) & 1, (n >> (2 * c + 1)) & 1) for c in range(3)]
            out.append(Case('selectors', '%s-%02d' % (sampling, n), size, sampling, coefs, q, {0: std['dc'][0], 1: std['dc'][1]},
                            {0: std['ac'][0], 1: std['ac'][1]}, sel=sel, plain=(n == 0)))
            out[-1].plain = out[-1 - n].plain
    return out


@functools.lru_cache(None)
def _header_cases():
    std = jw.standard_tables()
    rng = np.random.default_rng(11)
    size = (40, 56)
    (dc, ac) = ({0: std['dc'][0], 1: std['dc'][1]}, {0: std['ac'][0], 1: std['ac'][1]})
    img = _natural_image(rng, *size)
    out = []

    def add(group, name, qt, sel=None, **kw):
        s = sel or [(0, 0, 0), (1, 1, 1), (1, 1, 1)]
        coefs = jw.coefficients_from_image(img, '420', [qt[s[c][0]][0] for c in range(3)])
        out.append(Case(group, name, size, '420', coefs, qt, dc, ac, sel=sel, **kw))

    q8 = {0: (_q(3), False), 1: (_q(5), False)}
    # quantisation-table selectors: ids 0..3, Cb and Cr on different tables, 16-bit entries small and large
    add('tq', 'ids-3-0-2', {3: (_q(3), False), 0: (_q(5), False), 2: (_q(7), False), 1: ([255] * 64, False)}, sel=[(3, 0, 0), (0, 1, 1), (2, 1, 1)])
    add('tq', 'all-on-2', {2: (_q(4), False)}, sel=[(2, 0, 0), (2, 1, 1), (2, 1, 1)])
    add('tq', '16bit-small', {0: (_q(3), True), 1: (_q(5), True)})
    big = (np.array(_q(3), np.int64) + (np.arange(64) // 8 + np.arange(64) % 8 >= 6) * 900).tolist()
    add('tq', '16bit-1000', {0: (big, True), 1: (_q(5), False)})
    assert max(big) > 900
    for (name, ids, lay) in (('012', (0, 1, 2), {}), ('123', (1, 2, 3), {}), ('10-20-30', (10, 20, 30), {}), ('RGB-jfif', (82, 71, 66), {'jfif': True})):
        add('ids', name, q8, ids=ids, layout=lay)
    # header layouts, each option alone and all together (a restart interval, so that DRI takes part in the ordering)
    lays = {'sof1': dict(sof=0xC1), 'no-jfif': dict(jfif=False), 'merged': dict(merged=True), 'order-HRQF': dict(order='HRQF'),
            'order-FHQR': dict(order='FHQR'), 'order-RQHF': dict(order='RQHF'), 'decoy': dict(decoy=True),
            'decoy-merged': dict(decoy=True, merged=True), 'com-app': dict(filler=('com', 'app')), 'app-big': dict(filler=('app_big',)),
            'fill-ff': dict(fill_ff=3), 'garbage': dict(garbage=True), 'dri-twice': dict(dri_first=2),
            'all': dict(sof=0xC1, jfif=False, merged=True, order='HRQF', decoy=True, filler=('com', 'app', 'app_big'), fill_ff=2, garbage=True, dri_first=2)}
    for (name, lay) in lays.items():
        add('layout', name, q8, layout=lay, restart=5)
    return out


@functools.lru_cache(None)
def _restart_cases():
    """k_jpeg_huff_rst with the custom tables: the AC 'compare' table and the long-code DC table."""
    T = _tables()
    rng = np.random.default_rng(8)
    out = []
    (dc, ac) = ({0: T['e']['dc'], 1: T['d']['dc']}, {0: T['c']['ac'], 1: T['e']['ac']})
    q = {0: (_q(3), False), 1: (_q(5), False)}
    for (sampling, size) in (('420', (40, 56)), ('444', (40, 56)), ('grey', (40, 56)), ('422', (37, 51))):
        coefs = _image_coefs(rng, size, sampling, [q[0][0], q[1][0], q[1][0]])
        ((my, mx), _s) = jw.grid_shape(size, sampling)
        # 1; intervals that do not divide the MCU count and end inside an MCU row; the MCU count itself and more (DRI set, no
        # marker in the scan); a DRI of 0 behind a non-zero one
        for (name, kw) in (('1', dict(restart=1)), ('mid-row', dict(restart=mx - 1)), ('no-divisor', dict(restart=mx + 3)), ('all', dict(restart=my * mx)),
                           ('more', dict(restart=my * mx + 7)), ('zero-after', dict(restart=0, layout=dict(dri_first=3)))):
            assert (name != 'mid-row' or kw['restart'] % mx) and (name != 'no-divisor' or (my * mx) % kw['restart'])
            nc = jw.SAMPLING[sampling][0]
            out.append(Case('restart', '%s-%s' % (sampling, name), size, sampling, coefs, {t: q[t] for t in range(min(nc, 2))},
                            {t: dc[t] for t in range(min(nc, 2))}, {t: ac[t] for t in range(min(nc, 2))}, **kw))
    return out


def _unary_under_tables(s=5):
    """The undershoot stream's code sets: AC codes 1^j 0 -- j = 0: 0x01, j = 1: run 0 / size s (the one the stream uses), j = 2:
    end of block, j >= 3: run 0 / size j - 1 (distinct symbols through the run nibble); DC: 0 -> category 0, 10 / 110 / 1110 ->
    1, 2, 3.  The true stream is (0, 10 1^s, 110) per block: short blocks; read from the wrong phase its runs of ones are long
    codes with many magnitude bits, none of which ends a block."""
    ac = {1: [0x01], 2: [s], 3: [0x00]}
    used = {0x01, s, 0x00}
    for j in range(3, 12):
        sz = min(j - 1, 9)
        (sym, r) = (sz, 0)
        while sym in used:
            r += 1
            sym = (r << 4) | sz
        used.add(sym)
        ac[j + 1] = [sym]
    return jw.tables_from_lengths({1: [0], 2: [1], 3: [2], 4: [3]}), jw.tables_from_lengths(ac)


@functools.lru_cache(None)
def _sync_cases():
    T = _tables()
    std = jw.standard_tables()
    rng = np.random.default_rng(480)
    size = (480, 640)
    shapes = jw.grid_shape(size, '420')[1]
    out = []
    q = {0: (_q(3), False), 1: (_q(5), False)}
    (sdc, sac) = ({0: std['dc'][0], 1: std['dc'][1]}, {0: std['ac'][0], 1: std['ac'][1]})
    # 1: one 16 x 16 patch tiled over the frame: every MCU the same bits (but the first: its DC difference)
    patch = _natural_image(rng, 16, 16)
    coefs = jw.coefficients_from_image(np.tile(patch, (30, 40, 1)), '420', [q[0][0], q[1][0], q[1][0]])
    out.append(Case('sync', 'periodic', size, '420', coefs, q, sdc, sac))
    # 2: fixed-length codes (8-bit AC, 4-bit DC) on noise: no code is a prefix-shifted version of another, a wrong phase stays wrong
    coefs = _image_coefs(rng, size, '420', [_q(6, 8), _q(8, 10), _q(8, 10)], noise=True)
    out.append(Case('sync', 'fixed-length', size, '420', coefs, {0: (_q(6, 8), False), 1: (_q(8, 10), False)},
                    {0: T['f']['dc'], 1: T['f']['dc']}, {0: T['f']['ac'], 1: T['f']['ac']}))
    ones = {0: ([1] * 64, False), 1: ([1] * 64, False)}
    # 3: overshoot.  1-bit end of block and 1-bit DC category 0; four AC values of -(2^5 - 1) per block, whose magnitude bits
    # are zeros: a walk from the wrong phase reads every pair of zeros as a whole block
    over = []
    for (by, bx) in shapes:
        zz = np.zeros((by, bx, 64), np.int16)
        zz[..., 1:5] = -31
        g = np.zeros_like(zz)
        g[..., jw.ZIGZAG] = zz
        over.append(g)
    o_dc = jw.tables_from_lengths({1: [0], 2: [2], 3: [1]})
    o_ac = jw.tables_from_lengths({1: [0x00], 2: [0x05], 3: [0x01]})
    out.append(Case('sync', 'overshoot', size, '420', over, ones, {0: o_dc, 1: o_dc}, {0: o_ac, 1: o_ac}))
    # 4: undershoot (see _unary_under_tables): one AC value of 2^5 - 1 per block
    under = []
    for (by, bx) in shapes:
        zz = np.zeros((by, bx, 64), np.int16)
        zz[..., 1] = 31
        g = np.zeros_like(zz)
        g[..., jw.ZIGZAG] = zz
        under.append(g)
    (u_dc, u_ac) = _unary_under_tables()
    out.append(Case('sync', 'undershoot', size, '420', under, ones, {0: u_dc, 1: u_dc}, {0: u_ac, 1: u_ac}))
    return out


@functools.lru_cache(None)
def _refusal_cases():
    std = jw.standard_tables()
    size = (40, 56)
    out = []
    ones = {0: ([1] * 64, False), 1: ([1] * 64, False)}
    (sdc, sac) = ({0: std['dc'][0], 1: std['dc'][1]}, {0: std['ac'][0], 1: std['ac'][1]})

    def flat(sampling):
        return [np.zeros((s[0], s[1], 64), np.int16) for s in jw.grid_shape(size, sampling)[1]]

    def add(name, sampling='420', dc=sdc, ac=sac, **kw):
        out.append(Case('refusal', name, size, sampling, flat(sampling), ones, dc, ac, plain=False, **kw))

    add('over-subscribed', ac={0: jw.tables_from_lengths({1: [0x00], 2: [0x01, 0x02, 0x03]}), 1: std['ac'][1]})
    add('all-ones-code', ac={0: jw.tables_from_lengths({1: [0x00], 2: [0x01], 3: [0x02, 0x03]}), 1: std['ac'][1]})
    add('all-ones-code-dc', dc={0: jw.tables_from_lengths({1: [0], 2: [1], 2 + 1: [2, 3]}), 1: std['dc'][1]})
    add('dc-symbol-16', dc={0: jw.tables_from_lengths({1: [0], 2: [1], 3: [16]}), 1: std['dc'][1]})
    add('missing-ac-1', layout=dict(omit=(('ac', 1),)))
    add('missing-dc-0', layout=dict(omit=(('dc', 0),)))
    add('missing-dqt-1', layout=dict(omit=(('q', 1),)))
    add('bad-table-unused', dc={0: std['dc'][0], 1: std['dc'][0]}, ac={0: std['ac'][0], 1: jw.tables_from_lengths({1: [0x00, 0x01, 0x02]})},
        sel=[(0, 0, 0), (1, 1, 0), (1, 1, 0)])   # the over-subscribed table is defined, no component refers to it
    add('4:4:0', sampling='440')
    add('4:1:1', sampling='411')
    return out


def _equality_cases():
    return _class_cases() + _symbol_cases() + _selector_cases() + _header_cases() + _restart_cases() + _sync_cases()


# ------------------------------------------------------------------ CPU: the generator against the reference ----
def test_table_build_constants_are_the_ones_the_classes_assume():
    src = open(os.path.join(ROOT, 'meterelf_amd', 'csrc', 'k_jpeg.hip')).read()
    assert int(re.search(r'constexpr\s+int\s+TAB_BITS\s*=\s*(\d+)\s*;', src).group(1)) == 10 == jw.TAB_BITS
    assert int(re.search(r'constexpr\s+int\s+LONG_N\s*=\s*(\d+)\s*;', src).group(1)) == 512 == jw.LONG_N


def test_table_helpers():
    std = jw.standard_tables()
    assert jw.table_class(std['dc'][0], True) == 'short' and jw.table_class(std['dc'][1], True) == 'compare'
    assert jw.table_class(std['ac'][0], False) == 'longtab' and jw.table_class(std['ac'][1], False) == 'longtab'
    assert list(jw.ZIGZAG[:10]) == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and sorted(jw.ZIGZAG) == list(range(64))
    for max_len in (8, 10, 16):
        (bits, vals) = jw.length_limited_tables({s: _ac_freq(s) for s in AC_ALL}, max_len)
        assert sorted(vals) == sorted(AC_ALL) and not any(bits[max_len + 1:])
        assert sum(b * 2 ** (16 - l) for (l, b) in enumerate(bits) if l) < 65536   # the all-ones code stays free
        codes = jw.code_paths((bits, vals), False)
        assert codes[0x00][1] <= codes[0xFA][1]
    x = np.random.default_rng(1).normal(0, 50, (5, 8, 8))
    assert np.allclose(jw.idct(jw.fdct(x)), x) and np.isclose(jw.fdct(np.full((8, 8), 10.0))[0, 0], 80.0)


def test_greyscale_files_decode_like_a_float_idct():
    """Pillow's decode of a greyscale file differs from clip(round(float64 IDCT) + 128) by at most 1 per sample: the IEEE 1180
    peak-error bound a conforming inverse DCT meets.  Proves coefficient order, quantisation tables and entropy coding."""
    n = 0
    for case in _class_cases() + _symbol_cases() + _restart_cases():
        if case.sampling != 'grey':
            continue
        (H, W) = case.size
        got = _pillow_bgr(case.data)[..., 0].astype(np.int64)
        # the coefficients back out of the plain file's own arguments: decode what was written
        ref = _float_decode(case)
        assert np.abs(got - ref[:H, :W]).max() <= 1, case
        n += 1
    assert n >= 10


def _float_decode(case):
    """clip(round(IDCT(coefficients * table)) + 128) of a greyscale case, from the scan itself (a plain sequential decoder)."""
    (bits, dct, act) = (_scan_bits(case), _decoder(case.dc[0]), _decoder(case.ac[0]))
    (by, bx) = jw.grid_shape(case.size, 'grey')[1][0]
    zz = np.zeros((by * bx, 64), np.int64)
    (p, pred) = (0, 0)
    restart = case.restart

    def receive(p, n):
        v = 0
        for b in bits[p:p + n]:
            v = (v << 1) | b
        return v - (1 << n) + 1 if n and v < (1 << (n - 1)) else v

    for n in range(by * bx):
        if restart and n and n % restart == 0:
            p = (p + 7) // 8 * 8
            pred = 0
        (sym, l) = _next_code(bits, p, dct)
        pred += receive(p + l, sym)
        p += l + sym
        zz[n, 0] = pred
        k = 1
        while k < 64:
            (sym, l) = _next_code(bits, p, act)
            (r, s) = (sym >> 4, sym & 15)
            if s == 0:
                p += l
                if r != 15:
                    break
                k += 16
                continue
            k += r
            zz[n, k] = receive(p + l, s)
            p += l + s
            k += 1
    nat = np.zeros_like(zz)
    nat[:, jw.ZIGZAG] = zz
    q = np.array(case.q0, np.int64)
    px = jw.idct((nat * q).reshape(by, bx, 8, 8))
    return np.clip(np.rint(px) + 128, 0, 255).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8).astype(np.int64)


def _decoder(spec):
    return {(l, c): s for (s, (c, l, _p)) in jw.code_paths(spec, False).items()}


def _next_code(bits, p, tab):
    code = 0
    for l in range(1, 17):
        code = (code << 1) | (bits[p + l - 1] if p + l - 1 < len(bits) else 0)
        if (l, code) in tab:
            return tab[(l, code)], l
    return None, 16


def _scan_bits(case):
    return np.unpackbits(np.frombuffer(case.stats['scan'], np.uint8)).tolist()


def test_entropy_coding_and_layout_do_not_change_pixels():
    """Every case file of the GPU tests decodes in Pillow to the bytes of the plain file with the same coefficients."""
    ref = {}
    for case in _equality_cases():
        if id(case.plain) not in ref:
            ref[id(case.plain)] = _pillow_bgr(case.plain)
        got = _pillow_bgr(case.data)
        assert got.shape[:2] == case.size and np.array_equal(got, ref[id(case.plain)]), case


def test_cases_have_the_table_classes_they_claim():
    n = {'short': 0, 'longtab': 0, 'compare': 0}
    for case in _equality_cases():
        for (spec, is_dc, cls) in case.claims:
            assert jw.table_class(spec, is_dc) == cls, (case, is_dc, cls)
            n[cls] += 1
    assert min(n.values()) >= 8, n


def test_long_code_paths_are_actually_walked():
    """At least a quarter of the symbols of the 'compare' and 'longtab' cases use codes longer than 10 bits -- on the very path the
    case is named for (Annex K puts the frequent symbols on short codes: its cases are made of the symbols it puts on long ones)."""
    seen = set()
    for case in _class_cases():
        st = case.stats
        if case.walked:
            walked = st['long_symbols'] if case.walked == 'long' else st[case.walked]
            assert 4 * walked >= st['symbols'], (case, walked, st['symbols'])
            seen.add(case.walked)
    assert seen == {'compare', 'longtab', 'long'}


def test_probe_agrees_with_pillow_on_every_case_file():
    from meterelf_amd import _hip
    for case in _equality_cases():
        (H, W, ok, why) = _hip.jpeg_probe(case.data)
        assert ok and (H, W) == case.size, (case, why)
    verdicts = {}
    for case in _refusal_cases():
        (H, W, ok, why) = _hip.jpeg_probe(case.data)
        ref = _pillow_or_none(case.data)
        verdicts[case.name] = (ref is not None, ok)
        if ref is None:
            assert not ok and why, case        # Pillow raises: the probe must not say "supported"
        else:
            assert ok or why, case             # Pillow decodes: supported, or refused with a reason
    # what libjpeg does with each, pinned so that a change of the reference shows here first.  A missing Huffman table is not an
    # error to libjpeg-turbo: it installs the Annex K tables (Motion JPEG frames come without); the parser refuses such a file
    # with a reason, i.e. hands it to the host decoder
    assert verdicts == {'over-subscribed': (False, False), 'all-ones-code': (False, False), 'all-ones-code-dc': (False, False),
                        'dc-symbol-16': (False, False), 'missing-ac-1': (True, False), 'missing-dc-0': (True, False),
                        'missing-dqt-1': (False, False), 'bad-table-unused': (True, True), '4:4:0': (True, False), '4:1:1': (True, False)}, verdicts


def _walk_blocks(bits, start, span, dct, act, bpm=6, luma=4):
    """Blocks a state-only decoder completes in `span` bits from (block 0, DC next) at bit `start`; an impossible code counts as
    a 16-bit end of block / zero DC difference, like the kernel's."""
    (p, blk, k, nb) = (start, 0, 0, 0)
    while p < min(start + span, len(bits)):
        t = 0 if blk < luma else 1
        (sym, l) = _next_code(bits, p, dct[t] if k == 0 else act[t])
        sym = 0 if sym is None else sym
        p += l + (sym & 15)
        if k == 0:
            k = 1
        else:
            k += (sym >> 4) + 1 if sym & 15 else (16 if sym == 0xF0 else 64)
        if k >= 64:
            (k, nb, blk) = (0, nb + 1, (blk + 1) % bpm)
    return nb


def _phase_ratio(case):
    bits = _scan_bits(case)
    span = len(bits) // 512    # the usual lane count of k_jpeg_huff
    (dct, act) = ([_decoder(case.dc[0]), _decoder(case.dc[1])], [_decoder(case.ac[0]), _decoder(case.ac[1])])
    boundaries = set(case.stats['sym_at'].tolist())
    rng = np.random.default_rng(200)
    ratios = []
    while len(ratios) < 200:
        o = int(rng.integers(0, len(bits) - span))
        if o in boundaries:
            continue
        true = int(np.searchsorted(case.stats['blk_at'], o + span, 'right') - np.searchsorted(case.stats['blk_at'], o, 'right'))
        assert true >= 4
        ratios.append(_walk_blocks(bits, o, span, dct, act) / true)
    return float(np.median(ratios))


def test_overshoot_and_undershoot_streams_break_the_block_count_estimate():
    """Conditions on the inputs of the synchronisation tests: from 200 random bit offsets that are no symbol boundaries, a
    state-only walk over scan_bits / 512 bits counts at least 3 x the true number of blocks of that span (overshoot: median) and
    at most a third of it (undershoot)."""
    by_name = {c.name: c for c in _sync_cases()}
    over = _phase_ratio(by_name['overshoot'])
    under = _phase_ratio(by_name['undershoot'])
    print('median walked / true block counts: overshoot %.2f, undershoot %.2f' % (over, under))
    assert over >= 3.0 and under <= 1.0 / 3.0


# ------------------------------------------------------------------ GPU ----
@pytest.fixture(scope='module')
def ctx():
    from meterelf_amd import MeterReader, _hip, _params
    if _hip.device_count() < 1:
        pytest.fail('GPU tests need an MI355X: no HIP device visible (no CPU fallback exists)')
    reader = MeterReader(_params.load(os.path.join(GOLDEN, 'sample-images1', 'params.yml')))
    yield reader.ctx
    reader.close()


def _assert_equal_to_pillow(ctx, cases):
    by_size = {}
    for case in cases:
        by_size.setdefault(case.size, []).append(case)
    refs = {}
    for ((H, W), group) in by_size.items():
        (frames, status) = ctx.jpeg_decode([c.data for c in group], H, W)
        for (case, got, st) in zip(group, frames, status):
            key = id(case.plain) if case.plain is not None else id(case)
            if key not in refs:
                refs[key] = _pillow_bgr(case.data)   # the CPU test above: equal to the plain file's for every case
            ref = refs[key]
            assert st == 0, (case, int(st))
            assert np.array_equal(got, ref), (case, int((got != ref).sum()), np.argwhere(got != ref)[:3])


@pytest.mark.gpu
def test_table_classes(ctx):
    """(a) all codes <= 10 bits, (b) Annex K, (b') 'longtab' with the frequent symbols on the long codes, (c) AC 'compare', (d)
    long DC codes, (e) only 16-bit long codes, (f) fixed-length codes, (g) minimal tables, (h) two-bit blocks, (i) second
    symbols that end at bits 10 and 11 of the window -- greyscale, 4:4:4, 4:2:2, 4:2:0, sizes off the MCU grid included."""
    cases = _class_cases()
    assert len(cases) == 40 and {c.size for c in cases} == {(40, 56), (72, 104), (37, 51)}
    _assert_equal_to_pillow(ctx, cases)


@pytest.mark.gpu
def test_symbols(ctx):
    """DC category 11 and AC category 10, both signs at both ends of every category; a last coefficient at index 63 with no
    end of block behind it; one, two and three ZRLs in a row; size-0 symbols with runs 1..14 as end of block.  Pillow reads
    all of them (test_entropy_coding_and_layout_do_not_change_pixels): none had to be dropped."""
    _assert_equal_to_pillow(ctx, _symbol_cases())


@pytest.mark.gpu
@pytest.mark.parametrize('sampling', ['444', '422', '420'])
def test_selectors_all_64_combinations(ctx, sampling):
    cases = [c for c in _selector_cases() if c.sampling == sampling]
    assert len(cases) == 64 and len({tuple(c.sel) for c in cases}) == 64
    _assert_equal_to_pillow(ctx, cases)


@pytest.mark.gpu
def test_quantisation_selectors_component_ids_and_header_layouts(ctx):
    """tq over ids 0..3 with Cb and Cr on different tables, 16-bit DQT entries (<= 255, and up to ~1000); component ids
    0 1 2 / 1 2 3 / 10 20 30 / R G B with a JFIF segment (YCbCr to libjpeg and to the parser); SOF1, no JFIF, merged segments,
    segment orders, decoy tables, COM / APPn filler with one 65 533-byte APP segment, fill bytes, garbage between segments, two
    DRIs -- alone and all together."""
    cases = _header_cases()
    assert {c.group for c in cases} == {'tq', 'ids', 'layout'} and len(cases) == 22
    _assert_equal_to_pillow(ctx, cases)


@pytest.mark.gpu
def test_restart_intervals_with_custom_tables(ctx):
    cases = _restart_cases()
    assert sum(b'\xff\xdd' in c.data[:c.data.index(b'\xff\xda')] for c in cases) == len(cases)
    _assert_equal_to_pillow(ctx, cases)


@pytest.mark.gpu
def test_streams_that_do_not_synchronise(ctx):
    """480 x 640 4:2:0: a periodic stream, fixed-length codes on noise, the overshoot and the undershoot stream -- whole
    frames against Pillow, also mixed with ordinary files in one batch, and through melf_jpeg_process_batch with
    sample-images2's calibration (the window-limited rounds and their fall-back): records byte-equal to the reader's on
    Pillow's frames."""
    from meterelf_amd import MeterReader, _params
    from tests.test_jpeg import _encode
    cases = _sync_cases()
    _assert_equal_to_pillow(ctx, cases)
    rng = np.random.default_rng(3)
    ordinary = [_encode(_natural_image(rng, 480, 640), quality=q, subsampling='4:2:0') for q in (60, 90)]
    files = [ordinary[0], cases[2].data, ordinary[1], cases[3].data, ordinary[0], cases[0].data, cases[1].data]
    refs = [_pillow_bgr(d) for d in files]
    (frames, status) = ctx.jpeg_decode(files, 480, 640)
    assert (status == 0).all(), status
    for (i, (got, ref)) in enumerate(zip(frames, refs)):
        assert np.array_equal(got, ref), (i, int((got != ref).sum()))
    reader = MeterReader(_params.load(os.path.join(GOLDEN, 'sample-images2', 'params.yml')))
    try:
        (recs, status) = reader.ctx.jpeg_process_batch(files, 480, 640)
        assert (status == 0).all(), status
        assert recs.tobytes() == reader.read_frames(np.stack(refs)).tobytes()
    finally:
        reader.close()


@pytest.mark.gpu
def test_refusals(ctx):
    """Files libjpeg refuses (an over-subscribed table, a complete table using the all-ones code, a DC category above 15, a
    referenced table that is missing) come back with a status and a zero frame; 4:4:0 and 4:1:1, which libjpeg decodes and
    the kernels do not, come back unsupported (the host decoder's files); a bad table nobody refers to changes nothing.  The
    good files between them in the batch are untouched."""
    from meterelf_amd import _hip
    cases = _refusal_cases()
    good = _header_cases()[0]
    assert good.size == cases[0].size
    files = []
    for c in cases:
        files += [good.data, c.data]
    files.append(good.data)
    (H, W) = good.size
    (frames, status) = ctx.jpeg_decode(files, H, W)
    ref_good = _pillow_bgr(good.data)
    for i in range(0, len(files), 2):
        assert status[i] == 0 and np.array_equal(frames[i], ref_good), i
    for (k, c) in enumerate(cases):
        (got, st) = (frames[2 * k + 1], status[2 * k + 1])
        ref = _pillow_or_none(c.data)
        supported = _hip.jpeg_probe(c.data)[2]
        if ref is not None and supported:
            assert st == 0 and np.array_equal(got, ref), c
        elif ref is not None:
            assert st == _hip.JPEG_UNSUPPORTED and not got.any(), (c, int(st))
        else:
            assert st != 0 and not got.any(), (c, int(st))
