"""Planned ties: images whose TM_CCOEFF map has a known, small set of exactly equal maxima at chosen positions, and what a match
kernel that decided "first" wrongly at one of its folds would answer on them.

cv2.minMaxLoc returns the FIRST maximum in raster order.  The match stage decides "first" in many hand-written places: inside a
lane, between the two 32-lane halves of a wave, between the waves of a workgroup, between the partials of a frame (on the device
in every dial kernel's prologue, on the host in melf_match_ccoeff).  An all-equal map has its first maximum at (0, 0), which is
the first element of the first lane of the first partial of every kernel: most wrong rules still answer (0, 0) there.

The construction.  A template that is constant along a lattice of displacements -- lattice_template: T[y, x] = c[x mod 4], lattice
{(dy, 4 k)} -- pasted at A and at A + d, d in the lattice, over a random 0..255 background: the pastes agree where they overlap
and both windows hold the template exactly, so both map values are the same integers through the same float operations.  The
PLANNED TIE SET of a scene is every A + lattice point whose window lies wholly inside the union of the pasted windows; every
other position loses at least a row or a column of the template, or -- in the notch between two pastes -- a few pixels that
tie_scene fills with the template's complement.  tests/test_match_ties.py shows by tests/match_exact.py alone
that the positions attaining the exact map's maximum are exactly the planned set, for every scene.

numpy only; nothing here needs a GPU.  Geometry (partial_slot, half_of) restates kernel code; the lines restated are cited.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import match_exact as mx

LATTICE_C = (23, 201, 96, 250)     # T[y, x] = LATTICE_C[x % 4]
VALU_RBLK = 44                     # k_match.hip: MATCH_R * MATCH_WAVES map rows per workgroup (melf_internal.h:38)
VALU_CBLK = 64                     # ... and MATCH_CBLK map columns (melf_internal.h:39)
V_ROWS = 32                        # k_match_gen.hip: map rows of a V-form tile
GEN_VREM_MAX = 4                   # k_match_gen.hip:569: remainder columns that go through the V form
SEED0 = 1                          # of the scenes' backgrounds

# (th, tw, rows, cols) of every shape the GPU tests run
SHAPES = {
    't119x188_i250x250': (119, 188, 250, 250),   # map 132 x 63: the tuned kernel's two column blocks; the VALU kernel's one
    't119x188_i250x215': (119, 188, 250, 215),   # map 132 x 28: the tuned kernel's one-block forms
    't119x188_i135x220': (119, 188, 135, 220),   # map 17 x 33: the general kernel's column block + one V-form column
    't119x188_i300x223': (119, 188, 300, 223),   # map 182 x 36: four V-form columns, six V-form row blocks
    't33x33_i96x97': (33, 33, 96, 97),           # map 64 x 65: two column blocks + one V-form column
    't33x33_i96x161': (33, 33, 96, 161),         # map 64 x 129: the VALU kernel's three column blocks and two row blocks
}
NEGATIVE_SHAPE = (119, 188, 119, 189)            # map 1 x 2, in the tuned kernel's class


def lattice_template(th, tw):
    """T[y, x] = LATTICE_C[x mod 4]: the same under every displacement (dy, 4 k)."""
    return np.ascontiguousarray(np.broadcast_to(np.array(LATTICE_C, np.uint8)[np.arange(tw) % 4], (th, tw)))


def tie_scene(th, tw, rows, cols, anchors, seed):
    """-> (img (rows, cols) u8, planned tie set [(y, x)] in raster order).  anchors: map positions (y, x) whose x agree modulo 4;
    the lattice template is pasted at each over a random 0..255 background.  The planned set: every position on the anchors'
    lattice whose th x tw window lies wholly inside the union of the pasted windows."""
    (rh, rw) = (rows - th + 1, cols - tw + 1)
    tpl = lattice_template(th, tw)
    phase = anchors[0][1] % 4
    rng = np.random.default_rng([SEED0, seed, th, tw, rows, cols])
    img = rng.integers(0, 256, size=(rows, cols), dtype=np.uint8)
    pasted = np.zeros((rows, cols), bool)
    for (y, x) in anchors:
        assert 0 <= y < rh and 0 <= x < rw and x % 4 == phase, (y, x, rh, rw)
        img[y:y + th, x:x + tw] = tpl
        pasted[y:y + th, x:x + tw] = True
    S = np.zeros((rows + 1, cols + 1), np.int64)
    S[1:, 1:] = pasted.astype(np.int64).cumsum(axis=0).cumsum(axis=1)
    count = S[th:, tw:] - S[:rh, tw:] - S[th:, :rw] + S[:rh, :rw]
    on_lattice = (np.arange(rw) % 4 == phase)[None, :]
    inside = (count == th * tw) & on_lattice
    planned = [(int(y), int(x)) for (y, x) in zip(*np.nonzero(inside))]     # np.nonzero: raster order
    # A lattice position in the notch of two pastes (A + (0, -4) beside A and A + (1, -4)) misses only 4 k pixels of one template
    # row; random pixels there beat the template's own once in a hundred scenes.  Those pixels hold the template's complement,
    # under which every element of LATTICE_C loses against itself: such a position is below the planned ones whatever the seed.
    # (A position that misses a whole row or column is 7 standard deviations or more below.)
    comp = np.broadcast_to((255 - np.array(LATTICE_C, np.uint8))[(np.arange(cols) - phase) % 4], (rows, cols))
    for (y, x) in zip(*np.nonzero((count < th * tw) & (count > th * tw - tw) & on_lattice)):
        hole = ~pasted[y:y + th, x:x + tw]
        img[y:y + th, x:x + tw][hole] = comp[y:y + th, x:x + tw][hole]
    return img, planned


def _xs(rw):
    """The columns the issue names: both halves (x mod 8 in 0..3 / 4..7), the ends of a column block, the second block, the map's
    right edge."""
    return [x for x in (0, 4, 24, 28, 36, rw - 5) if 0 <= x and x + 4 < rw]


def gen_vform(rw):
    """(first V-form column, number of V-form columns) of the general kernel for a map of rw columns (gen_plan, k_match_gen.hip:602-606)."""
    (full, rem) = divmod(rw, 32)
    vcols = rem if (0 < rem <= GEN_VREM_MAX and full >= 1) else 0
    return 32 * full, vcols


def scene_anchors(th, tw, rows, cols):
    """The anchor lists of a shape's scenes, derived from the map size and the kernels' block sizes: [(family, [(y, x), ...])]."""
    (rh, rw) = (rows - th + 1, cols - tw + 1)
    xs = _xs(rw)
    out = []
    # same row, the half hh = (x >> 2) & 1 flips: the first in half 0 (x mod 8 in 0..3) and in half 1 (4..7: the second is then in
    # the next element group of half 0)
    for (i, x) in enumerate(xs):
        y = (37 * i + 5) % rh
        out.append(('row_half', [(y, x), (y, x + 4)]))
    # same lane, the other column block: a column segment x, x + 4, ..., x + 32
    for (i, x) in enumerate(x for x in xs if x + 32 < rw):
        y = (53 * i + 11) % rh
        out.append(('row_block', [(y, x), (y, x + 32)]))
    # upper right before lower left, at every map row where it fits: one pair straddles every boundary between map rows, whichever
    # rows a layout gives to which wave, slice, tile or workgroup
    near = [x for x in xs if x >= 4]
    far = [x for x in xs if x >= 32]
    for y in range(rh - 1):
        if far and y % 4 in (1, 2):     # both variants at even and at odd rows
            x = far[(y // 2) % len(far)]
            out.append(('up_right_32', [(y, x), (y + 1, x - 32)]))
        elif near:
            x = near[(y // 2) % len(near)]
            out.append(('up_right_4', [(y, x), (y + 1, x - 4)]))
    # column segments y .. y + 8 across the boundaries of V-form tiles, of the VALU kernel's row blocks, and at the map's end
    for (i, y) in enumerate(sorted({V_ROWS - 4, VALU_RBLK - 4, rh - 9})):
        if y >= 0 and y + 8 < rh and xs:
            x = xs[(2 * i + 1) % len(xs)]
            out.append(('column', [(y, x), (y + 8, x)]))
    # triples in the last map row
    for x in xs:
        if x + 8 < rw and x in (0, 4, 28):
            out.append(('triple', [(rh - 1, x), (rh - 1, x + 4), (rh - 1, x + 8)]))
    # V-form columns of the general kernel: the H-form block's last element group against a V-form column, in the same row and
    # with the V-form column first in raster order; first and last row of a 32-row V block
    (vx0, vcols) = gen_vform(rw)
    if vcols:
        ys = sorted({0, V_ROWS - 1, V_ROWS, rh - 2} & set(range(rh - 1)))
        for xv in sorted({vx0, vx0 + vcols - 1}):
            for y in ys:
                out.append(('v_same_row', [(y, xv - 4), (y, xv)]))
                out.append(('v_first', [(y, xv), (y + 1, xv - 4)]))
            out.append(('v_same_row', [(rh - 1, xv - 4), (rh - 1, xv)]))
    # the VALU kernel on a map wider than one column block: the first maximum in a HIGHER partial slot (cb * nrb + rb) than the second
    for cb in range(1, (rw + VALU_CBLK - 1) // VALU_CBLK):
        for (i, k) in enumerate((0, 3)):
            x = VALU_CBLK * cb + 4 * k
            if x < rw:
                y = (29 * (cb + i) + 3) % (rh - 1)
                out.append(('valu_block', [(y, x), (y + 1, x - VALU_CBLK + 4 * (i + 1))]))
    return out


_scene_cache = {}
_planned_cache = {}


def planned_sets(shape_id):
    """The planned tie sets of a shape's scenes alone (no reference: what the wrong rules are pure functions of)."""
    if shape_id not in _planned_cache:
        (th, tw, rows, cols) = SHAPES[shape_id]
        _planned_cache[shape_id] = [tie_scene(th, tw, rows, cols, a, k)[1] for (k, (_f, a)) in enumerate(scene_anchors(th, tw, rows, cols))]
    return _planned_cache[shape_id]


def scene_set(shape_id):
    """Every scene of a shape and its exact reference, computed once per process and never modified: dict(tpl, imgs (S, rows, cols),
    families, anchors, planned [[(y, x)]], map (S, rh, rw) float32, firsts [(value, x, y)], seconds): `seconds` is the CPU time the
    reference took."""
    import time
    if shape_id not in _scene_cache:
        (th, tw, rows, cols) = SHAPES[shape_id]
        lst = scene_anchors(th, tw, rows, cols)
        tpl = lattice_template(th, tw)
        imgs = np.empty((len(lst), rows, cols), np.uint8)
        planned = []
        for (k, (_fam, anchors)) in enumerate(lst):
            (imgs[k], p) = tie_scene(th, tw, rows, cols, anchors, k)
            planned.append(p)
        t0 = time.perf_counter()
        (rmap, firsts) = reference(imgs, tpl)
        seconds = time.perf_counter() - t0
        for a in (tpl, imgs, rmap):
            a.setflags(write=False)
        _scene_cache[shape_id] = dict(tpl=tpl, imgs=imgs, families=[f for (f, _a) in lst], anchors=[a for (_f, a) in lst], planned=planned,
                                      map=rmap, firsts=firsts, seconds=seconds, shape=(th, tw, rows, cols))
    return _scene_cache[shape_id]


def reference(imgs, tpl, chunk=8, threads=8):
    """tests/match_exact.exact_match over the frames, a few frames per call on a few threads (numpy releases the interpreter lock in
    its loops; the frames are independent) -> (map float32, firsts)."""
    cuts = list(range(0, len(imgs), chunk))
    with ThreadPoolExecutor(max_workers=threads) as pool:
        parts = list(pool.map(lambda a: mx.exact_match(imgs[a:a + chunk], tpl)[2:], cuts))
    rmap = np.concatenate([p[0] for p in parts])
    firsts = [f for p in parts for f in p[1]]
    return rmap, firsts


def negative_scene():
    """-> (tpl, img): a 1 x 2 map of two equal NEGATIVE values.  The template is constant along its rows, T[y, x] = r[y]; the crop of
    th x (tw + 1) holds 255 - T continued by one column, so both windows are the template's negative."""
    (th, tw, rows, cols) = NEGATIVE_SHAPE
    r = np.random.default_rng([th, tw, 255]).integers(0, 256, size=th, dtype=np.uint8)
    tpl = np.ascontiguousarray(np.broadcast_to(r[:, None], (th, tw)))
    img = np.ascontiguousarray(np.broadcast_to((255 - r)[:, None], (rows, cols)))
    return tpl, img


# ------------------------------------------------------------------ geometry restated ----
def geometry(kernel, shape, n, layout=None):
    """What partial_slot / half_of need of a (kernel, layout): a dict from the library's layout queries (host logic, no GPU).
    kernel 'mfma': layout = None (the planner's choice for n frames) or (rb, pairs, ks) as MELF_MATCH_LAYOUT forces it; the caller
    has set that variable.  kernel 'gen': the plan of match_gen_plan_query.  kernel 'dot4': fixed."""
    from meterelf_amd import _hip
    (th, tw, rows, cols) = shape
    (rh, rw) = (rows - th + 1, cols - tw + 1)
    g = dict(kernel=kernel, rh=rh, rw=rw)
    if kernel == 'dot4':
        g['nrb'] = (rh + VALU_RBLK - 1) // VALU_RBLK       # k_match.hip:311
        g['nparts'] = g['nrb'] * ((rw + VALU_CBLK - 1) // VALU_CBLK)
        g['layout'] = 'dot4'
    elif kernel == 'mfma':
        d = _hip.match_layout_query(th, tw, rows, cols, n)
        assert d['kernel'] == 'mfma', d
        g.update(rb=d['rows_per_wave'], na=d['full_waves'], np=d['pair_waves'] // 2, ks=d['k_slices'], layout=d['layout'])
        g['nparts'] = (g['na'] + 2 * g['np']) * g['ks']    # mfma_plan: nparts = ntiles * ks
        assert g['nparts'] * d['groups'] == d['waves']
    else:
        (d, tasks) = _hip.match_gen_plan_query(th, tw, rows, cols, n)
        tiles = {}
        for t in tasks:
            tiles[int(t['tile'])] = (int(t['y0']), int(t['rows']), int(t['xb0']), int(t['nxb']))
        (vx0, vcols) = gen_vform(rw)
        assert vcols == d['v_columns']
        g.update(tiles=tiles, nparts=d['tiles'], vx0=vx0 if vcols else rw, layout=d['layout'], slices=d['slices'])
    return g


def mfma_tile(g, y, x):
    """Tuned kernel: (tile, its first map row, its rows R) of a map position (match_block, k_match_mfma.hip:686-694: na blocks of
    rb rows, then pairs of (rb + 1)-row waves whose shared middle row is split by column block; `on`, :280-282)."""
    (rb, na) = (g['rb'], g['na'])
    if y < rb * na:
        return y // rb, (y // rb) * rb, rb
    (q, off) = divmod(y - rb * na, 2 * rb + 1)
    base = rb * na + (2 * rb + 1) * q
    if off < rb or (off == rb and x < 32):      # MLAST = 1: the first wave of the pair owns column block 0 of the middle row
        return na + 2 * q, base, rb + 1
    return na + 2 * q + 1, base + rb, rb + 1    # MFIRST = 2: the second owns column block 1 of it


def partial_slot(g, y, x):
    """The slot of a frame's (max, arg-max) partials that holds the tile of map position (y, x)."""
    if g['kernel'] == 'dot4':       # k_match.hip:63-64, :221: tile = cb * nrb + rb -- column-block-major
        return (x // VALU_CBLK) * g['nrb'] + y // VALU_RBLK
    if g['kernel'] == 'mfma':       # k_match_mfma.hip:658: rblk * KS + ks, the slice being the one mine(r) names (:290)
        (t, y0, R) = mfma_tile(g, y, x)
        return t * g['ks'] + ((y - y0) * g['ks']) // R
    hits = []                       # k_match_gen.hip:163: the tile id; tiles as gen_plan lists them (:670-688)
    for (ti, (y0, R, xb0, nxb)) in g['tiles'].items():
        if R:       # H form
            if y0 <= y < y0 + R and 32 * xb0 <= x < min(32 * (xb0 + nxb), g['vx0']):
                hits.append(ti)
        elif x == g['vx0'] + xb0 and y0 <= y < y0 + V_ROWS:     # V form: one column, 32 rows
            hits.append(ti)
    assert len(hits) == 1, (y, x, hits)
    return hits[0]


def half_of(g, y, x):
    """The 32-lane half of the matrix-core kernels' wave that holds map position (y, x): H form, element column
    x = 32 xb + (e & 3) + 8 (e >> 2) + 4 hh (k_match_mfma.hip:638, k_match_gen.hip:385); V form, the same along y (:490)."""
    if g['kernel'] == 'gen' and x >= g['vx0']:
        return ((y % V_ROWS) >> 2) & 1
    return (x >> 2) & 1


def gen_lane_visits(g, tile, w, hh):
    """The map positions that one lane (half hh) of wave w of a general-kernel tile's workgroup hands to tile_epilogue, in the order
    of its visits (k_match_gen.hip: H form, :381-388 for a lone wave and :404-413 for the row blocks dealt to the waves of a sliced
    tile, element e at column 4 hh + (e & 3) + 8 (e >> 2) of its block; V form, :490, :498, :505-511: wave 0, the same along y)."""
    (y0, R, xb0, nxb) = g['tiles'][tile]
    ns = g['slices']
    cells = [(e & 3) + 8 * (e >> 2) + 4 * hh for e in range(16)]
    if R == 0:
        seq = [(y0 + c, g['vx0'] + xb0) for c in cells] if w == 0 else []
    else:
        seq = [(y0 + b // nxb, 32 * (xb0 + b % nxb) + c) for b in range(w, R * nxb, ns) for c in cells]
    return [(y, x) for (y, x) in seq if y < g['rh'] and x < g['rw']]


# ------------------------------------------------------------------ wrong rules ----
# Each: (tie set [(y, x)] in raster order, geometry) -> the (y, x) a kernel misbuilt in that way would report.  The right answer is
# ties[0].
def rule_last(ties, g):
    return ties[-1]


def rule_column_major(ties, g):
    return min(ties, key=lambda p: (p[1], p[0]))


def rule_half_low(ties, g):
    return min(ties, key=lambda p: (half_of(g, *p) != 0, p))


def rule_half_high(ties, g):
    return min(ties, key=lambda p: (half_of(g, *p) != 1, p))


def rule_slot_low(ties, g):
    return min(ties, key=lambda p: (partial_slot(g, *p), p))


def rule_slot_high(ties, g):
    return min(ties, key=lambda p: (-partial_slot(g, *p), p))


WRONG_RULES = {'last': rule_last, 'column_major': rule_column_major, 'half_low': rule_half_low, 'half_high': rule_half_high,
               'slot_low': rule_slot_low, 'slot_high': rule_slot_high}


def rules_of(kernel):
    """The halves are the matrix-core kernels' (a VALU lane holds one column)."""
    return [r for r in WRONG_RULES if kernel != 'dot4' or not r.startswith('half')]


def slot_table(g):
    """partial_slot of every map position: (rh, rw) int array."""
    return np.array([[partial_slot(g, y, x) for x in range(g['rw'])] for y in range(g['rh'])], np.int32)


def inseparable(rule, g, slots):
    """True where NO tie set can tell the rule from the right one in this geometry: slot_low when the slots never decrease along
    the raster order (the lowest slot then holds the raster-first tie), slot_high when there is one slot."""
    if rule == 'slot_low':
        flat = slots.ravel()
        return bool((flat[1:] >= flat[:-1]).all())
    if rule == 'slot_high':
        return g['nparts'] == 1
    return False
