"""CPU census behind the fused mask's kernel selection (tests/fused_census.py): the facts the table design rests on,
checked over all 2^24 BGR triples with the oracle's bgr2hls.  No GPU, no product code."""
import numpy as np
import pytest

from tests import fused_census as fc


def test_hue_is_a_function_of_the_table_entry():
    """Test A.  H (hue shift 0) depends on (case, diff, num) alone, L and S on (vmax, vmin) alone, and the hue shift is a
    rotation mod 256.  So no entry ever sees an in-range and an out-of-range H: the tie count is 0 for every bounds and
    every shift, and variant 4's re-evaluation is unreachable by data."""
    (H, L, S) = fc.hls_of_all_triples(0)
    (e, li) = fc.table_index()
    first = np.zeros(3 * 65536, np.uint8)
    first[e] = H                                  # one representative per entry
    assert np.array_equal(first[e], H)            # ... equals every triple's H
    assert np.unique(e).size == 195841            # the entries that occur at all
    for plane in (L, S):
        rep = np.zeros(65536, np.uint8)
        rep[li] = plane
        assert np.array_equal(rep[li], plane)
    for shift in (1, 77, 128, 255):
        (Hs, Ls, Ss) = fc.hls_of_all_triples(shift)
        assert np.array_equal(Hs, H + np.uint8(shift))   # u8 arithmetic wraps mod 256
        assert np.array_equal(Ls, L) and np.array_equal(Ss, S)
    # the consequence, through the restated selection, for every bounds the suite uses
    for (name, b) in fc.BOUNDS.items():
        assert fc.selection(b['needle']['shift'], b['lo'], b['hi'])['ties'] == 0, name


@pytest.mark.parametrize('name', list(fc.BOUNDS))
def test_restated_selection_reproduces_the_census(name):
    """Test B.  The numpy restatement of the selection gives the recorded table (fused-mask section)."""
    b = fc.BOUNDS[name]
    n = b['needle']
    assert b['lo'] == tuple(max(0, c - r) for (c, r) in ((n['h'], n['rh']), (n['l'], n['rl']), (n['s'], n['rs'])))
    assert b['hi'] == tuple(min(255, c + r) for (c, r) in ((n['h'], n['rh']), (n['l'], n['rl']), (n['s'], n['rs'])))
    sel = fc.selection(n['shift'], b['lo'], b['hi'])
    assert (sel['ties'], sel['active'], sel['noniv'], sel['variant']) == (b['ties'], b['active'], b['noniv'], b['variant'])
    assert sel['in_range'].any()
    if name == 'red':
        assert int(sel['in_range'].sum()) == 162134


def test_variant_of():
    assert fc.variant_of(1, 1, (0, 0, 0)) == 4
    assert [fc.variant_of(0, a, (0, 0, 0)) for a in (1, 2, 4)] == [6, 7, 8]
    assert [fc.variant_of(0, a, (1, 2, 3)) for a in (1, 2, 4)] == [0, 1, 2]
    assert fc.variant_of(0, 2, (5, 0, 5)) == 7
    assert [fc.variant_of(0, a, (0, 0, 0)) for a in (0, 3, 5, 6, 7)] == [3] * 5


def test_bit_table_variants_are_unreachable_at_default_dispatch():
    """Test C.  Variants 0 / 1 / 2 need exactly one active hue sector AND a table row of that sector whose set bits are
    not one run.  Checked exhaustively, not argued:
      * L is non-decreasing and S non-increasing in vmin for every vmax, so {vmin : L and S within ANY bounds} is an
        interval: every L/S row is one run whatever the bounds;
      * the in-range hues of any bounds and shift are one arc (start, length) of the hue circle; for all 256 x 256 arcs,
        whenever exactly one sector has an in-range entry, every [diff] row of that sector is one run over num.
    Hence a single active sector always gets the interval tables (6 / 7 / 8); 0 / 1 / 2 run only under
    MELF_FUSED_VARIANT=bits."""
    (H, L, S) = fc.hls_of_all_triples(0)
    (e, li) = fc.table_index()
    (Lt, St) = (np.zeros(65536, np.int64), np.zeros(65536, np.int64))
    Lt[li] = L
    St[li] = S
    (Lt, St) = (Lt.reshape(256, 256), St.reshape(256, 256))       # [vmax][vmin]
    for vmax in range(256):
        assert (np.diff(Lt[vmax, :vmax + 1]) >= 0).all(), vmax
        assert (np.diff(St[vmax, :vmax + 1]) <= 0).all(), vmax
    # per-entry hue, as rows [sector * 256 + diff] of 2 * diff + 1 cells (num = -diff .. diff)
    occurs = np.zeros(3 * 65536, bool)
    occurs[e] = True
    hent = np.zeros(3 * 65536, np.int64)
    hent[e] = H
    idx = np.flatnonzero(occurs)
    local = idx & 65535
    diff = np.floor(np.sqrt(local)).astype(np.int64)
    diff -= diff * diff > local
    diff += (diff + 1) * (diff + 1) <= local
    row = (idx >> 16) * 256 + diff
    # idx is sorted, so within a row the cells come in num order; prev = the cell before, within the same row
    same_row = np.concatenate([[False], row[1:] == row[:-1]])
    # The GPU counts runs over all 512 cells of a [diff][num + 256] row, cells that never occur reading 0; counting over the
    # occurring cells alone is the same thing because within every row the occurring nums are consecutive (the cells that
    # never occur -- num = -diff in the g sector, |num| = diff in the b sector -- lie at a row's ends, never inside it)
    num = local - diff * (diff + 1)
    assert (num[1:][same_row[1:]] == num[:-1][same_row[1:]] + 1).all()
    assert np.unique(row).size == 768 - 2   # every (sector, diff) row occurs, but diff = 0 only in the r sector (greys)
    sector_of_row = np.arange(768) // 256
    single_sector_arcs = 0
    for start in range(256):
        rel = (hent[idx] - start) & 255             # cell is in range for arc length n iff rel < n
        prev = np.where(same_row, np.roll(rel, 1), 256)   # a row's first cell: as if preceded by an out-of-range cell
        # a run starts at a cell iff rel < n <= prev: +1 for n in (rel, prev]; runs[row][n] by a difference array
        rising = prev > rel
        d = np.zeros((768, 258), np.int64)
        np.add.at(d, (row[rising], rel[rising] + 1), 1)
        np.add.at(d, (row[rising], prev[rising] + 1), -1)
        runs = np.cumsum(d, axis=1)[:, :257]        # [row][n], n = 0 .. 256
        minrel = np.array([rel[(idx >> 16) == c].min() for c in range(3)])
        for n in range(257):
            act = [c for c in range(3) if minrel[c] < n]
            if len(act) != 1:
                continue
            single_sector_arcs += 1
            bad = (runs[sector_of_row == act[0], n] > 1).sum()
            assert bad == 0, (start, n, act, int(bad))
    assert single_sector_arcs > 3 * 80 * 40   # the check did see single-sector arcs: three sectors of about 85 hues each
