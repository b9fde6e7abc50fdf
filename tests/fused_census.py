"""Test-only census of the fused mask's table design over all 2^24 BGR triples, computed with the CPU oracle's bgr2hls.

The fused full-frame stage (k_hls.hip) looks a pixel's in-range answer up in tables indexed by small integers and picks
one of nine kernel bodies from three numbers the GPU computes while it builds those tables (melf_api.hip,
ensure_fused_tables).  This module restates those numbers and the choice in plain numpy, from the oracle's H, L and S of
every triple.  It never imports the product: the GPU tests compare the product's answer with this one."""
import functools

import numpy as np

from oracle import pyoracle as po

N_TRIPLES = 1 << 24

# Every set of needle bounds the fused-mask tests use: name -> (needle colour h, l, s; range h, l, s; hue shift) as
# written into params.yml, the inclusive bounds they make (colour -+ range, clipped to 0..255), and what the census gives for
# them: ties, active sectors (bit 0 = r, 1 = g, 2 = b), non-interval rows per sector, kernel variant at default dispatch.
BOUNDS = {
    'red': dict(needle=dict(h=125, l=80, s=130, rh=9, rl=45, rs=35, shift=128), lo=(116, 35, 95), hi=(134, 125, 165),
                ties=0, active=1, noniv=(0, 0, 0), variant=6),     # the two fixture params.yml files
    'green': dict(needle=dict(h=85, l=120, s=120, rh=12, rl=80, rs=100, shift=0), lo=(73, 40, 20), hi=(97, 200, 220),
                  ties=0, active=2, noniv=(0, 0, 0), variant=7),
    'blue': dict(needle=dict(h=170, l=120, s=120, rh=12, rl=80, rs=100, shift=0), lo=(158, 40, 20), hi=(182, 200, 220),
                 ties=0, active=4, noniv=(0, 0, 0), variant=8),
    'several': dict(needle=dict(h=128, l=128, s=128, rh=100, rl=120, rs=120, shift=0), lo=(28, 8, 8), hi=(228, 248, 248),
                    ties=0, active=7, noniv=(255, 0, 0), variant=3),
    'seam': dict(needle=dict(h=43, l=128, s=128, rh=1, rl=128, rs=128, shift=0), lo=(42, 0, 0), hi=(44, 255, 255),
                 ties=0, active=3, noniv=(0, 0, 0), variant=3),
    'oddshift': dict(needle=dict(h=200, l=100, s=200, rh=60, rl=90, rs=55, shift=77), lo=(140, 10, 145), hi=(255, 190, 255),
                     ties=0, active=6, noniv=(0, 0, 0), variant=3),
}


def all_triples_image():
    """All 2^24 triples as one 4096 x 4096 BGR image; pixel t (row-major) is b = t & 255, g = (t >> 8) & 255, r = t >> 16.
    4096 columns: a multiple of 256, so no pixel goes through the oracle's scalar-tail S formula."""
    t = np.arange(N_TRIPLES, dtype=np.uint32)
    return np.stack([t & 255, (t >> 8) & 255, t >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


@functools.lru_cache(maxsize=4)
def hls_of_all_triples(hue_shift):
    """(H, L, S) of every triple by the oracle, each a u8 array of 2^24."""
    hls = po.bgr2hls(all_triples_image(), hue_shift).reshape(-1, 3)
    return tuple(np.ascontiguousarray(hls[:, k]) for k in range(3))


@functools.lru_cache(maxsize=1)
def table_index():
    """Per triple: the hue-table entry e = case * 65536 + diff * (diff + 1) + num, with the case order of hue_entry (r is
    the maximum, else g, else b) and num = g - b / b - r / r - g; and the L/S-table entry li = vmax * 256 + vmin."""
    t = np.arange(N_TRIPLES, dtype=np.int32)
    (b, g, r) = (t & 255, (t >> 8) & 255, t >> 16)
    vmax = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = vmax - vmin
    e = np.where(r == vmax, g - b, np.where(g == vmax, 65536 + b - r, 131072 + r - g)) + diff * (diff + 1)
    return (e.astype(np.int32), (vmax * 256 + vmin).astype(np.int32))


def runs_per_row(rows):
    """Number of runs of set bits in every row of a 2-D bool array."""
    return rows[:, 0].astype(np.int64) + (rows[:, 1:] & ~rows[:, :-1]).sum(axis=1)


def sector_rows(bits):
    """One sector's 65536 entry bits as the [diff][num + 256] rows of the single-sector tables (unused cells False)."""
    local = np.arange(65536)
    diff = np.floor(np.sqrt(local)).astype(np.int64)
    diff -= diff * diff > local
    diff += (diff + 1) * (diff + 1) <= local
    num = local - diff * (diff + 1)
    assert (np.abs(num) <= diff).all()
    grid = np.zeros((256, 512), bool)
    grid[diff, num + 256] = bits
    return grid


def variant_of(ties, active, noniv):
    """The selection itself: ties -> 4; exactly one active sector -> 0 / 1 / 2, and 6 / 7 / 8 if all of that sector's rows
    are intervals; otherwise 3."""
    if ties > 0:
        return 4
    v = {1: 0, 2: 1, 4: 2}.get(active, 3)
    if v < 3 and noniv[v] == 0:
        v += 6
    return v


def selection(hue_shift, lo, hi):
    """dict(ties, active, noniv, variant, in_range): the three numbers, the variant, and the in-range bit of every triple
    straight from the oracle's H, L, S (no table involved)."""
    (H, L, S) = hls_of_all_triples(hue_shift)
    (e, li) = table_index()
    hin = (H >= lo[0]) & (H <= hi[0])
    lsin = (L >= lo[1]) & (L <= hi[1]) & (S >= lo[2]) & (S <= hi[2])
    (seen_in, seen_out) = (np.zeros(3 * 65536, bool), np.zeros(3 * 65536, bool))
    seen_in[e[hin]] = True
    seen_out[e[~hin]] = True
    ties = int((seen_in & seen_out).sum())
    hue1 = seen_in & ~seen_out
    ls = np.zeros(65536, bool)
    ls[li[lsin]] = True
    ls_bad = int((runs_per_row(ls.reshape(256, 256)) > 1).sum())   # rows [vmax], bits over vmin; the same rows for every sector
    active = 0
    noniv = []
    for c in range(3):
        bits = hue1[c * 65536:(c + 1) * 65536]
        active |= int(bits.any()) << c
        noniv.append(ls_bad + int((runs_per_row(sector_rows(bits)) > 1).sum()))
    noniv = tuple(noniv)
    return dict(ties=ties, active=active, noniv=noniv, variant=variant_of(ties, active, noniv), in_range=hin & lsin)
