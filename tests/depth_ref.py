"""Plain numpy statement of the depth build over a whole layout: `depths[t][s + fl : e - fl + 1] += 1` (GCI.py:302-306) as one
difference array over the concatenated contigs, and the number of events gci_depth_build_begin buckets per tile (k_evt_count:
one per start, one per stop that lies inside the contig's tiles) -- what the GPU tests of the size-selected paths assert their
shapes from.  Test infrastructure only: no torch, no GPU."""
from types import SimpleNamespace

import numpy as np

TILE = 4096                      # bases per tile (gci_common.h)
RANGE_TILES = 1 << 10            # tiles per range of the radix event partition below 2^20 tiles (k_depth.hip, evp_sh = 10)
EVP_CHUNK = 8192                 # intervals per workgroup of the partition passes
STAGE_CAP = (65536 - 8 * RANGE_TILES) // 2      # events of a range that k_evp_tiles<1> puts together in LDS
TABLE_BLOCK = 4096               # tiles per workgroup of the table scans


def slice_bound(v, L):
    """Python's slice bound: a negative value gets + L, then the value is clipped to [0, L]."""
    v = np.asarray(v, dtype=np.int64)
    return np.clip(np.where(v < 0, v + L, v), 0, L)


def tiles_of(lengths):
    """-> tile_first int64 [n + 1]: a contig occupies ceil(L / TILE) whole tiles, one of length zero none."""
    lengths = np.asarray(lengths, dtype=np.int64)
    tf = np.zeros(lengths.shape[0] + 1, dtype=np.int64)
    np.cumsum((lengths + TILE - 1) // TILE, out=tf[1:])
    return tf


def build(lengths, ivl, flank):
    """lengths: the layout; ivl: integer rows (contig, start, end, ...); rows whose contig is not of the layout count for nothing.
    -> depth int64 [sum(lengths)] (the contigs behind one another, no padding), off int64 [n + 1] (contig c is
    depth[off[c]:off[c + 1]]), sums int64 [n], tile_first int64 [n + 1], tile_events int64 [n_tiles], range_events int64
    [ceil(n_tiles / RANGE_TILES)]; lengths and flank as given."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = lengths.shape[0]
    ivl = np.asarray(ivl, dtype=np.int64)
    if ivl.size == 0:
        ivl = np.zeros((0, 3), dtype=np.int64)
    c, s, e = ivl[:, 0], ivl[:, 1], ivl[:, 2]
    live = (c >= 0) & (c < n)
    c, s, e = c[live], s[live], e[live]
    L = lengths[c]
    a = slice_bound(s + flank, L)
    b = slice_bound(e - flank + 1, L)
    live = a < b
    c, L, a, b = c[live], L[live], a[live], b[live]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    total = int(off[n])
    # b == L falls on the first base of the next contig (or one past the end): every contig's differences sum to zero there
    diff = np.bincount(off[c] + a, minlength=total + 1) - np.bincount(off[c] + b, minlength=total + 1)
    depth = np.cumsum(diff[:total], dtype=np.int64)
    csum = np.concatenate(([0], np.cumsum(depth)))
    sums = csum[off[1:]] - csum[off[:-1]]
    tf = tiles_of(lengths)
    n_tiles = int(tf[n])
    has_b = b < (L + TILE - 1) // TILE * TILE                      # a stop at b == L is an event only in tail padding
    tile_events = (np.bincount(tf[c] + a // TILE, minlength=n_tiles) +
                   np.bincount((tf[c] + b // TILE)[has_b], minlength=n_tiles)).astype(np.int64)
    n_ranges = (n_tiles + RANGE_TILES - 1) // RANGE_TILES
    range_events = np.bincount(np.arange(n_tiles) // RANGE_TILES, weights=tile_events, minlength=n_ranges).astype(np.int64)
    return SimpleNamespace(depth=depth, off=off, sums=sums.astype(np.int64), tile_first=tf, tile_events=tile_events,
                           range_events=range_events, lengths=lengths, flank=int(flank))


def contig(ref, c):
    return ref.depth[ref.off[c]:ref.off[c + 1]]


def padded_track(ref, dtype=np.int32):
    """The track as the device lays it out: contig c from base tile_first[c] * TILE on, zeros in the padding."""
    n_tiles = int(ref.tile_first[-1])
    out = np.zeros(max(n_tiles * TILE, 1), dtype=dtype)
    base = np.repeat(ref.tile_first[:-1] * TILE - ref.off[:-1], ref.lengths)
    out[base + np.arange(ref.depth.shape[0])] = ref.depth
    return out
