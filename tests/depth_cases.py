"""Interval sets for the depth build, shared by the reference's own test (test_depth_ref_cpu.py) and the GPU tests of the
size-selected paths (test_gpu_build_shapes.py).  The two small families restate, seed for seed, the sets of
test_depth_build_slice_semantics and test_fused_byproducts_sparse_and_dense_tiles (test_gpu_seams.py): negative-stop wraps,
empty slices, reads hanging over the end, tiny contigs, pile-ups next to empty tiles."""
import numpy as np

import depth_ref as R

TILE = R.TILE


def slice_semantics():
    """-> (lengths dict, [(contig index, start, end)])"""
    rng = np.random.default_rng(5)
    lengths = {"x": 10_000, "y": 4096, "z": 4097, "w": 50, "v": 123_457}
    ivls = []
    for c, t in enumerate(lengths):
        L = lengths[t]
        for _ in range(400):
            s = int(rng.integers(0, L))
            e = int(min(L + 40, s + rng.integers(1, max(2, L // 3))))
            ivls.append((c, s, e))
    ivls += [(3, 0, 10), (3, 0, 13), (3, 0, 14), (3, 20, 25), (0, 9_990, 10_050), (1, 0, 4096), (2, 4090, 4097)]
    return lengths, ivls


def sparse_and_dense(seed):
    rng = np.random.default_rng(100 + seed)
    lengths = {"a": 70_000, "b": 8192, "c": 4097, "d": 12_288, "e": 40, "f": 33_333, "g": 1, "h": 3, "i": 16, "j": 17, "k": 5}
    ivls = []
    for c, t in enumerate(lengths):
        L = lengths[t]
        for _ in range(max(2, L // 900)):
            s = int(rng.integers(0, L))
            ivls.append((c, s, int(min(L + 5, s + rng.integers(1, 2500)))))
        for _ in range(L // 20_000):
            s0 = int(rng.integers(0, max(1, L - 3000)))
            for _ in range(60):
                s = s0 + int(rng.integers(0, 2000))
                ivls.append((c, s, s + int(rng.integers(1, 800))))
    ivls += [(1, 0, 4096), (1, 4096, 8192), (3, 4095, 4097), (3, 8191, 8193), (0, 0, 1), (0, 69_999, 70_000), (4, 0, 40)]
    ivls += [(6, 0, 1), (7, 1, 3), (8, 0, 16), (8, 3, 9), (9, 0, 17), (9, 16, 17), (10, 2, 4)]
    if seed == 2:
        ivls += [(0, 5000, 60_000)] * 99 + [(0, 20_000, 40_000)] * 2 + [(5, 100, 33_000)] * 300 + [(5, 4090, 4100)] * 5
    if seed == 3:
        ivls += [(5, 3000, 30_000)] * 1100 + [(5, 10_000, 10_010)] * 9000
    return lengths, ivls


def _rows(*parts):
    return np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1, 3) for p in parts])


def _spread(rng, c, L, n, max_len, lo=0, hi=None):
    """n intervals on contig c that start in [lo, hi) and are 1 .. max_len long (they may hang over the end)."""
    hi = L if hi is None else hi
    s = rng.integers(lo, hi, n)
    return np.stack([np.full(n, c), s, s + rng.integers(1, max_len + 1, n)], axis=1)


# ---- (a) three ranges of the radix event partition, one of them too full for the staging area --------------------------------

THREE_RANGES_LENGTHS = [300 * TILE + 77,        # tiles 0 .. 300; ends off a tile boundary
                        0,                      # no tiles, in the middle
                        900 * TILE,             # tiles 301 .. 1200: over the seam 1023 | 1024, ends ON a tile boundary
                        50,                     # tile 1201
                        850 * TILE + 1,         # tiles 1202 .. 2052: over the seam 2047 | 2048, one base in its last tile
                        8 * TILE,               # tiles 2053 .. 2060, inside range 2
                        0]                      # no tiles, at the end


def three_ranges(flank):
    """~2 060 tiles and ~21 000 intervals.  Range 1 holds a pile-up of 15 800 short intervals (15 000 and more at a flank of 15) (more events than the staging area
    takes), ranges 0 and 2 ordinary coverage.  Behind the seeded part come single-event intervals -- a start whose stop is the
    contig's end on a tile boundary -- until range 0 holds an odd number of events and ranges 1 and 2 an even one at this flank:
    range 0's stretch of the bucket array then starts at an even index and has an odd tail, range 2's starts at an odd one and has
    a head and an odd tail.  -> int64 [n, 3]"""
    L = THREE_RANGES_LENGTHS
    rng = np.random.default_rng(2050)
    seam1, seam2 = (1024 - 301) * TILE, (2048 - 1202) * TILE          # the range seams in the coordinates of contigs 2 and 4
    rows = _rows(
        _spread(rng, 0, L[0], 700, 8000), _spread(rng, 2, L[2], 2000, 8000), _spread(rng, 3, L[3], 6, 60),
        _spread(rng, 4, L[4], 1900, 8000), _spread(rng, 5, L[5], 40, 9000),
        _spread(rng, 2, L[2], 700, 3000, 100 * TILE, 130 * TILE),                 # ~45 events a tile: the whole-wave class
        _spread(rng, 4, L[4], 15_800, 800, 100 * TILE, 140 * TILE),               # the pile-up, tiles 1302 .. 1341
        # starts in one range, stops in the next
        _spread(rng, 2, L[2], 60, 30_000, seam1 - 20_000, seam1), _spread(rng, 4, L[4], 60, 30_000, seam2 - 20_000, seam2),
        [(4, seam2 - 3 * TILE, L[4] - 3 * TILE), (2, seam1 - 1, seam1 + 40), (2, seam1 - 40, seam1 - 1), (4, seam2, seam2 + 1)],
        # up to b == L.  Without tail padding (no event, the coarse -1 alone): from range 0 into range 1, and inside range 2;
        # with tail padding (an event in the padding): from range 1 into range 2, and inside range 0
        [(2, seam1 - 5000, L[2] + 100), (2, seam1 + 7, L[2] - 1 + flank), (5, 100, L[5] + 9), (5, 3 * TILE, L[5] - 1 + flank)],
        [(4, seam2 - 9000, L[4] + 100), (4, seam2 + 7, L[4] - 1 + flank), (0, L[0] - 20_000, L[0] + 5), (0, 299 * TILE, L[0] - 1 + flank), (3, 0, 50 + flank)],
        [(7, 0, 100), (-1, 0, 100), (1, 0, 10), (6, 0, 10)])                      # no such contig; contigs without a base
    one_event = {0: (2, seam1 - 3 * TILE, L[2] + 1000), 1: (2, seam1 + 3 * TILE, L[2] + 1000), 2: (5, TILE, L[5] + 1000)}
    for _ in range(4):
        ev = R.build(L, rows, flank).range_events
        fix = [one_event[r] for r, odd in ((0, 1), (1, 0), (2, 0)) if int(ev[r]) % 2 != odd]
        if not fix:
            break
        rows = _rows(rows, fix)
    return rows


# ---- (b) more than eight blocks of the per-tile tables, 30 000 contigs, 2^20 intervals -----------------------------------------

def many_tiles():
    """-> (lengths int64 [30 004], intervals int64 [2^20 + 3000, 3]).  ~30 000 contigs of 0 .. 200 bases (one tile each, none for
    length zero); a contig of 3000 tiles over the table-block boundary at tile 8192, one of exactly 1024 tiles over the one at
    32 768, one of five tiles and a base, a short one at the very end.  60 % of the intervals lie on the long contigs: the
    first third of the 3000-tile contig and the 1024-tile contig are pile-ups throughout, the rest of the long one has some
    twenty events a tile on top of a carry."""
    rng = np.random.default_rng(32_769)
    small = rng.integers(0, 201, 30_000)
    k1, k2 = 6000, 29_000                                   # small contigs in front of the 3000-tile one / of the 1024-tile one
    lengths = np.concatenate([small[:k1], [3000 * TILE - 1234], small[k1:k2], [1024 * TILE], small[k2:], [5 * TILE + 1], [137]])
    big, mid, five = k1, k2 + 1, 30_002
    n = (1 << 20) + 3000
    n_small = int(0.4 * n)
    n_mid, n_five, n_far = 130_000, 300, 20_000
    extra = [(30_003, 0, 137), (30_003, 100, 300), (mid, 0, 1024 * TILE - 1), (five, 5 * TILE, 5 * TILE)]
    n_near = n - n_small - n_mid - n_five - n_far - len(extra)
    sc = rng.integers(0, 30_000, n_small)
    sc = np.where(sc < k1, sc, np.where(sc < k2, sc + 1, sc + 2))                 # index among all contigs
    sL = np.maximum(lengths[sc], 1)
    ss = (rng.random(n_small) * sL).astype(np.int64)
    small_rows = np.stack([sc, ss, ss + rng.integers(1, 260, n_small)], axis=1)
    rows = _rows(small_rows,
                 _spread(rng, big, lengths[big], n_near, 20_000, 0, 1000 * TILE),
                 _spread(rng, big, lengths[big], n_far, 20_000, 1000 * TILE, int(lengths[big])),
                 _spread(rng, mid, lengths[mid], n_mid, 20_000),
                 _spread(rng, five, lengths[five], n_five, 9000),
                 extra)
    return lengths.astype(np.int64), rows[rng.permutation(n)]
