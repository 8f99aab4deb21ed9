"""The shapes the bedGraph passes are tested on (tests/test_bedgraph_cpu.py: the CPU twin, tests/test_gpu_bedgraph.py: the device),
each a layout, a flat int32 track, windows in track elements, one name and one first coordinate per window.  The statement's
answer for a case is computed once (want())."""
import functools

import numpy as np

import bedgraph_ref as R

TILE = 4096
RPB = 256                                  # GCI_BG_RUNS_PER_BLOCK (include/gci_hip.h); test_the_block_size_is_the_header_s holds it
L3 = 3 * TILE + 5


def offsets(lengths):
    tiles = np.concatenate([[0], np.cumsum([(L + TILE - 1) // TILE for L in lengths])])
    return (tiles[:-1] * TILE).tolist(), int(tiles[-1]) * TILE


def flat(lengths, contigs):
    off, total = offsets(lengths)
    t = np.zeros(max(total, 1), dtype=np.int32)
    for o, a in zip(off, contigs):
        t[o:o + len(a)] = a
    return t


def whole(lengths, names=None):
    off, _ = offsets(lengths)
    names = names or [b"c%d" % i for i in range(len(lengths))]
    return [(o, o + L) for o, L in zip(off, lengths)], names, [0] * len(lengths)


def geometric(rng, n, mean, lo=0, hi=60):
    """n bases of runs with geometric lengths (mean `mean`), neighbouring runs of different depth."""
    k = int(n / mean * 1.3) + 16
    lens = rng.geometric(1.0 / mean, k)
    while int(lens.sum()) < n:
        lens = np.concatenate([lens, rng.geometric(1.0 / mean, k)])
    vals = rng.integers(lo, hi, lens.shape[0]).astype(np.int32)
    vals[1:][vals[1:] == vals[:-1]] += 1
    return np.repeat(vals, lens)[:n]


def _case(lengths, contigs, windows, names, coord0):
    return {"lengths": list(lengths), "track": flat(lengths, contigs), "windows": list(windows), "names": list(names), "coord0": list(coord0)}


def _one(contig, name=b"chr1"):
    return _case([len(contig)], [contig], [(0, len(contig))], [name], [0])


def tile_edges():
    t = np.full(L3, 5, dtype=np.int32)
    for k, i in enumerate((0, 4095, 4096, 4097, 8191, 8192, L3 - 1)):
        t[i] = 100 + k
    return _one(t)


def window_edges():
    t = geometric(np.random.default_rng(11), L3, 7)
    t[6000:6100] = 3                                          # a constant run to cut inside
    wins = [(a, b) for a in range(4093, 4100) for b in range(8189, 8196)]
    wins += [(4096, 4097), (10, 20), (30, 30), (40, 50), (6000, 6050), (6050, 6100), (100, 5000), (4000, 9000)]
    rng = np.random.default_rng(12)
    at = rng.integers(4096, 8192 - 9, 300)
    wins += [(int(a), int(a) + 1 + k % 9) for k, a in enumerate(at)]
    return _case([L3], [t], wins, [b"chr1"] * len(wins), [a for a, _ in wins])


def decimal_widths():
    """A run at every base of a 12-base window whose first coordinate is 10^k - 2: starts and ends cross every power of ten; and
    every width of a depth."""
    depths = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000,
              999999999, 1000000000, 2147483647, -1, -9, -10, -2147483648]
    ramp = np.arange(12, dtype=np.int32)
    lengths = [12, len(depths)]
    off, _ = offsets(lengths)
    coord0 = [10 ** k - 2 for k in range(1, 10)] + [2 ** 31 - 1 - 12]
    wins = [(off[0], off[0] + 12)] * len(coord0) + [(off[1], off[1] + len(depths))]
    return _case(lengths, [ramp, np.array(depths, dtype=np.int32)], wins, [b"s"] * len(wins), coord0 + [0])


def names():
    """Names of 1 .. 40 and 255 bytes over a two-run window: lines begin at every residue mod 16."""
    t = np.array([4, 4, 4, 8, 8], dtype=np.int32)
    nm = [bytes(33 + (k + j) % 90 for j in range(n)) for k, n in enumerate(list(range(1, 41)) + [255])]
    return _case([5], [t], [(0, 5)] * len(nm), nm, [0] * len(nm))


def chunk(total, split):
    ramp = np.arange(total, dtype=np.int32)
    wins = [(0, total)] if not split else [(0, total // 2 - 3), (total // 2 - 3, total)]
    return _case([total], [ramp], wins, [b"chrA"] * len(wins), [a for a, _ in wins])


def second_level():
    n = 4224 * TILE
    rng = np.random.default_rng(13)
    flag = np.zeros(n, dtype=bool)
    flag[::1021] = True
    flag[rng.integers(0, n, 1_200_000)] = True
    return _one((np.cumsum(flag) % 97).astype(np.int32), b"chr7")


def layout25():
    rng = np.random.default_rng(14)
    lengths = [int(x) for x in rng.integers(1, 5 * TILE, 25)]
    lengths[3], lengths[9] = TILE + 1, 2 * TILE - 1
    contigs = [geometric(rng, L, 200) for L in lengths]
    wins, nm, c0 = whole(lengths, [b"contig_%d" % i for i in range(25)])
    return _case(lengths, contigs, wins, nm, c0)


CASES = {
    "tile_edges": tile_edges,
    "all_zero": lambda: _one(np.zeros(L3, dtype=np.int32)),
    "all_37": lambda: _one(np.full(L3, 37, dtype=np.int32)),
    "alternating": lambda: _one((np.arange(2 * TILE + 3) & 1).astype(np.int32)),
    "ramp": lambda: _one(np.arange(2 * TILE + 3, dtype=np.int32)),
    "window_edges": window_edges,
    "decimal_widths": decimal_widths,
    "names": names,
    "layout25": layout25,
    "second_level": second_level,
}
for _n in (RPB - 1, RPB, RPB + 1, 2 * RPB, 2 * RPB + 1):
    CASES["chunk_%d" % _n] = functools.partial(chunk, _n, False)
    CASES["chunk_%d_split" % _n] = functools.partial(chunk, _n, True)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["track"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want(name):
    """-> (runs, run0, text, byte0) of the statement."""
    c = case(name)
    return R.runs(c["track"], c["windows"]) + R.text(c["track"], c["windows"], c["names"], c["coord0"])
