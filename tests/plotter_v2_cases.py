"""Shapes shared by test_plotter_v2_cpu.py and test_gpu_plotter_v2.py: one layout whose contigs end one base short of, on and one
base behind a tile of 4096 elements, tracks with a boundary nowhere / everywhere / at random, windows over them, and the rules of
utility/depth_plotter_v2.py stated in a few lines of numpy."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIN = os.path.join(GOLDEN, "dpv2_inputs")
# (a case is its manifest; expected/ holds its PNG figures and is absent when the case draws none: PDF figures are not kept)
CASES = sorted(d for d in os.listdir(GOLDEN) if d.startswith("dpv2_") and os.path.isfile(os.path.join(GOLDEN, d, "manifest.json")))
# the path each case must take: the device path unless the two files' headers do not line up
PATH_OF = {"dpv2_one_base_short": "host"}

LENGTHS = [1, 4095, 4096, 4097, 12289]
OFFSETS = [0, 4096, 8192, 12288, 20480]                 # every contig begins on a tile
TOTAL = 36864
LOW_BELOW = (1, 5, 2 ** 31 - 1)
TRACKS = ("zero", "low", "alternating", "random")


def track(kind: str) -> np.ndarray:
    """int32 [TOTAL]; the padding behind a contig stays 0, as every track of the project has it."""
    fill = {"zero": lambda n: np.zeros(n, np.int32), "low": lambda n: np.full(n, 3, np.int32),
            "alternating": lambda n: (np.arange(n) & 1).astype(np.int32),
            "random": lambda n: np.random.default_rng(n).choice(np.array([0, 0, 1, 4, 5, 9], np.int32), size=n)}[kind]
    t = np.zeros(TOTAL, dtype=np.int32)
    for o, n in zip(OFFSETS, LENGTHS):
        t[o:o + n] = fill(n)
    return t


def windows():
    """[begin, end) in track elements."""
    w = [(o, o + n) for o, n in zip(OFFSETS, LENGTHS)]                   # whole contigs
    w += [(20480 + 777, 20480 + 778)]                                    # one base
    w += [(8191, 8192), (8192, 8193), (8191, 8193), (12287, 12289)]      # one base either side of a tile boundary, and across it
    w += [(0, TOTAL), (0, TOTAL), (9000, 15000), (13000, 24000)]         # overlapping windows (two of them the whole track)
    w += [(500, 500), (600, 500)]                                        # empty
    w += [(TOTAL - 10, TOTAL + 50), (-5, 3)]                             # clipped at the track's end and at its beginning
    return w


def clip(w):
    a, b = max(w[0], 0), min(w[1], TOTAL)
    return a, max(a, b)


def runs(mask: np.ndarray) -> np.ndarray:
    """int64 [k, 2]: (first, last) of every maximal run of True."""
    edge = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    return np.stack([np.flatnonzero(edge == 1), np.flatnonzero(edge == -1) - 1], axis=1).astype(np.int64).reshape(-1, 2)


def rules(d: np.ndarray, window_size: int, low_below: int):
    """depth_plotter_v2.py for one region's depths d: zero runs, low runs, (means, starts, ends), (sum, number) of the depths > 0."""
    d = d.astype(np.int64)
    means, starts, ends = [], [], []
    for s, e in runs(d != 0).tolist():                                   # a stretch between two zero runs, cut from its first base on
        for a in range(s, e + 1, window_size):
            b = min(a + window_size, e + 1)
            means.append(np.mean(d[a:b]))
            starts.append(a)
            ends.append(b - 1)
    return (runs(d == 0), runs((d > 0) & (d < low_below)), (np.array(means, dtype=np.float64), np.array(starts, dtype=np.int64),
            np.array(ends, dtype=np.int64)), (int(d[d > 0].sum()), int((d > 0).sum())))


def items():
    """(contig index, start, end inclusive) for pipeline.depth_profile_v2."""
    out = [(c, 0, n - 1) for c, n in enumerate(LENGTHS)]
    out += [(4, 4095, 4095), (4, 4096, 4096), (4, 4095, 4096), (4, 100, 9000), (4, 5000, 12288), (3, 4096, 4096), (1, 7, 7)]
    return out


def same_profile(got: dict, d: np.ndarray, window_size: int, low_below: int) -> None:
    zero, low, (means, starts, ends), (s, n) = rules(d, window_size, low_below)
    assert np.array_equal(got["zero"], zero) and np.array_equal(got["low"], low)
    assert np.array_equal(got["starts"], starts) and np.array_equal(got["ends"], ends)
    assert got["means"].dtype == np.float64 and got["means"].tobytes() == means.tobytes()        # bit for bit
    assert (got["sum_pos"], got["n_pos"]) == (s, n)


def sub(t: str, out: str) -> str:
    return t.replace("{GOLDEN}", GOLDEN).replace("{DIN}", DIN).replace("{OUT}", out)


def norm(t: str, out: str) -> str:
    return t.replace(out, "{OUT}").replace(DIN, "{DIN}").replace(GOLDEN, "{GOLDEN}")
