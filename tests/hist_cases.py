"""The shapes gci_depth_hist is tested on (tests/test_hist_cpu.py: the CPU twin, tests/test_gpu_hist.py: the device), each a layout,
a flat int32 track and windows in track elements; some depend on n_bins (a ramp over every bin, the depths at the last bin's edge).
The statement's answer for a (case, n_bins) pair is computed once (want())."""
import functools
import gzip

import numpy as np

import bedgraph_cases as B
import hist_ref as R
from gci_amd import _lib, cpu, pipeline
from gci_amd.formats import depthfile

TILE = B.TILE
L3 = B.L3
CT = _lib.HIST_CHUNK_TILES                 # GCI_HIST_CHUNK_TILES (include/gci_hip.h); test_the_constants_are_the_header_s holds it
LDS = _lib.HIST_LDS_BINS                   # GCI_HIST_LDS_BINS (k_hist.hip), also Engine.HIST_LDS_BINS
I32_MAX, I32_MIN = R.I32_MAX, R.I32_MIN

SMALL_BINS = [0, 1, 2, 63, 64, 65]
LARGE_BINS = [LDS - 1, LDS, LDS + 1, 65536]


def _case(lengths, contigs, windows):
    return {"lengths": list(lengths), "track": B.flat(lengths, contigs), "windows": list(windows)}


def _one(contig, windows=None):
    return _case([len(contig)], [contig], [(0, len(contig))] if windows is None else windows)


def _from_bedgraph(name):
    c = B.CASES[name]()
    return {k: c[k] for k in ("lengths", "track", "windows")}


def window_edges(n_bins):
    """bedgraph_cases' windows -- begins at each residue mod 4, ends that cut a run mid-wave, (30, 30), one base, 300 windows of 1 .. 9
    bases inside one tile, overlapping ones -- and two pairs of identical windows."""
    c = _from_bedgraph("window_edges")
    c["windows"] += [(100, 5000), (6000, 6050), (6000, 6050), (-7, 3), (L3 - 2, L3 + 100000), (9, 2)]
    return c


def chunk_run(n_bins):
    """A run of 2000 equal depths across the boundary between the first and the second chunk of the whole window, and windows whose
    own chunks begin elsewhere."""
    n = (CT + 2) * TILE + 11
    t = B.geometric(np.random.default_rng(21), n, 50)
    t[CT * TILE - 1000:CT * TILE + 1000] = 9
    return _one(t, [(0, n), (CT * TILE - 500, CT * TILE + 500), (100, n), (TILE + 1, n - 1)])


def extremes(n_bins):
    a = np.array([-1, I32_MIN, I32_MAX, 5, 0, -1, -1, I32_MAX, I32_MAX, 7, 7, 7], dtype=np.int32)
    b = np.full(5000, I32_MIN, dtype=np.int32)
    off, _ = B.offsets([len(a), len(b)])
    return _case([len(a), len(b)], [a, b], [(off[0], off[0] + len(a)), (off[1], off[1] + len(b)), (0, off[1] + len(b))])


def last_bin(n_bins):
    """Depths exactly n_bins - 1 (the last bin; -1 is `under` at n_bins == 0), n_bins and n_bins + 1 (both `over`), in runs and alone."""
    v = np.array([n_bins - 1] * 7 + [n_bins] * 5 + [n_bins - 1, n_bins, n_bins + 1, n_bins - 1] * 300 + [n_bins] * 700, dtype=np.int32)
    return _one(v, [(0, len(v)), (3, 9), (7, 12)])


def wide(n_bins):
    """Depths on both sides of the LDS-resident bound, the value 65535 and its neighbours, among ordinary ones."""
    rng = np.random.default_rng(22)
    n = 3 * TILE + 77
    pool = np.array(list(range(0, 40)) + [LDS - 2, LDS - 1, LDS, LDS + 1, LDS + 2, 30000, 65534, 65535, 65535, 65536, 70000], dtype=np.int32)
    lens = rng.geometric(1.0 / 9, n // 4)
    t = np.repeat(pool[rng.integers(0, len(pool), lens.shape[0])], lens)[:n]
    assert t.shape[0] == n
    t[TILE - 2:TILE + 2] = 65535
    t[2 * TILE - 1] = LDS
    t[2 * TILE] = LDS - 1
    return _one(t, [(0, n), (TILE - 1, TILE + 1), (5, 2 * TILE + 1), (2 * TILE - 1, 2 * TILE + 1)])


def flush_path(n_bins):
    """4224 tiles (bedgraph_cases' second_level size) of geometric(mean 200) runs in three windows: 66 chunks, depths to 299."""
    n = 4224 * TILE
    t = B.geometric(np.random.default_rng(23), n, 200, 0, 300)
    return _one(t, [(0, n // 3 + 1), (n // 3 + 1, n - 4099), (n - 4099, n)])


CASES = {
    "tile_edges": lambda n_bins: _from_bedgraph("tile_edges"),
    "all_zero": lambda n_bins: _one(np.zeros(L3, dtype=np.int32)),
    "all_37": lambda n_bins: _one(np.full((2 * CT + 1) * TILE, 37, dtype=np.int32)),         # one bin from every wave, two flushes and a partial chunk
    "alternating": lambda n_bins: _one((np.arange(2 * TILE + 3) & 1).astype(np.int32)),
    "ramp": lambda n_bins: _one(np.arange(n_bins + 3, dtype=np.int32)),                       # every bin once, over = 3
    "geometric_7": lambda n_bins: _one(B.geometric(np.random.default_rng(24), 5 * TILE + 17, 7)),
    "geometric_200": lambda n_bins: _one(B.geometric(np.random.default_rng(25), 5 * TILE + 17, 200, 0, 300)),
    "window_edges": window_edges,
    "chunk_run": chunk_run,
    "extremes": extremes,
    "last_bin": last_bin,
    "layout25": lambda n_bins: _from_bedgraph("layout25"),
    "wide": wide,
}
DEPENDS_ON_BINS = ("ramp", "last_bin")
BIG = {"flush_path": flush_path}                                 # the device alone, one n_bins
# every case at the small n_bins; the large ones over the tracks that hold depths up there
PAIRS = [(name, nb) for name in sorted(CASES) for nb in SMALL_BINS] + [(name, nb) for name in ("wide", "ramp", "last_bin", "extremes", "layout25")
                                                                         for nb in LARGE_BINS]


@functools.lru_cache(maxsize=None)
def _made(name, key):
    c = (CASES.get(name) or BIG[name])(key)
    c["track"].setflags(write=False)
    return c


def case(name, n_bins):
    return _made(name, n_bins if name in DEPENDS_ON_BINS else None)


@functools.lru_cache(maxsize=None)
def want(name, n_bins):
    """-> (hist, stats) of the statement."""
    c = case(name, n_bins)
    return R.hist(c["track"], c["windows"], n_bins)


class HostEngine(cpu.CpuEngine):
    def to_device(self, a):
        return np.ascontiguousarray(a)


def host_tracks(path):
    """A `.depth.gz` through the CPU twin's reader (gci_depth_text_index / _parse over the gunzipped text), for the command line on
    the CPU twin -> (engine, DepthTracks, the gunzipped text)."""
    text = gzip.open(path, "rb").read()
    e = HostEngine()
    arr = np.frombuffer(text, dtype=np.uint8)
    tiles, keys, bad = e.depth_text_index(arr)
    line0 = np.concatenate([[0], np.cumsum(tiles.astype(np.uint64))]).astype(np.uint64)
    names, lengths, segs = depthfile.header_segments(arr, keys, line0)
    e.set_layout(lengths)
    track = e.new_track()
    e.depth_text_parse(arr, line0, segs(e.offsets), track)
    return e, pipeline.DepthTracks(e, dict(zip(names, lengths)), track), text
