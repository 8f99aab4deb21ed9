"""Named inputs of the allele kernels (gci_bam_allele_*, gci_allele_sites_*).  The record cases are those of tests/mismatch_cases.py,
unchanged and by import -- operations of 0, 1, 65 and 129 bases, rounds of 255 / 256 / 257 bases, more than 2048 operations, both
nibble phases, the CG array, the contig's end, l_seq, the malformed records -- plus `every_base`: a 1024-base M in which EVERY base
is a mismatch, so that every lane holds its full share of events of mixed classes in every step.  case(name) -> dict(stream, offs,
lengths, ref_sel, codes, runs); want(name, run) -> (four lists, six counts, status word) from tests/allele_ref.py, computed once.
EXPECTED holds the lists written by hand.  site_case(name) -> dict(lengths, a, c, g, t, depth, codes, runs) with runs of (min_reads,
frac_ppm, windows); SITES_EXPECTED the sites written by hand."""
import functools

import numpy as np

import allele_ref as R
import mismatch_cases as MC
from mismatch_cases import EXCL, M, MALFORMED      # noqa: F401

INT_MAX = 2 ** 31 - 1


def _every_base():
    """Every base of the M reads one of the three OTHER bases (seeded); an odd position, so the M begins in a low nibble of no byte
    but its own; a second record whose M begins behind a 1-base S."""
    refs = [("c", MC.contig_seq(1500, 40))]
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def other(pos, n):
        idx = np.searchsorted(acgt, np.frombuffer(refs[0][1][pos:pos + n], dtype=np.uint8))
        return bytes(acgt[(idx + rng.integers(1, 4, n)) % 4])
    recs = [MC.mrec(refs, 0, 101, [(M, 1024)], seq=other(101, 1024)),
            MC.mrec(refs, 0, 300, [(MC.S, 1), (M, 777)], seq=b"A" + other(300, 777))]
    return MC.build(refs, recs)


OWN = {"every_base": _every_base}
NAMES = MC.NAMES + list(OWN)

# by hand, from the records of mismatch_cases._phases and _letters: the event of mismatch_cases.EXPECTED in the list of the READ's base
EXPECTED = {
    ("phases", (EXCL, 0)): ([], [(0, 4), (0, 6), (0, 0)], [], [(0, 4), (0, 14)]),
    ("letters", (EXCL, 0)): ([(0, 7), (0, 3)], [], [(0, 1), (1, 1)], []),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return OWN[name]() if name in OWN else MC.case(name)


@functools.lru_cache(maxsize=None)
def want(name, run):
    c = case(name)
    return R.stream_events(c["stream"], c["offs"], c["lengths"], c["ref_sel"], c["codes"], *run)


def pairs():
    return [(name, run) for name in NAMES for run in case(name)["runs"]]


# ---- sites: tracks written by hand -----------------------------------------------------------------------------------------------------
SITE_KEYS = ("a", "c", "g", "t", "depth", "codes")


def _site_planted():
    """Two contigs, the second beginning at a tile's first element (12288).  What is planted, by flat element -- (A, C, G, T), depth:
         0      (0,0,0,6) 10   the first element; ref code 15            4095   (0,9,0,0) 9    a tile's last element; ref code 0
         100    (5,0,0,0) 8    two adjacent hot bases: two sites         4096   (0,0,9,1) 10   the next tile's first; ref code 238
         101    (0,0,7,1) 9                                              8999   (8,0,0,0) 8    the last base of contig 0
         200    (0,5,0,5) 10   a two-way tie: C; 5 of 10 is exactly half 9500   (9,9,9,9) 9    padding: never a site
         300    (4,4,4,4) 8    a four-way tie: A                         12288  (0,0,0,5) 5    the first base of contig 1
         400    (3,0,0,0) 4    best == min_reads 3                       17287  (0,6,0,0) 6    the last base of contig 1
         402    (0,0,2,0) 2    best == min_reads - 1                     17288  (7,0,0,0) 7    padding
         500    (0,3,0,0) 6    3 * 10^6 == 500000 * 6 exactly; one part per million more and it is cold
         502    (0,3,0,0) 7    below a half
         600    (0,0,0,4) 0    depth 0 with best > 0: hot at every fraction
         700    (2^31-1,0,0,0) 2^31-1   the product needs 64 bits; hot at 1000000 ppm
         701    (0,0,2^31-2,0) 2^31-1   one short of it: cold at 1000000 ppm"""
    lengths = [9000, 5000]
    offs, total = R.layout(lengths)
    assert offs == [0, 12288] and total == 20480
    t = {k: np.zeros(total, dtype=np.int32) for k in "acgt"}
    depth = np.full(total, 10, dtype=np.int32)
    codes = np.full(total, 2, dtype=np.uint8)
    planted = {0: ((0, 0, 0, 6), 10), 100: ((5, 0, 0, 0), 8), 101: ((0, 0, 7, 1), 9), 200: ((0, 5, 0, 5), 10), 300: ((4, 4, 4, 4), 8),
               400: ((3, 0, 0, 0), 4), 402: ((0, 0, 2, 0), 2), 500: ((0, 3, 0, 0), 6), 502: ((0, 3, 0, 0), 7), 600: ((0, 0, 0, 4), 0),
               700: ((INT_MAX, 0, 0, 0), INT_MAX), 701: ((0, 0, INT_MAX - 1, 0), INT_MAX), 4095: ((0, 9, 0, 0), 9), 4096: ((0, 0, 9, 1), 10),
               8999: ((8, 0, 0, 0), 8), 9500: ((9, 9, 9, 9), 9), 12288: ((0, 0, 0, 5), 5), 17287: ((0, 6, 0, 0), 6), 17288: ((7, 0, 0, 0), 7)}
    for p, (n, d) in planted.items():
        for k, v in zip("acgt", n):
            t[k][p] = v
        depth[p] = d
    codes[0], codes[100], codes[4095], codes[4096] = 15, 8, 0, 238
    runs = [(3, 500000, ()), (3, 500001, ()), (3, 1000000, ()), (1, 0, ()), (2, 1000000, ()), (4, 0, ()),
            (3, 500000, ((50, 101), (101, 150), (4090, 4096), (4096, 4100))),          # windows that begin and end inside a tile, two touching
            (3, 500000, ((1000, 2000),)),                                              # a window that holds no site
            (3, 500000, ((101, 8999), (9000, 12289))),                                 # 8999 is outside, the padding inside
            (3, 500000, ((-5, 10 ** 9),))]
    return dict(lengths=lengths, depth=depth, codes=codes, runs=runs, **t)


def _site_random():
    lengths = [5000, 4097, 3, 20000]
    offs, total = R.layout(lengths)
    rng = np.random.default_rng(8)
    depth = rng.integers(0, 40, total).astype(np.int32)
    t = {k: (rng.integers(0, 12, total) * (rng.random(total) < 0.2)).astype(np.int32) for k in "acgt"}
    for a, n in zip(rng.integers(0, total, 60), rng.integers(1, 40, 60)):          # stretches where one allele is all the depth
        t["acgt"[int(a) % 4]][a:a + n] = depth[a:a + n]
    codes = rng.integers(0, 16, total).astype(np.uint8)
    return dict(lengths=lengths, depth=depth, codes=codes, **t,
                runs=[(1, 0, ()), (3, 500000, ()), (5, 900000, ()), (2, 250000, ((17, 4100), (4100, 9000), (16384, 16390), (20000, 30001))),
                      (30, 1000000, ())])


SITE_BUILDERS = {"planted": _site_planted, "random": _site_random}
SITE_NAMES = list(SITE_BUILDERS)
M31 = INT_MAX
SITES_EXPECTED = {
    # (contig, pos, ref, alt, nA, nC, nG, nT, depth)
    ("planted", 0): [(0, 0, 15, 8, 0, 0, 0, 6, 10), (0, 100, 8, 1, 5, 0, 0, 0, 8), (0, 101, 2, 4, 0, 0, 7, 1, 9), (0, 200, 2, 2, 0, 5, 0, 5, 10),
                     (0, 300, 2, 1, 4, 4, 4, 4, 8), (0, 400, 2, 1, 3, 0, 0, 0, 4), (0, 500, 2, 2, 0, 3, 0, 0, 6), (0, 600, 2, 8, 0, 0, 0, 4, 0),
                     (0, 700, 2, 1, M31, 0, 0, 0, M31), (0, 701, 2, 4, 0, 0, M31 - 1, 0, M31), (0, 4095, 0, 2, 0, 9, 0, 0, 9),
                     (0, 4096, 238, 4, 0, 0, 9, 1, 10), (0, 8999, 2, 1, 8, 0, 0, 0, 8), (1, 0, 2, 8, 0, 0, 0, 5, 5), (1, 4999, 2, 2, 0, 6, 0, 0, 6)],
    # at 1000000 ppm best must be the whole depth
    ("planted", 2): [(0, 600, 2, 8, 0, 0, 0, 4, 0), (0, 700, 2, 1, M31, 0, 0, 0, M31), (0, 4095, 0, 2, 0, 9, 0, 0, 9), (0, 8999, 2, 1, 8, 0, 0, 0, 8),
                     (1, 0, 2, 8, 0, 0, 0, 5, 5), (1, 4999, 2, 2, 0, 6, 0, 0, 6)],
    ("planted", 6): [(0, 100, 8, 1, 5, 0, 0, 0, 8), (0, 101, 2, 4, 0, 0, 7, 1, 9), (0, 4095, 0, 2, 0, 9, 0, 0, 9), (0, 4096, 238, 4, 0, 0, 9, 1, 10)],
    ("planted", 7): [],
}


@functools.lru_cache(maxsize=None)
def site_case(name):
    return SITE_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def want_sites(name, k):
    c = site_case(name)
    min_reads, frac, windows = c["runs"][k]
    return R.sites_of(*(c[key] for key in SITE_KEYS), c["lengths"], min_reads, frac, windows)


def site_rows(sites):
    """The rows of an ALLELE_SITE_DTYPE array as the statement's tuples."""
    return [(c, p, r, a, *n, d) for c, p, r, a, n, d in zip(sites["contig"].tolist(), sites["pos"].tolist(), sites["ref"].tolist(),
                                                            sites["alt"].tolist(), sites["n"].reshape(-1, 4).tolist(), sites["depth"].tolist())]
