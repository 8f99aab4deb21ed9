"""Named inputs of the indel kernels (gci_bam_indel_*, gci_indel_sites_*), made with the record helpers of tests/cover_cases.py: the
smallest shapes at which the kernels can go wrong.  case(name) -> dict(stream, offs, lengths, ref_sel, runs); every run is (excl,
min_mapq, min_len).  want(name, run) -> (deletions, insertions, counts, status word) from tests/indels_ref.py, computed once.  EXPECTED
holds the answers written by hand.  site_case(name) -> dict(lengths, del, ins, depth, runs); every run is (min_reads, windows)."""
import functools

import numpy as np

import clips_cases as CLIPS
import cover_cases as CC
import indels_ref as R
from cover_cases import CH, D, EQ, H, I, M, N, P, S, X, assemble, rec, to_heads      # noqa: F401
from gci_amd.formats import bam as bamfmt

EXCL = R.EXCL_DEFAULT


def _thresholds():
    """D and I one base short of min_len and at it; 5D5D is two deletions of 5, never one of 10; N, P, S, H and operations of length
    zero are no events."""
    recs = [rec(0, 100, [(M, 10), (D, 9), (M, 10), (D, 10), (M, 10), (I, 9), (M, 5), (I, 10), (M, 5)]),
            rec(0, 300, [(M, 5), (D, 5), (D, 5), (M, 5)]),
            rec(0, 400, [(S, 30), (M, 5), (N, 20), (M, 5), (P, 12), (EQ, 3), (X, 2), (D, 0), (I, 0), (M, 3), (H, 30)]),
            rec(0, 500, [])]
    return assemble([("c", 1000)], recs, runs=[(EXCL, 0, 10), (EXCL, 0, 11), (EXCL, 0, 5), (EXCL, 0, 6), (EXCL, 0, 1)])


# the answers by hand: (deletions, insertions, records counted)
EXPECTED = {
    # 10M 9D 10M 10D 10M 9I 5M 10I 5M at 100: the D at 110 and 129, the I behind base 148 and 153; 5M 5D 5D 5M at 300: D at 305 and 310
    ("thresholds", (EXCL, 0, 10)): ([(0, 129, 138)], [(0, 153)], 4),
    ("thresholds", (EXCL, 0, 11)): ([], [], 4),
    ("thresholds", (EXCL, 0, 5)): ([(0, 110, 118), (0, 129, 138), (0, 305, 309), (0, 310, 314)], [(0, 148), (0, 153)], 4),
    ("thresholds", (EXCL, 0, 6)): ([(0, 110, 118), (0, 129, 138)], [(0, 148), (0, 153)], 4),
    # the example alignment of the SAM specification, section 1.1: r001 8M2I4M1D3M at 0-based 6 (I behind base 13, D over base 18),
    # r002 3S6M1P1I4M at 0-based 8 (I behind base 13)
    ("sam_spec", (EXCL, 0, 1)): ([(0, 18, 18)], [(0, 13), (0, 13)], 6),
    ("sam_spec", (EXCL, 0, 2)): ([], [(0, 13)], 6),
    # 5M 12D 3M 15I 4M inside the tag at 50; without the tag, behind a first CG tag that is no array, and 8S16M: nothing
    ("placeholder", (EXCL, 0, 12)): ([(0, 55, 66)], [(0, 69)], 5),
    ("placeholder", (EXCL, 0, 13)): ([], [(0, 69)], 5),
    ("ends", (EXCL, 0, 3)): ([(0, 99, 99), (1, 0, 0), (0, 50, 52)], [(0, 0), (0, 99), (1, 0), (1, 0)], 10),
    ("ends", (EXCL, 0, 4)): ([(0, 99, 99)], [], 10),
}


def _sam_spec():
    c = dict(CC._sam_spec())
    c["runs"] = [(EXCL, 0, 1), (EXCL, 0, 2), (EXCL | 0x800, 0, 1)]
    return c


def _wave_rounds():
    """Events at operation 63 and 64 of a chunk (the last lane of a round, the first of the next), 64 events in one round, and events
    of both kinds alternating across three rounds."""
    recs = [rec(0, 100, [(M, 1)] * 63 + [(D, 7), (I, 7)] + [(M, 1)] * 3),
            rec(0, 1000, [(M, 1)] * 63 + [(I, 7), (D, 7)] + [(M, 1)] * 3),
            rec(0, 2000, [(D, 3)] * 64 + [(M, 1)]),
            rec(0, 3000, [(I, 3)] * 64 + [(M, 1)]),
            rec(0, 4000, [(M, 2)] + [(I, 3), (D, 4)] * 70)]
    return assemble([("c", 10000)], recs, runs=[(EXCL, 0, 3), (EXCL, 0, 4), (EXCL, 0, 7), (EXCL, 0, 8)])


def _chunks():
    """n_ops = 2048, 2049, 2050 and 4097: a long D as the last operation of chunk 0, as the first of chunk 1, a long I directly behind
    the boundary; the filler holds short D, I and N, so every position behind a boundary needs the carry of the chunks in front."""
    fill = CC._pattern
    recs = [rec(0, 100, fill(CH - 1, 1) + [(D, 20)]),
            rec(0, 10000, fill(CH - 1, 2) + [(D, 20), (I, 20)]),
            rec(0, 20000, fill(CH, 3) + [(D, 20), (M, 4)]),
            rec(0, 30000, fill(CH - 1, 4) + [(D, 20), (D, 21)] + fill(CH - 2, 5) + [(I, 22), (D, 23)]),
            rec(0, 45000, [(M, 1)] * CH + [(I, 20)] + [(M, 1)] * 3)]
    return assemble([("c", 100000)], recs, runs=[(EXCL, 0, 20), (EXCL, 0, 21), (EXCL, 0, 23), (EXCL, 0, 24), (EXCL, 0, 1), (EXCL, 0, 3)])


def _phases():
    """The operation array at byte phases 0 - 3 (the name's length), short and longer than a chunk."""
    recs = []
    for k, name in enumerate(["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg"]):
        recs += [rec(0, 50 * k, CC._pattern(70, 100 + k) + [(D, 9), (M, 2), (I, 9 + k)], name),
                 rec(0, 1000 * k + 3000, [(M, 1), (I, 9)] + CC._pattern(CH + 1, 200 + k) + [(D, 9 + k), (M, 1)], name, l_seq=k)]
    return assemble([("c", 30000)], recs, runs=[(EXCL, 0, 9), (EXCL, 0, 12), (EXCL, 0, 2)])


def _placeholder():
    other = bamfmt.encode_aux([("NM", "i", 3), ("XS", "Z", "behind other tags"), ("XB", "B:C", [1, 2, 3])])
    small = [(M, 5), (D, 12), (M, 3), (I, 15), (M, 4)]
    cg_i = bamfmt.encode_aux([("CG", "B:i", [(l << 4) | o for o, l in small])])
    cg_z = bamfmt.encode_aux([("CG", "Z", "not an array")])
    big = CLIPS.case("placeholder")                     # its last record: 30S (1M 1I) x 32768 1M 40H at 1000, 65539 operations behind CG:B,I
    recs = [rec(0, 50, [(S, 9), (N, 24)], l_seq=9, aux=other + cg_i),          # I and D inside the tag
            rec(0, 100, [(S, 9), (N, 24)], l_seq=9, aux=other),                # the placeholder without the tag: counted, no event
            rec(0, 150, [(S, 9), (N, 24)], l_seq=9, aux=cg_z + cg_i),          # the FIRST CG tag counts: no array, no event
            rec(0, 200, [(S, 8), (M, 16)], l_seq=9, aux=cg_i),                 # not the placeholder: op0 is not <l_seq>S
            big["stream"][int(big["offs"][-1]):].tobytes()]
    return assemble([("c", 300000)], recs, runs=[(EXCL, 0, 12), (EXCL, 0, 13), (EXCL, 0, 1), (EXCL, 0, 2)])


def _skip_rule():
    body = [(M, 20), (D, 20), (M, 20), (I, 20), (M, 5)]
    refs = [("a", 300), ("b", 300)]
    recs = [rec(0, 10 * k, body, flag=f) for k, f in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0x1, 0x10 | 0x80))]
    recs += [rec(0, 100, body, mapq=10), rec(0, 105, body, mapq=9), rec(0, 110, body, mapq=0)]
    recs += [rec(-1, 120, body), rec(1, 130, body), rec(2, 130, body), rec(0, -1, body), rec(0, 140, body, flag=0x100 | 0x400),
             rec(1, 5, [(D, 20), (M, 4), (9, 3)]), rec(-1, 150, [(9, 9), (D, 20)], flag=0x4)]     # code 9 in skipped records is not looked at
    runs = [(EXCL, 0, 20), (EXCL & ~0x100, 0, 20), (EXCL | 0x800, 0, 20), (EXCL, 10, 20), (0, 0, 20), (EXCL, 0, 21)]
    return assemble(refs, recs, ref_sel=[0, -1], runs=runs)


def _ends():
    recs = [rec(0, 0, [(S, 5), (I, 3), (M, 10)]),                            # at = 0: the site is base 0
            rec(0, 90, [(M, 10), (I, 3)]),                                   # I as the last operation with at = L: the site L - 1
            rec(0, 91, [(M, 10), (I, 3)]),                                   # at - 1 = L: dropped, not counted
            rec(0, 95, [(M, 4), (D, 10), (M, 3)]),                           # D starting at L - 1: clamped to one base
            rec(0, 96, [(M, 4), (D, 10)]),                                   # D starting at L: dropped, not counted
            rec(1, 0, [(M, 1), (I, 3)]), rec(1, 0, [(D, 3), (M, 1)]), rec(1, 0, [(I, 3), (M, 1)]),      # a contig of one base
            rec(0, 2 ** 31 - 10, [(M, (1 << 28) - 1), (D, 5), (I, 5)]),      # pos + reference length overflows int32: beyond the contig
            rec(0, 50, [(D, 3)] + [(N, (1 << 28) - 1)] * 9 + [(D, 3), (I, 3), (M, 1)])]      # the carry itself is past 2^31
    return assemble([("a", 100), ("b", 1)], recs, runs=[(EXCL, 0, 3), (EXCL, 0, 4)])


def _malformed(builder):
    def make():
        c = dict(builder())
        c["runs"] = [(EXCL, 0, 1)]
        return c
    return make


def _many(n_rec, seed):
    rng = np.random.default_rng(seed)
    refs = [("x", 5000), ("y", 4097), ("z", 12000)]
    recs = []
    for k in range(n_rec):
        c = int(rng.integers(-1, 3))
        L = refs[c][1] if c >= 0 else 1000
        flag = int(rng.choice([0, 0, 0, 0x10, 0x800, 0x4, 0x100, 0x200, 0x400, 0x1 | 0x40]))
        body = [(o, l * 3 if o in (D, I) else l) for o, l in CC._pattern(int(rng.integers(0, 14)), seed * 100000 + k)]
        recs.append(rec(c, int(rng.integers(0, L)), body, "q%d" % k, int(rng.integers(0, 61)), flag, int(rng.integers(0, 9))))
    return assemble(refs, recs, runs=[(EXCL, 0, 6), (EXCL, 20, 1)])


BUILDERS = {
    "thresholds": _thresholds, "sam_spec": _sam_spec, "wave_rounds": _wave_rounds, "chunks": _chunks, "phases": _phases,
    "placeholder": _placeholder, "skip_rule": _skip_rule, "ends": _ends, "op9": _malformed(CC._op9), "cut_off": _malformed(CC._cut_off),
    "op9_then_cut_off": _malformed(CC._op9_then_cut_off),
    "records_0": lambda: assemble([("a", 100)], [], runs=[(EXCL, 0, 5)]),
    "records_1": lambda: assemble([("a", 100)], [rec(0, 3, [(M, 5), (D, 6), (M, 5), (I, 7), (M, 2)])], runs=[(EXCL, 0, 5)]),
    "records_63": lambda: _many(63, 12), "records_64": lambda: _many(64, 13), "records_65": lambda: _many(65, 14),
    "records_257": lambda: _many(257, 15), "records_4097": lambda: _many(4097, 16), "random_2000": lambda: _many(2000, 17),
}
NAMES = list(BUILDERS)
# the record the status word must name: a counted record with a code 9 - 15 is malformed whatever else it holds, so in op9_then_cut_off
# the word names record 1 (code 10 alone), not record 2, which runs past the stream
MALFORMED = {"op9": 3, "cut_off": 2, "op9_then_cut_off": 1}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def heads(name):
    c = case(name)
    return to_heads(c["stream"], c["offs"])


@functools.lru_cache(maxsize=None)
def want(name, run):
    c = case(name)
    return R.stream_events(c["stream"], c["offs"], c["lengths"], c["ref_sel"], *run)


def pairs():
    return [(name, run) for name in NAMES for run in case(name)["runs"]]


# ---- sites: tracks written by hand ---------------------------------------------------------------------------------------------------
def _tracks(lengths, seed=0):
    offs, total = R.layout(lengths)
    rng = np.random.default_rng(seed)
    return offs, total, np.zeros(total, dtype=np.int32), np.zeros(total, dtype=np.int32), rng.integers(0, 60, total).astype(np.int32)


def _site_runs():
    """Runs of 1, 63, 64, 65 and 9000 elements, one across a tile edge (4095 - 4096), one from a tile's first element; the maxima at a
    run's first and at its last element; windows that cut a run at their end, and two touching windows that cut one in two."""
    offs, total, dele, ins, depth = _tracks([20000], 1)
    for a, n in ((100, 1), (200, 63), (300, 64), (1024, 64), (500, 65), (4090, 10), (8192, 3)):
        dele[a:a + n] = 3
    ins[10000:19000] = 4                               # 9000 elements over three tile edges, to the window's end below
    dele[300], depth[300] = 9, 99                      # maxima at the first element
    ins[564], depth[564] = 8, 98                       # ... and at the last
    dele[10000], ins[18999], depth[18999] = 7, 11, 97
    runs = [(3, ()), (4, ()), (5, ()), (3, ((0, 12000),)), (3, ((0, 12000), (12000, 20000))), (3, ((4096, 4097),)), (3, ((4093, 4099),)),
            (3, ((250, 330), (330, 340), (500, 565), (1030, 1031))), (3, ((0, 4096), (4096, 8193))), (3, ((-5, 10 ** 9),)), (12, ())]
    return dict(lengths=[20000], dele=dele, ins=ins, depth=depth, runs=runs)


def _site_contigs():
    """A run to the last base of a contig that fills its tiles, the next contig hot from its first base: two sites, also inside one
    window over both; a run into the padding behind a contig ends with the contig; a run in the padding only is none."""
    lengths = [4096, 5000, 100, 1]
    offs, total, dele, ins, depth = _tracks(lengths, 2)
    assert offs == [0, 4096, 12288, 16384]
    dele[4090:4100] = 3                                # contig 0's last six bases, contig 1's first four
    ins[4096 + 4990:4096 + 5100] = 5                   # contig 1's last ten bases, then padding
    ins[4096 + 6000:4096 + 6010] = 9                   # padding only
    dele[12288 + 95:12288 + 300] = 4                   # contig 2's last five bases, then padding
    dele[16384:16390] = 6                              # the contig of one base, then padding
    runs = [(3, ()), (3, ((-5, 10 ** 9),)), (3, ((4000, 4098),)), (5, ((0, 20480),)), (4, ((12288 + 96, 12288 + 99), (12288 + 99, 16385))), (7, ())]
    return dict(lengths=lengths, dele=dele, ins=ins, depth=depth, runs=runs)


def _site_either():
    """Hot by del only, by ins only, by either on alternating bases: one run each; values of min_reads - 1 break a run."""
    offs, total, dele, ins, depth = _tracks([3000], 3)
    dele[10:20] = 3
    ins[30:40] = 3
    dele[50:70:2] = 3
    ins[51:70:2] = 3
    dele[100:110] = [3, 3, 2, 3, 3, 2, 2, 3, 4, 3]     # min_reads 3: 100-101, 103-104, 107-109; min_reads 2: one run; min_reads 4: one base
    ins[100:110] = [0, 0, 1, 0, 0, 0, 2, 0, 0, 0]
    return dict(lengths=[3000], dele=dele, ins=ins, depth=depth, runs=[(3, ()), (2, ()), (4, ()), (1, ()), (3, ((15, 35), (55, 56), (104, 108)))])


def _site_none():
    offs, total, dele, ins, depth = _tracks([5000])
    dele[5000:] = 7                                    # padding
    ins[:5000] = 2
    return dict(lengths=[5000], dele=dele, ins=ins, depth=depth, runs=[(3, ()), (3, ((0, 8192),)), (3, ((10, 10),))])


def _site_random():
    lengths = [5000, 4097, 3, 20000]
    offs, total, dele, ins, depth = _tracks(lengths, 5)
    rng = np.random.default_rng(6)
    for track in (dele, ins):
        for a, n, v in zip(rng.integers(0, total, 200), rng.integers(1, 90, 200), rng.integers(1, 6, 200)):
            track[a:a + n] = np.maximum(track[a:a + n], v)
    return dict(lengths=lengths, dele=dele, ins=ins, depth=depth,
                runs=[(1, ()), (3, ()), (5, ()), (2, ((17, 4100), (4100, 9000), (16384, 16390), (20000, 30001))), (6, ())])


SITE_BUILDERS = {"runs": _site_runs, "contigs": _site_contigs, "either": _site_either, "none": _site_none, "random": _site_random}
SITE_NAMES = list(SITE_BUILDERS)
# by hand: (contig, start, end, del, ins) of the first run of some site cases
SITES_EXPECTED = {
    ("contigs", 0): [(0, 4090, 4096, 3, 0), (1, 0, 4, 3, 0), (1, 4990, 5000, 0, 5), (2, 95, 100, 4, 0), (3, 0, 1, 6, 0)],
    ("contigs", 1): [(0, 4090, 4096, 3, 0), (1, 0, 4, 3, 0), (1, 4990, 5000, 0, 5), (2, 95, 100, 4, 0), (3, 0, 1, 6, 0)],
    ("contigs", 4): [(2, 96, 99, 4, 0), (2, 99, 100, 4, 0), (3, 0, 1, 6, 0)],
    ("either", 0): [(0, 10, 20, 3, 0), (0, 30, 40, 0, 3), (0, 50, 70, 3, 3), (0, 100, 102, 3, 0), (0, 103, 105, 3, 0), (0, 107, 110, 4, 0)],
    ("either", 1): [(0, 10, 20, 3, 0), (0, 30, 40, 0, 3), (0, 50, 70, 3, 3), (0, 100, 110, 4, 2)],
    ("either", 2): [(0, 108, 109, 4, 0)],
    ("runs", 4): [(0, 100, 101, 3, 0), (0, 200, 263, 3, 0), (0, 300, 364, 9, 0), (0, 500, 565, 3, 8), (0, 1024, 1088, 3, 0), (0, 4090, 4100, 3, 0),
                  (0, 8192, 8195, 3, 0), (0, 10000, 12000, 7, 4), (0, 12000, 19000, 0, 11)],
    ("none", 0): [],
}


@functools.lru_cache(maxsize=None)
def site_case(name):
    return SITE_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def want_sites(name, k, with_depth=True):
    c = site_case(name)
    min_reads, windows = c["runs"][k]
    return R.sites_of(c["dele"], c["ins"], c["depth"] if with_depth else None, c["lengths"], min_reads, windows)
