"""Named inputs of the clip kernels (gci_bam_clip_*, gci_clip_sites_*), made with the record helpers of tests/cover_cases.py: the smallest
shapes at which the kernels can go wrong.  case(name) -> dict(stream, offs, lengths, ref_sel, runs); every run is (excl, min_mapq,
min_clip).  want(name, run) -> (left events, right events, counts, status word) from tests/clips_ref.py, computed once.  EXPECTED holds
the answers written by hand.  site_case(name) -> dict(lengths, left, right, depth, runs); every run is (min_reads, windows)."""
import functools

import numpy as np

import clips_ref as R
import cover_cases as CC
from cover_cases import CH, D, EQ, H, I, M, N, P, S, X, assemble, rec, to_heads
from gci_amd.formats import bam as bamfmt

EXCL = R.EXCL_DEFAULT


def _end_operations():
    cig = [[(M, 10)], [(S, 5), (M, 10)], [(M, 10), (S, 5)], [(H, 5), (S, 5), (M, 10), (S, 5), (H, 5)], [(S, 5), (H, 5), (M, 10)],
           [(S, 5), (D, 10), (S, 5)], [(S, 3)], [(S, 5), (S, 5)], [(I, 5), (M, 10)], [(M, 10), (N, 5)], [(15, 1)],
           [(S, 6), (I, 2), (S, 9), (EQ, 4), (X, 3), (H, 9), (P, 1), (H, 7)], []]
    return assemble([("c", 1000)], [rec(0, 100 + 10 * k, c) for k, c in enumerate(cig)],
                    runs=[(EXCL, 0, 5), (EXCL, 0, 6), (EXCL, 0, 10), (EXCL, 0, 11), (EXCL, 0, 1)])


# the answers by hand: (left events, right events, records counted); a record with R == 0 (3S, 5S5S, a lone code 15, no operation) is
# skipped without a word, 5I10M and 10M5N have no clip at their ends, and the last record's 6S and 7H stand alone (I and P are no clips)
EXPECTED = {
    ("end_operations", (EXCL, 0, 5)): ([(0, 110), (0, 130), (0, 140), (0, 150), (0, 210)], [(0, 129), (0, 139), (0, 159), (0, 216)], 9),
    ("end_operations", (EXCL, 0, 6)): ([(0, 130), (0, 140), (0, 210)], [(0, 139), (0, 216)], 9),
    ("end_operations", (EXCL, 0, 10)): ([(0, 130), (0, 140)], [(0, 139)], 9),
    ("end_operations", (EXCL, 0, 11)): ([], [], 9),
    # the example alignment of the SAM specification, section 1.1: r002 3S.., r003 5S.., the supplementary r003 6H5M
    ("sam_spec", (EXCL, 0, 3)): ([(0, 8), (0, 8), (0, 28)], [], 6),
    ("sam_spec", (EXCL, 0, 5)): ([(0, 8), (0, 28)], [], 6),
    ("sam_spec", (EXCL, 0, 6)): ([(0, 28)], [], 6),
    ("sam_spec", (EXCL | 0x800, 0, 3)): ([(0, 8), (0, 8)], [], 5),
    # clips inside the tag; without the tag, and behind a first CG tag that is no array: skipped; 65539 operations with 32769 M
    ("placeholder", (EXCL, 0, 8)): ([(0, 50), (0, 200), (0, 1000)], [(0, 59), (0, 1000 + 32769 - 1)], 3),
    ("ends", (EXCL, 0, 10)): ([(0, 90), (0, 91), (0, 99), (0, 99), (1, 0), (0, 50)], [(0, 99), (0, 99), (1, 0)], 7),
}


def _sam_spec():
    c = dict(CC._sam_spec())
    c["runs"] = [(EXCL, 0, 3), (EXCL, 0, 5), (EXCL, 0, 6), (EXCL | 0x800, 0, 3)]
    return c


def _chunks():
    """n_ops = 2048, 2049, 2050 and 4097: the trailing clip in a chunk of its own (2049, 4097), the last two operations in different
    chunks (2049, 4097) or together behind the boundary (2050)."""
    def fill(n, seed):
        m = [(o, l) for o, l in CC._pattern(2 * n, seed) if o != S][:n]
        assert len(m) == n
        return m
    recs = [rec(0, 100, [(S, 7)] + fill(CH - 2, 1) + [(S, 9)]),
            rec(0, 5000, [(S, 7)] + fill(CH - 1, 2) + [(S, 9)]),
            rec(0, 10000, [(H, 3), (S, 4)] + fill(CH - 2, 3) + [(S, 5), (H, 6)]),
            rec(0, 15000, [(S, 7)] + fill(2 * CH - 2, 4) + [(S, 8), (H, 9)]),
            rec(0, 25000, [(M, 1)] * CH + [(H, 12)]),
            rec(0, 30000, [(H, 12)] + [(M, 1)] * CH)]
    return assemble([("c", 60000)], recs, runs=[(EXCL, 0, 7), (EXCL, 0, 10), (EXCL, 0, 17), (EXCL, 0, 18)])


def _phases():
    """The operation array at byte phases 0 - 3 (the name's length), short and longer than a chunk."""
    recs = []
    for k, name in enumerate(["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg"]):
        recs += [rec(0, 50 * k, [(S, 7 + k)] + CC._pattern(70, 100 + k) + [(M, 2), (H, 8 + k)], name),
                 rec(0, 1000 * k + 3000, [(H, 2), (S, 9)] + CC._pattern(CH + 1, 200 + k) + [(M, 1), (S, 11)], name, l_seq=k)]
    return assemble([("c", 30000)], recs, runs=[(EXCL, 0, 9), (EXCL, 0, 12)])


def _placeholder():
    other = bamfmt.encode_aux([("NM", "i", 3), ("XS", "Z", "behind other tags"), ("XB", "B:C", [1, 2, 3])])
    small = [(S, 12), (M, 5), (D, 2), (M, 3), (H, 20)]
    cg_i = bamfmt.encode_aux([("CG", "B:i", [(l << 4) | o for o, l in small])])
    cg_z = bamfmt.encode_aux([("CG", "Z", "not an array")])
    big = [(S, 30)] + [(M, 1), (I, 1)] * 32768 + [(M, 1), (H, 40)]           # 65539 operations: encode_record writes the placeholder + CG:B,I
    recs = [rec(0, 50, [(S, 9), (N, 10)], l_seq=9, aux=other + cg_i),          # clips inside the tag
            rec(0, 100, [(S, 9), (N, 16)], l_seq=9, aux=other),                # the placeholder without the tag: skipped
            rec(0, 150, [(S, 9), (N, 16)], l_seq=9, aux=cg_z + cg_i),          # the FIRST CG tag counts: not an array, skipped
            rec(0, 200, [(S, 8), (M, 16)], l_seq=9, aux=cg_i),                 # not the placeholder: op0 is not <l_seq>S
            rec(0, 1000, big, l_seq=10, aux=other)]
    return assemble([("c", 300000)], recs, runs=[(EXCL, 0, 8), (EXCL, 0, 13), (EXCL, 0, 31)])


def _skip_rule():
    clipped = [(S, 20), (M, 20), (H, 20)]
    refs = [("a", 300), ("b", 300)]
    recs = [rec(0, 10 * k, clipped, flag=f) for k, f in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0x1, 0x10 | 0x80))]
    recs += [rec(0, 100, clipped, mapq=10), rec(0, 105, clipped, mapq=9), rec(0, 110, clipped, mapq=0)]
    recs += [rec(-1, 120, clipped), rec(1, 130, clipped), rec(2, 130, clipped), rec(0, -1, clipped), rec(0, 140, clipped, flag=0x100 | 0x400),
             rec(1, 5, [(S, 20), (M, 4), (9, 3)]), rec(0, 150, [(9, 9), (S, 20)], flag=0x4)]      # code 9 in skipped records is not looked at
    runs = [(EXCL, 0, 20), (EXCL & ~0x100, 0, 20), (EXCL | 0x800, 0, 20), (EXCL, 10, 20), (0, 0, 20), (EXCL, 0, 21)]
    return assemble(refs, recs, ref_sel=[0, -1], runs=runs)


def _ends():
    c10 = lambda m: [(S, 10), (M, m), (S, 10)]                                # noqa: E731
    recs = [rec(0, 90, c10(10)),                                             # the right site at length - 1: kept
            rec(0, 91, c10(10)),                                             # ... at length: dropped, not counted
            rec(0, 99, c10(1)),                                              # pos = length - 1
            rec(0, 99, c10(5)),
            rec(1, 0, c10(1)),                                               # a contig of one base
            rec(0, 2 ** 31 - 10, c10((1 << 28) - 1)),                        # pos + R overflows int32: both sites lie beyond the contig
            rec(0, 50, [(S, 10)] + [(N, (1 << 28) - 1)] * 9 + [(H, 10)])]     # R itself is past 2^31
    return assemble([("a", 100), ("b", 1)], recs, runs=[(EXCL, 0, 10)])


def _malformed(builder):
    def make():
        c = dict(builder())
        c["runs"] = [(EXCL, 0, 5)]
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
        lead = [(int(rng.choice([S, H])), int(rng.integers(0, 20))) for _ in range(int(rng.integers(0, 3)))]
        trail = [(int(rng.choice([S, H])), int(rng.integers(0, 20))) for _ in range(int(rng.integers(0, 3)))]
        body = CC._pattern(int(rng.integers(0, 12)), seed * 100000 + k)
        recs.append(rec(c, int(rng.integers(0, L)), lead + body + trail, "q%d" % k, int(rng.integers(0, 61)), flag, 250 + int(rng.integers(0, 9))))
    return assemble(refs, recs, runs=[(EXCL, 0, 8), (EXCL, 20, 1)])


BUILDERS = {
    "end_operations": _end_operations, "sam_spec": _sam_spec, "chunks": _chunks, "phases": _phases, "placeholder": _placeholder,
    "skip_rule": _skip_rule, "ends": _ends, "op9": _malformed(CC._op9), "cut_off": _malformed(CC._cut_off),
    "op9_then_cut_off": _malformed(CC._op9_then_cut_off),
    "records_0": lambda: assemble([("a", 100)], [], runs=[(EXCL, 0, 5)]),
    "records_1": lambda: assemble([("a", 100)], [rec(0, 3, [(S, 9), (M, 5), (H, 9)])], runs=[(EXCL, 0, 5)]), "records_63": lambda: _many(63, 12), "records_64": lambda: _many(64, 13), "records_65": lambda: _many(65, 14),
    "records_257": lambda: _many(257, 15), "records_4097": lambda: _many(4097, 16), "random_2000": lambda: _many(2000, 17),
}
NAMES = list(BUILDERS)
# the record the status word must name: in op9_then_cut_off record 1 holds code 10 alone, so its R is 0 and it is skipped like any
# record without reference bases -- the word names record 2, which runs past the stream
MALFORMED = {"op9": 3, "cut_off": 2, "op9_then_cut_off": 2}


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


# ---- sites -----------------------------------------------------------------------------------------------------------------------------
def _tracks(lengths, seed=0, noise=0):
    offs, total = R.layout(lengths)
    rng = np.random.default_rng(seed)
    left, right = np.zeros(total, dtype=np.int32), np.zeros(total, dtype=np.int32)
    depth = rng.integers(0, 60, total).astype(np.int32)
    if noise:
        at = rng.integers(0, total, noise)
        left[at] = rng.integers(0, 6, noise)
        at = rng.integers(0, total, noise)
        right[at] = rng.integers(0, 6, noise)
    return offs, total, left, right, depth


def _site_small():
    """A layout smaller than a tile; the padding behind the contig holds values that must never become sites."""
    offs, total, left, right, depth = _tracks([100])
    left[0], right[99], left[50], right[50], left[60] = 3, 4, 2, 2, 3
    left[100:] = 9
    return dict(lengths=[100], left=left, right=right, depth=depth,
                runs=[(3, ()), (4, ()), (5, ()), (2, ()), (3, ((0, 1),)), (3, ((1, 99),)), (3, ((10, 10),)), (3, ((99, 4096),)), (1, ((-5, 10 ** 9),))])


def _site_tiles():
    """Contig lengths that are no multiple of 4 and one of a single base; sites at element 0, 4095, 4096 and the last element; every
    element of a tile a site; left only, right only and both; windows that begin and end mid-tile, empty, of one element, on a later
    contig, over padding."""
    lengths = [8195, 1, 4096, 5]
    offs, total, left, right, depth = _tracks(lengths, 1)
    for p, l, r in ((0, 3, 0), (4095, 0, 3), (4096, 3, 3), (8194, 4, 0), (5000, 2, 0), (5001, 0, 4), (12288, 3, 0), (20484, 0, 3)):
        left[p], right[p] = l, r
    left[16384:20480] = 3                              # contig 2: every element of its tile
    right[16384:20480:2] = 5
    for c, L in enumerate(lengths):                    # padding
        left[offs[c] + L:offs[c] + (L + 4095) // 4096 * 4096] = 9
    runs = [(3, ()), (4, ()), (5, ()), (6, ()), (3, ((10, 10),)), (3, ((4095, 4096),)), (3, ((100, 5000), (5000, 9000))), (3, ((4096, 4097), (8194, 8195))),
            (3, ((12288, 12289),)), (3, ((16384 + 100, 16384 + 200), (20480, 20485))), (3, ((8000, 12288),)), (3, ((3, 3), (4000, 4200), (4200, 4200), (12000, 24576))),
            (4, ((5000, 5002),))]
    return dict(lengths=lengths, left=left, right=right, depth=depth, runs=runs)


def _site_none():
    offs, total, left, right, depth = _tracks([5000])
    left[5000:] = 7
    return dict(lengths=[5000], left=left, right=right, depth=depth, runs=[(1, ()), (3, ((0, 8192),))])


def _site_random():
    lengths = [5000, 4097, 3, 20000]
    offs, total, left, right, depth = _tracks(lengths, 5, noise=300)
    return dict(lengths=lengths, left=left, right=right, depth=depth,
                runs=[(1, ()), (3, ()), (5, ()), (2, ((17, 4100), (4100, 9000), (16384, 16390), (20000, 30001))), (6, ())])


SITE_BUILDERS = {"small": _site_small, "tiles": _site_tiles, "none": _site_none, "random": _site_random}
SITE_NAMES = list(SITE_BUILDERS)


@functools.lru_cache(maxsize=None)
def site_case(name):
    return SITE_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def want_sites(name, k, with_depth=True):
    c = site_case(name)
    min_reads, windows = c["runs"][k]
    return R.sites_of(c["left"], c["right"], c["depth"] if with_depth else None, c["lengths"], min_reads, windows)
