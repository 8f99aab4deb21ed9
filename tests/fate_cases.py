"""Named inputs of gci_bam_fate / gci_bam_cover_size_sel: a header plus records made with cover_cases.rec / assemble, the smallest
shapes at which the kernels can go wrong.  case(name) -> dict(stream, offs, lengths, ref_sel, runs); every run is (map_qual, cp, ip).
want(name, run) -> (class per record, records per class, status word) from tests/fate_ref.py, computed once."""
import functools

import numpy as np

import cover_cases as C
import fate_ref as F
from cover_cases import CH, D, EQ, I, M, N, P, S, X, assemble, rec
from gci_amd.formats import bam as bamfmt

DEFAULT = (30, 0.1, 0.9)                               # -mq, -cp, -ip of the command line
REFS = [("a", 300000), ("b", 300)]
SEL = [0, -1]                                          # contig b is not selected


def nm(v, t="i"):
    return bamfmt.encode_aux([("NM", t, v)])


def _one_per_class():
    return assemble(REFS, [
        rec(1, 5, [(M, 20)], aux=nm(0)),                                                               # none: contig not selected
        rec(0, 10, [(M, 20)], flag=0x100, aux=nm(0)), rec(0, 20, [(M, 20)], flag=0x800, aux=nm(0)), rec(0, 30, [(M, 20)], mapq=29, aux=nm(0)),
        rec(0, 40, [(S, 5), (M, 10)], aux=nm(0)), rec(0, 50, [(M, 10)], aux=nm(5)), rec(0, 60, [(M, 20)], aux=nm(0)),
        rec(0, 70, [(M, 20)], mapq=30, aux=nm(0))], ref_sel=SEL, runs=[DEFAULT])


def _several_tests():
    """The first failing test names the class."""
    return assemble(REFS, [
        rec(0, 10, [(M, 20)], flag=0x900, aux=nm(0)),                                                  # secondary
        rec(0, 20, [(S, 30), (M, 10)], mapq=3),                                                        # low MAPQ, clipped, no NM: mapq, no status
        rec(0, 30, [(S, 30), (M, 10)], aux=nm(9)),                                                     # clipped, low identity: clip
        rec(0, 40, [(M, 20)], flag=0x4 | 0x100, aux=nm(0)),                                            # none
        rec(0, 50, [(M, 20)], flag=0x800, mapq=0),                                                     # supplementary (no NM: never looked for)
        rec(1, 60, [(S, 30), (M, 10)], flag=0x100, mapq=0)], ref_sel=SEL, runs=[DEFAULT])             # none


def _on_the_thresholds():
    return assemble(REFS, [
        rec(0, 10, [(S, 1), (M, 9)], aux=nm(0)),                                                       # 0.1 <= 0.1: not clip
        rec(0, 20, [(S, 2), (M, 17)], aux=nm(0)),                                                      # 2 / 19: clip
        rec(0, 30, [(M, 10)], aux=nm(1)),                                                              # 0.9 >= 0.9: kept
        rec(0, 40, [(M, 100000)], aux=nm(10000)), rec(0, 50, [(M, 100000)], aux=nm(10001)),            # inside ratio_cmp's f32 band
        rec(0, 60, [(S, 10000), (EQ, 90000)], aux=nm(0)), rec(0, 70, [(S, 10001), (X, 89999)], aux=nm(0))], ref_sel=SEL, runs=[DEFAULT])


def _pieces(total):
    out = []
    while total > 0:
        out.append(min(total, (1 << 28) - 1))
        total -= out[-1]
    return out


BAND_SHAPES = [  # (S, M, I, D, mismatches under M): small exact fractions, denominators beyond 2^24 and beyond 2^30, quotients of 0 and 1
    (10, 90, 0, 0, 9), (11, 89, 0, 0, 10), (1, 9, 0, 0, 1), (0, 100, 0, 0, 0), (333, 2667, 30, 0, 270), (1801, 16203, 7, 9, 1620),
    (1677722, 15099494, 3, 5, 1509949), (16777217, 150994943, 11, 13, 15099494), (99999, 900001, 0, 0, 90000), (2, 17, 1, 0, 2),
    (214748364, 1932735283, 0, 0, 193273528)]


def _threshold_band():
    """Every record's f64 quotient as the threshold itself, one ulp either side of it, and +- 1e-7 .. 1e-3: on, just inside and just
    outside the band in which ratio_cmp falls back to the f64 division (the construction of
    test_filter_thresholds_at_and_around_every_quotient)."""
    recs, cands = [], ([], [])
    for k, (s, m, i, d, mm) in enumerate(BAND_SHAPES):
        ops = [(S, p) for p in _pieces(s)] + [((M, EQ, X)[(k + j) % 3], p) for j, p in enumerate(_pieces(m))] + [(I, i)] * bool(i) + [(D, d)] * bool(d)
        recs.append(rec(0, 10 + k, ops, aux=nm(mm + i + d, "I")))
        for which, q in enumerate((s / (m + i + s), (m - mm) / (m + i + d))):
            c = [q, np.nextafter(q, np.inf), np.nextafter(q, -np.inf)]
            for e in (1e-7, 1e-5, 9.9e-5, 1.01e-4, 1e-3):
                c += [q + e, q - e]
            cands[which].extend(float(x) for x in c)
    runs = [(30, c, 0.5) for c in sorted(set(cands[0]))] + [(30, 0.75, c) for c in sorted(set(cands[1]))]
    return assemble([("a", 2_000_000_000), ("b", 300)], recs, ref_sel=SEL, runs=runs)


def _nm_forms():
    z, b = ("XS", "Z", "a string in front"), ("XB", "B:S", [1, 2, 3, 4, 5])
    enc = bamfmt.encode_aux
    return assemble(REFS, [rec(0, 10 * k, [(M, 100)], aux=nm(v, t)) for k, (t, v) in enumerate(
        [("c", 10), ("c", 11), ("C", 10), ("C", 200), ("s", 10), ("s", 300), ("S", 10), ("S", 40000), ("i", 10), ("i", 70000), ("I", 10), ("I", 11),
         ("c", -1), ("s", -300), ("i", -70000)])] + [
        rec(0, 200, [(M, 100)], aux=enc([z, ("NM", "C", 10)])), rec(0, 210, [(M, 100)], aux=enc([z, b, ("NM", "C", 11)])),
        rec(0, 220, [(M, 100)], aux=enc([b, ("NM", "s", 10), z])),
        rec(0, 230, [(M, 100)], aux=enc([("NM", "C", 0), ("NM", "C", 50)])), rec(0, 240, [(M, 100)], aux=enc([("NM", "C", 50), ("NM", "C", 0)])),
        rec(0, 250, [(M, 100)], aux=enc([("Nm", "C", 50), ("MN", "C", 50), ("NM", "C", 0)]))], ref_sel=SEL, runs=[DEFAULT])


def _pattern(n, seed):
    rng = np.random.default_rng(seed)
    ops = rng.choice([M] * 14 + [I, D, N, EQ, X, S, P], size=n)
    lens = rng.integers(0, 40, size=n)
    return [(int(o), int(l)) for o, l in zip(ops, lens)]


def _nm_for(cigar, mm=0):
    return nm(sum(l for o, l in cigar if o in (I, D)) + mm, "I")


def _chunks():
    """CIGARs of CH - 1, CH, CH + 1 and 2 CH + 1 operations: a record whose only soft clip is its last operation (for 2 CH + 1 alone in
    chunk 2) and alone makes it `clip`, its twin without the clip, and patterns whose sums cross the 64-lane rounds."""
    recs = []
    for k, n in enumerate((CH - 1, CH, CH + 1, 2 * CH + 1)):
        recs += [rec(0, 1000 * k, [(M, 1)] * (n - 1) + [(S, n)], aux=nm(0)), rec(0, 1000 * k + 1, [(M, 1)] * n, aux=nm(0))]
        for j, mm in enumerate((0, 0, 8000)):
            pat = _pattern(n, 10 * n + j)
            recs.append(rec(0, 1000 * k + 10 + j, pat, aux=_nm_for(pat, mm)))
    recs += [rec(0, 9000, [(M, 3)] * 63 + [(S, 40)] + [(M, 3)] * 64 + [(I, 2)] + [(M, 1)] * 10, aux=nm(2)),       # at the 64-lane rounds
             rec(0, 9100, [(M, 3)] * 64 + [(S, 50)], aux=nm(0)), rec(0, 9200, [(M, 3)] * 64 + [(S, 5)], aux=nm(0))]
    return assemble(REFS, recs, ref_sel=SEL, runs=[DEFAULT, (30, 0.5, 0.9)])


def _phases():
    """Read names of 0 to 7 bytes: the CIGAR begins at every byte phase (the stream's own phase varies with the records too)."""
    recs = []
    for k, name in enumerate(["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg"]):
        a, b = _pattern(70, 100 + k), _pattern(CH + 1, 200 + k)
        recs += [rec(0, 50 * k, a, name, aux=_nm_for(a)), rec(0, 1000 * k + 3000, b, name, l_seq=k, aux=_nm_for(b))]
    return assemble(REFS, recs, ref_sel=SEL, runs=[DEFAULT, (30, 0.045, 0.905)])


def _placeholder():
    big = [(M, 9), (I, 1), (EQ, 9), (D, 1)] * 16384 + [(M, 5)]                                         # 65537 operations
    small = [(M, 50), (D, 1), (M, 30), (N, 4), (M, 20)]
    other = bamfmt.encode_aux([("XS", "Z", "behind other tags"), ("NM", "i", 1), ("XB", "B:C", [1, 2, 3])])
    cg = lambda t: bamfmt.encode_aux([("CG", t, [(l << 4) | o for o, l in small])])                    # noqa: E731
    cg_z = bamfmt.encode_aux([("CG", "Z", "not an array")])
    return assemble(REFS, [
        rec(0, 1000, big, l_seq=10, aux=nm(2 * 16384)),                                                # encode_record: <l_seq>S<n>N + CG:B,I
        rec(0, 1100, big, l_seq=10, aux=nm(2 * 16384 + 40000)),                                        # ... of low identity
        rec(0, 50, [(S, 9), (N, 105)], l_seq=9, aux=other + cg("B:I")), rec(0, 60, [(S, 9), (N, 105)], l_seq=9, aux=other + cg("B:i")),   # kept
        rec(0, 100, [(S, 9), (N, 105)], l_seq=9, aux=other),                                           # the placeholder without a tag: clip
        rec(0, 150, [(S, 9), (N, 105)], l_seq=9, aux=other + cg_z + cg("B:I")),                        # the FIRST CG tag counts: clip
        rec(0, 200, [(S, 8), (M, 160)], l_seq=9, aux=other + cg("B:I"))], ref_sel=SEL, runs=[DEFAULT])  # op0 is not <l_seq>S: its own CIGAR


def _none_op9():
    """Records of class `none` -- unselected contig, refID -1, pos -1, refID beyond the table, unmapped, whatever else their flags and
    MAPQ say -- whose CIGARs hold code 9 and that carry no NM: not looked at."""
    return assemble(REFS, [rec(1, 5, [(M, 4), (9, 3)]), rec(-1, 5, [(9, 9)]), rec(0, -1, [(9, 9)]), rec(2, 5, [(9, 9)]), rec(0, 5, [(9, 9)], flag=0x4),
                           rec(0, 10, [(M, 4)], aux=nm(0)), rec(1, 20, [(9, 3)], flag=0x100), rec(-1, 30, [(9, 3)], flag=0x800), rec(0, -1, [(9, 3)], mapq=1)],
                    ref_sel=SEL, runs=[DEFAULT])


def _errors(recs, run=DEFAULT, cut=0):
    return assemble(REFS, [rec(0, 5, [(M, 9)], aux=nm(0))] + recs + [rec(0, 900, [(M, 9)], aux=nm(0))], ref_sel=SEL, runs=[run], cut=cut)


def _random(n_rec, seed):
    rng = np.random.default_rng(seed)
    refs = [("x", 5000), ("y", 4097), ("z", 12000)]
    recs = []
    for k in range(n_rec):
        c = int(rng.integers(-1, 3))
        L = refs[c][1] if c >= 0 else 1000
        flag = int(rng.choice([0, 0, 0, 0, 0x10, 0x10, 0x1 | 0x40, 0x100, 0x800, 0x4, 0x900, 0x400, 0x200]))
        mapq = int(rng.choice([60, 60, 60, 50, 31, 30, 29, 3]))
        body = [(int(o), int(l)) for o, l in zip(rng.choice([M, M, M, M, EQ, X, I, D, N, P], size=int(rng.integers(1, 40))), rng.integers(1, 30, size=40))]
        clip = [(S, int(rng.integers(1, 25)))] if rng.random() < 0.3 else []
        cigar = clip + body + ([(S, int(rng.integers(1, 5)))] if rng.random() < 0.1 else [])
        m = sum(l for o, l in cigar if o in (M, EQ, X))
        mm = int(rng.choice([0, 0, 1, m // 8, m // 5]))
        recs.append(rec(c, int(rng.integers(0, L)), cigar, "q%d" % k, mapq, flag, int(rng.integers(0, 9)), aux=_nm_for(cigar, mm)))
    return refs, recs


def _scan_blocks():
    """More than 4096 records AND more than 4096 chunks, so that the device scan and the class histogram cross a workgroup: 4095 records
    that reach the CIGAR tests (one chunk each), then one of three chunks -- chunks 4095, 4096 and 4097 --, then 600 of the random kind."""
    rng = np.random.default_rng(3)
    refs, tail = _random(600, 4)
    recs = []
    for k in range(C.SCAN_BLOCK - 1):
        c = int(rng.integers(0, 2))
        cigar = [(S, int(rng.integers(0, 4)))] + [(int(o), int(l)) for o, l in zip(rng.choice([M, EQ, I, D], size=int(rng.integers(1, 12))), rng.integers(1, 30, size=12))]
        recs.append(rec(c, int(rng.integers(0, refs[c][1])), cigar, "s%d" % k, int(rng.integers(30, 61)), int(rng.choice([0, 0x10])), int(rng.integers(0, 9)),
                        aux=_nm_for(cigar, int(rng.integers(0, 6)))))
    straddle = [(M, 2)] * (2 * CH) + [(S, 1000)]
    recs.append(rec(2, 100, straddle, "straddle", aux=nm(0)))
    return assemble(refs, recs + tail, runs=[DEFAULT])


BUILDERS = {
    "one_per_class": _one_per_class, "several_tests": _several_tests, "on_the_thresholds": _on_the_thresholds, "threshold_band": _threshold_band,
    "nm_forms": _nm_forms, "chunks": _chunks, "phases": _phases, "placeholder": _placeholder, "none_op9": _none_op9,
    "no_records": lambda: assemble(REFS, [], ref_sel=SEL, runs=[DEFAULT]),
    "clip_no_nm": lambda: _errors([rec(0, 10, [(S, 30), (M, 10)])]),
    "nm_float": lambda: _errors([rec(0, 10, [(M, 10)], aux=nm(1.0, "f"))]),
    "zero_div_clip": lambda: _errors([rec(0, 10, [(D, 5), (N, 3)], aux=nm(0))]),
    "zero_div_identity": lambda: _errors([rec(0, 10, [(M, 9)], aux=nm(0)), rec(0, 20, [(S, 5)], aux=nm(0))], run=(30, 1.0, 0.9)),
    "no_operations": lambda: _errors([rec(0, 10, [], aux=nm(0)), rec(0, 20, [])]),
    "two_errors": lambda: _errors([rec(0, 10, [(M, 9)]), rec(0, 20, [(D, 5)], aux=nm(0))]),
    "cut_off": lambda: _errors([], cut=5),
    "random_3000": lambda: assemble(*_random(3000, 1), ref_sel=[0, -1, 1], runs=[DEFAULT, (50, 0.05, 0.85)]),
    "scan_blocks": _scan_blocks,
}
NAMES = list(BUILDERS)
# the record the status word must name, and what it says of it
ERRORS = {"clip_no_nm": (1, F.E_NO_NM), "nm_float": (1, F.E_BAD_NM_TYPE), "zero_div_clip": (1, F.E_ZERO_DIV), "zero_div_identity": (2, F.E_ZERO_DIV),
          "no_operations": (1, F.E_ZERO_DIV), "two_errors": (1, F.E_NO_NM), "cut_off": (1, F.E_MALFORMED)}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def heads(name):
    c = case(name)
    return C.to_heads(c["stream"], c["offs"])


@functools.lru_cache(maxsize=None)
def want(name, run):
    c = case(name)
    return F.stream_classes(c["stream"], c["offs"], c["ref_sel"], *run)


@functools.lru_cache(maxsize=None)
def want_depth(name, run, cls, count_del=False):
    c = case(name)
    return F.class_depth(c["stream"], c["offs"], c["lengths"], c["ref_sel"], want(name, run)[0], cls, count_del)


def pairs():
    """(name, run) of every case but threshold_band (hundreds of runs over eleven records: one test walks them)."""
    return [(name, run) for name in NAMES if name != "threshold_band" for run in case(name)["runs"]]


def depth_pairs():
    """(name, run) of the cases whose per-class depths are compared: those without a malformed record, threshold_band left out (its
    records cover 10^9 bases)."""
    return [(name, case(name)["runs"][0]) for name in NAMES if name not in ("threshold_band", "cut_off")]
