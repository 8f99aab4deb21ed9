"""Named inputs of gci_bam_reads_size / _write: a header plus records made with cover_cases.rec / assemble, each a few KB, the smallest
shapes at which the kernels can go wrong.  case(name) -> dict(stream, offs, lengths, ref_sel, names, run, mask, win, win0): run is the
(map_qual, cp, ip) the classes are made with, names the selected contigs' names, win / win0 the windows as the exports take them
(None: no window test).  classes(name) -> fate_ref's class per record, want(name) -> (rows, status word) from tests/reads_ref.py;
both computed once and left as they are."""
import functools

import numpy as np

import cover_cases as C
import fate_cases as FC
import fate_ref as F
import reads_ref as RR
from cover_cases import CH, D, EQ, I, M, N, S, X, assemble, rec
from fate_cases import nm
from gci_amd.formats import bam as bamfmt

ALL = 0x7E                                             # every class of the record filter but none and error
GROUP = 256                                            # records a workgroup of the row kernels takes
STAGE = 49152                                          # RD_STAGE (k_reads.hip): bytes of rows a workgroup renders in LDS
WINDOWED_WITHOUT_BOTH = ("no_records", "no_row")       # the windowed cases that need not hold a listed and an unlisted record


def windows(per_contig):
    """[[(B, E), ...] per selected contig], each sorted, disjoint and not abutting -> (win, win0)."""
    win, win0 = [], [0]
    for ws in per_contig:
        assert all(a < b for a, b in ws) and all(ws[k][1] < ws[k + 1][0] for k in range(len(ws) - 1))
        win += [list(w) for w in ws]
        win0.append(len(win))
    return np.asarray(win, dtype=np.int64).reshape(-1, 2), np.asarray(win0, dtype=np.uint32)


def make(refs, records, ref_sel=None, run=FC.DEFAULT, mask=ALL, wins=None, cut=0):
    c = assemble(refs, records, ref_sel=ref_sel, runs=[run], cut=cut)
    return finish(c, refs, run, mask, wins)


def finish(c, refs, run, mask, wins):
    order = sorted((int(s), n) for (n, _), s in zip(refs, c["ref_sel"].tolist()) if s >= 0)
    c = dict(c, names=[n.encode() for _, n in order], run=run, mask=mask, win=None, win0=None)
    if wins is not None:
        c["win"], c["win0"] = windows(wins)
    return c


def from_fate(name, run=None, mask=ALL, wins=None):
    """A case of tests/fate_cases.py (contig a selected, b not)."""
    refs = [("a", 2_000_000_000), ("b", 300)] if name == "threshold_band" else FC.REFS
    return finish(FC.case(name), refs, run or FC.DEFAULT, mask, wins)


A = [("a", 300000), ("b", 300)]


def _window_edges():
    """One window [100, 200), then [300, 400): a record ending on B, beginning on E, one base inside at either side, inside the window,
    around it, over both windows (listed once), and between the two."""
    return make(A, [rec(0, 80, [(M, 20)], "ends_on_B", aux=nm(0)), rec(0, 81, [(M, 20)], "one_base_left", aux=nm(0)),
                    rec(0, 120, [(M, 10)], "inside", aux=nm(0)), rec(0, 50, [(M, 200)], "around", aux=nm(0)),
                    rec(0, 150, [(M, 200)], "over_both", aux=nm(0)), rec(0, 199, [(M, 20)], "one_base_right", aux=nm(0)),
                    rec(0, 200, [(M, 20)], "begins_on_E", aux=nm(0)), rec(0, 210, [(M, 80)], "between", aux=nm(0)),
                    rec(0, 399, [(M, 1)], "last_base", aux=nm(0)), rec(0, 400, [(M, 1)], "behind", aux=nm(0)),
                    rec(1, 120, [(M, 10)], "unselected_contig", aux=nm(0))], ref_sel=[0, -1], wins=[[(100, 200), (300, 400)]])


def _no_reference():
    """R = 0 (S and I only): the record sits on the one base at pos."""
    ops = [(S, 5), (I, 5)]
    return make(A, [rec(0, p, ops, "at%d" % p, aux=nm(5)) for p in (98, 99, 100, 150, 199, 200)], ref_sel=[0, -1], wins=[[(100, 200)]])


def _through_n_and_d():
    return make(A, [rec(0, 50, [(M, 10), (N, 100), (M, 10)], "through_N", aux=nm(0)), rec(0, 50, [(M, 10), (D, 100), (M, 10)], "through_D", aux=nm(100)),
                    rec(0, 50, [(M, 10), (I, 100), (M, 10)], "not_through_I", aux=nm(100)), rec(0, 50, [(M, 10), (S, 100)], "not_through_S", aux=nm(0))],
                ref_sel=[0, -1], wins=[[(100, 110)]])


def _window_counts():
    """Contigs with 0, 1, 2, 3 and 1000 windows, and an unselected one between them."""
    refs = [("w0", 20000), ("w1", 20000), ("un", 20000), ("w2", 20000), ("w3", 20000), ("w1000", 20000)]
    sel = [0, 1, -1, 2, 3, 4]
    wins = [[], [(100, 110)], [(100, 110), (200, 210)], [(100, 110), (200, 210), (300, 310)], [(10 * k, 10 * k + 5) for k in range(1000)]]
    recs = []
    for ref in range(6):
        recs += [rec(ref, p, [(M, 4)], "r%d_%d" % (ref, p), aux=nm(0)) for p in (96, 97, 105, 110, 204, 296, 309, 310)]
    recs += [rec(5, p, [(M, n)], "k%d_%d" % (p, n), aux=nm(0)) for p, n in ((0, 1), (4, 1), (5, 5), (5, 6), (5003, 2), (9985, 5), (9994, 1), (9995, 100), (19000, 5))]
    return make(refs, recs, ref_sel=sel, wins=wins)


def _groups(n_rec, listed):
    """n_rec records 1000 bases apart, a window on those of `listed`."""
    return make(A, [rec(0, 1000 * k, [(M, 10)], "g%d" % k, aux=nm(0)) for k in range(n_rec)], ref_sel=[0, -1],
                wins=[[(1000 * k + 3, 1000 * k + 4) for k in listed]])


def _names():
    """Read names of 1 - 4 bytes (every byte phase of what follows them), of 254 bytes, and none at all."""
    long_name = "n" * 250 + "_254"
    return make(A, [rec(0, 10 * k, [(M, 20)], n, aux=nm(0)) for k, n in enumerate(["a", "ab", "abc", "abcd", long_name, "", "abcde"])], ref_sel=[0, -1])


def _stage_overflow():
    """200 rows of more than 300 bytes in one workgroup: more than the stage holds; 56 short ones behind them, and a second workgroup."""
    recs = [rec(0, 10 * k, [(M, 20)], ("%03d" % k) + "x" * 251, aux=nm(0)) for k in range(200)]
    recs += [rec(0, 10 * k, [(M, 20)], "s%d" % k, aux=nm(0)) for k in range(200, 300)]
    return make(A, recs, ref_sel=[0, -1])


def _long_contig_name():
    refs = [("c" * 300, 5000), ("short", 5000)]
    return make(refs, [rec(0, 10, [(M, 20)], "on_long", aux=nm(0)), rec(1, 10, [(M, 20)], "on_short", aux=nm(0)), rec(0, 3000, [(M, 20)], "far", aux=nm(0))],
                wins=[[(0, 100)], [(0, 100)]])


def _nm_types():
    """NM of every integer type, negative too; of a type that is no integer and absent on records their core fields settle (`.`)."""
    enc = bamfmt.encode_aux
    recs = [rec(0, 10 * k, [(M, 100)], "nm_%s" % t, aux=nm(v, t)) for k, (t, v) in enumerate(
        [("c", -3), ("c", 7), ("C", 200), ("s", -300), ("s", 300), ("S", 40000), ("i", -70000), ("i", 70000), ("I", 11)])]
    recs += [rec(0, 200, [(M, 100)], "nm_Z", mapq=3, aux=enc([("NM", "Z", "12")])), rec(0, 210, [(M, 100)], "nm_f", flag=0x100, aux=nm(1.0, "f")),
             rec(0, 220, [(M, 100)], "no_nm", mapq=3), rec(0, 230, [(M, 100)], "no_nm_supp", flag=0x800),
             rec(0, 240, [(M, 100)], "second_nm", aux=enc([("XS", "Z", "in front"), ("NM", "C", 1), ("NM", "C", 50)]))]
    return make(A, recs, ref_sel=[0, -1])


def _identity_range():
    """Identity above 1 (a negative NM), below 0 (NM beyond the alignment), exactly 0 and 1; clip of 0 and of nearly 1."""
    return make(A, [rec(0, 10, [(M, 10)], "above_1", aux=nm(-5)), rec(0, 20, [(M, 10)], "below_0", aux=nm(25)), rec(0, 30, [(M, 10)], "zero", aux=nm(10)),
                    rec(0, 40, [(M, 10)], "one", aux=nm(0)), rec(0, 50, [(S, 999999), (M, 1)], "clipped", aux=nm(0)),
                    rec(0, 60, [(M, 3), (I, 3), (D, 1)], "sevenths", aux=nm(1)), rec(0, 70, [(D, 5), (N, 5)], "no_quotient", mapq=3, aux=nm(0)),
                    rec(0, 80, [], "no_operations", mapq=3)], ref_sel=[0, -1])


def _extremes():
    """pos = 2^31 - 2 (the end lies beyond 2^31), every flag bit but 0x4, mapq 255; flag 65535 is unmapped: class none, never listed."""
    refs = [("big", 2 ** 31 - 1), ("b", 300)]
    return make(refs, [rec(0, 2 ** 31 - 2, [(M, 5), (D, 2 ** 28 - 1)], "far", mapq=255, flag=0xFFFB, aux=nm(0)),
                       rec(0, 2 ** 31 - 2, [(M, 5)], "unmapped", mapq=255, flag=65535, aux=nm(0)),
                       rec(0, 2 ** 31 - 2, [(M, 3)], "kept_far", mapq=255, flag=0x10, aux=nm(0))],                    # (spans that cross 2^31: bin 0)
                ref_sel=[0, -1], wins=[[(2 ** 31 - 2, 2 ** 31 - 1)]])


def _from_cover(name):
    """A case of tests/cover_cases.py whose records carry no NM: -mq 61 settles them by their MAPQ (class mapq), so they are listed."""
    c = C.case(name)
    refs = [("a", 300), ("b", 300)] if name == "op9" else [("a", 300)]
    return finish(dict(c), refs, (61, 0.1, 0.9), ALL, None)


BUILDERS = {
    "one_per_class": lambda: from_fate("one_per_class"), "one_class": lambda: from_fate("one_per_class", mask=1 << F.CLIP),
    "several_tests": lambda: from_fate("several_tests"),
    "window_edges": _window_edges, "no_reference": _no_reference, "through_n_and_d": _through_n_and_d, "window_counts": _window_counts,
    "groups_257": lambda: _groups(2 * GROUP - 255, [GROUP - 1, GROUP]), "groups_513": lambda: _groups(2 * GROUP + 1, [GROUP - 1, 2 * GROUP]),
    "chunks": lambda: from_fate("chunks"), "chunks_windowed": lambda: from_fate("chunks", wins=[[(1500, 2500)]]),
    "placeholder": lambda: from_fate("placeholder"), "phases": lambda: from_fate("phases"),
    "names": _names, "stage_overflow": _stage_overflow, "long_contig_name": _long_contig_name,
    "nm_forms": lambda: from_fate("nm_forms"), "nm_types": _nm_types, "identity_range": _identity_range,
    "beyond_2_31": lambda: from_fate("threshold_band", run=(30, 0.1, 0.9)), "extremes": _extremes,
    "op9": lambda: _from_cover("op9"), "cut_off": lambda: _from_cover("cut_off"),
    "none_op9": lambda: from_fate("none_op9"),
    "no_records": lambda: make(A, [], ref_sel=[0, -1], wins=[[(100, 200)]]),
    "no_row": lambda: make(A, [rec(0, 10, [(M, 20)], aux=nm(0)), rec(0, 500, [(M, 20)], aux=nm(0))], ref_sel=[0, -1], wins=[[(100, 200)]]),
}
NAMES = list(BUILDERS)
STATUS = {"op9": (3, RR.E_MALFORMED)}                  # the record the status word must name; every other case: none


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def heads(name):
    c = case(name)
    return C.to_heads(c["stream"], c["offs"])


@functools.lru_cache(maxsize=None)
def classes(name):
    c = case(name)
    return F.stream_classes(c["stream"], c["offs"], c["ref_sel"], *c["run"])[0]


@functools.lru_cache(maxsize=None)
def want(name):
    c = case(name)
    return RR.stream_rows(c["stream"], c["offs"], c["ref_sel"], c["names"], classes(name), c["mask"], c["win"], c["win0"])
