"""Named inputs of gci_bam_sweep: a header plus records made with cover_cases.rec / assemble, the smallest shapes at which each part
can go wrong.  case(name) -> dict(stream, offs, lengths, ref_sel, runs, win, win0): every run is (map_qual, cp, ip), win / win0 the
windows as the export takes them (None: no window test).  want(name, run, digits) -> (table, status word) from tests/sweep_ref.py;
the records are decoded once per case and every answer is computed once and left as it is."""
import functools

import cover_cases as C
import fate_cases as FC
import sweep_ref as SR
from cover_cases import CH, D, EQ, I, M, N, S, X, assemble, rec
from fate_cases import nm
from reads_cases import windows

DEFAULT = FC.DEFAULT
OTHER = (50, 0.05, 0.85)
DIGITS = (1, 2, 3)
GROUP = 256                                            # records a workgroup of k_sweep_bin takes a round
A = [("a", 300000), ("b", 300)]
SEL = [0, -1]                                          # contig b is not selected


def make(refs, records, ref_sel=None, runs=(DEFAULT,), wins=None, cut=0):
    return finish(assemble(refs, records, ref_sel=ref_sel, runs=list(runs), cut=cut), wins)


def finish(c, wins=None, runs=None):
    c = dict(c, win=None, win0=None)
    if runs is not None:
        c["runs"] = list(runs)
    if wins is not None:
        c["win"], c["win0"] = windows(wins)
    return c


def _special_rows():
    """A record on every special row -- `<0`, `>1` (NM of type c, negative), `undefined` of each kind (no NM, NM of type f, M + I + S = 0,
    M + I + D = 0) --, one whose clip is defined and whose identity is not, and the reverse; no operations at all."""
    return make(A, [rec(0, 10, [(M, 10)], "below_0", aux=nm(25)), rec(0, 20, [(M, 10)], "above_1", aux=nm(-5, "c")),
                    rec(0, 30, [(M, 10)], "no_nm"), rec(0, 40, [(M, 10)], "nm_f", aux=nm(1.0, "f")),
                    rec(0, 50, [(D, 5), (N, 3)], "no_clip_identity_1", aux=nm(0)), rec(0, 60, [(S, 5)], "clip_1_no_identity", aux=nm(0)),
                    rec(0, 70, [], "no_operations", aux=nm(0)), rec(0, 80, [], "nothing"),
                    rec(0, 90, [(M, 10)], "plain", aux=nm(0))], ref_sel=SEL, runs=(DEFAULT, (0, 1.0, 0.0)))


def _edges():
    """Quotients exactly on a row edge for K = 1, 2, 3 (S = k of 1000 bases; identity (1000 - k) / 1000), one base below and one above;
    clip 0 and 1, identity 0 and 1; quotients that never end (sevenths, thirds)."""
    ks = (0, 1, 9, 10, 11, 99, 100, 101, 499, 500, 501, 899, 900, 901, 989, 990, 991, 999, 1000)
    recs = [rec(0, 10 + k, [(S, k), (M, 1000 - k)] if k else [(M, 1000)], "clip%d" % k, aux=nm(0)) for k in ks]
    recs += [rec(0, 2000 + k, [(M, 1000)], "iden%d" % k, aux=nm(k)) for k in ks]
    recs += [rec(0, 4000, [(S, 1), (M, 6)], "seventh", aux=nm(1)), rec(0, 4010, [(S, 6), (M, 1)], "six_sevenths", aux=nm(0)),
             rec(0, 4020, [(S, 1), (M, 2)], "third", aux=nm(1)), rec(0, 4030, [(M, 3), (I, 3), (D, 1)], "sevenths", aux=nm(1)),
             rec(0, 4040, [(S, 1), (M, 999999)], "millionth", aux=nm(1))]
    return make(A, recs, ref_sel=SEL, runs=(DEFAULT, (30, 0.5, 0.5)))


def _all_clip_rows():
    """All 1001 clip rows of K = 3 hit once each."""
    return make(A, [rec(0, k, ([(S, k)] if k else []) + ([(M, 1000 - k)] if k < 1000 else []), "k%d" % k, aux=nm(k % 7)) for k in range(1001)],
                ref_sel=SEL)


def _identical(n):
    """One row, every lane colliding."""
    one = rec(0, 77, [(S, 3), (M, 90), (I, 2), (D, 5)], "same", aux=nm(9))
    return make(A, [one] * n, ref_sel=SEL)


def _wave_rows():
    """A wave with 64 distinct rows in every table, then a wave with 2, then one of a single row with a hole (a secondary record)."""
    recs = [rec(0, k, [(S, 10 * k), (M, 1000 - 10 * k)] if k else [(M, 1000)], "d%d" % k, mapq=k, aux=nm(k)) for k in range(64)]
    recs += [rec(0, 100 + k, [(S, 50 * (k % 2)), (M, 1000)], "t%d" % k, mapq=60 - 30 * (k % 2), aux=nm(200 * (k % 2))) for k in range(64)]
    recs += [rec(0, 200 + k, [(M, 100)], "s%d" % k, flag=0x100 if k == 17 else 0, aux=nm(0)) for k in range(64)]
    return make(A, recs, ref_sel=SEL)


def _big_operations():
    """Operation lengths of 2^28 - 1: the totals need 64 bits."""
    big = (1 << 28) - 1
    return make([("a", 2_000_000_000), ("b", 300)],
                [rec(0, 5, [(S, big)] * 3 + [(M, big)] * 20 + [(I, big)] + [(D, big)] * 2, "big", aux=nm(3 * big + 5, "I")),
                 rec(0, 6, [(S, big)] * 17 + [(EQ, big)] * 3 + [(X, big)], "big_clipped", aux=nm(big, "I")),
                 rec(0, 7, [(M, big)] * 20, "big_twin", aux=nm(0))], ref_sel=SEL)


def _who_is_counted():
    """none, secondary and supplementary records between primary ones; MAPQ 0 without NM: counted, no status; codes 9 - 15 in a
    secondary record: not read."""
    return make(A, [rec(0, 10, [(M, 20)], "p1", aux=nm(0)), rec(1, 5, [(M, 20)], "unselected", aux=nm(0)), rec(0, 20, [(M, 20)], "secondary", flag=0x100, aux=nm(0)),
                    rec(0, 30, [(M, 20)], "p2", mapq=0), rec(0, 40, [(M, 20)], "supplementary", flag=0x800, aux=nm(0)),
                    rec(0, 50, [(M, 20)], "unmapped", flag=0x4, aux=nm(0)), rec(-1, 60, [(M, 20)], "no_ref", aux=nm(0)), rec(0, -1, [(M, 20)], "no_pos", aux=nm(0)),
                    rec(2, 70, [(M, 20)], "beyond_the_table", aux=nm(0)), rec(0, 80, [(9, 3), (M, 4)], "secondary_op9", flag=0x100),
                    rec(0, 90, [(S, 30), (M, 10)], "p3_clipped_mapq3", mapq=3), rec(0, 100, [(M, 20)], "both", flag=0x900, aux=nm(0)),
                    rec(0, 110, [(M, 20)], "p4_other_flags", flag=0x1 | 0x10 | 0x40 | 0x200 | 0x400, aux=nm(2))], ref_sel=SEL)


def _op9():
    """Codes 9 - 15 in a primary record: reported and counted; the codes add to no total."""
    return make(A, [rec(0, 10, [(M, 20)], aux=nm(0)), rec(0, 20, [(9, 3), (M, 4)], flag=0x800), rec(0, 30, [(M, 4), (9, 3), (M, 2)], aux=nm(1)),
                    rec(0, 40, [(15, 1)], aux=nm(0)), rec(0, 50, [(M, 20)], aux=nm(0))], ref_sel=SEL)


def _cigar_shapes():
    """CH - 1, CH, CH + 1 and 2 CH + 1 operations, a soft clip as the last one, and their twins of MAPQ 3 (read here, not by gci_bam_fate)."""
    recs = []
    for k, n in enumerate((CH - 1, CH, CH + 1, 2 * CH + 1)):
        pat = FC._pattern(n, 10 * n)
        recs += [rec(0, 1000 * k, [(M, 1)] * (n - 1) + [(S, n)], aux=nm(0)), rec(0, 1000 * k + 1, [(M, 1)] * n, mapq=3, aux=nm(0)),
                 rec(0, 1000 * k + 10, pat, aux=FC._nm_for(pat, 3)), rec(0, 1000 * k + 11, pat, mapq=3)]
    return make(A, recs, ref_sel=SEL)


def _window_edges():
    """Windows [100, 200) and [300, 400): pos = E, pos + R = B, one base inside at either side, a zero-span record on B, on E and one
    base in front of B; a record through N and D into the window, one that I and S do not carry there; behind the last window."""
    zero = [(S, 5), (I, 5)]
    return make(A, [rec(0, 80, [(M, 20)], "ends_on_B", aux=nm(0)), rec(0, 81, [(M, 20)], "one_base_left", aux=nm(0)),
                    rec(0, 199, [(M, 20)], "one_base_right", aux=nm(0)), rec(0, 200, [(M, 20)], "begins_on_E", aux=nm(0)),
                    rec(0, 99, zero, "zero_before_B", aux=nm(5)), rec(0, 100, zero, "zero_on_B", aux=nm(5)), rec(0, 199, zero, "zero_last", aux=nm(5)),
                    rec(0, 200, zero, "zero_on_E", aux=nm(5)), rec(0, 50, [(M, 10), (N, 100), (M, 10)], "through_N", aux=nm(0)),
                    rec(0, 50, [(M, 10), (D, 45), (M, 10)], "through_D", aux=nm(45)), rec(0, 50, [(M, 10), (I, 100), (M, 10)], "not_through_I", aux=nm(100)),
                    rec(0, 150, [(M, 200)], "over_both", aux=nm(0)), rec(0, 399, [(M, 1)], "last_base", aux=nm(0)), rec(0, 400, [(M, 1)], "behind", aux=nm(0)),
                    rec(0, 5000, [(M, 50)], "far_behind", aux=nm(0)), rec(1, 120, [(M, 10)], "unselected_contig", aux=nm(0))],
                ref_sel=SEL, wins=[[(100, 200), (300, 400)]])


def _window_contigs():
    """A contig without windows between contigs with them, an unselected one, and a contig of 1000 windows."""
    refs = [("w0", 20000), ("w1", 20000), ("un", 20000), ("w2", 20000), ("w1000", 20000)]
    wins = [[], [(100, 110)], [(100, 110), (200, 210)], [(10 * k, 10 * k + 5) for k in range(1000)]]
    recs = []
    for ref in range(5):
        recs += [rec(ref, p, [(M, 4)], "r%d_%d" % (ref, p), aux=nm(0)) for p in (96, 97, 105, 110, 204, 296)]
    recs += [rec(4, p, [(M, n)], "k%d_%d" % (p, n), aux=nm(0)) for p, n in ((0, 1), (4, 1), (5, 5), (5, 6), (5003, 2), (9994, 1), (9995, 100), (19000, 5))]
    return make(refs, recs, ref_sel=[0, 1, -1, 2, 3], wins=wins)


def _plain(n_rec, **kw):
    """n_rec records 100 bases apart, their rows spread over the tables."""
    return make(A, [rec(0, 100 * k, [(S, k % 50), (M, 100 + k % 7), (I, k % 3)], "g%d" % k, mapq=(k * 7) % 61, flag=0x100 if k % 11 == 5 else 0,
                        aux=nm(k % 13)) for k in range(n_rec)], ref_sel=SEL, **kw)


BUILDERS = {
    "special_rows": _special_rows, "edges": _edges, "all_clip_rows": _all_clip_rows, "identical_3000": lambda: _identical(3000),
    "wave_rows": _wave_rows, "big_operations": _big_operations,
    "who_is_counted": _who_is_counted, "none_op9": lambda: finish(FC.case("none_op9")), "op9": _op9,
    "cut_off": lambda: make(A, [rec(0, 5, [(M, 9)], aux=nm(0)), rec(0, 10, [(M, 9)], aux=nm(0)), rec(0, 20, [(M, 9)], aux=nm(1))], ref_sel=SEL, cut=5),
    "cigar_shapes": _cigar_shapes, "chunks": lambda: finish(FC.case("chunks")), "phases": lambda: finish(FC.case("phases")),
    "placeholder": lambda: finish(FC.case("placeholder")), "nm_forms": lambda: finish(FC.case("nm_forms")),
    "on_the_thresholds": lambda: finish(FC.case("on_the_thresholds")),
    "window_edges": _window_edges, "window_contigs": _window_contigs,
    "chunks_windowed": lambda: finish(FC.case("chunks"), wins=[[(1500, 2500)]]),
    "no_windows_at_all": lambda: finish(FC.case("one_per_class"), wins=[[]]),
    "no_records": lambda: make(A, [], ref_sel=SEL), "no_records_windowed": lambda: make(A, [], ref_sel=SEL, wins=[[(100, 200)]]),
    "one_record": lambda: _plain(1), "records_255": lambda: _plain(GROUP - 1), "records_256": lambda: _plain(GROUP), "records_257": lambda: _plain(GROUP + 1),
    "records_769": lambda: _plain(3 * GROUP + 1, wins=[[(0, 30000), (50000, 70000)]]),
    "random_3000": lambda: finish(FC.case("random_3000"), runs=(DEFAULT, OTHER)),
}
NAMES = list(BUILDERS)
STATUS = {"op9": (2, SR.E_MALFORMED), "cut_off": (2, SR.E_MALFORMED)}      # the record the status word must name; every other case: none
GRID_CASE = "records_769"                                  # 3 * 256 + 1 records: under GCI_SWEEP_GRID=2 a workgroup goes round its loop twice


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def heads(name):
    c = case(name)
    return C.to_heads(c["stream"], c["offs"])


@functools.lru_cache(maxsize=None)
def entries(name):
    c = case(name)
    return SR.entries(c["stream"], c["offs"], c["ref_sel"])


@functools.lru_cache(maxsize=None)
def want(name, run, digits):
    c = case(name)
    table, status = SR.table_of(entries(name), run, digits, c["win"], c["win0"])
    table.setflags(write=False)
    return table, status


def triples():
    """(name, run, digits) of every case."""
    return [(name, run, K) for name in NAMES for run in case(name)["runs"] for K in DIGITS]
