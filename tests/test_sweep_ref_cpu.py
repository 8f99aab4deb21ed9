"""The statement of filter_sweep.py's tables (tests/sweep_ref.py) against the statement of filter_depth.py's classes (tests/fate_ref.py):
what a threshold's own row says would be kept is what the record filter keeps; the tables count the records of the classes mapq, clip,
identity and kept; their bases are the kept records' depth; long division and exact fractions bin alike; and the cases hold what they
are named for."""
import numpy as np
import pytest

import fate_cases as FC
import fate_ref as F
import sweep_cases as SC
import sweep_ref as SR

RUNS = (FC.DEFAULT, (50, 0.05, 0.85))
RANDOM = ("random_3000", "scan_blocks")


def on_the_grid(x: float, digits: int) -> bool:
    """x is a multiple of 10^-digits (as the decimal a command line would give)."""
    return abs(x * 10 ** digits - round(x * 10 ** digits)) < 1e-9


@pytest.fixture(scope="module")
def random_sets():
    """fate_cases' random sets: the case, its entries, and per run fate_ref's (classes, counts, status)."""
    out = {}
    for name in RANDOM:
        c = FC.case(name)
        out[name] = (c, SR.entries(c["stream"], c["offs"], c["ref_sel"]), {run: F.stream_classes(c["stream"], c["offs"], c["ref_sel"], *run) for run in RUNS})
    return out


@pytest.mark.parametrize("digits", SC.DIGITS)
@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("name", RANDOM)
def test_a_thresholds_own_row_keeps_what_the_filter_keeps(random_sets, name, run, digits):
    c, ents, fate = random_sets[name]
    cls, counts, status = fate[run]
    # (where fate_ref reports a status it is for a record GCI.py would raise on -- class error, a primary record all the same, with an
    #  undefined quantity that fails its test here --, never a malformed one: what follows holds with and without)
    assert status == F.NO_STATUS or (status & 0xFF) != -F.E_MALFORMED
    table, st = SR.table_of(ents, run, digits)
    assert st == SR.NO_STATUS
    rows, kept = SR.Rows(digits), SR.kept_at(table, digits)
    n_kept = int(counts[F.KEPT])
    assert n_kept > 0
    # the records of every table are those of the classes mapq, clip, identity and kept (and error, where there is one)
    primary = int(counts[F.MAPQ] + counts[F.CLIP] + counts[F.IDENTITY] + counts[F.KEPT] + counts[F.ERROR])
    assert (status == F.NO_STATUS) == (int(counts[F.ERROR]) == 0)
    for a, b in ((rows.mapq0, rows.clip0), (rows.clip0, rows.iden_below), (rows.iden_below, rows.rows)):
        assert int(table[a:b, 0].sum()) == primary
    # the covered bases of the kept records: their depth, summed (contigs long enough that every record lies inside its own)
    depth = F.class_depth(c["stream"], c["offs"], [L + 2000 for L in c["lengths"]], c["ref_sel"], cls, F.KEPT)
    kept_bases = int(sum(int(d.sum()) for d in depth))
    mq, cp, ip = run
    assert kept[rows.mapq0 + mq] == (n_kept, kept_bases)
    checked = 1
    if on_the_grid(cp, digits):
        assert kept[rows.clip0 + round(cp * rows.bins)] == (n_kept, kept_bases)
        checked += 1
    if on_the_grid(ip, digits):
        assert kept[rows.iden0 + round(ip * rows.bins)] == (n_kept, kept_bases)
        checked += 1
    assert checked == (3 if digits > 1 or run == FC.DEFAULT else 1)


@pytest.mark.parametrize("name", SC.NAMES)
def test_long_division_and_fractions_bin_alike(name):
    c = SC.case(name)
    for run in c["runs"]:
        for digits in SC.DIGITS:
            table, status = SC.want(name, run, digits)
            other, status2 = SR.table_of(SC.entries(name), run, digits, c["win"], c["win0"], digits_of=SR.digits_fraction)
            assert status == status2 and np.array_equal(table, other)


def test_the_digits_of_a_quotient():
    for n, d in ((0, 7), (1, 7), (6, 7), (7, 7), (1, 3), (2, 3), (1, 1000), (999, 1000), (1, 10 ** 6), (2 ** 57 - 2, 2 ** 57 - 1), (1, 2 ** 57 - 1)):
        for K in SC.DIGITS:
            q, rest = SR.digits_long(n, d, K)
            assert (q, rest) == SR.digits_fraction(n, d, K)
            assert q * d <= n * 10 ** K < (q + 1) * d and rest == (q * d != n * 10 ** K)


def test_the_cases_hold_what_they_are_for():
    rows = SR.Rows(3)
    want = lambda name, K=3: SC.want(name, SC.case(name)["runs"][0], K)                     # noqa: E731
    for name in SC.NAMES:
        code = ((SC.STATUS[name][0] << 8) | -SC.STATUS[name][1]) if name in SC.STATUS else SR.NO_STATUS
        assert all(SC.want(name, run, K)[1] == code for run in SC.case(name)["runs"] for K in SC.DIGITS), name
    t, _ = want("special_rows")
    assert [int(t[r, 0]) for r in (rows.iden_below, rows.iden_above, rows.clip_undef)] == [1, 1, 3] and int(t[rows.iden_undef, 0]) == 5
    assert int(t[rows.clip0 + rows.bins, 0]) == 1 and int(t[rows.iden0 + rows.bins, 0]) == 2        # clip 1; identity 1 twice (one without a clip)
    t, _ = want("all_clip_rows")
    assert (t[rows.clip0:rows.clip0 + 1001, 0] == 1).all() and int(t[rows.clip_undef, 0]) == 0
    t, _ = want("identical_3000")
    assert sorted(int(x) for x in t[:, 0] if x) == [3000, 3000, 3000]
    per_wave = [[SR.record_rows(e, FC.DEFAULT, rows)[0] for e in SC.entries("wave_rows")[w:w + 64] if e is not None] for w in (0, 64, 128)]
    assert [[len({r[k] for r in wave}) for k in range(3)] for wave in per_wave] == [[64, 64, 64], [2, 2, 2], [1, 1, 1]] and len(per_wave[2]) == 63
    t, _ = want("big_operations")
    assert int(t[:256, 1].sum()) > 2 ** 32
    t, _ = want("who_is_counted")
    assert int(t[:256, 0].sum()) == 4 and int(t[0, 0]) == 1 and int(t[3, 0]) == 1       # p1 .. p4; MAPQ 0 and 3 without NM are counted
    t, _ = want("op9")
    assert int(t[:256, 0].sum()) == 4                     # the supplementary record's code 9 is not read, the two primary ones are counted
    t, _ = want("cut_off")
    assert int(t[:256, 0].sum()) == 2
    t, _ = want("no_windows_at_all")
    assert int(t.sum()) == 0
    # the edges: S = k of 1000 bases is rounded up, (1000 - k) of 1000 truncated
    at = {e[1]: e for e in SC.entries("edges") if e not in (None, "malformed")}
    for K, clip_rows, iden_rows in ((1, {99: 1, 100: 1, 101: 2, 0: 0, 1: 1, 1000: 10}, {99: 9, 100: 9, 101: 8, 0: 10, 1: 9, 1000: 0}),
                                    (2, {99: 10, 100: 10, 101: 11, 9: 1, 10: 1, 11: 2}, {99: 90, 100: 90, 101: 89, 9: 99, 10: 99, 11: 98}),
                                    (3, {99: 99, 100: 100, 101: 101, 999: 999}, {99: 901, 100: 900, 101: 899, 999: 1})):
        r = SR.Rows(K)
        for k, b in clip_rows.items():
            assert SR.record_rows(at[10 + k], FC.DEFAULT, r)[0][1] == r.clip0 + b, (K, k)
        for k, b in iden_rows.items():
            assert SR.record_rows(at[2000 + k], FC.DEFAULT, r)[0][2] == r.iden0 + b, (K, k)
    # windows: counted and uncounted primary records in every windowed case that is about both
    for name in ("window_edges", "window_contigs", "chunks_windowed", "records_769"):
        c = SC.case(name)
        n = int(want(name)[0][:256, 0].sum())
        everything = int(SR.table_of(SC.entries(name), c["runs"][0], 3)[0][:256, 0].sum())
        assert 0 < n < everything, name
    c, ents = SC.case("window_edges"), SC.entries("window_edges")
    counted = [i for i, e in enumerate(ents) if int(SR.table_of([e], FC.DEFAULT, 3, c["win"], c["win0"])[0][:256, 0].sum())]
    assert counted == [1, 2, 5, 6, 8, 9, 11, 12]          # one_base_left, one_base_right, zero_on_B, zero_last, through_N, through_D, over_both, last_base
