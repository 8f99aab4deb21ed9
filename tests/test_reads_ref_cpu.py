"""The statement of filter_reads.py's rows (tests/reads_ref.py) against checks that do not share its code, on the cases of
tests/reads_cases.py; and pipeline.merge_windows, the host function that makes the windows of a BED file."""
import random
from fractions import Fraction

import numpy as np
import pytest

import fate_ref as F
import reads_cases as RC
import reads_ref as RR
from gci_amd import pipeline


def parsed(rows):
    return [(i, dict(zip(RR.COLUMNS, r[:-1].decode().split("\t")))) for i, r in rows]


@pytest.mark.parametrize("name", [n for n in RC.NAMES if RC.case(n)["win0"] is not None])
def test_the_windowed_rows_are_the_rows_that_overlap(name):
    """The rows with windows == the rows without windows whose [start, max(end, start + 1)) meets a window of their contig, base by base."""
    c = RC.case(name)
    every, _ = RR.stream_rows(c["stream"], c["offs"], c["ref_sel"], c["names"], RC.classes(name), c["mask"])
    keep = []
    for (i, cols), (_, row) in zip(parsed(every), every):
        sel = [n.decode() for n in c["names"]].index(cols["contig"])
        start, end = int(cols["start"]), int(cols["end"])
        lo, hi = start, max(end, start + 1)
        if any(max(lo, int(b)) < min(hi, int(e)) for b, e in c["win"][int(c["win0"][sel]):int(c["win0"][sel + 1])].tolist()):
            keep.append((i, row))
    assert keep == RC.want(name)[0]


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_rows_agree_with_the_classes_and_the_spans(name):
    c = RC.case(name)
    cls = F.stream_classes(c["stream"], c["offs"], c["ref_sel"], *c["run"])[0]
    rows = RC.want(name)[0]
    assert [i for i, _ in rows] == sorted(i for i, _ in rows)
    for i, cols in parsed(rows):
        assert cols["class"] == F.NAMES[cls[i]] and (c["mask"] >> int(cls[i])) & 1
        assert int(cols["M"]) + int(cols["D"]) <= int(cols["end"]) - int(cols["start"])
        assert cols["file"] == "1" and cols["strand"] == ("-" if int(cols["flag"]) & 0x10 else "+")
    if c["win0"] is None:                                  # every record of the asked classes, once
        assert [i for i, _ in rows] == [i for i in range(len(cls)) if (c["mask"] >> int(cls[i])) & 1 and cls[i] != F.ERROR]


def test_dec6_is_the_truncated_quotient():
    rng = random.Random(7)
    pairs = [(0, 1), (1, 1), (1, 3), (2, 3), (999999, 1000000), (1, 1000001), (10, 7), (-1, 3), (-7, 7), (-1, 10 ** 9), (2 ** 57 - 1, 2 ** 57), (2 ** 58, 3),
             (3 * 2 ** 57 - 1 + 2 ** 31, 3 * 2 ** 57 - 1), (-(2 ** 32), 1)]
    pairs += [(rng.randrange(-2 ** 33, 2 ** 59), rng.randrange(1, 2 ** 59)) for _ in range(2000)]
    pairs += [(rng.randrange(0, 10 ** 6), rng.randrange(1, 10 ** 6)) for _ in range(2000)]
    for n, d in pairs:
        q = Fraction(abs(n), d)
        whole = q.numerator // q.denominator
        digits = ((q - whole) * 10 ** 6).numerator // ((q - whole) * 10 ** 6).denominator
        assert RR.dec6(n, d) == ("-" if n < 0 else "") + "%d.%06d" % (whole, digits), (n, d)
        assert abs(Fraction(RR.dec6(abs(n), d)) - q) < Fraction(1, 10 ** 6) and Fraction(RR.dec6(abs(n), d)) <= q


def test_the_quotient_columns():
    cols = dict(parsed(RC.want("identity_range")[0]))
    by_name = {v["name"]: v for v in cols.values()}
    assert by_name["above_1"]["identity"] == "1.500000" and by_name["below_0"]["identity"] == "-1.500000"
    assert by_name["zero"]["identity"] == "0.000000" and by_name["one"]["identity"] == "1.000000"
    assert by_name["clipped"]["clip"] == "0.999999" and by_name["one"]["clip"] == "0.000000"
    assert by_name["sevenths"]["identity"] == "0.857142" and by_name["sevenths"]["clip"] == "0.000000"
    assert by_name["no_quotient"]["clip"] == "." and by_name["no_quotient"]["identity"] == "1.000000"
    assert by_name["no_operations"]["clip"] == "." and by_name["no_operations"]["identity"] == "." and by_name["no_operations"]["NM"] == "."
    far = {v["name"]: v for v in dict(parsed(RC.want("extremes")[0])).values()}
    assert far["far"]["end"] == str(2 ** 31 - 2 + 5 + 2 ** 28 - 1) and far["far"]["flag"] == "65531" and far["far"]["mapq"] == "255" and "unmapped" not in far


# ---- pipeline.merge_windows ---------------------------------------------------------------------------------------------------------

LENGTHS = {"c1": 1000, "c2": 500, "c3": 10}


def merged(regions):
    win, win0 = pipeline.merge_windows(regions, LENGTHS)
    assert win.dtype == np.int64 and win0.dtype == np.uint32 and win.shape == (int(win0[-1]), 2) and win0.shape == (len(LENGTHS) + 1,)
    return [[tuple(w) for w in win[int(a):int(b)].tolist()] for a, b in zip(win0[:-1], win0[1:])]


def test_merge_windows():
    assert merged([]) == [[], [], []]
    assert merged([("c2", 5, 9), ("c1", 300, 400), ("c1", 10, 20)]) == [[(10, 20), (300, 400)], [(5, 9)], []]            # unsorted, per contig
    assert merged([("c1", 10, 100), ("c1", 20, 30), ("c1", 90, 120), ("c1", 5, 10)]) == [[(5, 120)], [], []]              # nested, overlapping, abutting
    assert merged([("c1", 10, 20), ("c1", 21, 30)]) == [[(10, 20), (21, 30)], [], []]                                      # one base apart: two windows
    assert merged([("c1", -5, 3), ("c2", 490, 600), ("c3", 10, 20), ("c3", 12, 11), ("c3", 4, 4)]) == [[(0, 3)], [(490, 500)], []]   # clamped; empty ones dropped
    assert merged([("nope", 0, 10), ("c3", 0, 10), ("c3", 0, 10)]) == [[], [], [(0, 10)]]                                  # a contig that is not selected
    rng = np.random.default_rng(5)
    rows = [("c1", int(a), int(a + l)) for a, l in zip(rng.integers(-20, 1020, 300), rng.integers(0, 12, 300))]
    covered = np.zeros(1000, dtype=bool)
    for _, a, b in rows:
        covered[max(a, 0):max(min(b, 1000), 0)] = True
    got = merged(rows)[0]
    again = np.zeros(1000, dtype=bool)
    for a, b in got:
        assert 0 <= a < b <= 1000 and not again[a:b].any()
        again[a:b] = True
    assert np.array_equal(again, covered) and all(got[k][1] < got[k + 1][0] for k in range(len(got) - 1))
