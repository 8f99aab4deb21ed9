"""The statement of tests/allele_ref.py on its own: the lists written by hand; on every record case its four lists, merged, are the
events of tests/mismatch_ref.py (another walk: whole operations with numpy) and the outer counts agree; the sites written by hand."""
import pytest

import allele_cases as C
import allele_ref as R
import mismatch_cases as MC


def test_the_hand_written_lists_are_the_mismatch_events_by_read_base():
    for key, lists in C.EXPECTED.items():
        events, counts = MC.EXPECTED[key]
        assert sorted(e for lst in lists for e in lst) == sorted(events), key
        assert sum(len(lst) for lst in lists) == counts[1], key


def test_the_statement_gives_the_hand_written_lists():
    for (name, run), lists in C.EXPECTED.items():
        got, counts, status = C.want(name, run)
        want_counts = MC.EXPECTED[(name, run)][1]
        assert tuple(got) == lists and status == R.NO_STATUS, name
        assert counts == [want_counts[0]] + [len(lst) for lst in lists] + [want_counts[2]], name


@pytest.mark.parametrize("name", MC.NAMES)
def test_the_four_lists_merged_are_the_mismatch_events(name):
    for run in MC.case(name)["runs"]:
        lists, counts, status = C.want(name, run)
        events, mm_counts, mm_status = MC.want(name, run)
        assert sorted(e for lst in lists for e in lst) == sorted(events), run
        assert (counts[0], sum(counts[1:5]), counts[5], status) == (mm_counts[0], mm_counts[1], mm_counts[2], mm_status), run


def test_every_base_of_the_added_case_is_an_event_of_mixed_classes():
    lists, counts, status = C.want("every_base", (C.EXCL, 0))
    assert status == R.NO_STATUS and counts[0] == 2 and sum(counts[1:5]) == counts[5] == 1024 + 777
    assert min(counts[1:5]) > 300                                # all four classes, about a quarter each
    first = sorted(p for lst in lists for c, p in lst)[:1024]
    assert first[:3] == [101, 102, 103]                           # consecutive bases: every lane's share is full


def test_the_statement_gives_the_hand_written_sites():
    for (name, k), rows in C.SITES_EXPECTED.items():
        assert C.want_sites(name, k) == rows, (name, k)
    planted = {k: [r[:2] for r in C.want_sites("planted", k)] for k in range(len(C.site_case("planted")["runs"]))}
    assert (0, 500) not in planted[1] and (0, 502) not in planted[0]                 # the fraction exactly, and one part per million beside it
    assert (0, 402) in planted[3] and (0, 402) in planted[4] and (0, 402) not in planted[0]      # best == min_reads - 1
    assert (0, 400) not in planted[5]
    assert planted[8][0] == (0, 101) and (0, 8999) not in planted[8] and planted[8][-1] == (1, 0)
    assert planted[9] == planted[0]
    assert all(pos < length for rows in planted.values() for c, pos in rows for length in [C.site_case("planted")["lengths"][c]])
