"""The statement of clip_sites.py's semantics (tests/clips_ref.py) against the answers written by hand (tests/clips_cases.py: EXPECTED),
against a second, per-operation loop, and that the cases hold what they are named for."""
import numpy as np
import pytest

import clips_cases as C
import clips_ref as R
from gci_amd import _lib


@pytest.mark.parametrize("key", list(C.EXPECTED), ids=lambda k: "%s-%x-%d-%d" % ((k[0],) + k[1]))
def test_the_statement_gives_the_hand_written_events(key):
    left, right, counted = C.EXPECTED[key]
    got_left, got_right, counts, status = C.want(*key)
    assert (got_left, got_right) == (left, right)
    assert counts == [counted, len(left), len(right)] and status == R.NO_STATUS


@pytest.mark.parametrize("name", C.NAMES)
def test_the_statement_equals_a_per_operation_loop(name):
    c = C.case(name)
    for run in c["runs"]:
        slow = R.stream_events(c["stream"], c["offs"], c["lengths"], c["ref_sel"], *run, per_record=R.record_by_operation)
        assert slow == C.want(name, run), run


@pytest.mark.parametrize("name", C.NAMES)
def test_the_heads_form_gives_the_same_events(name):
    c = C.case(name)
    stream, offs = C.heads(name)
    for run in c["runs"]:
        assert R.stream_events(stream, offs, c["lengths"], c["ref_sel"], *run, has_seq=False) == C.want(name, run), run


def test_the_statement_names_the_first_malformed_record():
    for name, run in C.pairs():
        assert C.want(name, run)[3] == (((C.MALFORMED[name] << 8) | 7) if name in C.MALFORMED else R.NO_STATUS), name


def test_the_cases_hold_what_they_are_named_for():
    c = C.case("chunks")
    n_ops = [R.parse(c["stream"], o)[4].shape[0] for o in c["offs"]]
    assert n_ops[:4] == [C.CH, C.CH + 1, C.CH + 2, 2 * C.CH + 1] and C.CH == _lib.COVER_CHUNK_OPS
    c = C.case("phases")
    assert {(int(o) + 36 + int(c["stream"][int(o) + 12])) % 4 for o in c["offs"]} == {0, 1, 2, 3}
    c = C.case("placeholder")
    assert [R.parse(c["stream"], o)[4].shape[0] for o in c["offs"]] == [5, 0, 0, 2, 65539]
    assert [len(C.case("records_%d" % n)["offs"]) for n in (0, 1, 63, 64, 65, 257, 4097)] == [0, 1, 63, 64, 65, 257, 4097]
    for run in C.case("records_4097")["runs"]:          # events on both sides of the scan's 4096-record block
        left, right, counts, _ = C.want("records_4097", run)
        assert counts[1] > 100 and counts[2] > 100
    # every run of every case but the malformed and the empty ones counts a record; most have events on both sides
    both = [k for k in C.pairs() if C.want(*k)[2][1] and C.want(*k)[2][2]]
    assert len(both) > len(C.pairs()) // 2


def test_the_site_statement_on_a_track_written_by_hand():
    lengths = [5, 3]
    offs, total = R.layout(lengths)
    assert offs == [0, 4096] and total == 8192
    left, right, depth = (np.zeros(total, dtype=np.int32) for _ in range(3))
    left[[0, 4, 5, 4096]] = [3, 2, 9, 3]               # element 5 is padding
    right[[2, 4, 4098]] = [3, 3, 1]
    depth[:] = 7
    assert R.sites_of(left, right, depth, lengths, 3) == [(0, 0, 3, 0, 7), (0, 2, 0, 3, 7), (0, 4, 2, 3, 7), (1, 0, 3, 0, 7)]
    assert R.sites_of(left, right, None, lengths, 1, [(1, 3), (4, 4097)]) == [(0, 2, 0, 3, 0), (0, 4, 2, 3, 0), (1, 0, 3, 0, 0)]
    assert R.sites_of(left, right, depth, lengths, 4) == []
    assert np.array_equal(np.flatnonzero(R.track_of([(0, 1), (1, 2), (0, 1)], lengths)), [1, 4098])
