"""The statement of indel_sites.py's semantics (tests/indels_ref.py) against the answers written by hand (tests/indels_cases.py: EXPECTED,
SITES_EXPECTED), against code that was not written for this feature -- the cover statement of tests/cover_ref.py: what counting
deletions as covered adds to the depth is the del track at min_len 1 --, and that the cases hold what they are named for."""
import numpy as np
import pytest

import cover_ref
import indels_cases as C
import indels_ref as R
from gci_amd import _lib


@pytest.mark.parametrize("key", list(C.EXPECTED), ids=lambda k: "%s-%x-%d-%d" % ((k[0],) + k[1]))
def test_the_statement_gives_the_hand_written_events(key):
    dels, inss, counted = C.EXPECTED[key]
    got_dels, got_inss, counts, status = C.want(*key)
    assert (got_dels, got_inss) == (dels, inss)
    assert counts == [counted, len(dels), len(inss)] and status == R.NO_STATUS


@pytest.mark.parametrize("name", C.NAMES)
def test_counting_deletions_as_covered_adds_the_del_track(name):
    """cover_ref's depth with count_del minus the one without it is, per base, the D operations over it: the del track at min_len 1."""
    c = C.case(name)
    offs, _ = R.layout(c["lengths"])
    for excl, min_mapq in sorted({run[:2] for run in c["runs"]}):
        with_del, _ = cover_ref.stream_depth(c["stream"], c["offs"], c["lengths"], c["ref_sel"], excl, min_mapq, True)
        without, _ = cover_ref.stream_depth(c["stream"], c["offs"], c["lengths"], c["ref_sel"], excl, min_mapq, False)
        dels = R.stream_events(c["stream"], c["offs"], c["lengths"], c["ref_sel"], excl, min_mapq, 1)[0]
        track = R.track_of(dels, c["lengths"])
        for k, L in enumerate(c["lengths"]):
            assert np.array_equal(with_del[k] - without[k], track[offs[k]:offs[k] + L]), (excl, min_mapq, k)
        assert int(track.sum()) == sum(b - a + 1 for _, a, b in dels)      # nothing of a track lies in the padding


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
    ops = [R.parse(c["stream"], o)[4] for o in c["offs"]]
    assert [o.shape[0] for o in ops[:4]] == [C.CH, C.CH + 1, C.CH + 2, 2 * C.CH + 1] and C.CH == _lib.COVER_CHUNK_OPS
    word = lambda op, n: (n << 4) | op                   # noqa: E731
    assert int(ops[0][C.CH - 1]) == word(C.D, 20) and int(ops[1][C.CH]) == word(C.I, 20) and int(ops[2][C.CH]) == word(C.D, 20)
    assert [int(ops[3][k]) for k in (C.CH - 1, C.CH, 2 * C.CH - 1, 2 * C.CH)] == [word(C.D, 20), word(C.D, 21), word(C.I, 22), word(C.D, 23)]
    # the long D behind a boundary lies where the chunks in front put it: not at pos, not at pos + what chunk 1 alone holds
    (_, start, _), = [d for d in C.want("chunks", (C.EXCL, 0, 23))[0]]
    assert start > 30000 + 2 * C.CH // 2
    c = C.case("wave_rounds")
    ops = [R.parse(c["stream"], o)[4] for o in c["offs"]]
    assert int(ops[0][63]) & 0xF == C.D and int(ops[0][64]) & 0xF == C.I and int(ops[1][63]) & 0xF == C.I and int(ops[1][64]) & 0xF == C.D
    assert C.want("wave_rounds", (C.EXCL, 0, 3))[2] == [5, 2 + 64 + 70, 2 + 64 + 70] and C.want("wave_rounds", (C.EXCL, 0, 4))[2] == [5, 2 + 70, 2]
    c = C.case("phases")
    assert {(int(o) + 36 + int(c["stream"][int(o) + 12])) % 4 for o in c["offs"]} == {0, 1, 2, 3}
    c = C.case("placeholder")
    assert [R.parse(c["stream"], o)[4].shape[0] for o in c["offs"]] == [5, 2, 2, 2, 65539]
    assert C.want("placeholder", (C.EXCL, 0, 1))[2] == [5, 1, 1 + 32768] and C.want("placeholder", (C.EXCL, 0, 2))[2] == [5, 1, 1]
    assert [len(C.case("records_%d" % n)["offs"]) for n in (0, 1, 63, 64, 65, 257, 4097)] == [0, 1, 63, 64, 65, 257, 4097]
    for run in C.case("records_4097")["runs"]:          # events of both kinds on both sides of the scan's 4096-record block
        _, _, counts, _ = C.want("records_4097", run)
        assert counts[1] > 100 and counts[2] > 100
    # the skip rule: every run drops other records
    counted = [C.want("skip_rule", run)[2][0] for run in C.case("skip_rule")["runs"]]
    assert len(set(counted[:5])) == 5 and counted[5] == counted[0] and C.want("skip_rule", C.case("skip_rule")["runs"][5])[2][1:] == [0, 0]


@pytest.mark.parametrize("key", list(C.SITES_EXPECTED), ids=lambda k: "%s-%d" % k)
def test_the_site_statement_gives_the_hand_written_sites(key):
    assert [s[:5] for s in C.want_sites(*key)] == C.SITES_EXPECTED[key]
    c = C.site_case(key[0])
    offs, _ = R.layout(c["lengths"])
    for (contig, start, end, _, _, depth), bare in zip(C.want_sites(*key), C.want_sites(*key, with_depth=False)):
        assert depth == int(c["depth"][offs[contig] + start:offs[contig] + end].max()) and bare[:5] + (0,) == bare


def test_the_site_cases_hold_what_they_are_named_for():
    lengths = [end - start for _, start, end, _, _, _ in C.want_sites("runs", 0)]
    assert sorted(lengths) == [1, 3, 10, 63, 64, 64, 65, 9000]
    by_start = {s[1]: s for s in C.want_sites("runs", 0)}
    c = C.site_case("runs")
    assert by_start[300][3:] == (9, 0, 99) and c["dele"][300] == 9 and c["depth"][300] == 99             # the maxima at the first element
    assert by_start[500][4:] == (8, 98) and c["ins"][564] == 8 and c["depth"][564] == 98                 # ... at the last
    assert by_start[10000][3:] == (7, 11, 97)
    assert [s[:3] for s in C.want_sites("runs", 3)][-1] == (0, 10000, 12000)                             # cut by the window's end
    assert [s[:3] for s in C.want_sites("runs", 5)] == [(0, 4096, 4097)] and [s[:3] for s in C.want_sites("runs", 6)] == [(0, 4093, 4099)]
