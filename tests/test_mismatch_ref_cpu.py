"""The statement of mismatch_sites.py's semantics (tests/mismatch_ref.py) against the answers written by hand (tests/mismatch_cases.py:
EXPECTED, FASTA_EXPECTED, SITES_EXPECTED) and against code that was not written for this feature -- the cover statement of
tests/cover_ref.py: every mismatch lies on a base its record covers, so the mismatch track never exceeds the depth."""
import numpy as np
import pytest

import cover_ref
import mismatch_cases as C
import mismatch_ref as R
from gci_amd import _lib


def test_the_statement_gives_the_hand_written_events():
    for (name, run), (events, counts) in C.EXPECTED.items():
        got = C.want(name, run)
        assert (got[0], got[1]) == (events, counts), (name, run)


def test_the_statement_names_the_malformed_record():
    for name, rec in C.MALFORMED.items():
        assert C.want(name, C.case(name)["runs"][0])[2] == (rec << 8) | -_lib.GCI_E_MALFORMED, name
    for name in ("phases", "letters", "ends", "cg"):
        assert C.want(name, C.case(name)["runs"][0])[2] == R.NO_STATUS, name


def test_the_statement_gives_the_hand_written_codes_and_sites():
    for name, spans in C.FASTA_EXPECTED.items():
        codes = C.want_codes(name)
        for at, want in spans.items():
            assert codes[at:at + len(want)].tolist() == want, (name, at)
        assert (np.delete(codes, [at + k for at, want in spans.items() for k in range(len(want))]) == C.FILL).all()
    for (name, k), want in C.SITES_EXPECTED.items():
        assert C.want_sites(name, k) == want, (name, k)


def test_the_code_of_every_byte():
    want = {c: k for k, c in enumerate("=ACMGRSVTWYHKDBN") if k}
    for b in range(256):
        c = chr(b).upper() if b < 128 else "?"
        assert R.fasta_code(b) == (8 if c == "U" else want.get(c, 15)), b


@pytest.mark.parametrize("name", [n for n in C.NAMES if n not in C.MALFORMED])
def test_every_mismatch_lies_on_a_covered_base(name):
    c = C.case(name)
    offs, _ = R.layout(c["lengths"])
    for excl, min_mapq in c["runs"]:
        depth, _ = cover_ref.stream_depth(c["stream"], c["offs"], c["lengths"], c["ref_sel"], excl, min_mapq, False)
        events, counts, _ = C.want(name, (excl, min_mapq))
        track = R.track_of(events, c["lengths"])
        assert counts[1] <= counts[2]
        for k, L in enumerate(c["lengths"]):
            mine = track[offs[k]:offs[k] + L]
            assert (mine <= depth[k][:L]).all(), (name, k)
            assert (track[offs[k] + L:(offs[k + 1] if k + 1 < len(offs) else track.shape[0])] == 0).all()


def test_the_cases_hold_what_they_are_named_for():
    ops = lambda name, k: R.IR.parse(C.case(name)["stream"], C.case(name)["offs"][k])[4]        # noqa: E731
    assert ops("ops_64", 0).shape[0] == 64 and ops("ops_65", 0).shape[0] == 65
    assert ops("ops_2048", 0).shape[0] == C.CH and ops("ops_2049", 1).shape[0] == C.CH + 1
    assert ops("cg", 0).shape[0] > 65535
    assert max(int(w) >> 4 for w in ops("ont_hifi", 0)) <= 20 and max(int(w) >> 4 for w in ops("ont_hifi", 1)) >= 9000
    assert C.case("records_4097")["offs"].shape[0] == 4097
    # the walk of "ends" passes 2^31
    assert sum(int(w) >> 4 for w in ops("ends", 4)) + 50 > 2 ** 31
    edges = C.fasta_case("titles_on_edges")
    b = edges["bodies"]
    assert b[1, 0] > 4096 > b[0, 1] and b[2, 0] > 8192 > b[1, 1]                       # title lines over the tile edges
