"""The tables of tests/paf_cases.py before a GPU sees them: for every case the oracle (oracle.paf_filter, GCI.py:211-254 statement for
statement: the authority) against the plain-Python statement of the rules (tests/paf_ref.py) and the native host filter
(pipeline.paf_filter, host_io.cpp, which shares the kernels' grammar).  Where the reference raises, the class of its exception is the
status of the host filter and the line is the one the case names -- shown on the oracle itself: the file cut in front of that line goes
through, cut behind it it raises.  And the geometry the cases' names claim -- every seam position, every delta, the 49152 / 49153 pair of
the tokeniser's workgroups -- computed from the bytes."""
import os

import pytest

import paf_cases as P
from gci_amd._lib import GciError, GCI_E_MALFORMED, GCI_E_ZERO_DIV
from gci_amd.pipeline import paf_filter
from paf_ref import paf_filter_py

STATUS_OF = {IndexError: GCI_E_MALFORMED, ValueError: GCI_E_MALFORMED, ZeroDivisionError: GCI_E_ZERO_DIV}


def write_files(tmp, name, files):
    paths = []
    for k, b in enumerate(files):
        p = os.path.join(str(tmp), "%s.%d.paf" % (name, k))
        with open(p, "wb") as f:
            f.write(b)
        paths.append(p)
    return paths


def outcome(fn, paths, targets, args):
    """("ok", dicts, high-quality set) or ("err", status, line or None)."""
    try:
        d, hq = fn(paths, targets, *args)
        return ("ok", d, hq)
    except tuple(STATUS_OF) as e:
        return ("err", STATUS_OF[type(e)], None)
    except GciError as e:
        return ("err", e.status, e.rec)


def oracle_outcomes(oracle, tmp, name, files, targets, args, expect):
    """The oracle on the case and, for a raising one, on the file cut in front of and behind the line it names."""
    paths = write_files(tmp, name, files)
    want = outcome(oracle.paf_filter, paths, targets, args)
    if expect is not None and expect[0] == "raises":
        _, f, line = expect
        assert want[0] == "err", name
        if line > 0:
            st = P.line_starts(files[f]).tolist() + [len(files[f])]
            for upto, raises in ((line - 1, False), (line, True)):
                cut = write_files(tmp, name + ".cut", files[:f] + [files[f][:st[upto]]])
                o = outcome(oracle.paf_filter, cut, targets, args)
                assert (o[0] == "err") == raises and (not raises or o[1] == want[1]), (name, upto)
        else:                                                  # raised while scoring file f: reading the files up to it goes through
            for p in paths[:f + 1]:
                for ln in open(p, "rb").read().splitlines():
                    assert P.replay(ln, targets) is None, name
    else:
        assert want[0] == "ok", (name, want)
    return paths, want


@pytest.mark.parametrize("table", sorted(P.TABLES))
def test_cases_against_the_oracle(oracle, tmp_path, table):
    for name, files, targets, args in P.TABLES[table]:
        expect = P.EXPECT[name]
        paths, want = oracle_outcomes(oracle, tmp_path, name, files, targets, args, expect)
        py = outcome(paf_filter_py, paths, targets, args)
        host = outcome(paf_filter, paths, targets, args)
        assert py[:2] == want[:2] and (want[0] == "err" or py[2] == want[2]), name
        if expect is None:
            assert host == want, name
        elif expect[0] == "raises":
            assert host == ("err", want[1], expect[2]), (name, host, want)
        else:
            _, status, line = expect
            assert host[:2] == ("err", status) and (line is None or host[2] == line), (name, host)


def test_global_path_table_is_the_same_table(oracle, tmp_path):
    """c_accepted_global is c_accepted with padding: the same dicts but for the one line added at the end."""
    res = []
    for name in ("c_accepted", "c_accepted_global"):
        _, files, targets, args = P.case(name)
        d, hq = oracle.paf_filter(write_files(tmp_path, name, files), targets, *args)
        res.append(({q: v for q, v in d[0].items() if q != P.GLOBAL_EXTRA}, hq - {P.GLOBAL_EXTRA}))
    assert res[0] == res[1] and len(res[0][0]) > 250


def test_seams_are_where_the_names_say():
    deltas = set()
    for name, g in P.SEAMS.items():
        files = P.case(name)[1]
        B, place = g["B"], g["place"]
        delta, before, at, starts_at, starts_behind, starts_in_tile = P.seam_geometry(files, g["file"], B)
        assert delta == g["delta"], name
        if place == "last":
            assert before in (b"\n", b"\r") and at not in (b"\n", b"\r") and starts_at, name
            if "crlf" in name or "mix" in name:
                assert files[g["file"]][B - delta - 2:B - delta] == b"\r\n", name
        elif place == "first":
            assert before == b"\r" and at == b"\n" and starts_behind and not starts_at, name
        else:
            assert before == b"\r" and at not in (b"\n", b"\r") and starts_at, name
            if "mix" not in name:                               # the only "\r" of the file that no "\n" follows
                assert files[g["file"]].count(b"\r") - files[g["file"]].count(b"\r\n") == 1, name
        if B == 8192:
            assert starts_in_tile == 0, name                    # a tile of k_paf_lines without a line start
        if g["file"] == 1:
            deltas.add(delta)
    assert deltas == set(range(16))
    assert {(g["B"], g["place"]) for g in P.SEAMS.values()} == {(B, p) for B in P.BOUNDS for p in ("last", "first", "lone")}


def test_workgroup_stretches_are_what_the_names_say():
    for name, (f, want) in P.STRETCHES.items():
        got = P.stretches(P.case(name)[1], f)
        if want == "lds":
            assert max(got) <= P.LDS_BYTES, name
        elif want == "global":
            assert min(got) > P.LDS_BYTES, name
        else:
            assert got == want, (name, got)
    assert P.STRETCHES["lds_limit"][1][1:] == [49152, 49153] and P.STRETCHES["lds_limit_delta5"][1][1:] == [49152, 49153]
    # the alignment term is part of the two sums: the groups' own bytes fall short of them by it
    for name in ("lds_limit", "lds_limit_delta5"):
        f = P.STRETCHES[name][0]
        files = P.case(name)[1]
        st = P.line_starts(files[f])
        base = sum(len(x) for x in files[:f])
        al = [(base + int(st[g])) % 16 for g in (0, 256, 512)]
        assert int(st[512] - st[256]) == 49152 - al[1] and len(files[f]) - int(st[512]) == 49153 - al[2] and st.shape[0] == 768, name
    assert any(a for a in al[1:])
