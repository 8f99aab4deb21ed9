"""The statement of the join's record verdicts (tests/joinfate_ref.py) against the oracle's name_join -- the names it calls `joined`
and their intervals are the oracle's file1 -- and against a per-item replay of the reference's dict overwrite for `shadowed`."""
import numpy as np
import pytest

import joinfate_cases as JC
import joinfate_ref as J


def as_dicts(files):
    """What read_sam / the PAF filter leave per file: name -> (contig, start, end, qlen), inserted contig by contig in file order, a
    later record of a name overwriting the earlier (GCI.py:166, 269); and the high-quality names."""
    dicts, hq, last = [], set(), []
    for recs, names in files:
        d, where = {}, {}
        idx = [i for i in range(recs.shape[0]) if int(recs["flags"][i]) & J.PASS]
        for i in sorted(idx, key=lambda i: (int(recs["contig"][i]), i)):
            k = J.key_of(recs, names, i)
            d[k] = tuple(int(recs[f][i]) for f in ("contig", "start", "end", "qlen"))
            where[k] = i
            if int(recs["flags"][i]) & J.HQ:
                hq.add(k)
        dicts.append(d)
        last.append(where)
    return dicts, hq, last


@pytest.mark.parametrize("name, op", [p for p in JC.pairs() if JC.want(*p)[2] == J.NO_STATUS])       # (with a status the reference raises)
def test_joined_is_what_the_oracle_keeps(oracle, name, op):
    fate, counts, status, kept = JC.want(name, op)
    dicts, hq, _ = as_dicts(JC.case(name)["files"])
    want = {k: tuple(v[:3]) for k, v in oracle.name_join(dicts, hq, op).items()}
    assert kept == want
    joined = set()
    for (recs, names), b in zip(JC.case(name)["files"], fate):
        joined |= {J.key_of(recs, names, i) for i in np.flatnonzero(b == J.JOINED).tolist()}
    assert joined == set(want)


@pytest.mark.parametrize("name", JC.NAMES)
def test_shadowed_is_the_dict_overwrite_and_the_counts_add_up(name):
    c = JC.case(name)
    fate, counts, _, _ = JC.want(name, c["ops"][0])
    _, _, last = as_dicts(c["files"])
    for f, ((recs, names), b) in enumerate(zip(c["files"], fate)):
        passing = (recs["flags"] & J.PASS) != 0
        assert np.array_equal(b != 0, passing)
        for i in np.flatnonzero(passing).tolist():
            assert (b[i] == J.SHADOWED) == (last[f][J.key_of(recs, names, i)] != i), (f, i)
        assert int(counts[f].sum()) == recs.shape[0] and int(counts[f][J.SHADOWED:J.JOINED + 1].sum()) == int(passing.sum())


def test_the_cases_reach_every_verdict_and_every_branch():
    seen = set()
    for name, op in JC.pairs():
        fate, _, status, _ = JC.want(name, op)
        seen |= set(np.concatenate(fate).tolist())
        if name == "zero_qlen_reached":
            assert status == J.word(7, J.E_ZERO_DIV)
        elif name.startswith("zero_qlen"):
            assert status == J.NO_STATUS
    assert seen == {0, J.SHADOWED, J.UNPAIRED, J.CONTIG, J.OVERLAP, J.JOINED}
    by = {n: [b.tolist() for b in JC.want(n, JC.case(n)["ops"][0])[0]] for n in JC.NAMES}
    assert [JC.want("quotient", op)[0][1].tolist() for op in JC.case("quotient")["ops"]] == [
        [J.JOINED, J.OVERLAP, J.JOINED], [J.OVERLAP, J.OVERLAP, J.JOINED], [J.JOINED, J.OVERLAP, J.JOINED]]
    assert by["hq_shadowed"][0] == [J.SHADOWED, J.JOINED, J.SHADOWED, J.UNPAIRED]
    assert by["hq_absent_from_file0"][1] == [J.JOINED, J.UNPAIRED]
    assert by["delete_resurrect"][2] == [J.JOINED, J.CONTIG]
    assert by["delete_resurrect_delete"][3] == [J.OVERLAP, J.CONTIG]
    assert by["winner_by_contig"] == [[J.JOINED, J.SHADOWED], [J.JOINED]]
    assert by["one_file"] == [[J.SHADOWED, 0, J.JOINED, J.JOINED]]
    assert by["empty_file_of_three"] == [[J.JOINED, J.UNPAIRED], [], [J.JOINED, J.UNPAIRED]]
