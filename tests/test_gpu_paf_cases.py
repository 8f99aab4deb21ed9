"""K2 (k_paf.hip) on the tables of tests/paf_cases.py -- line starts at every seam of k_paf_lines, both instantiations of the tokeniser
and the limit between them, the grammar byte by byte, the scoring's block shapes, the first error -- against the oracle
(oracle.paf_filter).  Three forms of the filter: engine.paf_filter over files, engine.paf_filter_text over the files back to back, and
for tables A and B the two halves of the sharded run (paf_hits_text -> route_hits -> paf_score_hits) with 1 and 3 ranks played in turn.
tests/test_paf_cases_cpu.py shows that the cases are sound and have the geometry their names claim."""
import numpy as np
import pytest

import paf_cases as P
from gci_amd._lib import GciError, REC_HQ
from gci_amd.device import REC_DTYPE
from test_paf_cases_cpu import STATUS_OF, write_files

pytestmark = pytest.mark.gpu


def dicts_of(inputs, targets):
    """JoinInputs as the reference's (paf_lines, high_qual)."""
    per_file, hq = [], set()
    for ji in inputs:
        r = ji.recs.cpu().numpy().reshape(-1).view(REC_DTYPE)
        off = ji.name_off.cpu().numpy()
        text = ji.name_base.cpu().numpy()
        d = {}
        for i in range(r.shape[0]):
            q = bytes(text[int(off[i]):int(off[i]) + int(r["name_len"][i])]).decode()
            assert q not in d
            d[q] = (targets[int(r["contig"][i])], int(r["start"][i]), int(r["end"][i]), int(r["qlen"][i]))
            if int(r["flags"][i]) & REC_HQ:
                hq.add(q)
        per_file.append(d)
    return per_file, hq


def from_files(engine, paths, files, targets, args):
    return dicts_of(engine.paf_filter(paths, targets, *args), targets)


def from_text(engine, paths, files, targets, args):
    text = np.frombuffer(b"".join(files) + bytes(16), dtype=np.uint8)
    return dicts_of(engine.paf_filter_text(engine.to_device(text), np.cumsum([len(f) for f in files], dtype=np.uint64), targets, *args), targets)


def two_stage(world):
    """Stage A over every rank's byte range of every file, the hits routed by query hash, stage B per owner on what its all-to-all would
    deliver: the union over the owners."""
    def run(engine, paths, files, targets, args):
        import torch
        from gci_amd import shard
        from gci_amd.device import name_hash_np
        raws = [np.frombuffer(f, dtype=np.uint8) for f in files]
        dev, B = engine.device, engine.PAF_HIT_BYTES
        slot_bytes = 16 * (max([len(ln.split(b"\t")[0]) for f in files for ln in f.splitlines()] + [1]) // 16 + 1)
        sent = []                                                     # [rank][file] = (buckets, names, cap)
        for r in range(world):
            parts = [raw[slice(*shard.byte_range_of_rank(raw, r, world))] for raw in raws]
            ends = np.cumsum([x.shape[0] for x in parts], dtype=np.uint64)
            d_text = engine.to_device(np.concatenate(parts + [np.zeros(16, np.uint8)]))
            per_file = []
            for h in engine.paf_hits_text(d_text, ends, targets, *args):
                cap = int(h.shape[0]) + 8
                sh = torch.zeros((world * (cap + 1), B), dtype=torch.uint8, device=dev)
                sn = torch.zeros(world * cap * slot_bytes, dtype=torch.uint8, device=dev)
                st = torch.full((1,), -1, dtype=torch.int64, device=dev)
                engine.route_hits(h, d_text, world, cap, sh, sn, slot_bytes, st)
                assert int(st.item()) == -1
                per_file.append((sh.view(world, cap + 1, B), sn.view(world, cap, slot_bytes), cap))
            sent.append(per_file)
        got, got_hq = [dict() for _ in files], set()
        for d in range(world):
            dense, names, upto, base = [], [], [0], 0
            for f in range(len(files)):
                n_f = 0
                for r in range(world):
                    bk, nm, cap = sent[r][f]
                    c = int(bk[d, 0, 8:16].contiguous().view(torch.int64).item())
                    part = bk[d, 1:1 + c].clone()
                    if c:
                        part[:, 0:8] = (base + torch.arange(c, dtype=torch.int64, device=dev) * slot_bytes).view(torch.uint8).view(c, 8)
                    dense.append(part)
                    names.append(nm[d, :c].reshape(-1))
                    base += c * slot_bytes
                    n_f += c
                upto.append(upto[-1] + n_f)
            d_names = torch.cat(names + [torch.zeros(16, dtype=torch.uint8, device=dev)])
            d_hits = torch.cat(dense) if upto[-1] else torch.zeros((1, B), dtype=torch.uint8, device=dev)
            per_file, hq = dicts_of(engine.paf_score_hits(d_names, d_hits, upto, targets), targets)
            for f, dd in enumerate(per_file):
                for q in dd:
                    assert q not in got[f] and (int(name_hash_np([q.encode()])[0]) >> 33) % world == d
                got[f].update(dd)
            got_hq |= hq
        return got, got_hq
    return run


FORMS = {"files": from_files, "text": from_text, "two_stage_1": two_stage(1), "two_stage_3": two_stage(3)}


@pytest.fixture(scope="module")
def wanted(oracle, tmp_path_factory):
    """name -> (paths, what the oracle does with the case: ("ok", dicts, hq) or ("err", status)), computed once."""
    tmp = tmp_path_factory.mktemp("paf_cases")
    memo = {}

    def get(name):
        if name not in memo:
            _, files, targets, args = P.case(name)
            paths = write_files(tmp, name, files)
            try:
                memo[name] = (paths, ("ok",) + tuple(oracle.paf_filter(paths, targets, *args)))
            except tuple(STATUS_OF) as e:
                memo[name] = (paths, ("err", STATUS_OF[type(e)]))
        return memo[name]
    return get


def check(engine, wanted, name, forms):
    _, files, targets, args = P.case(name)
    expect = P.EXPECT[name]
    paths, want = wanted(name)
    for form in forms:
        if expect is None:
            assert want[0] == "ok", name
            got = FORMS[form](engine, paths, files, targets, args)
            assert got[1] == want[2] and got[0] == want[1], (name, form)
            continue
        if expect[0] == "raises":
            assert want[0] == "err", name
            status, line = want[1], expect[2]
        else:
            assert want[0] == "ok", name                               # the reference goes on; the status is this project's
            _, status, line = expect
        with pytest.raises(GciError) as e:
            FORMS[form](engine, paths, files, targets, args)
        assert e.value.status == status and (line is None or e.value.rec == line), (name, form, e.value.status, e.value.rec)


@pytest.mark.parametrize("table", ["A", "B"])
def test_line_starts_and_tokeniser_paths(engine, wanted, table):
    for name in P.GPU[table]:
        # (the halves of the sharded run report a line by its place in the rank's range, and no scoring error of the reference's
        # order: a case that raises goes through the whole-file forms)
        check(engine, wanted, name, FORMS if P.EXPECT[name] is None else ("files", "text"))


def test_both_tokeniser_paths_give_the_same_table(engine, wanted):
    """Table C through the LDS instantiation and, padded, through the global one: the same dicts but for the one line the padded file
    ends with -- and each equal to the oracle's (test_line_starts_and_tokeniser_paths[B], test_grammar_scoring_first_error[C])."""
    res = []
    for name in ("c_accepted", "c_accepted_global"):
        _, files, targets, args = P.case(name)
        d, hq = from_files(engine, wanted(name)[0], files, targets, args)
        res.append(({q: v for q, v in d[0].items() if q != P.GLOBAL_EXTRA}, hq - {P.GLOBAL_EXTRA}))
    assert res[0] == res[1] and len(res[0][0]) > 250


def test_which_workgroups_leave_lds(engine, wanted):
    """The two walks give the same hits, so the results above cannot say which one ran: the library counts the workgroups that
    walked global memory.  Their number is the number of stretches beyond 49152 bytes computed from the bytes (the uploaded text
    begins at a 16-byte boundary: asserted) -- one of three for lds_limit, whose second stretch is 49152 and whose third 49153."""
    for name, (f, _) in P.STRETCHES.items():
        _, files, targets, args = P.case(name)
        text = engine.to_device(np.frombuffer(b"".join(files) + bytes(16), dtype=np.uint8))
        assert text.data_ptr() % 16 == 0
        try:
            engine.paf_filter_text(text, np.cumsum([len(x) for x in files], dtype=np.uint64), targets, *args)
        except GciError:
            assert P.EXPECT[name] is not None, name
        want = sum(s > P.LDS_BYTES for k in range(len(files)) for s in P.stretches(files, k))
        assert engine.paf_global_groups() == want, (name, engine.paf_global_groups(), want)
    for name, n in (("lds_limit", 1), ("lds_limit_delta5", 1), ("c_accepted", 0), ("c_accepted_global", 2), ("one_long_line", 1)):
        assert sum(s > P.LDS_BYTES for s in P.stretches(P.case(name)[1], P.STRETCHES[name][0])) == n, name


@pytest.mark.parametrize("table", ["C", "D", "E"])
def test_grammar_scoring_first_error(engine, wanted, table):
    for name in P.GPU[table]:
        check(engine, wanted, name, ("files", "text"))
    if table == "D":                                                     # the scoring once more behind the routing: stage B alone
        for name in P.GPU[table]:
            check(engine, wanted, name, ("two_stage_1", "two_stage_3"))
