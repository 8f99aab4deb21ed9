"""tests/route_ref.py (the vectorised statement the routing and seal kernels are held to in test_gpu_route.py) against per-item
loops: the `_NumpyOps` stand-ins of test_dist_cpu.py where they state a rule, a loop written here for the rules they leave out
(dropped intervals, PAF hits, names longer than their slot)."""
import types

import numpy as np
import pytest
import torch

import route_ref as R
from gci_amd.device import IVL_DTYPE, REC_DTYPE, name_hash_np
from test_dist_cpu import _NumpyOps

N = 389
SLOT = 32


@pytest.fixture(scope="module")
def case():
    """One input of a few hundred records: names of 1 .. SLOT bytes (repeated ones among them) behind one another in a blob."""
    rng = np.random.default_rng(401)
    pool = [bytes(rng.integers(33, 127, int(rng.integers(1, SLOT + 1)), dtype=np.uint8)) for _ in range(150)]
    pool[0], pool[1] = pool[0][:1], (pool[1] * SLOT)[:SLOT]              # the shortest and the longest a slot holds
    pick = rng.integers(0, len(pool), N)
    names = [pool[i] for i in pick]
    recs = np.zeros(N, dtype=REC_DTYPE)
    recs["name_hash"] = name_hash_np(names)
    recs["contig"] = rng.integers(0, 9, N)
    recs["start"] = rng.integers(0, 1 << 20, N)
    recs["end"] = recs["start"] + rng.integers(1, 30000, N)
    recs["qlen"] = rng.integers(1, 30000, N)
    recs["rec_idx"] = rng.permutation(N) + 1000
    recs["mapq"] = rng.integers(0, 61, N)
    recs["flags"] = rng.integers(0, 4, N)
    recs["name_len"] = [len(x) for x in names]
    delta = 36
    off = np.zeros(N, dtype=np.int64)
    blob = bytearray(b"\xee" * delta)
    for i, x in enumerate(names):
        blob += b"\xee" * int(rng.integers(0, 5))
        off[i] = len(blob) - delta
        blob += x
    blob += b"\xee" * 8
    return types.SimpleNamespace(recs=recs, blob=np.frombuffer(bytes(blob), dtype=np.uint8).copy(), off=off, delta=delta, names=names)


def _largest(dest, n_parts):
    return int(np.bincount(dest[dest >= 0], minlength=n_parts).max())


def _caps(largest):
    return [largest + 9, largest, largest - 1, largest // 2, 0]


@pytest.mark.parametrize("n_parts", [1, 3, 7])
def test_records_and_their_seal_equal_the_per_record_loop(case, n_parts):
    ops = _NumpyOps(None, None, REC_DTYPE)
    ji = types.SimpleNamespace(recs=torch.from_numpy(case.recs.view(np.uint8).reshape(N, 32).copy()), name_base=torch.from_numpy(case.blob.copy()),
                               name_off=torch.from_numpy(case.off.copy()), name_delta=case.delta)
    largest = _largest(R.record_dest(case.recs, n_parts), n_parts)
    assert 0 < largest < N
    rng = np.random.default_rng(7)
    for cap in _caps(largest):
        fill = rng.integers(1, 256, n_parts * (cap + 1) * 32, dtype=np.uint8)
        want_recs = torch.from_numpy(fill.reshape(-1, 32).copy())
        want_names = torch.zeros(n_parts * cap * SLOT, dtype=torch.uint8)
        want_status = np.zeros(1, dtype=np.int64)
        ops.route_records(ji, n_parts, cap, want_recs, want_names, SLOT, want_status)
        got_recs = fill.copy().view(REC_DTYPE)
        got_names = np.zeros(n_parts * cap * SLOT, dtype=np.uint8)       # (the loop zeroes every name slot, the contract only the written ones)
        status = R.route_records(case.recs, case.blob, case.off, case.delta, n_parts, cap, SLOT, got_recs, got_names)
        assert status == want_status[0] == (8 if largest > cap else -1)
        assert np.array_equal(got_recs.view(np.uint8), want_recs.numpy().reshape(-1))
        assert np.array_equal(got_names, want_names.numpy())
        # the receiving side: what arrived, with garbage flags beyond the counts
        got_recs["flags"] |= 0x80
        want_recs = torch.from_numpy(got_recs.view(np.uint8).reshape(-1, 32).copy())
        ops.route_seal_records(want_recs, n_parts, cap, want_status)
        assert R.seal_records(got_recs, n_parts, cap) == (8 if largest > cap else -1)
        assert np.array_equal(got_recs.view(np.uint8), want_recs.numpy().reshape(-1))
        dest = R.record_dest(case.recs, n_parts)
        assert (got_recs["flags"] != 0).sum() == np.minimum(np.bincount(dest[dest >= 0], minlength=n_parts), cap).sum()


@pytest.mark.parametrize("n_parts", [1, 3, 7])
def test_intervals_and_their_seal_equal_the_per_interval_loop(n_parts):
    ops = _NumpyOps(None, None, REC_DTYPE)
    rng = np.random.default_rng(402 + n_parts)
    n_contigs, max_n, count = 11, 300, 271
    ivl = np.zeros(max_n, dtype=IVL_DTYPE)
    ivl["contig"] = rng.integers(0, n_contigs, max_n)
    ivl["start"] = rng.integers(0, 1 << 20, max_n)
    ivl["end"] = ivl["start"] + rng.integers(1, 30000, max_n)
    owner = rng.integers(0, n_parts, n_contigs).astype(np.int32)
    cmap = rng.integers(-1, 5, n_contigs).astype(np.int32)
    largest = _largest(R.interval_dest(ivl, count, owner, n_parts), n_parts)
    for cap in _caps(largest):
        fill = rng.integers(1, 1 << 30, n_parts * (cap + 1) * 4).astype(np.int32)
        want = torch.from_numpy(fill.reshape(-1, 4).copy())
        want_status = np.zeros(1, dtype=np.int64)
        ops.route_intervals(torch.from_numpy(ivl.view(np.int32).reshape(max_n, 4).copy()), [count], owner, n_parts, cap, want, want_status)
        got = fill.copy().view(IVL_DTYPE)
        assert R.route_intervals(ivl, count, owner, n_parts, cap, got) == want_status[0] == (8 if largest > cap else -1)
        assert np.array_equal(got.view(np.int32), want.numpy().reshape(-1))
        # (the loop maps every contig it finds: keep the ones beyond the counts in range)
        b = got.reshape(n_parts, cap + 1)
        beyond = np.arange(cap + 1)[None, :] > np.minimum(b[:, 0]["start"], cap)[:, None]
        b["contig"][beyond] = rng.integers(0, n_contigs, int(beyond.sum()))
        want = torch.from_numpy(got.view(np.int32).reshape(-1, 4).copy())
        ops.route_seal_intervals(want, n_parts, cap, cmap, want_status)
        assert R.seal_intervals(got, n_parts, cap, cmap) == (8 if largest > cap else -1)
        assert np.array_equal(got.view(np.int32), want.numpy().reshape(-1))


def test_interval_drop_rules_equal_a_loop():
    rng = np.random.default_rng(403)
    n_parts, n_contigs, max_n = 3, 6, 200
    ivl = np.zeros(max_n, dtype=IVL_DTYPE)
    ivl["contig"] = rng.integers(-2, n_contigs + 2, max_n)
    ivl["start"] = np.arange(max_n)
    ivl["end"] = ivl["start"] + 5
    ivl["pad"] = 77
    owner = np.array([0, -1, 2, 3, 1, 2], dtype=np.int32)               # -1 and n_parts: nobody's
    cmap = np.array([4, -1, 0, 1, -1, 2], dtype=np.int32)
    for count in (0, 150, max_n, max_n + 50):
        for cap in (80, 20, 0):
            fill = rng.integers(1, 1 << 30, n_parts * (cap + 1) * 4).astype(np.int32)
            want, cnt = fill.copy().reshape(n_parts, cap + 1, 4), [0] * n_parts
            for i in range(min(count, max_n)):
                c = int(ivl["contig"][i])
                if 0 <= c < n_contigs and 0 <= owner[c] < n_parts:
                    if cnt[owner[c]] < cap:
                        want[owner[c], 1 + cnt[owner[c]]] = ivl[i].tolist()
                    cnt[owner[c]] += 1
            want[:, 0] = [(-1, x, 0, 0) for x in cnt]
            got = fill.copy().view(IVL_DTYPE)
            assert R.route_intervals(ivl, count, owner, n_parts, cap, got) == (8 if max(cnt) > cap else -1)
            assert np.array_equal(got.view(np.int32), want.reshape(-1))
            # seal: contigs outside the map and slots beyond the count become -1, a header count beyond cap keeps all cap slots
            got["contig"][1::3] = rng.integers(-9, n_contigs + 9, got[1::3].shape[0])
            got["start"][0] = cap + 5
            want = got.copy().reshape(n_parts, cap + 1)
            for d in range(n_parts):
                for k in range(1, cap + 1):
                    c = int(want[d, k]["contig"])
                    want[d, k]["contig"] = cmap[c] if k <= min(int(want[d, 0]["start"]), cap) and 0 <= c < n_contigs else -1
            assert R.seal_intervals(got, n_parts, cap, cmap) == 8
            assert np.array_equal(got, want.reshape(-1))


@pytest.mark.parametrize("n_parts", [1, 5])
def test_hits_and_names_longer_than_a_slot_equal_a_loop(case, n_parts):
    rng = np.random.default_rng(404)
    slot = 16                                                            # many of the names are longer
    hits = np.zeros(N, dtype=R.HIT_DTYPE)
    hits["qn_off"], hits["qn_len"], hits["qhash"] = case.off + case.delta, case.recs["name_len"], case.recs["name_hash"]
    for f in ("qlen", "qs", "qe", "ts", "te", "t", "hq", "slot"):
        hits[f] = rng.integers(1, 1000, N)
    hits["identity"] = rng.random(N)
    largest = _largest(R.hash_dest(hits["qhash"], n_parts), n_parts)
    for cap in _caps(largest):
        fill_h = rng.integers(1, 256, n_parts * (cap + 1) * 80, dtype=np.uint8)
        fill_n = rng.integers(1, 256, n_parts * cap * slot, dtype=np.uint8)
        want_h, want_n, cnt, long_name = fill_h.copy().view(R.HIT_DTYPE).reshape(n_parts, cap + 1), fill_n.copy().reshape(n_parts, cap, slot), [0] * n_parts, False
        for i in range(N):
            d = (int(hits["qhash"][i]) >> 33) % n_parts
            if cnt[d] < cap:
                want_h[d, 1 + cnt[d]] = hits[i]
                o, l = int(hits["qn_off"][i]), int(hits["qn_len"][i])
                want_n[d, cnt[d]] = list(case.blob[o:o + min(l, slot)]) + [0] * (slot - min(l, slot))
                long_name |= l > slot
            cnt[d] += 1
        want_h[:, 0] = np.zeros((), dtype=R.HIT_DTYPE)
        want_h[:, 0]["qhash"], want_h[:, 0]["t"] = cnt, -1
        got_h, got_n = fill_h.copy().view(R.HIT_DTYPE), fill_n.copy()
        status = R.route_hits(hits, case.blob, n_parts, cap, slot, got_h, got_n)
        assert status == (8 if max(cnt) > cap or long_name else -1)
        assert np.array_equal(got_h, want_h.reshape(-1)) and np.array_equal(got_n, want_n.reshape(-1))
        # the same names as records: one loop states both kinds
        recs = case.recs.copy()
        recs["flags"] |= 1
        got_r, got_n = np.zeros(n_parts * (cap + 1), dtype=REC_DTYPE), fill_n.copy()
        assert R.route_records(recs, case.blob, case.off, case.delta, n_parts, cap, slot, got_r, got_n) == status
        assert np.array_equal(got_n, want_n.reshape(-1))
    assert (case.recs["name_len"] > slot).any() and (case.recs["name_len"] <= slot).any()
