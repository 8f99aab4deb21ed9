"""The exchange steps of the name-hash-sharded join (gci_amd/csrc/k_shard.hip) held directly to tests/route_ref.py: every byte of
the bucket array, of the name slots and of the status word, the outputs pre-filled so that "left alone" is compared as well.
The shapes are the ones the product never runs: up to 64 parts, a count table longer than one scan tile, chunk edges, buckets
filled to cap and one over, names at every alignment and as long as their slot, counts beyond the arrays, garbage beyond the counts."""
import functools
import types

import numpy as np
import pytest
import torch

import route_ref as R
from gci_amd import shard
from gci_amd._lib import GCI_E_INVALID, GciError
from gci_amd.device import IVL_DTYPE, REC_DTYPE, JoinInput, name_hash_np

pytestmark = pytest.mark.gpu

FILL = 0xA5
ST_FILL = 0x5A5A5A5A5A5A5A5A
CHUNK = 4096                       # ROUTE_CHUNK
SIZES = [0, 1, 255, 256, 4095, 4096, 4097, 12_289]


# ---- inputs, built with numpy ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pool(seed, n_pool, lo, hi):
    """n_pool distinct-looking names of lo .. hi bytes as a fixed-width matrix (zero behind a name), their lengths and hashes."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n_pool)
    lens[:min(n_pool, hi - lo + 1)] = np.arange(lo, hi + 1)[:n_pool]           # every length, if the pool is large enough
    mat = rng.integers(33, 127, (n_pool, max(hi, 1)), dtype=np.uint8)
    mat[np.arange(max(hi, 1))[None, :] >= lens[:, None]] = 0
    hashes = name_hash_np([mat[i, :lens[i]].tobytes() for i in range(n_pool)])
    return types.SimpleNamespace(mat=mat, lens=lens, hashes=hashes)


def _blob(mat, lens, start):
    """The names behind one another at `start` (ascending, not overlapping), every other byte non-zero."""
    n = int(lens.shape[0])
    size = (int((start + lens).max()) if n else 0) + 64
    blob = np.full(size, 0xEE, dtype=np.uint8)
    if n:
        col = np.arange(mat.shape[1])
        use = col[None, :] < lens[:, None]
        blob[(start[:, None] + col[None, :])[use]] = mat[use]
    return blob


@functools.lru_cache(maxsize=None)
def _records(seed, n, n_pool=4096, lo=1, hi=40, delta=0, drop_seventh=True):
    """n records whose names come from a pool (so names repeat), at starts of every residue mod 4."""
    rng = np.random.default_rng(seed)
    pool = _pool(seed + 1, n_pool, lo, hi)
    pick = rng.integers(0, n_pool, n)
    lens = pool.lens[pick]
    gap = rng.integers(1, 5, n)
    start = 40 + np.cumsum(gap + lens) - lens
    recs = np.zeros(n, dtype=REC_DTYPE)
    recs["name_hash"] = pool.hashes[pick]
    recs["contig"] = rng.integers(0, 50, n)
    recs["start"] = rng.integers(0, 1 << 24, n)
    recs["end"] = recs["start"] + rng.integers(1, 30_000, n)
    recs["qlen"] = rng.integers(1, 30_000, n)
    recs["rec_idx"] = np.arange(n)
    recs["mapq"] = rng.integers(0, 61, n)
    recs["flags"] = 1 | (rng.integers(0, 2, n) << 1)
    if drop_seventh:
        recs["flags"][6::7] &= 2
    recs["name_len"] = lens
    return types.SimpleNamespace(recs=recs, blob=_blob(pool.mat[pick], lens, start), off=(start - delta).astype(np.int64), delta=delta)


def _as_hits(case, seed=5):
    """The same names as PAF hits: qn_off / qn_len / qhash from the records, the other fields anything."""
    rng = np.random.default_rng(seed)
    n = case.recs.shape[0]
    hits = np.zeros(n, dtype=R.HIT_DTYPE)
    hits["qn_off"], hits["qn_len"], hits["qhash"] = case.off + case.delta, case.recs["name_len"], case.recs["name_hash"]
    for f in ("qlen", "qs", "qe", "ts", "te"):
        hits[f] = rng.integers(-5, 1 << 40, n)
    hits["identity"] = rng.random(n)
    hits["t"], hits["hq"], hits["slot"] = rng.integers(0, 50, n), rng.integers(0, 2, n), np.arange(n)
    return hits


def _aligned_names(slot, delta, extra_long=False):
    """Every length 0 .. slot at each of the four residues of (name_off + name_delta) mod 4; extra_long: one name of slot + 1 bytes more."""
    rng = np.random.default_rng(slot + delta)
    lens = np.repeat(np.arange(slot + 1), 4)
    res = np.tile(np.arange(4), slot + 1)
    if extra_long:
        lens, res = np.append(lens, slot + 1), np.append(res, 3)
    n = lens.shape[0]
    stride = (slot + 12) // 4 * 4
    start = 40 + np.arange(n) * stride + res
    mat = rng.integers(33, 127, (n, slot + 1), dtype=np.uint8)
    recs = np.zeros(n, dtype=REC_DTYPE)
    recs["name_hash"] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    recs["rec_idx"], recs["flags"], recs["name_len"], recs["qlen"] = np.arange(n), 1, lens, 100
    off = (start - delta).astype(np.int64)
    seen = {(int(l), int(r)) for l, r in zip(lens, (off + delta) % 4)}
    assert all((l, r) in seen for l in range(slot + 1) for r in range(4)) and off.min() >= 0
    return types.SimpleNamespace(recs=recs, blob=_blob(mat, lens, start), off=off, delta=delta)


def _largest(dest, n_parts):
    return int(np.bincount(dest[dest >= 0], minlength=n_parts).max()) if dest.shape[0] else 0


# ---- one call on the device against the statement ----------------------------------------------------------------------------------

def _up(engine, a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape[0], a.dtype.itemsize)
    return torch.from_numpy(a.copy()).to(engine.device)


def _filled(engine, *shape):
    return torch.full(shape, FILL, dtype=torch.uint8, device=engine.device)


def _status(engine):
    return torch.full((1,), ST_FILL, dtype=torch.int64, device=engine.device)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.shape[0] == 0, "%s: %d bytes differ, the first at %d (got %d, want %d)" % (what, bad.shape[0], bad[0], got[bad[0]], want[bad[0]])


def _route_records(engine, case, n_parts, cap, slot):
    """-> (buckets REC_DTYPE [n_parts, cap + 1], names uint8 [n_parts, cap, slot], status) of the device, equal to the statement's."""
    out_r, out_n, st = _filled(engine, n_parts * (cap + 1), 32), _filled(engine, n_parts * cap * slot), _status(engine)
    ji = JoinInput(_up(engine, case.recs), _up(engine, case.blob), _up(engine, case.off), case.delta)
    engine.route_records(ji, n_parts, cap, out_r, out_n, slot, st)
    want_r = np.full(n_parts * (cap + 1) * 32, FILL, dtype=np.uint8).view(REC_DTYPE)
    want_n = np.full(n_parts * cap * slot, FILL, dtype=np.uint8)
    status = R.route_records(case.recs, case.blob, case.off, case.delta, n_parts, cap, slot, want_r, want_n)
    assert int(st.item()) == status
    got_r, got_n = out_r.cpu().numpy(), out_n.cpu().numpy()
    _same(got_r, want_r, "record buckets")
    _same(got_n, want_n, "name slots")
    return got_r.reshape(-1).view(REC_DTYPE).reshape(n_parts, cap + 1), got_n.reshape(n_parts, cap, slot), status


def _route_hits(engine, hits, blob, n_parts, cap, slot):
    out_h, out_n, st = _filled(engine, n_parts * (cap + 1), 80), _filled(engine, n_parts * cap * slot), _status(engine)
    engine.route_hits(_up(engine, hits), _up(engine, blob), n_parts, cap, out_h, out_n, slot, st)
    want_h = np.full(n_parts * (cap + 1) * 80, FILL, dtype=np.uint8).view(R.HIT_DTYPE)
    want_n = np.full(n_parts * cap * slot, FILL, dtype=np.uint8)
    status = R.route_hits(hits, blob, n_parts, cap, slot, want_h, want_n)
    assert int(st.item()) == status
    got_h, got_n = out_h.cpu().numpy(), out_n.cpu().numpy()
    _same(got_h, want_h, "hit buckets")
    _same(got_n, want_n, "name slots")
    return got_h.reshape(-1).view(R.HIT_DTYPE).reshape(n_parts, cap + 1), got_n.reshape(n_parts, cap, slot), status


def _route_intervals(engine, ivl, count, owner, n_parts, cap):
    out, st = _filled(engine, n_parts * (cap + 1), 16).view(torch.int32), _status(engine)
    d_ivl = torch.from_numpy(ivl.view(np.int32).reshape(-1, 4).copy()).to(engine.device)
    d_count = torch.tensor([count], dtype=torch.int32, device=engine.device)
    engine.route_intervals(d_ivl, d_count, _up(engine, owner), n_parts, cap, out, st)
    want = np.full(n_parts * (cap + 1) * 16, FILL, dtype=np.uint8).view(IVL_DTYPE)
    status = R.route_intervals(ivl, count, owner, n_parts, cap, want)
    assert int(st.item()) == status
    got = out.cpu().numpy()
    _same(got, want, "interval buckets")
    return got.reshape(-1).view(IVL_DTYPE).reshape(n_parts, cap + 1), status


# ---- records -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_parts", [1, 2, 3, 5, 63, 64])
def test_records_parts_and_chunk_edges(engine, n_parts, n):
    case = _records(11, n)
    cap = _largest(R.record_dest(case.recs, n_parts), n_parts) + 3
    got, _, status = _route_records(engine, case, n_parts, cap, 48)
    assert status == -1 and int(got[:, 0]["name_hash"].sum()) == n - len(range(6, n, 7))


def test_records_count_table_longer_than_a_scan_tile(engine):
    """64 parts x 66 chunks = 4224 table entries: the second level of the scan adds the first tile's total to the rest."""
    n_parts, n = 64, 262_145 + CHUNK
    assert n_parts * ((n + CHUNK - 1) // CHUNK) > 4096
    case = _records(12, n)
    cap = _largest(R.record_dest(case.recs, n_parts), n_parts) + 1
    got, _, status = _route_records(engine, case, n_parts, cap, 48)
    assert status == -1 and int(got[:, 0]["name_hash"].sum()) == n - len(range(6, n, 7))


@pytest.mark.parametrize("skew", ["one part", "two parts, lane by lane", "64 parts, one per lane"])
def test_records_skewed_destinations(engine, skew):
    n, n_parts = 4097, 64
    base = _records(13, n, drop_seventh=False)
    i = np.arange(n, dtype=np.uint64)
    d = {"one part": np.full(n, 37, dtype=np.uint64), "two parts, lane by lane": np.where(i % 2 == 0, 17, 42).astype(np.uint64),
         "64 parts, one per lane": i % np.uint64(64)}[skew]
    recs = base.recs.copy()
    recs["name_hash"] = (d << np.uint64(33)) | (recs["name_hash"] & np.uint64((1 << 33) - 1))
    case = types.SimpleNamespace(recs=recs, blob=base.blob, off=base.off, delta=base.delta)
    dest = R.record_dest(recs, n_parts)
    assert np.array_equal(dest, d.astype(np.int64))
    got, _, status = _route_records(engine, case, n_parts, _largest(dest, n_parts) + 2, 48)
    assert status == -1 and int(got[:, 0]["name_hash"].sum()) == n


def test_records_with_the_same_name_keep_their_order(engine):
    n, n_parts = 5000, 3
    case = _records(14, n, n_pool=30)
    assert np.unique(case.recs["name_hash"]).shape[0] <= 30
    cap = _largest(R.record_dest(case.recs, n_parts), n_parts) + 5
    got, _, _ = _route_records(engine, case, n_parts, cap, 48)
    for d in range(n_parts):
        c = int(got[d, 0]["name_hash"])
        assert c > 1000 and np.all(np.diff(got[d, 1:1 + c]["rec_idx"].astype(np.int64)) > 0)


def _check_overflow(got_idx, count, dest, idx, n_parts, cap):
    """Headers hold the true counts; a bucket holds the stable first cap of its items."""
    for d in range(n_parts):
        mine = idx[dest == d]
        assert count[d] == mine.shape[0]
        assert np.array_equal(got_idx[d, 1:1 + min(cap, mine.shape[0])], mine[:cap])


CAPS = {"the largest bucket": (lambda largest: largest, -1), "one less": (lambda largest: largest - 1, 8), "zero": (lambda largest: 0, 8)}


def _not_the_last(dest, n_parts):
    """The size of the largest bucket -- which must be the only one of its size and not the last part: with cap one less, a kernel
    that lets the item of rank cap through then writes it over the NEXT bucket's header and first name slot, inside the arrays
    this test compares, and not behind them.  (The capacity tests run at two sizes for the same error: in one chunk that header
    and the stray item come from ONE workgroup, the header first, so the stray item is what stays; with more chunks they come from
    two workgroups -- on two dies, each with its own L2 -- and which one stays is not defined.)"""
    totals = np.bincount(dest[dest >= 0], minlength=n_parts)
    assert (totals == totals.max()).sum() == 1 and int(totals.argmax()) < n_parts - 1
    return int(totals.max())


@pytest.mark.parametrize("cap_is", list(CAPS))
@pytest.mark.parametrize("n", [3000, 5000])
def test_records_capacity(engine, n, cap_is):
    n_parts = 5
    case = _records(15, n)
    dest = R.record_dest(case.recs, n_parts)
    largest = _not_the_last(dest, n_parts)
    assert largest > 500
    cap, want = CAPS[cap_is][0](largest), CAPS[cap_is][1]
    got, _, status = _route_records(engine, case, n_parts, cap, 48)
    assert status == want
    _check_overflow(got["rec_idx"], got[:, 0]["name_hash"], dest, case.recs["rec_idx"], n_parts, cap)


@pytest.mark.parametrize("delta", [0, 36])
@pytest.mark.parametrize("slot", [16, 48, 64])
def test_record_names_every_length_and_alignment(engine, slot, delta):
    case = _aligned_names(slot, delta)
    n = case.recs.shape[0]
    for n_parts in (1, 3):
        cap = _largest(R.record_dest(case.recs, n_parts), n_parts)
        _, _, status = _route_records(engine, case, n_parts, cap, slot)
        assert status == -1
    # one name a byte longer than the slot: reported, and cut to the slot
    long_case = _aligned_names(slot, delta, extra_long=True)
    _, names, status = _route_records(engine, long_case, 1, n + 1, slot)
    o = int(long_case.off[n]) + delta
    assert status == 8 and np.array_equal(names[0, n], long_case.blob[o:o + slot]) and names[0, n].all()


# ---- PAF hits ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_parts", [2, 64])
def test_hits_parts_and_chunk_edges(engine, n_parts, n):
    case = _records(21, n)
    hits = _as_hits(case)
    cap = _largest(R.hash_dest(hits["qhash"], n_parts), n_parts) + 3
    got, _, status = _route_hits(engine, hits, case.blob, n_parts, cap, 48)
    assert status == -1 and int(got[:, 0]["qhash"].sum()) == n


@pytest.mark.parametrize("cap_is", list(CAPS))
@pytest.mark.parametrize("n", [3000, 5000])
def test_hits_capacity(engine, n, cap_is):
    n_parts = 5
    case = _records(22, n)
    hits = _as_hits(case)
    dest = R.hash_dest(hits["qhash"], n_parts)
    largest = _not_the_last(dest, n_parts)
    cap, want = CAPS[cap_is][0](largest), CAPS[cap_is][1]
    got, _, status = _route_hits(engine, hits, case.blob, n_parts, cap, 48)
    assert status == want
    _check_overflow(got["slot"], got[:, 0]["qhash"], dest, hits["slot"], n_parts, cap)


@pytest.mark.parametrize("slot", [16, 48, 64])
def test_hit_names_every_length_and_alignment(engine, slot):
    case = _aligned_names(slot, 0)
    n = case.recs.shape[0]
    for n_parts in (1, 3):
        hits = _as_hits(case)
        _, _, status = _route_hits(engine, hits, case.blob, n_parts, _largest(R.hash_dest(hits["qhash"], n_parts), n_parts), slot)
        assert status == -1
    long_case = _aligned_names(slot, 0, extra_long=True)
    _, names, status = _route_hits(engine, _as_hits(long_case), long_case.blob, 1, n + 1, slot)
    o = int(long_case.off[n])
    assert status == 8 and np.array_equal(names[0, n], long_case.blob[o:o + slot]) and names[0, n].all()


# ---- intervals ---------------------------------------------------------------------------------------------------------------------

N_OWNER = 70


def _intervals(seed, max_n, n_parts):
    """Contigs -1 .. N_OWNER (both ends nobody's), owners -1 .. n_parts (both ends nobody's), start = input position."""
    rng = np.random.default_rng(seed)
    ivl = np.zeros(max_n, dtype=IVL_DTYPE)
    ivl["contig"] = rng.integers(-1, N_OWNER + 1, max_n)
    ivl["contig"][:4] = [-1, N_OWNER, 0, N_OWNER - 1][:max_n]
    ivl["start"] = np.arange(max_n)
    ivl["end"] = ivl["start"] + rng.integers(1, 30_000, max_n)
    ivl["pad"] = rng.integers(1, 1 << 30, max_n)
    owner = rng.integers(-1, n_parts + 1, N_OWNER).astype(np.int32)
    owner[:4] = [0, -1, n_parts, n_parts - 1]
    return ivl, owner


@pytest.mark.parametrize("max_n", [0, 1, 4096, 4097, 20_000])
@pytest.mark.parametrize("n_parts", [1, 2, 64])
def test_intervals_counts_contigs_and_owners(engine, n_parts, max_n):
    ivl, owner = _intervals(31 + n_parts, max_n, n_parts)
    for count in (max_n // 2, max_n, max_n + 100):
        dest = R.interval_dest(ivl, count, owner, n_parts)
        got, status = _route_intervals(engine, ivl, count, owner, n_parts, _largest(dest, n_parts) + 2)
        assert status == -1 and int(got[:, 0]["start"].sum()) == int((dest >= 0).sum())
        for d in range(n_parts):
            assert np.all(np.diff(got[d, 1:1 + got[d, 0]["start"]]["start"]) > 0)            # input order
    if max_n >= 4096:
        assert 0 < (dest >= 0).sum() < max_n


@pytest.mark.parametrize("cap_is", list(CAPS))
@pytest.mark.parametrize("n_parts", [2, 64])
@pytest.mark.parametrize("max_n,seed", [(3000, 35), (9000, 33)])            # (seeds whose largest bucket is not the last part)
def test_intervals_capacity(engine, max_n, seed, n_parts, cap_is):
    ivl, owner = _intervals(seed, max_n, n_parts)
    dest = R.interval_dest(ivl, max_n, owner, n_parts)
    largest = _not_the_last(dest, n_parts)
    assert largest > 50
    cap, want = CAPS[cap_is][0](largest), CAPS[cap_is][1]
    got, status = _route_intervals(engine, ivl, max_n, owner, n_parts, cap)
    assert status == want
    _check_overflow(got["start"], got[:, 0]["start"], dest, ivl["start"], n_parts, cap)


# ---- seal --------------------------------------------------------------------------------------------------------------------------

SEAL_SHAPES = [(n_parts, cap) for n_parts in (1, 2, 64) for cap in (0, 1, 255, 256, 70_000) if n_parts * cap < 1 << 20]


@pytest.mark.parametrize("n_parts,cap", SEAL_SHAPES)
def test_seal_records(engine, n_parts, cap):
    """Buckets as gci_route_records leaves them (about 0.6 cap records each) in a receive buffer whose other slots hold garbage
    with every flag set; then the same with one header claiming cap + 5."""
    rng = np.random.default_rng(41)
    case = _records(42, int(0.6 * cap * n_parts) if cap > 1 else n_parts)
    raw = rng.integers(1, 256, n_parts * (cap + 1) * 32, dtype=np.uint8)
    buckets = raw.view(REC_DTYPE)
    buckets["flags"] = 0xFF
    names = np.zeros(n_parts * cap * 48, dtype=np.uint8)
    R.route_records(case.recs, case.blob, case.off, case.delta, n_parts, cap, 48, buckets, names)
    for over in (False, True):
        if over:
            buckets["name_hash"][(n_parts - 1) * (cap + 1)] = cap + 5
        d_b, st = _up(engine, buckets), _status(engine)
        engine.route_seal_records(d_b, n_parts, cap, st)
        want = buckets.copy()
        status = R.seal_records(want, n_parts, cap)
        over_by_routing = bool((buckets["name_hash"][::cap + 1] > cap).any())
        assert int(st.item()) == status == (8 if over or over_by_routing else -1)
        _same(d_b.cpu().numpy(), want, "sealed records")
        if over:
            last = want.reshape(n_parts, cap + 1)[n_parts - 1]
            assert np.all(last["flags"][1:] == buckets.reshape(n_parts, cap + 1)[n_parts - 1]["flags"][1:])     # all cap slots kept


@pytest.mark.parametrize("n_parts,cap", SEAL_SHAPES)
def test_seal_intervals(engine, n_parts, cap):
    rng = np.random.default_rng(43)
    max_n = int(0.6 * cap * n_parts) if cap > 1 else 2 * n_parts
    ivl, owner = _intervals(44, max_n, n_parts)
    buckets = np.zeros(n_parts * (cap + 1), dtype=IVL_DTYPE)
    buckets["contig"] = np.resize(np.array([-7, N_OWNER - 20, 2**31 - 1], dtype=np.int32), buckets.shape[0])
    buckets["start"], buckets["end"], buckets["pad"] = (rng.integers(1, 1 << 30, buckets.shape[0]) for _ in range(3))
    R.route_intervals(ivl, max_n, owner, n_parts, cap, buckets)
    cmap = rng.integers(-1, 9, N_OWNER - 20).astype(np.int32)            # n_map below some of the contigs that arrive; -1: not this rank's
    cmap[:3] = [-1, 5, -1]
    for over in (False, True):
        if over:
            buckets["start"][(n_parts - 1) * (cap + 1)] = cap + 5
        d_b, st = torch.from_numpy(buckets.view(np.int32).reshape(-1, 4).copy()).to(engine.device), _status(engine)
        engine.route_seal_intervals(d_b, n_parts, cap, _up(engine, cmap), st)
        want = buckets.copy()
        status = R.seal_intervals(want, n_parts, cap, cmap)
        over_by_routing = bool((buckets["start"][::cap + 1].astype(np.uint32) > cap).any())
        assert int(st.item()) == status == (8 if over or over_by_routing else -1)
        _same(d_b.cpu().numpy(), want, "sealed intervals")
    if cap >= 255:
        inside = want.reshape(n_parts, cap + 1)[:, 1:]["contig"]
        assert (inside >= 0).any() and (inside == -1).any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def _refused(call, *outputs):
    with pytest.raises(GciError) as e:
        call()
    assert e.value.status == GCI_E_INVALID
    for o in outputs:
        flat = o.cpu().numpy().view(np.uint8)
        assert np.all(flat == (FILL if o.dtype != torch.int64 else ST_FILL & 0xFF))


def test_argument_refusals(engine):
    case = _records(51, 300)
    hits = _as_hits(case)
    ivl, owner = _intervals(52, 300, 2)
    ji = JoinInput(_up(engine, case.recs), _up(engine, case.blob), _up(engine, case.off), case.delta)
    d_hits, d_blob = _up(engine, hits), _up(engine, case.blob)
    d_ivl = torch.from_numpy(ivl.view(np.int32).reshape(-1, 4).copy()).to(engine.device)
    d_count, d_owner = torch.tensor([300], dtype=torch.int32, device=engine.device), _up(engine, owner)
    cmap = _up(engine, np.arange(N_OWNER, dtype=np.int32))
    cap = 400
    for n_parts, slot in ((0, 48), (65, 48), (2, 8), (2, 24), (2, 65_552)):
        rows = max(n_parts, 2) * (cap + 1)
        out_r, out_h, out_n, st = _filled(engine, rows, 32), _filled(engine, rows, 80), _filled(engine, 65 * cap * 64), _status(engine)
        _refused(lambda: engine.route_records(ji, n_parts, cap, out_r, out_n, slot, st), out_r, out_n, st)
        _refused(lambda: engine.route_hits(d_hits, d_blob, n_parts, cap, out_h, out_n, slot, st), out_h, out_n, st)
        if slot == 48:
            out_i = _filled(engine, rows, 16).view(torch.int32)
            _refused(lambda: engine.route_intervals(d_ivl, d_count, d_owner, n_parts, cap, out_i, st), out_i, st)
            _refused(lambda: engine.route_seal_records(out_r, n_parts, cap, st), out_r, st)
            _refused(lambda: engine.route_seal_intervals(out_i, n_parts, cap, cmap, st), out_i, st)


# ---- the steps together, the ranks played one after the other on this GPU ----------------------------------------------------------

def _join_files(seed, n_files, n, n_contigs):
    """Files whose names repeat within and across them: a name has a home (contig, start), most of its records lie there (they
    overlap and survive the join), some on another contig (the join drops the name)."""
    rng = np.random.default_rng(seed)
    pool = _pool(seed, 6000, 5, 40)
    home_c, home_s = rng.integers(0, n_contigs, 6000), rng.integers(0, 1 << 22, 6000)
    files = []
    for _ in range(n_files):
        pick = rng.integers(0, 6000, n)
        contig = np.where(rng.random(n) < 0.9, home_c[pick], rng.integers(0, n_contigs, n))
        order = np.argsort(contig, kind="stable")                          # (a sorted BAM file)
        pick, contig = pick[order], contig[order]
        lens = pool.lens[pick]
        start = 40 + np.cumsum(rng.integers(1, 5, n) + lens) - lens
        recs = np.zeros(n, dtype=REC_DTYPE)
        recs["name_hash"] = pool.hashes[pick]
        recs["contig"] = contig
        recs["start"] = home_s[pick] + rng.integers(0, 200, n)
        recs["end"] = recs["start"] + 10_000
        recs["qlen"] = 10_000
        recs["rec_idx"] = np.arange(n)
        recs["flags"] = 1 | (rng.integers(0, 2, n) << 1)
        recs["flags"][6::7] &= 2
        recs["name_len"] = lens
        files.append(types.SimpleNamespace(recs=recs, blob=_blob(pool.mat[pick], lens, start), off=start.astype(np.int64), delta=0))
    return files


@pytest.mark.parametrize("W", [3, 8, 64])
def test_the_steps_together_equal_the_join_on_one_gpu(engine, W):
    """Deal three files to W ranks by contig owner, route, exchange by indexing, seal, join per name owner, route the intervals to
    their contig's owner, seal: over all owners exactly the intervals of gci_name_join over the undealt files."""
    dev, slot, n_contigs = engine.device, 48, 2 * W + 5
    files = _join_files(60 + W, 3, 20_000, n_contigs)
    owner = np.random.default_rng(W).permutation(n_contigs).astype(np.int32) % W
    # the join this must equal (test_gpu_seams.py holds it to the oracle)
    whole = [JoinInput(_up(engine, f.recs), _up(engine, f.blob), _up(engine, f.off), 0) for f in files]
    ivl, cnt = engine.name_join(whole, 0.9)
    one = ivl[:int(cnt.item())].cpu().numpy()
    assert one.shape[0] > 1000
    cmaps = [shard.contig_map_for(owner.tolist(), o)[0] for o in range(W)]
    want = sorted((int(owner[c]), int(cmaps[owner[c]][c]), int(s), int(e)) for c, s, e, _ in one.tolist())

    status = torch.full((3 * W * 2 + 3 * W,), ST_FILL, dtype=torch.int64, device=dev)   # per file W routes + W seals; W joins, W routes, W seals
    used = []

    def word():
        """The next status word: every call of the seven steps gets its own, all read once at the end."""
        used.append(len(used))
        return status[used[-1]:used[-1] + 1]
    recv_r, recv_n, caps = [], [], []
    for fi, f in enumerate(files):
        rank_of = owner[f.recs["contig"]]
        passing = (f.recs["flags"] & 1) != 0
        cap = int(np.bincount(rank_of[passing] * W + R.hash_dest(f.recs["name_hash"][passing], W), minlength=W * W).max())
        send_r, send_n = _filled(engine, W, W, cap + 1, 32), _filled(engine, W, W, cap, slot)
        d_blob = whole[fi].name_base
        for r in range(W):                                            # steps 1 and 2
            mine = np.flatnonzero(rank_of == r)
            ji = JoinInput(_up(engine, f.recs[mine]), d_blob, _up(engine, f.off[mine]), 0)
            engine.route_records(ji, W, cap, send_r[r].view(-1, 32), send_n[r].view(-1), slot, word())
        got_r, got_n = send_r.transpose(0, 1).contiguous(), send_n.transpose(0, 1).contiguous()        # step 3: [owner][source]
        for d in range(W):                                            # step 4
            engine.route_seal_records(got_r[d].view(-1, 32), W, cap, word())
        recv_r.append(got_r)
        recv_n.append(got_n)
        caps.append(cap)
    name_off = []
    for c in caps:                                                    # as shard.ShardedJoin._alloc
        i = torch.arange(W * (c + 1), dtype=torch.int64, device=dev)
        d, k = i // (c + 1), i % (c + 1) - 1
        name_off.append(((d * c + k.clamp(min=0)) * slot).contiguous())
    ivl_cap = int(np.bincount(owner[one[:, 0]], minlength=W).max()) + 1
    send_i = _filled(engine, W, W, ivl_cap + 1, 16).view(torch.int32)
    rows = sum(W * (c + 1) for c in caps)
    for d in range(W):                                                # steps 5 and 6
        inputs = [JoinInput(recv_r[fi][d].view(-1, 32), recv_n[fi][d].view(-1), name_off[fi], 0) for fi in range(3)]
        out, count = torch.zeros((rows, 4), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        engine.name_join(inputs, 0.9, None, out, count, False, None, status=word())
        engine.route_intervals(out, count, _up(engine, owner), W, ivl_cap, send_i[d].view(-1, 4), word())
    got_i = send_i.transpose(0, 1).contiguous()
    for o in range(W):                                                # step 7
        engine.route_seal_intervals(got_i[o].view(-1, 4), W, ivl_cap, _up(engine, cmaps[o]), word())
    assert len(used) == int(status.shape[0]) and np.all(status.cpu().numpy() == -1)
    rows = got_i.cpu().numpy().reshape(W, -1, 4)
    got = sorted((o, int(c), int(s), int(e)) for o in range(W) for c, s, e, _ in rows[o][rows[o][:, 0] >= 0].tolist())
    assert got == want
