"""Plain numpy statement of the bucket layouts of the name-hash-sharded join (include/gci_hip.h, "multi-GPU"; the layout
comment at the top of gci_amd/csrc/k_shard.hip): what gci_route_records, gci_route_hits, gci_route_intervals and the two
seal calls must leave in their outputs, byte for byte.  Every function takes its output arrays as they are before the call
and writes only what the contract says is written; what it returns is the status word as an int64 (-1: clean, 8:
GCI_E_CAPACITY).  Test infrastructure only: no torch, no GPU."""
import numpy as np

from gci_amd.device import IVL_DTYPE, REC_DTYPE

# gci_paf_hit (include/gci_hip.h)
HIT_DTYPE = np.dtype([("qn_off", "<u8"), ("qhash", "<u8"), ("qlen", "<i8"), ("qs", "<i8"), ("qe", "<i8"), ("ts", "<i8"), ("te", "<i8"),
                      ("identity", "<f8"), ("qn_len", "<u4"), ("t", "<i4"), ("hq", "<u4"), ("slot", "<u4")])
assert HIT_DTYPE.itemsize == 80 and REC_DTYPE.itemsize == 32 and IVL_DTYPE.itemsize == 16

REC_PASS, REC_NAME16 = 1, 4
CLEAN, E_CAPACITY = -1, 8


def hash_dest(hashes, n_parts):
    """The part that owns a name: (hash >> 33) % n_parts."""
    return ((np.asarray(hashes, dtype=np.uint64) >> np.uint64(33)) % np.uint64(n_parts)).astype(np.int64)


def record_dest(recs, n_parts):
    return np.where((recs["flags"] & REC_PASS) != 0, hash_dest(recs["name_hash"], n_parts), -1)


def interval_dest(ivl, count, owner, n_parts):
    """ivl: IVL_DTYPE [max_n]; count: what the device-side counter holds (below, at or above max_n)."""
    owner = np.asarray(owner, dtype=np.int64)
    c = ivl["contig"].astype(np.int64)
    live = (np.arange(ivl.shape[0]) < min(int(count), ivl.shape[0])) & (c >= 0) & (c < owner.shape[0])
    o = owner[np.where(live, c, 0)] if owner.shape[0] else np.full(c.shape, -1, dtype=np.int64)
    return np.where(live & (o >= 0) & (o < n_parts), o, -1)


def place(dest, n_parts, cap):
    """Stable placement.  dest int64 [n], -1: no destination.  -> (totals [n_parts]: the TRUE number routed to each part; then for
    the items that are written, in bucket order: their index in the input, their part d, their rank k < cap inside it)."""
    dest = np.asarray(dest, dtype=np.int64)
    keep = np.flatnonzero(dest >= 0)
    src = keep[np.argsort(dest[keep], kind="stable")]
    d = dest[src]
    totals = np.bincount(d, minlength=n_parts).astype(np.int64)
    k = np.arange(src.shape[0], dtype=np.int64) - (np.cumsum(totals) - totals)[d]
    w = k < cap
    return totals, src[w], d[w], k[w]


def _status(totals, cap, long_name=False):
    return np.int64(E_CAPACITY if (totals > cap).any() or long_name else CLEAN)


def _names(out_names, base, start, length, d, k, cap, name_slot):
    """The name slots of the written items: min(length, name_slot) bytes of base from `start`, then zeros."""
    if d.shape[0] == 0:
        return
    col = np.arange(name_slot, dtype=np.int64)
    use = col[None, :] < np.minimum(length.astype(np.int64), name_slot)[:, None]
    at = np.where(use, start.astype(np.int64)[:, None] + col[None, :], 0)
    out_names.reshape(-1, name_slot)[d * cap + k] = np.where(use, base[at], 0).astype(np.uint8)


def route_records(recs, name_base, name_off, name_delta, n_parts, cap, name_slot, out_recs, out_names):
    """recs REC_DTYPE [n]; name_off int64 by POSITION in recs; out_recs REC_DTYPE [n_parts * (cap + 1)];
    out_names uint8 [n_parts * cap * name_slot]."""
    totals, src, d, k = place(record_dest(recs, n_parts), n_parts, cap)
    r = recs[src].copy()
    r["flags"] |= REC_NAME16
    out_recs[d * (cap + 1) + 1 + k] = r
    head = np.zeros(n_parts, dtype=REC_DTYPE)
    head["name_hash"], head["contig"] = totals, -1
    out_recs[np.arange(n_parts) * (cap + 1)] = head
    _names(out_names, name_base, np.asarray(name_off)[src] + int(name_delta), r["name_len"], d, k, cap, name_slot)
    return _status(totals, cap, bool((r["name_len"] > name_slot).any()))


def route_hits(hits, name_base, n_parts, cap, name_slot, out_hits, out_names):
    """hits HIT_DTYPE [n] (names: name_base[qn_off : qn_off + qn_len]); out_hits HIT_DTYPE [n_parts * (cap + 1)]."""
    totals, src, d, k = place(hash_dest(hits["qhash"], n_parts), n_parts, cap)
    h = hits[src]
    out_hits[d * (cap + 1) + 1 + k] = h
    head = np.zeros(n_parts, dtype=HIT_DTYPE)
    head["qhash"], head["t"] = totals, -1
    out_hits[np.arange(n_parts) * (cap + 1)] = head
    _names(out_names, name_base, h["qn_off"], h["qn_len"], d, k, cap, name_slot)
    return _status(totals, cap, bool((h["qn_len"] > name_slot).any()))


def route_intervals(ivl, count, owner, n_parts, cap, out):
    """ivl IVL_DTYPE [max_n]; out IVL_DTYPE [n_parts * (cap + 1)]."""
    totals, src, d, k = place(interval_dest(ivl, count, owner, n_parts), n_parts, cap)
    out[d * (cap + 1) + 1 + k] = ivl[src]
    head = np.zeros(n_parts, dtype=IVL_DTYPE)
    head["contig"], head["start"] = -1, totals
    out[np.arange(n_parts) * (cap + 1)] = head
    return _status(totals, cap)


def seal_records(recs, n_parts, cap):
    """recs REC_DTYPE [n_parts * (cap + 1)] as received: flags = 0 in every header and in the slots beyond the count."""
    b = recs.reshape(n_parts, cap + 1)
    count = b[:, 0]["name_hash"].copy()
    dead = np.arange(cap + 1, dtype=np.uint64)[None, :] > np.minimum(count, np.uint64(cap))[:, None]
    dead[:, 0] = True
    b["flags"][dead] = 0
    return _status(count, np.uint64(cap))


def seal_intervals(ivl, n_parts, cap, cmap):
    """ivl IVL_DTYPE [n_parts * (cap + 1)] as received: contig -> cmap[contig] inside the count, -1 everywhere else from slot 1 up."""
    cmap = np.asarray(cmap, dtype=np.int32)
    b = ivl.reshape(n_parts, cap + 1)
    count = b[:, 0]["start"].astype(np.uint32).astype(np.int64)
    c = b["contig"].astype(np.int64)
    live = (np.arange(cap + 1)[None, :] <= np.minimum(count, cap)[:, None]) & (c >= 0) & (c < cmap.shape[0])
    new = np.where(live, cmap[np.where(live, c, 0)] if cmap.shape[0] else -1, -1).astype(np.int32)
    b["contig"][:, 1:] = new[:, 1:]
    return _status(count, cap)
