"""The statement of clip_sites.py's semantics in plain Python / numpy, per record and per element, from the text of include/gci_hip.h
(gci_bam_clip_size, gci_clip_sites_size) and from nothing else: the bytes of a record are read here, not through formats.bam, so that
the FIRST CG tag and the heads form are this file's own reading.

  skipped    the skip rule of gci_bam_cover_size (flag & excl, mapq < min_mapq, refID outside the table, pos < 0, an unselected contig);
             also a record whose R is 0.
  operations the record's own, or the first CG:B,I / B,i array behind a first operation <l_seq>S; such a first operation without a
             usable tag: R counts as 0.
  R          the bases under M, =, X, D and N.   lead / trail: S and H among the first / last two operations, the inner one only when
             the outer one is a clip too.
  events     left at pos if lead >= min_clip, right at pos + R - 1 if trail >= min_clip; a site at or beyond the contig's length is
             not emitted and not counted.
  status     GCI_E_MALFORMED for a record that runs past the stream or contradicts its block_size, and for codes 9 - 15 in a record
             that is not skipped; the smallest record index wins."""
import struct

import numpy as np

EXCL_DEFAULT = 0x704
GCI_E_MALFORMED = -7
NO_STATUS = (1 << 64) - 1
TILE = 4096
REF_OPS = (0, 2, 3, 7, 8)                              # M D N = X
CLIP_OPS = (4, 5)                                      # S H
_AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def _first_cg(buf, at, end):
    """The operation words of the first CG tag of the aux bytes [at, end) when it is a B,I / B,i array; None otherwise."""
    while at + 3 <= end:
        tag, t = bytes(buf[at:at + 2]), chr(buf[at + 2])
        v = at + 3
        if t in _AUX_SIZE:
            size = _AUX_SIZE[t]
        elif t in "ZH":
            z = v
            while z < end and buf[z]:
                z += 1
            if z >= end:
                return None
            size = z - v + 1
        elif t == "B":
            if v + 5 > end or chr(buf[v]) not in "cCsSiIf":
                return None
            size = 5 + struct.unpack_from("<I", buf, v + 1)[0] * _AUX_SIZE[chr(buf[v])]
        else:
            return None
        if v + size > end:
            return None
        if tag == b"CG":
            if t == "B" and chr(buf[v]) in "Ii":
                n = struct.unpack_from("<I", buf, v + 1)[0]
                return np.frombuffer(buf, dtype="<u4", count=n, offset=v + 5)
            return None
        at = v + size
    return None


def parse(stream, off, has_seq=True):
    """None for a record that runs past the stream or contradicts its block_size; else (ref_id, pos, mapq, flag, ops) with ops the
    uint32 operation words that count (empty: none)."""
    n, off = int(stream.shape[0]), int(off)
    if off + 36 > n:
        return None
    buf = memoryview(stream)
    bs, ref_id, pos, l_rn, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", buf, off)
    end = off + 4 + bs
    cig = off + 36 + l_rn
    if bs < 32 or end > n or l_seq < 0:
        return None
    aux = cig + 4 * n_cig + (((l_seq + 1) // 2 + l_seq) if has_seq else 0)
    if aux > end:
        return None
    ops = np.frombuffer(buf, dtype="<u4", count=n_cig, offset=cig)
    if n_cig and int(ops[0]) == ((l_seq << 4) | 4):
        real = _first_cg(buf, aux, end)
        ops = real if real is not None and n_cig <= real.shape[0] < (1 << 29) else ops[:0]
    return ref_id, pos, mapq, flag, ops


def is_skipped(ref_id, pos, mapq, flag, ref_sel, excl, min_mapq):
    return bool(flag & excl) or mapq < min_mapq or ref_id < 0 or ref_id >= len(ref_sel) or pos < 0 or ref_sel[ref_id] < 0


def ends_of(ops):
    """(lead, trail) of the operation words."""
    def side(outer, inner):
        if outer is None or (outer & 0xF) not in CLIP_OPS:
            return 0
        return (outer >> 4) + ((inner >> 4) if inner is not None and (inner & 0xF) in CLIP_OPS else 0)
    w = [int(x) for x in (ops[:2].tolist() + ops[-2:].tolist())] if ops.shape[0] > 1 else [int(x) for x in ops.tolist()]
    if not w:
        return 0, 0
    if len(w) == 1:
        return side(w[0], None), side(w[0], None)
    return side(w[0], w[1]), side(w[-1], w[-2])


def record(stream, off, lengths, ref_sel, excl, min_mapq, min_clip, has_seq=True):
    """-> (counted, left site or None, right site or None, contig, malformed)."""
    rv = parse(stream, off, has_seq)
    if rv is None:
        return False, None, None, -1, True
    ref_id, pos, mapq, flag, ops = rv
    if is_skipped(ref_id, pos, mapq, flag, ref_sel, excl, min_mapq):
        return False, None, None, -1, False
    code, length = ops & 0xF, (ops >> 4).astype(np.int64)
    R = int(length[np.isin(code, REF_OPS)].sum())
    if R == 0:
        return False, None, None, -1, False
    contig = int(ref_sel[ref_id])
    L = int(lengths[contig]) if contig < len(lengths) else 0
    lead, trail = ends_of(ops)
    left = pos if lead >= min_clip and pos < L else None
    right = pos + R - 1 if trail >= min_clip and pos + R - 1 < L else None
    return True, left, right, contig, bool((code > 8).any())


def record_by_operation(stream, off, lengths, ref_sel, excl, min_mapq, min_clip, has_seq=True):
    """The same answer the slow way: one step per operation, the clip runs found by walking inwards from both ends."""
    rv = parse(stream, off, has_seq)
    if rv is None:
        return False, None, None, -1, True
    ref_id, pos, mapq, flag, ops = rv
    if is_skipped(ref_id, pos, mapq, flag, ref_sel, excl, min_mapq):
        return False, None, None, -1, False
    cigar = [(int(w) & 0xF, int(w) >> 4) for w in ops.tolist()]
    at, bad = pos, False
    for op, n in cigar:
        if op > 8:
            bad = True
        elif op in REF_OPS:
            at += n
    if at == pos:
        return False, None, None, -1, False
    lead = trail = 0
    for k, (op, n) in enumerate(cigar[:2]):
        if op not in CLIP_OPS:
            break
        lead += n
    for k, (op, n) in enumerate(reversed(cigar[-2:])):
        if op not in CLIP_OPS:
            break
        trail += n
    contig = int(ref_sel[ref_id])
    L = int(lengths[contig]) if contig < len(lengths) else 0
    return True, (pos if lead >= min_clip and pos < L else None), (at - 1 if trail >= min_clip and at - 1 < L else None), contig, bad


def stream_events(stream, offs, lengths, ref_sel, excl=EXCL_DEFAULT, min_mapq=0, min_clip=100, has_seq=True, per_record=record):
    """-> (left events [(contig, site)], right events, [records counted, left events, right events], the status word), in record order."""
    left, right, counted, status = [], [], 0, NO_STATUS
    for i, off in enumerate(np.asarray(offs).tolist()):
        c, l, r, contig, bad = per_record(stream, off, lengths, ref_sel, excl, min_mapq, min_clip, has_seq)
        if bad:
            status = min(status, (i << 8) | -GCI_E_MALFORMED)
        counted += int(c)
        if l is not None:
            left.append((contig, l))
        if r is not None:
            right.append((contig, r))
    return left, right, [counted, len(left), len(right)], status


# ---- tracks and sites ------------------------------------------------------------------------------------------------------------------
def layout(lengths):
    """(offsets, total) of the track layout: every contig at a multiple of TILE."""
    offs, at = [], 0
    for L in lengths:
        offs.append(at)
        at += (int(L) + TILE - 1) // TILE * TILE
    return offs, max(at, TILE)


def track_of(events, lengths):
    """The flat int32 track of a list of (contig, site) events."""
    offs, total = layout(lengths)
    t = np.zeros(total, dtype=np.int32)
    for c, s in events:
        t[offs[c] + s] += 1
    return t


def sites_of(left, right, depth, lengths, min_reads, windows=()):
    """-> [(contig, pos, left, right, depth)] of the flat tracks, ascending; windows: sorted, disjoint [begin, end) of flat elements,
    none: every contig."""
    offs, total = layout(lengths)
    if not windows:
        windows = [(o, o + int(L)) for o, L in zip(offs, lengths)]
    out = []
    for a, b in windows:
        a, b = max(int(a), 0), min(int(b), total)
        for p in (a + np.flatnonzero((left[a:b] >= min_reads) | (right[a:b] >= min_reads))).tolist():
            c = max(k for k, o in enumerate(offs) if o <= p)
            if p - offs[c] < int(lengths[c]):
                out.append((c, p - offs[c], int(left[p]), int(right[p]), int(depth[p]) if depth is not None else 0))
    return out
