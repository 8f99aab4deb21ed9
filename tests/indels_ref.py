"""The statement of indel_sites.py's semantics in plain Python / numpy, per operation and per element, from the text of include/gci_hip.h
(gci_bam_indel_size, gci_indel_sites_size).  The bytes of a record are read here, with the aux walk of tests/clips_ref.py (the FIRST CG
tag counts); a first operation <l_seq>S without a usable tag leaves the record's own operations, as the cover pass leaves them.

  counted    a record the skip rule of gci_bam_cover_size does not skip (flag & excl, mapq < min_mapq, refID outside the table, pos < 0,
             an unselected contig) -- with or without operations.
  operations the record's own, or the first CG:B,I / B,i array behind a first operation <l_seq>S; such a first operation without a
             usable tag: the record's own (a true placeholder, <l_seq>S<n>N, holds no I or D).
  at         pos plus the lengths of all M, =, X, D and N operations in front of the operation.   L: the contig's length, capped at
             0x7FFFFFFE.
  deletion   D of length >= min_len with at < L: [at, min(at + len, L) - 1].
  insertion  I of length >= min_len: the site at - 1 (0 for at == 0) if it is below L.
  status     GCI_E_MALFORMED for a record that runs past the stream or contradicts its block_size, and for codes 9 - 15 in a counted
             record; the smallest record index wins.
  site       a maximal run of consecutive elements with del >= min_reads or ins >= min_reads of one contig inside one window: contig,
             start, end (exclusive), and the maxima of the three tracks over the run."""
import bisect
import struct

import numpy as np

from clips_ref import EXCL_DEFAULT, GCI_E_MALFORMED, NO_STATUS, REF_OPS, TILE, _first_cg, is_skipped, layout      # noqa: F401

L_CAP = 0x7FFFFFFE


def parse(stream, off, has_seq=True):
    """None for a record that runs past the stream or contradicts its block_size; else (ref_id, pos, mapq, flag, ops) with ops the
    uint32 operation words that count."""
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
        if real is not None and n_cig <= real.shape[0] < (1 << 29):
            ops = real
    return ref_id, pos, mapq, flag, ops


def record(stream, off, lengths, ref_sel, excl, min_mapq, min_len, has_seq=True):
    """-> (counted, [(start, end)] of the deletions, [site] of the insertions, contig, malformed), in operation order."""
    rv = parse(stream, off, has_seq)
    if rv is None:
        return False, [], [], -1, True
    ref_id, pos, mapq, flag, ops = rv
    if is_skipped(ref_id, pos, mapq, flag, ref_sel, excl, min_mapq):
        return False, [], [], -1, False
    contig = int(ref_sel[ref_id])
    L = min(int(lengths[contig]), L_CAP) if contig < len(lengths) else 0
    at, bad, dels, inss = pos, False, [], []
    for w in ops.tolist():
        op, n = w & 0xF, w >> 4
        if op > 8:
            bad = True
        elif op == 2 and n >= min_len and at < L:
            dels.append((at, min(at + n, L) - 1))
        elif op == 1 and n >= min_len and max(at - 1, 0) < L:
            inss.append(max(at - 1, 0))
        if op in REF_OPS:
            at += n
    return True, dels, inss, contig, bad


def stream_events(stream, offs, lengths, ref_sel, excl=EXCL_DEFAULT, min_mapq=0, min_len=50, has_seq=True):
    """-> (deletions [(contig, start, end)], insertions [(contig, site)], [records counted, deletions, insertions], the status word), each
    list in (record, operation) order."""
    dels, inss, counted, status = [], [], 0, NO_STATUS
    for i, off in enumerate(np.asarray(offs).tolist()):
        c, d, s, contig, bad = record(stream, off, lengths, ref_sel, excl, min_mapq, min_len, has_seq)
        if bad:
            status = min(status, (i << 8) | -GCI_E_MALFORMED)
        counted += int(c)
        dels += [(contig, a, b) for a, b in d]
        inss += [(contig, p) for p in s]
    return dels, inss, [counted, len(dels), len(inss)], status


# ---- tracks and sites ------------------------------------------------------------------------------------------------------------------
def track_of(events, lengths):
    """The flat int32 track of a list of (contig, start, end) or (contig, site) events: per base the events over it."""
    offs, total = layout(lengths)
    diff = np.zeros(total + 1, dtype=np.int64)
    for e in events:
        diff[offs[e[0]] + e[1]] += 1
        diff[offs[e[0]] + e[-1] + 1] -= 1
    return np.cumsum(diff[:-1]).astype(np.int32)


def sites_of(dele, ins, depth, lengths, min_reads, windows=()):
    """-> [(contig, start, end, del, ins, depth)] of the flat tracks, ascending; windows: sorted, disjoint [begin, end) of flat elements,
    none: every contig.  An element at a time."""
    offs, total = layout(lengths)
    if not windows:
        windows = [(o, o + int(L)) for o, L in zip(offs, lengths)]
    out = []
    for a, b in windows:
        a, b = max(int(a), 0), min(int(b), total)
        run = None                                     # [contig, start, end, del, ins, depth] of the run that is open
        for p in range(a, b):
            c = bisect.bisect_right(offs, p) - 1
            pos = p - offs[c]
            hot = pos < int(lengths[c]) and (dele[p] >= min_reads or ins[p] >= min_reads)
            if run is not None and (not hot or run[0] != c):
                out.append(tuple(run))
                run = None
            if hot:
                d = int(depth[p]) if depth is not None else 0
                if run is None:
                    run = [c, pos, pos + 1, int(dele[p]), int(ins[p]), d]
                else:
                    run[2:] = [pos + 1, max(run[3], int(dele[p])), max(run[4], int(ins[p])), max(run[5], d)]
        if run is not None:
            out.append(tuple(run))
    return out
