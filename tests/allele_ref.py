"""The statement of allele_sites.py's semantics in plain Python, one base and one element at a time, from the text of include/gci_hip.h
(gci_bam_allele_size, gci_allele_sites_size) -- not from the kernels, and not from tests/mismatch_ref.py's walk either: only the record
parser, the skip rule and the layout are shared with it (tests/indels_ref.py, tests/clips_ref.py).

  counted    a record the skip rule of gci_bam_cover_size does not skip.
  positions  q from 0, advancing under M = X I S; p from pos, advancing under M = X D N.  Under M = X base q faces base p if p < L.
  compared   the SEQ nibble (high nibble = even q) and the assembly's code are each one of 1 2 4 8.
  event      a compared pair whose codes differ, in the list of the READ's base: A (1), C (2), G (4), T (8).
  l_seq      0: counted, nothing compared.  > 0 and S + M + I != l_seq: malformed, nothing compared.
  counts     [records counted, A events, C events, G events, T events, pairs compared].
  best       the largest of the four tracks at an element; alt the first of A C G T that reaches it.
  hot        best >= min_reads and best * 1000000 >= frac_ppm * depth.
  site       a single hot element inside a window and its contig: (contig, pos, ref code, alt code, nA, nC, nG, nT, depth)."""
import bisect
import struct

import numpy as np

import indels_ref as IR
from clips_ref import EXCL_DEFAULT, GCI_E_MALFORMED, NO_STATUS, is_skipped, layout      # noqa: F401

BASES = (1, 2, 4, 8)                                   # A C G T, in list order
track_of = IR.track_of


def record(stream, raw, off, lengths, offsets, ref_sel, codes, excl, min_mapq):
    """-> (counted, four lists of p, pairs compared, contig, malformed).  raw, codes: the stream and the code array as bytes (plain
    integers, a base at a time)."""
    lists = ([], [], [], [])
    rv = IR.parse(stream, off, True)
    if rv is None:
        return False, lists, 0, -1, True
    ref_id, pos, mapq, flag, ops = rv
    if is_skipped(ref_id, pos, mapq, flag, ref_sel, excl, min_mapq):
        return False, lists, 0, -1, False
    off = int(off)
    l_rn, n_cig = int(stream[off + 12]), struct.unpack_from("<H", stream, off + 16)[0]
    l_seq = struct.unpack_from("<i", stream, off + 20)[0]
    seq = off + 36 + l_rn + 4 * n_cig                  # behind the in-record CIGAR words, also when the operations come from CG
    contig = int(ref_sel[ref_id])
    L = min(int(lengths[contig]), IR.L_CAP) if contig < len(lengths) else 0
    words = ops.tolist()
    bad = any((w & 15) > 8 for w in words)
    qlen = sum(w >> 4 for w in words if (w & 15) in (0, 1, 4, 7, 8))
    if l_seq > 0 and qlen != l_seq:
        bad = True
    if l_seq == 0 or qlen != l_seq:
        return True, lists, 0, contig, bad
    base = offsets[contig] if L else 0
    p, q, compared = pos, 0, 0
    for w in words:
        op, n = w & 15, w >> 4
        if op in (0, 7, 8):
            for j in range(min(n, max(L - p, 0))):
                byte = raw[seq + ((q + j) >> 1)]
                nib = (byte & 15) if (q + j) & 1 else (byte >> 4)
                rc = codes[base + p + j]
                if nib in BASES and rc in BASES:
                    compared += 1
                    if nib != rc:
                        lists[BASES.index(nib)].append(p + j)
        if op in (0, 2, 3, 7, 8):
            p += n
        if op in (0, 1, 4, 7, 8):
            q += n
    return True, lists, compared, contig, bad


def stream_events(stream, offs, lengths, ref_sel, codes, excl=EXCL_DEFAULT, min_mapq=0):
    """-> (four lists of (contig, p), each in (record, position) order; the six counts; the status word)."""
    offsets, _ = layout(lengths)
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    raw, codes = stream.tobytes(), np.ascontiguousarray(codes, dtype=np.uint8).tobytes()
    out, counted, compared, status = ([], [], [], []), 0, 0, NO_STATUS
    for i, off in enumerate(np.asarray(offs).tolist()):
        c, lists, n, contig, bad = record(stream, raw, off, lengths, offsets, ref_sel, codes, excl, min_mapq)
        if bad:
            status = min(status, (i << 8) | -GCI_E_MALFORMED)
        counted += int(c)
        compared += n
        for k in range(4):
            out[k].extend((contig, p) for p in lists[k])
    return list(out), [counted] + [len(x) for x in out] + [compared], status


def sites_of(a, c, g, t, depth, codes, lengths, min_reads, frac_ppm, windows=()):
    """-> [(contig, pos, ref, alt, nA, nC, nG, nT, depth)] of the flat tracks, ascending; windows: sorted, disjoint [begin, end) of flat
    elements, none: every contig.  An element at a time."""
    offs, total = layout(lengths)
    if not windows:
        windows = [(o, o + int(L)) for o, L in zip(offs, lengths)]
    out = []
    for lo, hi in windows:
        for p in range(max(int(lo), 0), min(int(hi), total)):
            k = bisect.bisect_right(offs, p) - 1
            pos = p - offs[k]
            if pos >= int(lengths[k]):
                continue                               # padding
            n = [int(a[p]), int(c[p]), int(g[p]), int(t[p])]
            best = max(n)
            if best >= min_reads and best * 1000000 >= frac_ppm * int(depth[p]):
                out.append((k, pos, int(codes[p]), BASES[n.index(best)], *n, int(depth[p])))
    return out
