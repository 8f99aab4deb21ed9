"""The statement of mismatch_sites.py's semantics in plain Python / numpy, per base and per element, from the text of include/gci_hip.h
(gci_fasta_codes, gci_bam_mismatch_size, gci_mismatch_sites_size).  Records are parsed by tests/indels_ref.py (the skip rule, the first
CG array behind a <l_seq>S placeholder).

  counted    a record the skip rule of gci_bam_cover_size does not skip.
  positions  q from 0, advancing under M = X I S; p from pos, advancing under M = X D N.  Under M = X base q faces base p if p < L.
  codes      the read's: the SEQ nibble, high nibble = even q; SEQ lies behind the in-record CIGAR words.  The assembly's: BAM's
             "=ACMGRSVTWYHKDBN" code of the upper-cased FASTA byte, U as T, anything else 15.
  compared   both codes one of 1 2 4 8; a mismatch: compared and different.
  l_seq      0: counted, nothing compared.  > 0 and S + M + I != l_seq: malformed, nothing compared.
  status     GCI_E_MALFORMED for a record out of bounds, codes 9 - 15 in a counted record, and the l_seq rule; the smallest index wins.
  hot        mismatch >= min_reads and mismatch * 1000000 >= frac_ppm * depth.
  site       a maximal run of hot elements of one contig inside one window: contig, start, end (exclusive), the largest mismatch count
             and the depth at the first base that reaches it."""
import bisect
import struct

import numpy as np

import indels_ref as IR
from clips_ref import EXCL_DEFAULT, GCI_E_MALFORMED, NO_STATUS, REF_OPS, TILE, is_skipped, layout      # noqa: F401

L_CAP = IR.L_CAP
QRY_OPS = (0, 1, 4, 7, 8)                              # M I S = X
MATCH_OPS = (0, 7, 8)
BASES = (1, 2, 4, 8)
IUPAC = "=ACMGRSVTWYHKDBN"


# ---- the assembly ----------------------------------------------------------------------------------------------------------------------
def fasta_code(byte):
    c = chr(byte).upper()
    if c == "U":
        c = "T"
    k = IUPAC.find(c)
    return k if k >= 1 and c.isalpha() else 15


def fasta_records(text):
    """[(id, body begin, body end)] of the bytes of a FASTA file: a title line begins with '>' at offset 0 or behind a line feed; the
    body runs from behind the title line to the next title line."""
    data = bytes(text)
    starts = [i for i in range(len(data)) if data[i] == 0x3E and (i == 0 or data[i - 1] == 0x0A)]
    out = []
    for k, hs in enumerate(starts):
        stop = starts[k + 1] if k + 1 < len(starts) else len(data)
        nl = data.find(b"\n", hs, stop)
        he = nl if nl >= 0 else stop
        parts = data[hs + 1:he].decode(errors="replace").rstrip().split(None, 1)
        out.append((parts[0] if parts else "", min(he + 1, stop), stop))
    return out


def fasta_codes(text, bodies, dst, total, fill=0xEE):
    """The code array of gci_fasta_codes: `fill` wherever no base goes."""
    data = bytes(text)
    codes = np.full(total, fill, dtype=np.uint8)
    for (a, b), d in zip(bodies, dst):
        if d < 0:
            continue
        k = 0
        for i in range(int(a), int(b)):
            if data[i] in b"\n\r ":
                continue
            if d + k < total:
                codes[d + k] = fasta_code(data[i])
            k += 1
    return codes


def seq_length(text, a, b):
    return sum(1 for c in bytes(text)[int(a):int(b)] if c not in b"\n\r ")


# ---- the records -----------------------------------------------------------------------------------------------------------------------
def record(stream, off, lengths, offsets, ref_sel, codes, excl, min_mapq):
    """-> (counted, [p] of the mismatches in position order, pairs compared, contig, malformed)."""
    rv = IR.parse(stream, off, True)
    if rv is None:
        return False, [], 0, -1, True
    ref_id, pos, mapq, flag, ops = rv
    if is_skipped(ref_id, pos, mapq, flag, ref_sel, excl, min_mapq):
        return False, [], 0, -1, False
    off = int(off)
    l_rn, n_cig, l_seq = int(stream[off + 12]), struct.unpack_from("<H", stream, off + 16)[0], struct.unpack_from("<i", stream, off + 20)[0]
    seq = off + 36 + l_rn + 4 * n_cig
    contig = int(ref_sel[ref_id])
    L = min(int(lengths[contig]), L_CAP) if contig < len(lengths) else 0
    words = ops.tolist()
    bad = any((w & 0xF) > 8 for w in words)
    qlen = sum(w >> 4 for w in words if (w & 0xF) in QRY_OPS)
    if l_seq > 0 and qlen != l_seq:
        bad = True
    if l_seq == 0 or qlen != l_seq:
        return True, [], 0, contig, bad
    p, q, mm, compared = pos, 0, [], 0
    base = offsets[contig] if L else 0
    for w in words:
        op, n = w & 0xF, w >> 4
        if op in MATCH_OPS and p < L:
            m = min(n, L - p)
            qi = np.arange(q, q + m)
            sb = stream[seq + (qi >> 1)]
            nib = np.where(qi & 1, sb & 15, sb >> 4).astype(np.int64)
            rc = codes[base + p:base + p + m].astype(np.int64)
            both = np.isin(nib, BASES) & np.isin(rc, BASES)
            compared += int(both.sum())
            mm += (p + np.flatnonzero(both & (nib != rc))).tolist()
        if op in REF_OPS:
            p += n
        if op in QRY_OPS:
            q += n
    return True, mm, compared, contig, bad


def stream_events(stream, offs, lengths, ref_sel, codes, excl=EXCL_DEFAULT, min_mapq=0):
    """-> ([(contig, p)] in (record, position) order, [records counted, mismatches, pairs compared], the status word)."""
    offsets, _ = layout(lengths)
    events, counted, compared, status = [], 0, 0, NO_STATUS
    for i, off in enumerate(np.asarray(offs).tolist()):
        c, mm, n, contig, bad = record(stream, off, lengths, offsets, ref_sel, codes, excl, min_mapq)
        if bad:
            status = min(status, (i << 8) | -GCI_E_MALFORMED)
        counted += int(c)
        compared += n
        events += [(contig, p) for p in mm]
    return events, [counted, len(events), compared], status


track_of = IR.track_of


# ---- sites -----------------------------------------------------------------------------------------------------------------------------
def is_hot(m, d, min_reads, frac_ppm):
    return int(m) >= min_reads and int(m) * 1000000 >= frac_ppm * int(d)


def sites_of(mism, depth, lengths, min_reads, frac_ppm, windows=()):
    """-> [(contig, start, end, mismatch, depth)] of the flat tracks, ascending; windows: sorted, disjoint [begin, end) of flat
    elements, none: every contig.  An element at a time."""
    offs, total = layout(lengths)
    if not windows:
        windows = [(o, o + int(L)) for o, L in zip(offs, lengths)]
    out = []
    for a, b in windows:
        a, b = max(int(a), 0), min(int(b), total)
        run = None
        for p in range(a, b):
            c = bisect.bisect_right(offs, p) - 1
            pos = p - offs[c]
            hot = pos < int(lengths[c]) and is_hot(mism[p], depth[p], min_reads, frac_ppm)
            if run is not None and (not hot or run[0] != c):
                out.append(tuple(run))
                run = None
            if hot:
                if run is None:
                    run = [c, pos, pos + 1, int(mism[p]), int(depth[p])]
                else:
                    run[2] = pos + 1
                    if int(mism[p]) > run[3]:
                        run[3:] = [int(mism[p]), int(depth[p])]
        if run is not None:
            out.append(tuple(run))
    return out
