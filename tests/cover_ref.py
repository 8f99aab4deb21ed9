"""The statement of bam_depth.py's semantics in plain Python / numpy over formats.bam.decode_record: which reference bases a record
covers, the depth of a stream, and the status word a malformed stream gives.

THE READING IS PINNED HERE.  Neither samtools nor pysam is available where this project is built, so nothing below was compared
with a run of `samtools depth`; it follows the samtools-depth manual page (samtools 1.13 and later):

  * "-a  Output all positions (including those with zero depth)"                -> every base of every selected contig has a value;
  * "-g FLAGS  By default, reads that have any of the flags UNMAP, SECONDARY, QCFAIL, or DUP set are skipped. To include these reads
    back in the analysis, use this option together with the desired flag or flag combination." / "-G FLAGS  Discard reads that have
    any of the flags specified by FLAGS set. FLAGS are specified as for the -g option."
                                                                                -> excl = (0x704 | G) & ~g; SUPPLEMENTARY counts;
  * "-Q, --min-MQ INT  Only count reads with mapping quality greater than or equal to INT [0]";
  * "-J  Include reads with deletions in depth computation." and "-s  For the overlapping section of a read pair, count only the bases
    of the first read. ..." (not offered), "-q, --min-BQ INT" (not offered: 0 by default), "-l INT" (not offered);
  * the depth at a position is the number of reads with a base aligned there: M, = and X.  A deletion (D) has no base (counted only
    with -J), a reference skip (N) never counts; I, S, H and P consume no reference (SAM specification, section 1.4, CIGAR table).

What the manual does not say is pinned as include/gci_hip.h states it: a record with refID < 0, pos < 0 or an unselected contig is
skipped; zero-length operations cover nothing; what reaches beyond the contig's end is dropped; operation codes 9 - 15 in a record
that is not skipped, and a record that runs past the end of the stream (skipped or not), are GCI_E_MALFORMED; a <l_seq>S<n>N placeholder
with a CG:B,I / B,i tag stands for the tag's operations (formats/bam.py::decode_record, as htslib restores it)."""
import struct

import numpy as np

from gci_amd.formats import bam as bamfmt

EXCL_DEFAULT = 0x704
COVERING = (1 << 0) | (1 << 7) | (1 << 8)              # M = X
GCI_E_MALFORMED = -7
NO_STATUS = (1 << 64) - 1


def bounds_ok(stream, off, has_seq=True) -> bool:
    """The record at `off` lies inside the stream and its lengths agree with its block_size (the record filter's rule)."""
    n, off = int(stream.shape[0]), int(off)
    if off + 36 > n:
        return False
    bs, _ref, _pos, l_rn, _mq, _bin, n_cig, _flag, l_seq = struct.unpack_from("<iiiBBHHHi", memoryview(stream), off)
    if bs < 32 or off + 4 + bs > n or l_seq < 0:
        return False
    aux = off + 36 + l_rn + 4 * n_cig + (((l_seq + 1) // 2 + l_seq) if has_seq else 0)
    return aux <= off + 4 + bs


def is_skipped(rv, ref_sel, excl=EXCL_DEFAULT, min_mapq=0) -> bool:
    return bool(rv.flag & excl) or rv.mapq < min_mapq or rv.ref_id < 0 or rv.ref_id >= len(ref_sel) or rv.pos < 0 or ref_sel[rv.ref_id] < 0


def record_intervals(rv, count_del=False):
    """[(start, end)] with `end` the last covered base: one per maximal run of covering operations; not clamped."""
    out, at, start = [], rv.pos, None
    for op, length in rv.cigar:
        if op > 8 or not (bamfmt.REF_CONSUMING >> op) & 1 or length == 0:
            continue
        if (COVERING >> op) & 1 or (count_del and op == bamfmt.OP["D"]):
            if start is None:
                start = at
        elif start is not None:
            out.append((start, at - 1))
            start = None
        at += length
    if start is not None:
        out.append((start, at - 1))
    return out


def stream_depth(stream, offs, lengths, ref_sel, excl=EXCL_DEFAULT, min_mapq=0, count_del=False):
    """-> (per selected contig its int64 depths, the status word).  Records that are malformed cover nothing here."""
    diff = [np.zeros(int(L) + 1, dtype=np.int64) for L in lengths]
    status = NO_STATUS
    for i, off in enumerate(np.asarray(offs).tolist()):
        if not bounds_ok(stream, off):
            status = min(status, (i << 8) | -GCI_E_MALFORMED)
            continue
        rv = bamfmt.decode_record(stream, off)
        if is_skipped(rv, ref_sel, excl, min_mapq):
            continue
        if any(op > 8 for op, _ in rv.cigar):
            status = min(status, (i << 8) | -GCI_E_MALFORMED)
        c = int(ref_sel[rv.ref_id])
        L = int(lengths[c])
        for a, b in record_intervals(rv, count_del):
            if a < L:
                diff[c][a] += 1
                diff[c][min(b + 1, L)] -= 1
    return [np.cumsum(d[:-1]) for d in diff], status


def stream_depth_per_base(stream, offs, lengths, ref_sel, excl=EXCL_DEFAULT, min_mapq=0, count_del=False):
    """The same depths the slow way: one increment per covered base of every operation (what the statement above is checked against)."""
    depth = [np.zeros(int(L), dtype=np.int64) for L in lengths]
    for off in np.asarray(offs).tolist():
        if not bounds_ok(stream, off):
            continue
        rv = bamfmt.decode_record(stream, off)
        if is_skipped(rv, ref_sel, excl, min_mapq):
            continue
        c, at = int(ref_sel[rv.ref_id]), rv.pos
        for op, length in rv.cigar:
            if op > 8 or not (bamfmt.REF_CONSUMING >> op) & 1:
                continue
            if op in (0, 7, 8) or (count_del and op == 2):
                for p in range(at, min(at + length, int(lengths[c]))):
                    depth[c][p] += 1
            at += length
    return depth
