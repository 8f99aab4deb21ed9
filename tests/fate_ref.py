"""The statement of filter_depth.py's classes in plain Python over formats.bam.decode_record: every record falls into exactly one
class, named after the FIRST test of read_sam (the reference's GCI.py:152-168) it fails, in the reference's order.

  0 none           flag 0x4, refID < 0 or >= n_ref, pos < 0 or an unselected contig: the reference's fetch never yields the record
                   (the skip rule of gci_bam_cover_size with excl = 0x4)
  1 secondary      flag & 0x100
  2 supplementary  flag & 0x800
  3 mapq           mapq < -mq
  4 clip           not S / (M + I + S) <= cp                        (M: the bases under M, = and X together)
  5 identity       not (M - mm) / (M + I + D) >= ip
  6 kept           oracle.bam_filter_record_py(...) is not None: the record reaches GCI.py:166
  7 error          a record the status word reports: malformed, or one the reference raises on (KeyError for no NM, a non-integer NM,
                   ZeroDivisionError) -- a run ends there

A record of class 0 - 3 is settled by its core fields: its tags and its CIGAR are not looked at.  The depth of a class is
cover_ref.stream_depth over the offsets of that class's records with excl = 0 (their flags are what put them in the class)."""
import numpy as np

import cover_ref as R
from gci_amd.formats import bam as bamfmt
from oracle import gci_oracle

NAMES = ("none", "secondary", "supplementary", "mapq", "clip", "identity", "kept", "error")
NONE, SECONDARY, SUPPLEMENTARY, MAPQ, CLIP, IDENTITY, KEPT, ERROR = range(8)
E_NO_NM, E_ZERO_DIV, E_BAD_NM_TYPE, E_MALFORMED = -3, -4, -5, -7
NO_STATUS = R.NO_STATUS


def record_class(stream, off, ref_sel, map_qual, cp, ip):
    """-> (class, status code): the status code is 0 unless the class is `error`."""
    if not R.bounds_ok(stream, off):
        return ERROR, E_MALFORMED
    rv = bamfmt.decode_record(stream, off)
    if R.is_skipped(rv, ref_sel, 0x4, 0):
        return NONE, 0
    if rv.flag & 0x100:
        return SECONDARY, 0
    if rv.flag & 0x800:
        return SUPPLEMENTARY, 0
    if rv.mapq < map_qual:
        return MAPQ, 0
    if "NM" in rv.aux and rv.aux["NM"][0] not in "cCsSiI":                     # (pysam would hand the reference a float)
        return ERROR, E_BAD_NM_TYPE
    references = ["ref%d" % k for k in range(len(ref_sel))]
    targets = [references[k] for k in range(len(ref_sel)) if ref_sel[k] >= 0]
    try:
        if gci_oracle.bam_filter_record_py(rv, references, targets, map_qual, 0, cp, ip) is not None:
            return KEPT, 0
    except KeyError:
        return ERROR, E_NO_NM
    except ZeroDivisionError:
        return ERROR, E_ZERO_DIV
    tot = [0] * 16
    for op, ln in rv.cigar:
        tot[op] += ln
    M, I, S = tot[0] + tot[7] + tot[8], tot[1], tot[4]
    return (IDENTITY if S / (M + I + S) <= cp else CLIP), 0


def stream_classes(stream, offs, ref_sel, map_qual, cp, ip):
    """-> (class per record uint8, records per class uint64 [8], status word)."""
    cls = np.zeros(len(offs), dtype=np.uint8)
    status = NO_STATUS
    for i, off in enumerate(np.asarray(offs).tolist()):
        c, code = record_class(stream, off, ref_sel, map_qual, cp, ip)
        cls[i] = c
        if code:
            status = min(status, (i << 8) | -code)
    return cls, np.bincount(cls, minlength=8).astype(np.uint64), status


def class_depth(stream, offs, lengths, ref_sel, cls, c, count_del=False, excl=0):
    """The per-base depth of the records of class c (per selected contig, int64)."""
    return R.stream_depth(stream, np.asarray(offs)[cls == c], lengths, ref_sel, excl, 0, count_del)[0]
