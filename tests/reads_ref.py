"""The statement of filter_reads.py's rows in plain Python over formats.bam.decode_record (include/gci_hip.h: gci_bam_reads_size).

A record is LISTED when its class (tests/fate_ref.py, or the join's) is a bit of the mask and -- with windows -- its reference span
[pos, pos + max(R, 1)) overlaps one of its contig's windows [B, E): pos < E and pos + max(R, 1) > B.  R is the bases under M, D, N, =
and X.  Its row is

    file name contig start end strand flag mapq M I D S NM clip identity class        tab-separated, '\\n' at the end

with M the bases under M, = and X together, NM the first NM tag of an integer type (else `.`), clip = dec6(S, M + I + S), identity =
dec6(M + I + D - NM, M + I + D), `.` where the denominator is 0 (identity also where NM is `.`), and dec6 truncated in exact integers.
The status word names the first record whose class bit is set and that is malformed (no row), cannot have that class at all (refID,
pos or contig say `none`: GCI_E_INVALID, no row), or is listed and holds an operation code 9 - 15 (the row stays)."""
import numpy as np

import cover_ref as R
from gci_amd.formats import bam as bamfmt

CLASS_NAMES = ("none", "secondary", "supplementary", "mapq", "clip", "identity", "kept", "error", "shadowed", "unpaired", "contig", "overlap", "joined")
COLUMNS = ("file", "name", "contig", "start", "end", "strand", "flag", "mapq", "M", "I", "D", "S", "NM", "clip", "identity", "class")
E_INVALID, E_MALFORMED = -1, -7
NO_STATUS = R.NO_STATUS


def dec6(n: int, d: int) -> str:
    a = abs(n)
    return ("-" if n < 0 else "") + "%d.%06d" % (a // d, ((a % d) * 10 ** 6) // d)


def totals(cigar):
    """-> (M, I, D, S, R, an operation code 9 - 15 turned up)."""
    t = [0] * 16
    for op, ln in cigar:
        t[op] += ln
    return t[0] + t[7] + t[8], t[1], t[2], t[4], t[0] + t[7] + t[8] + t[2] + t[3], any(t[9:])


def record_fields(rv):
    """What a row says of a decoded record, but its file, contig and class."""
    M, I, D, S, span, bad = totals(rv.cigar)
    nm = rv.aux["NM"][1] if "NM" in rv.aux and rv.aux["NM"][0] in "cCsSiI" else None
    clip = dec6(S, M + I + S) if M + I + S else "."
    identity = dec6(M + I + D - nm, M + I + D) if (M + I + D and nm is not None) else "."
    cols = [rv.pos, rv.pos + span, "-" if rv.flag & 0x10 else "+", rv.flag, rv.mapq, M, I, D, S, "." if nm is None else nm, clip, identity]
    return cols, span, bad


def overlaps(pos, span, windows) -> bool:
    return any(pos < e and pos + max(span, 1) > b for b, e in windows)


def stream_rows(stream, offs, ref_sel, names, classes, mask, win=None, win0=None, file_no=1):
    """-> ([(record index, row bytes)] in record order, the status word).  names: the selected contigs' names (bytes); win / win0: the
    windows as gci_bam_reads_size takes them, or None.  The heads form of a stream (cover_cases.to_heads) holds the same records: its
    rows and status word are these."""
    rows, status = [], NO_STATUS
    for i, off in enumerate(np.asarray(offs).tolist()):
        c = int(classes[i])
        if not (c < 32 and (mask >> c) & 1):
            continue
        if not R.bounds_ok(stream, off):
            status = min(status, (i << 8) | -E_MALFORMED)
            continue
        rv = bamfmt.decode_record(stream, off)
        if R.is_skipped(rv, ref_sel, 0, 0) or int(ref_sel[rv.ref_id]) >= len(names):
            status = min(status, (i << 8) | -E_INVALID)
            continue
        sel = int(ref_sel[rv.ref_id])
        cols, span, bad = record_fields(rv)
        if win0 is not None and not overlaps(rv.pos, span, [tuple(w) for w in np.asarray(win)[int(win0[sel]):int(win0[sel + 1])].tolist()]):
            continue
        if bad:
            status = min(status, (i << 8) | -E_MALFORMED)
        row = b"\t".join([str(file_no).encode(), rv.name.encode(), names[sel]] + [str(x).encode() for x in cols] + [CLASS_NAMES[c].encode()]) + b"\n"
        rows.append((i, row))
    return rows, status


def text(rows) -> bytes:
    return b"".join(r for _, r in rows)
