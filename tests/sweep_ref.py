"""The statement of filter_sweep.py's tables in plain Python over formats.bam.decode_record, integers only (include/gci_hip.h:
gci_bam_sweep).

A record is PRIMARY when fate_ref would call it mapq, clip, identity, kept or error for a reference-side reason: it lies inside the
stream, and is not none (flag 0x4, refID outside the table, pos < 0, an unselected contig), secondary or supplementary.  With windows
it counts only if its reference span [pos, pos + max(R, 1)) overlaps one of its contig's windows [B, E): pos < E and pos + max(R, 1) > B,
R the bases under M, D, N, = and X.  S, M (M, = and X together), I, D, N are the totals of its CIGAR (decode_record restores a CG:B,I
array behind the placeholder), NM its first NM tag.  With B = 10^K:

    mapq      row = the MAPQ byte
    clip      S / (M + I + S) ROUNDED UP to K digits: row b holds ((b - 1) / B, b / B]; `undefined` when the denominator is 0
    identity  (M + I + D - NM) / (M + I + D) TRUNCATED to K digits: row b holds [b / B, (b + 1) / B); `<0` for a negative numerator, `>1`
              for one beyond the denominator; `undefined` without NM, with an NM of a non-integer type, with a zero denominator

Every row carries records (1 a record), bases (M a record) and, in the _others columns, those of the records that pass the OTHER TWO
tests at the run's thresholds: pm = mapq >= mq, pc = S / (M + I + S) <= cp, pi = (M + I + D - NM) / (M + I + D) >= ip, each on its own,
an undefined quantity failing.  The status word names the first record that runs past the stream or contradicts its block_size (not
counted) or is counted and holds an operation code 9 - 15; nothing else is reported."""
from fractions import Fraction

import numpy as np

import cover_ref as R
from gci_amd import _lib
from gci_amd.formats import bam as bamfmt

E_MALFORMED = -7
NO_STATUS = R.NO_STATUS
COLUMNS = ("value", "records", "bases", "records_others", "bases_others", "kept_at", "kept_bases_at")
Rows = _lib.SweepRows                                      # the row numbers, as the macros of include/gci_hip.h give them


def digits_long(n: int, d: int, K: int):
    """floor(n * 10^K / d) by long division, 0 <= n <= d -> (the quotient, a remainder is left)."""
    q, r = divmod(n, d)
    for _ in range(K):
        r *= 10
        assert r < 1 << 64                                 # (every total is below 2^57)
        q, r = q * 10 + r // d, r % d
    return q, r != 0


def digits_fraction(n: int, d: int, K: int):
    """The same from the exact quotient: a second opinion."""
    x = Fraction(n, d) * 10 ** K
    return x.numerator // x.denominator, x.denominator != 1


def totals(cigar):
    """-> (S, M, I, D, N, an operation code 9 - 15 turned up)."""
    t = [0] * 16
    for op, ln in cigar:
        t[op] += ln
    return t[4], t[0] + t[7] + t[8], t[1], t[2], t[3], any(t[9:])


def entries(stream, offs, ref_sel):
    """Per record None (not primary), "malformed", or (sel, pos, mapq, S, M, I, D, N, NM or None, bad): what the tables are made of."""
    out = []
    for off in np.asarray(offs).tolist():
        if not R.bounds_ok(stream, off):
            out.append("malformed")
            continue
        rv = bamfmt.decode_record(stream, off)
        if R.is_skipped(rv, ref_sel, 0x904, 0):
            out.append(None)
            continue
        nm = rv.aux["NM"][1] if "NM" in rv.aux and rv.aux["NM"][0] in "cCsSiI" else None
        out.append((int(ref_sel[rv.ref_id]), rv.pos, rv.mapq) + totals(rv.cigar)[:5] + (nm, totals(rv.cigar)[5]))
    return out


def record_rows(e, run, rows, digits_of=digits_long):
    """-> ((mapq row, clip row, identity row), (pm, pc, pi)) of a primary record's entry."""
    _sel, _pos, mapq, S, M, I, D, _N, nm, _bad = e
    mq, cp, ip = run
    den1, den2 = M + I + S, M + I + D
    if den1 == 0:
        row_c, pc = rows.clip_undef, False
    else:
        q, rest = digits_of(S, den1, rows.digits)
        row_c, pc = rows.clip0 + q + (1 if rest else 0), S / den1 <= cp
    if nm is None or den2 == 0:
        row_i, pi = rows.iden_undef, False
    else:
        num = den2 - nm
        row_i = rows.iden_below if num < 0 else rows.iden_above if num > den2 else rows.iden0 + digits_of(num, den2, rows.digits)[0]
        pi = num / den2 >= ip
    return (rows.mapq0 + mapq, row_c, row_i), (mapq >= mq, pc, pi)


def table_of(ents, run, digits, win=None, win0=None, digits_of=digits_long):
    """-> (the table uint64 [rows, 4], the status word) from entries()."""
    rows = Rows(digits)
    table = [[0, 0, 0, 0] for _ in range(rows.rows)]
    status = NO_STATUS
    for i, e in enumerate(ents):
        if e == "malformed":
            status = min(status, (i << 8) | -E_MALFORMED)
        if e is None or e == "malformed":
            continue
        sel, pos, M, D, N = e[0], e[1], e[4], e[6], e[7]
        if win0 is not None:
            if sel + 1 >= len(win0):
                continue
            span = max(M + D + N, 1)
            if not any(pos < b and pos + span > a for a, b in np.asarray(win)[int(win0[sel]):int(win0[sel + 1])].tolist()):
                continue
        if e[9]:
            status = min(status, (i << 8) | -E_MALFORMED)
        which, passes = record_rows(e, run, rows, digits_of)
        for k in range(3):
            row = table[which[k]]
            row[0] += 1
            row[1] += M
            if passes[(k + 1) % 3] and passes[(k + 2) % 3]:
                row[2] += 1
                row[3] += M
    return np.asarray(table, dtype=np.uint64).reshape(rows.rows, 4), status


def stream_table(stream, offs, ref_sel, run, digits, win=None, win0=None):
    """The heads form of a stream (cover_cases.to_heads) holds the same records: its table and status word are these."""
    return table_of(entries(stream, offs, ref_sel), run, digits, win, win0)


def kept_at(table, digits):
    """Per numeric row (records, bases) that would be `kept` with this one threshold at the row's value: {row: (records, bases)}."""
    rows, t = Rows(digits), [[int(x) for x in r] for r in np.asarray(table).tolist()]
    passing = lambda rs: (sum(t[r][2] for r in rs), sum(t[r][3] for r in rs))          # noqa: E731
    kept = {}
    for v in range(256):
        kept[rows.mapq0 + v] = passing(range(rows.mapq0 + v, rows.mapq0 + 256))
    for b in range(rows.bins + 1):
        kept[rows.clip0 + b] = passing(range(rows.clip0, rows.clip0 + b + 1))
        kept[rows.iden0 + b] = passing(list(range(rows.iden0 + b, rows.iden0 + rows.bins + 1)) + [rows.iden_above])
    return kept


def value_of(rows, r: int) -> str:
    special = {rows.clip_undef: "undefined", rows.iden_undef: "undefined", rows.iden_below: "<0", rows.iden_above: ">1"}
    if r in special:
        return special[r]
    if r < rows.clip0:
        return str(r - rows.mapq0)
    digits = "%0*d" % (rows.digits + 1, r - (rows.clip0 if r < rows.clip_undef else rows.iden0))       # the integer row, never a float
    return digits[0] + "." + digits[1:]


def render(table, digits) -> str:
    """The three tables of one file as filter_sweep.py writes them."""
    rows, kept = Rows(digits), kept_at(table, digits)
    lines = []
    for name, a, b in (("mapq", rows.mapq0, rows.clip0), ("clip", rows.clip0, rows.clip_undef + 1), ("identity", rows.iden_below, rows.iden_undef + 1)):
        lines += ["#" + name, "\t".join(COLUMNS)]
        for r in range(a, b):
            k = kept.get(r, ("-", "-"))
            lines.append("\t".join([value_of(rows, r)] + [str(int(x)) for x in table[r]] + [str(k[0]), str(k[1])]))
    return "\n".join(lines) + "\n"


def file_text(k, path, table, digits) -> str:
    return "#file\t%d\t%s\tprimary=%d\n" % (k, path, int(sum(int(x) for x in table[:256, 0]))) + render(table, digits)
