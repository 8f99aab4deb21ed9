"""Named inputs of the PAF filter (k_paf.hip, and host_io.cpp, which shares its grammar): the smallest files at which the line-start
kernel, the two instantiations of the tokeniser and the scoring can go wrong.  Nothing here is random.

A case is (name, [file bytes ...], targets, (map_qual, mq_cutoff, iden_percent)); TABLES["A" .. "E"] hold them in the order of the
sections below.  EXPECT[name] says what the reference (the oracle) does with the case:

    None                          it goes through: the per-file dicts and the high-quality set are compared
    ("raises", file, line)        it raises on line `line` (1-based) of file `file`; line 0 = while it scores that file
    ("documented", status, line)  it goes through, and this project documents an error status instead (line None: not reported)

GPU[table] names the cases the GPU test runs: every case that goes through, and a chosen part of the raising ones (each of those is a
call of its own).  Every line has a query name of its own (L00017) and coordinates that carry its number, so a misplaced line start shows
as a wrong name, a wrong column or an error -- except in table D, which is about the scoring of one query's lines.

Geometry: the files of a call lie back to back in ONE device buffer, assumed to begin at a 16-byte boundary.  k_paf_lines lays its
16-byte windows, 1024-byte waves and 4096-byte tiles over a file from the 16-byte boundary at or below its first byte, `delta` bytes in
front of it, so the boundary B of a file lies at its byte B - delta.  A workgroup of k_paf_tokenise takes 256 lines and copies them into
LDS if s1 - s0 + al <= 49152, al = the distance of s0 from the 16-byte boundary at or below it.  line_starts(), seam_geometry() and
stretches() compute all of this from the bytes; tests/test_paf_cases_cpu.py holds the cases' names against them."""
import numpy as np

from gci_amd._lib import GCI_E_INVALID, GCI_E_MALFORMED, GCI_E_ZERO_DIV

ARGS = (30, 50, 0.9)
T = ["t0", "t1", "t2"]
LDS_BYTES = 49152
GROUP = 256                                  # lines of one tokeniser workgroup

TABLES = {k: [] for k in "ABCDE"}
EXPECT = {}
GPU = {k: [] for k in "ABCDE"}
SEAMS = {}                                   # name -> dict(file, B, place, delta): what a seam case's name claims
STRETCHES = {}                               # name -> (file, [s1 - s0 + al of every workgroup]) or (file, "global")


def _add(table, name, files, expect=None, targets=T, args=ARGS, gpu=True):
    assert name not in EXPECT and all(max(f, default=0) < 0x80 for f in files), name
    TABLES[table].append((name, [bytes(f) for f in files], list(targets), tuple(args)))
    EXPECT[name] = expect
    if gpu:
        GPU[table].append(name)


def case(name):
    for rows in TABLES.values():
        for c in rows:
            if c[0] == name:
                return c
    raise KeyError(name)


# ---- rows -------------------------------------------------------------------------------------------------------------------------

def cols(i, q=None, qlen=1000, qs=None, qe=None, t="t0", ts=None, te=None, nm=500, aln=500, mapq=60):
    """The twelve columns of line number i, as bytes; the coordinates carry i."""
    v = (q if q is not None else "L%05d" % i, qlen, i % 400 if qs is None else qs, i % 400 + 500 if qe is None else qe, "+", t, 100000,
         100 + i if ts is None else ts, 600 + i if te is None else te, nm, aln, mapq)
    return [x if isinstance(x, bytes) else str(x).encode() for x in v]


def hit(i, **kw):
    return b"\t".join(cols(i, **kw))


def padded(line, n, key=b"cg:Z:"):
    """`line` with one more column that brings it to n bytes."""
    fill = n - len(line) - 1 - len(key)
    assert fill >= 0, (len(line), n)
    return line + b"\t" + key + b"M" * fill


def join(lines, seps, final=True):
    """The lines with the separators of `seps` in turn behind them."""
    out = bytearray()
    for k, ln in enumerate(lines):
        out += ln
        if final or k + 1 < len(lines):
            out += seps[k % len(seps)]
    return bytes(out)


def line_starts(b):
    """Universal newlines: a line starts at byte 0, behind '\\n', and behind a '\\r' that no '\\n' follows."""
    a = np.frombuffer(b, dtype=np.uint8)
    if a.shape[0] == 0:
        return np.zeros(0, np.int64)
    prev, cur = a[:-1], a[1:]
    return np.concatenate([[0], np.flatnonzero((prev == 10) | ((prev == 13) & (cur != 10))) + 1]).astype(np.int64)


def delta_of(files, f):
    return sum(len(x) for x in files[:f]) % 16


def stretches(files, f):
    """s1 - s0 + al of every tokeniser workgroup of file f."""
    base, b = sum(len(x) for x in files[:f]), files[f]
    st = line_starts(b)
    out = []
    for g in range(0, st.shape[0], GROUP):
        s0 = int(st[g])
        s1 = int(st[g + GROUP]) if g + GROUP < st.shape[0] else len(b)
        out.append(s1 - s0 + (base + s0) % 16)
    return out


def seam_geometry(files, f, B):
    """What lies at boundary B of file f: (delta, byte at B - 1, byte at B, whether a line starts at B, whether one starts at B + 1,
    the number of line starts in the tile in front of B)."""
    d, b = delta_of(files, f), files[f]
    p = B - d
    st = set(line_starts(b).tolist())
    return d, b[p - 1:p], b[p:p + 1], p in st, p + 1 in st, sum(1 for s in st if B - 4096 <= s + d < B)


def replay(line, targets=T):
    """The exception class GCI.py:217-229 ends with on this line, or None."""
    try:
        c = line.decode("ascii").strip().split("\t")
        if c[5] in targets:
            for k in (1, 2, 3, 7, 8):
                int(c[k])
            a, b = int(c[9]), int(c[10])
            int(c[11])
            a / b
    except (IndexError, ValueError, ZeroDivisionError) as e:
        return type(e)
    return None


MIX = [b"\n", b"\r\n", b"\r"]
SEPS = {"lf": [b"\n"], "crlf": [b"\r\n"], "cr": [b"\r"], "mix": MIX}

# ---- A: line starts at their seams ---------------------------------------------------------------------------------------------------
# place: "last"  = the separator's last byte at B - 1 (the next line starts at B);
#        "first" = the separator's first byte at B - 1: "\r" | "\n" (the next line starts at B + 1);
#        "lone"  = a lone "\r" at B - 1 and an ordinary byte at B, in a file whose other lines end otherwise.
# B = 16: the line in front of the seam is too short for twelve columns; it names no selected target (six columns).  Behind B = 8192
# the tile 4096 .. 8191 has no line start: the line in front of the seam begins in the first tile.
PLACES = {"lf": ("last", "lone"), "crlf": ("last", "first", "lone"), "cr": ("last",), "mix": ("last", "first", "lone")}
BOUNDS = (16, 1024, 4096, 8192)


def seam_file(sep, B, place, delta, tag, bad=None):
    """-> (bytes, index of the line behind the seam).  tag: first digit of the line numbers.  bad: a line to put behind the seam."""
    seps = SEPS[sep]
    seam_sep = b"\r" if place == "lone" else seps[0] if len(seps) == 1 else b"\r\n"
    assert place != "first" or seam_sep == b"\r\n"
    next_start = B - delta + (1 if place == "first" else 0)
    n0 = tag * 100
    if B == 16:
        n = next_start - len(seam_sep)
        assert n >= 8
        head, k = b"", 0
        lines = [b"s" * (n - 7) + b"\t\t\t\t\tzz"]
    else:
        first = hit(n0)
        head, k = first + seps[0], 1
        lines = [first, padded(hit(n0 + 1), next_start - len(seam_sep) - len(head))]
    lines += [bad if bad is not None else hit(n0 + 2), hit(n0 + 3)]
    out = bytearray()
    for j, ln in enumerate(lines):
        out += ln
        if j == k:
            out += seam_sep
        elif j + 1 < len(lines) or place == "last":                  # (no final separator behind the other two placements)
            out += seps[j % len(seps)]
    return bytes(out), k + 1


def pad_file(k, tag=9):
    """Two lines that pass, k bytes beyond a multiple of 16 in all."""
    a = hit(tag * 100, q="P%05d" % (tag * 100)) + b"\n"
    b = hit(tag * 100 + 1, q="P%05d" % (tag * 100 + 1))
    n = len(b) + 8
    n += (k - (len(a) + n + 1)) % 16
    out = a + padded(b, n) + b"\n"
    assert len(out) % 16 == k
    return out


def _seams():
    n_wide = 0
    bad_turn = 0
    for sep in ("lf", "crlf", "cr", "mix"):
        for B in BOUNDS:
            for place in PLACES[sep]:
                name = "%s_%d_%s" % (sep, B, place)
                f, k = seam_file(sep, B, place, 0, 1)
                _add("A", "seam_" + name, [f])
                SEAMS["seam_" + name] = dict(file=0, B=B, place=place, delta=0)
                # the same as the second file of a call: delta takes every value (B = 16 leaves room for 0 .. 6 only)
                if B == 16:
                    d = (len(sep) + len(place)) % 7
                else:
                    d, n_wide = n_wide % 16, n_wide + 1
                f2, _ = seam_file(sep, B, place, d, 2)
                _add("A", "seam2_" + name, [pad_file(d), f2])
                SEAMS["seam2_" + name] = dict(file=1, B=B, place=place, delta=d)
                # E: a line the reference raises on, behind the seam -- a missing column and a zero alignment length in turn
                bad = b"L%05d\tx" % 102 if bad_turn % 2 == 0 else hit(102, aln=0)
                bad_turn += 1
                f3, k3 = seam_file(sep, B, place, 0, 1, bad=bad)
                _add("E", "seam_err_" + name, [f3], ("raises", 0, k3 + 1))
                SEAMS["seam_err_" + name] = dict(file=0, B=B, place=place, delta=0)


_seams()


def _further():
    three = [hit(i) for i in range(3)]
    for sep in ("lf", "crlf", "cr"):
        _add("A", "final_%s_with" % sep, [join(three, SEPS[sep])])
        _add("A", "final_%s_without" % sep, [join(three, SEPS[sep], final=False)])
    _add("A", "only_lf", [b"\n"], ("raises", 0, 1))
    a = join([hit(i) for i in range(10, 14)], MIX)
    b = join([hit(i) for i in range(20, 24)], MIX, final=False)
    none = join([hit(30, t="other"), hit(31, mapq=29), hit(32, nm=449), hit(33, t="t00")], MIX)
    _add("A", "empty_between", [a, b"", b])
    _add("A", "none_pass", [none])
    _add("A", "all_pass", [join([hit(i) for i in range(300)], MIX)])                   # n_hits == n_lines, two workgroups
    _add("A", "one_file_with_hits", [none, a, none.replace(b"L0003", b"L0004")])        # with_hits == 1
    _add("A", "two_files_with_hits", [a, none, b])


_further()

# ---- C: grammar ------------------------------------------------------------------------------------------------------------------------
# (in front of B: B runs this table a second time through the other instantiation of the tokeniser)
BYTES = [b for b in range(0x80) if b not in (9, 10, 13)]
C_LINES = []                                  # (tag, line): every line of the table, in order
C_DOCUMENTED = {}                             # tag -> (status, reason)

# the raising lines the GPU test runs, one call each; the CPU test runs every one
C_GPU_BYTES = (0x00, 0x1b, 0x1c, 0x1f, 0x2e, 0x5f, 0x61, 0x7f)          # (those of them that raise in the position)
C_GPU_RAISING = (["%s_%02x" % (p, b) for p in ("last", "numfirst", "numlast") for b in C_GPU_BYTES] +
                 ["int__1", "int_1_", "int_1__0", "int_plus_blank", "int_empty", "int_2p63", "tab_eleven_and_tab", "tab_empty_tenth",
                  "blank_only", "cols5", "cols6_sel", "cols11_sel", "alnlen0", "qlen0_one", "qlen0_many", "int32_one", "int32_many"])


def _grammar():
    n = [0]

    def line(tag, make, lead=b"", trail=b""):
        i = n[0]
        n[0] += 1
        c = cols(i)
        c = make(c, i) or c
        C_LINES.append((tag, lead + b"\t".join(c) + trail))

    def setcol(k, f):
        def make(c, i):
            c[k] = f(c[k])
        return make

    for b in BYTES:
        x = bytes([b])
        line("first_%02x" % b, lambda c, i: None, lead=x)
        line("last_%02x" % b, lambda c, i: None, trail=x)
        line("numfirst_%02x" % b, setcol(7, lambda v: x + v))
        line("numlast_%02x" % b, setcol(7, lambda v: v + x))
        line("inname_%02x" % b, setcol(0, lambda v: v[:3] + x + v[3:]))
    # int(): signs, zeros, underscores, blanks of int()'s own set inside a column
    for tag, v in (("plus5", b"+5"), ("minus0", b"-0"), ("minus5", b"-5"), ("zeros30", b"0" * 30 + b"7"), ("1_000", b"1_000"),
                   ("blanks", b" \x0b5\x0c "), ("_1", b"_1"), ("1_", b"1_"), ("1__0", b"1__0"), ("plus_blank", b"+ 5"), ("empty", b"")):
        line("int_" + tag, setcol(2, lambda _v, v=v: v))
    # 18 and 19 digits, 2^63 - 1 and 2^63 as the mapping quality: compared with the two thresholds and nowhere else
    for tag, v in (("18digits", b"9" * 18), ("19digits", b"1" + b"0" * 18), ("2p63m1", b"9223372036854775807"), ("2p63", b"9223372036854775808")):
        line("int_" + tag, setcol(11, lambda _v, v=v: v))
    # the reference goes on with a big integer (a mapping quality above both thresholds); the kernel's parse_int documents
    # GCI_E_MALFORMED for a value beyond 63 bits
    C_DOCUMENTED["int_2p63"] = GCI_E_MALFORMED
    # tabs at the end of the line: strip() takes them unless something stands behind them
    line("tab_trailing", lambda c, i: None, trail=b"\t\t\t")
    line("tab_columns", lambda c, i: None, trail=b"\t\t\tz")
    line("tab_blank_mix", lambda c, i: None, lead=b" \x1c", trail=b" \t\x1f\t ")
    line("tab_eleven_and_tab", lambda c, i: c[:11], trail=b"\t")                       # an empty last column: strip() eats it
    line("tab_empty_tenth", lambda c, i: c[:10] + [b"", c[11]])
    C_LINES.append(("blank_only", b" \x0b\t \x1c"))
    # 5, 6, 11 and 12 columns, for a selected and an unselected target
    line("cols5", lambda c, i: c[:5])
    line("cols6_sel", lambda c, i: c[:6])
    line("cols6_unsel", lambda c, i: c[:5] + [b"other"])
    line("cols11_sel", lambda c, i: c[:11])
    line("cols11_unsel", lambda c, i: c[:5] + [b"other"] + c[6:11])
    line("cols12_sel", lambda c, i: None)
    line("cols12_unsel", lambda c, i: c[:5] + [b"other"] + c[6:9] + [b"x", b"0", b""])  # never parsed
    line("alnlen0", setcol(10, lambda v: b"0"))
    line("int32_max", setcol(8, lambda v: b"2147483647"))


_grammar()
C_RAISING = [(tag, ln) for tag, ln in C_LINES if replay(ln) is not None or tag in C_DOCUMENTED]
C_ACCEPTED = [(tag, ln) for tag, ln in C_LINES if replay(ln) is None and tag not in C_DOCUMENTED]


def filler_call(bad_lines, at=5, n=8, long=False):
    """Filler lines that pass with `bad_lines` from index `at` on; long: every line long enough for the tokeniser's global path."""
    lines = [hit(900 + i, q="F%05d" % i) for i in range(n)]
    lines[at:at] = bad_lines
    return join(lines, MIX)


def _grammar_cases():
    _add("C", "c_accepted", [join([ln for _, ln in C_ACCEPTED], MIX)])
    done = {"qlen0_one", "qlen0_many", "int32_one", "int32_many"}
    for tag, ln in C_RAISING:
        exp = ("documented", C_DOCUMENTED[tag], 6) if tag in C_DOCUMENTED else ("raises", 0, 6)
        _add("C", "c_raise_" + tag, [filler_call([ln])], exp, gpu=tag in C_GPU_RAISING)
        done.add(tag)
    # errors of the scoring: a query length of 0 divides (GCI.py:249), through the one-line path and the general one
    _add("C", "c_raise_qlen0_one", [filler_call([hit(1, qlen=0)])], ("raises", 0, 0))
    _add("C", "c_raise_qlen0_many", [filler_call([hit(1, qlen=0), hit(1, qlen=0, ts=5000, te=5600)])], ("raises", 0, 0))
    # coordinates beyond int32: the reference goes on, a gci_rec cannot hold them -- the documented GCI_E_INVALID
    _add("C", "c_raise_int32_one", [filler_call([hit(1, te=1 << 31)])], ("documented", GCI_E_INVALID, None))
    _add("C", "c_raise_int32_many", [filler_call([hit(1), hit(1, ts=(1 << 40), te=(1 << 40) + 9000)])], ("documented", GCI_E_INVALID, None))
    # (a byte of C_GPU_BYTES that goes through in a position is in c_accepted; every other name must exist)
    missing = [t for t in C_GPU_RAISING if t not in done and not any(t == "%s_%02x" % (p, b) for p in ("last", "numfirst", "numlast") for b in C_GPU_BYTES)]
    assert not missing, missing


_grammar_cases()

# ---- B: the two instantiations of the tokeniser -------------------------------------------------------------------------------------------


def _group_of(i0, total):
    """GROUP lines that pass, '\\n' behind each, `total` bytes in all."""
    each = total // GROUP
    return b"".join(padded(hit(i), each + (total - each * GROUP if i == i0 + GROUP - 1 else 0) - 1) + b"\n" for i in range(i0, i0 + GROUP))


def lds_limit_file(base):
    """3 x 256 lines behind `base` bytes of other files: the first workgroup's stretch far below the limit, the second's
    s1 - s0 + al exactly the limit, the third's one byte beyond it."""
    g0 = _group_of(0, 100 * GROUP + 7)
    al1 = (base + len(g0)) % 16
    g1 = _group_of(GROUP, LDS_BYTES - al1)
    al2 = (base + len(g0) + len(g1)) % 16
    g2 = _group_of(2 * GROUP, LDS_BYTES + 1 - al2)
    return g0 + g1 + g2


def globalised(lines):
    """Every line with padding that takes its workgroup beyond the limit, whatever 256 lines it is grouped with: 200 bytes in the strand
    column, which no statement of the reference reads -- the line's ends and its number of columns stay what the case is about -- (a line
    of fewer than five columns stays as it is), and one line of more than the limit at the end for the last workgroup."""
    out = []
    for ln in lines:
        c = ln.split(b"\t")
        if len(c) > 4:
            c[4] += b"~" * 200
        out.append(b"\t".join(c))
    return out + [padded(hit(999, q="G00999"), LDS_BYTES + 50)]


def _paths():
    f = lds_limit_file(0)
    _add("B", "lds_limit", [f])
    STRETCHES["lds_limit"] = (0, [100 * GROUP + 7, LDS_BYTES, LDS_BYTES + 1])
    p = pad_file(5)
    _add("B", "lds_limit_delta5", [p, lds_limit_file(len(p))])
    STRETCHES["lds_limit_delta5"] = (1, [100 * GROUP + 7 + 5, LDS_BYTES, LDS_BYTES + 1])
    _add("B", "one_long_line", [padded(hit(0), 50000) + b"\n"])
    STRETCHES["one_long_line"] = (0, [50001])
    # 5000 and 9000 bytes: once a cg:Z: thirteenth column, once a long query name; tiles of k_paf_lines without a line start
    longs = [hit(0), padded(hit(1), 5000), hit(2), padded(hit(3), 9000), hit(4, q="N5" + "n" * (5000 - len(hit(4, q="N5")))),
             hit(5, q="N9" + "n" * (9000 - len(hit(5, q="N9")))), hit(6)]
    assert [len(x) for x in longs[1:6:2] + longs[4:5]] == [5000, 9000, 9000, 5000]
    _add("B", "long_lines", [join(longs, MIX)])
    STRETCHES["long_lines"] = (0, "lds")
    _add("B", "long_lines_global", [join(longs + [padded(hit(7), LDS_BYTES)], MIX, final=False)])
    STRETCHES["long_lines_global"] = (0, "global")
    # a query name of 65535 bytes passes, one of 65536 is the documented GCI_E_INVALID (gci_rec.name_len has sixteen bits)
    _add("B", "name_65535", [join([hit(0), hit(1, q="Q" * 65535), hit(2)], MIX)])
    _add("B", "name_65536", [join([hit(0), hit(1, q="Q" * 65536), hit(2)], MIX)], ("documented", GCI_E_INVALID, None))
    # table C once more, every workgroup on the global path: the same dicts as c_accepted but for the one line at the end
    _add("B", "c_accepted_global", [join(globalised([ln for _, ln in C_ACCEPTED]), MIX)])
    STRETCHES["c_accepted_global"] = (0, "global")
    STRETCHES["c_accepted"] = (0, "lds")
    for tag in ("last_7f", "numfirst_1c", "int_1__0", "cols11_sel", "alnlen0", "blank_only"):
        ln = dict(C_RAISING)[tag]
        lines = globalised([hit(900 + i, q="F%05d" % i) for i in range(5)] + [ln] + [hit(906, q="F00906")])
        _add("B", "c_raise_global_" + tag, [join(lines, MIX)], ("raises", 0, 6))
        STRETCHES["c_raise_global_" + tag] = (0, "global")


_paths()
GLOBAL_EXTRA = "G00999"                       # the query of the line globalised() adds

# ---- D: scoring ------------------------------------------------------------------------------------------------------------------------
D_TARGETS = ["t2", "t0", "t1"]                # unsorted: the tie between two targets goes to the greater NAME, not the greater index


def _scoring():
    def r(q, qs, qe, t, ts, te, nm=None, aln=100, mapq=60, qlen=1000):
        return hit(0, q=q, qlen=qlen, qs=qs, qe=qe, t=t, ts=ts, te=te, nm=aln if nm is None else nm, aln=aln, mapq=mapq)

    L = [r("one", 0, 500, "t0", 100, 600),
         r("one_and_fail", 0, 500, "t0", 100, 600), r("one_and_fail", 0, 900, "t1", 7000, 7900, mapq=29),
         r("twice", 0, 500, "t0", 100, 600), r("twice", 0, 500, "t0", 100, 600),                     # the general path
         r("touching", 0, 100, "t0", 1000, 1100), r("touching", 100, 200, "t0", 1100, 1200),
         r("nested", 100, 200, "t0", 1100, 1200), r("nested", 0, 500, "t0", 1000, 1500),
         r("equal_longest", 0, 100, "t0", 2000, 2100), r("equal_longest", 200, 300, "t0", 1000, 1100),
         r("equal_longest", 400, 450, "t0", 3000, 3050),
         # a block whose end lies before its start, alone: the one-line path (the issue's line, and the query side)
         r("inv_t_alone", 0, 50, "t0", 100, 50, aln=50, qlen=100), r("inv_q_alone", 50, 0, "t0", 100, 150),
         r("zero_t_alone", 0, 50, "t0", 100, 100), r("zero_q_alone", 50, 50, "t0", 100, 150),
         r("minus1_t_alone", 0, 50, "t0", 51, 50),
         # ... alone on the general path (the same line twice: the first sorted block is held against itself)
         r("inv_t_twice", 0, 50, "t0", 100, 50), r("inv_t_twice", 0, 50, "t0", 100, 50),
         r("minus1_t_twice", 0, 50, "t0", 51, 50), r("minus1_t_twice", 0, 50, "t0", 51, 50),
         # ... beside proper ones: the first of the sorted list, behind a proper one, nothing but such blocks
         r("inv_t_first", 0, 50, "t0", 100, 50), r("inv_t_first", 50, 100, "t0", 100, 200), r("inv_t_first", 100, 150, "t0", 300, 350),
         r("inv_t_later", 0, 50, "t0", 0, 10), r("inv_t_later", 50, 100, "t0", 100, 50),
         r("inv_t_inside", 0, 50, "t0", 0, 100), r("inv_t_inside", 50, 100, "t0", 50, 20),
         r("inv_t_all", 0, 50, "t0", 100, 50), r("inv_t_all", 50, 100, "t0", 200, 120),
         r("zero_t_beside", 0, 50, "t0", 100, 100), r("zero_t_beside", 50, 100, "t0", 100, 100), r("zero_t_beside", 100, 150, "t0", 300, 301),
         # ... on the query side, where the covered length decides between targets: t0 covers -50 - 50 + 100 = 0 and loses to t1's 10
         # (counted once, 50, it would win)
         r("inv_q_first", 100, 50, "t0", 100, 150), r("inv_q_first", 100, 200, "t0", 200, 300), r("inv_q_first", 0, 10, "t1", 500, 510),
         # behind a proper block it is counted once: t0 covers 10 - 5 = 5 and loses to t1's 6 (dropped, 10, it would win)
         r("inv_q_later", 0, 10, "t0", 100, 110), r("inv_q_later", 100, 95, "t0", 200, 205), r("inv_q_later", 0, 6, "t1", 500, 506),
         r("zero_q_beside", 50, 50, "t0", 100, 150), r("zero_q_beside", 50, 50, "t0", 200, 250), r("zero_q_beside", 0, 1, "t1", 500, 501),
         # an exact tie between targets: the greater name wins, whatever the order of `targets` and of the lines
         r("tie", 0, 100, "t1", 100, 200), r("tie", 0, 100, "t2", 300, 400), r("tie", 0, 100, "t0", 500, 600)]
    # 300 hits over 3 targets, coordinates descending as the lines go on
    for j in range(300):
        L.append(r("many", (299 - j) * 10, (299 - j) * 10 + 15, "t%d" % (j % 3), 90000 - j * 10, 90000 - j * 10 + 15, nm=15 - (j % 7 == 0), aln=15,
                   qlen=5000, mapq=30 + j % 40))
    _add("D", "scoring", [join(L, MIX)], targets=D_TARGETS)
    # two files.  `sum`: the identities 0.1, 0.2, 0.3 of t0 add up to 0.6000000000000001 in line order and to 0.6 in any order that
    # begins with the second file; t1's single 0.2 lies between the two means.  `late`: one line in file 0 (the one-line path), its
    # second in file 1 (the general path).  `only0` is emitted again by file 1.
    f0 = [r("sum", 0, 100, "t0", 0, 100, nm=10, qlen=300), r("sum", 0, 300, "t1", 1000, 1300, nm=60, aln=300, qlen=300),
          r("late", 0, 100, "t0", 100, 200), r("only0", 0, 100, "t2", 100, 200)]
    f1 = [r("sum", 100, 200, "t0", 100, 200, nm=20, qlen=300), r("late", 100, 400, "t1", 5000, 5300), r("sum", 200, 300, "t0", 200, 300, nm=30, qlen=300),
          r("only1", 0, 100, "t2", 100, 200)]
    assert (0.1 + 0.2 + 0.3) / 3 > 60 / 300 > (0.2 + 0.3 + 0.1) / 3
    _add("D", "two_files", [join(f0, MIX), join(f1, MIX, final=False)], targets=D_TARGETS, args=(30, 50, 0.0))


_scoring()

# ---- E: the first error ------------------------------------------------------------------------------------------------------------------


def _first_error():
    mal, zero = b"L%05d\t100\t0\tx", hit(0, q="Z", aln=0)
    for a, b in ((256, 600), (257, 258)):                    # 1-based lines: two workgroups apart, and side by side in one
        for tag, first, second in (("mz", mal % a, zero), ("zm", zero, mal % b)):
            lines = [hit(i) for i in range(700)]
            lines[a - 1], lines[b - 1] = first, second
            _add("E", "first_%d_%d_%s" % (a, b, tag), [join(lines, MIX)], ("raises", 0, a))
    # a scoring error in file 0 comes before a malformed line of file 1: the reference reads and scores file after file
    _add("E", "score_before_line", [hit(0, q="q", qlen=0) + b"\n", b"x\n"], ("raises", 0, 0))
    _add("E", "line_in_second_file", [join([hit(i) for i in range(5)], MIX), join([hit(10), hit(11), b"x", hit(12, aln=0)], MIX)], ("raises", 1, 3))


_first_error()
