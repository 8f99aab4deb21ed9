"""Named inputs of the mismatch kernels (gci_fasta_codes, gci_bam_mismatch_*, gci_mismatch_sites_*): the smallest shapes at which the
kernels can go wrong.  case(name) -> dict(stream, offs, lengths, ref_sel, codes, runs); every run is (excl, min_mapq).  want(name, run)
-> (events, counts, status word) from tests/mismatch_ref.py, computed once.  EXPECTED holds the answers written by hand.
fasta_case(name) -> dict(text, bodies, dst, lengths); site_case(name) -> dict(lengths, mism, depth, runs) with runs of (min_reads,
frac_ppm, windows)."""
import functools

import numpy as np

import cover_cases as CC
import mismatch_ref as R
from cover_cases import CH, D, EQ, H, I, M, N, P, S, X, assemble      # noqa: F401
from gci_amd.formats import bam as bamfmt

EXCL = R.EXCL_DEFAULT
ACGT = b"ACGT"
QRY, REF = (M, I, S, EQ, X), (M, D, N, EQ, X)


def contig_seq(n, seed):
    return bytes(np.frombuffer(ACGT, dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def read_for(ref, pos, cigar, seed, sub=0.05):
    """The bases of a read that follows `ref` from `pos` under `cigar`: a slice of the reference under M = X with a seeded share of
    substituted bases (beyond the contig's end: random bases), random bases under I and S."""
    rng = np.random.default_rng(seed)
    out, p = [], pos
    for op, n in cigar:
        if op in (M, EQ, X):
            piece = np.frombuffer(ref[p:p + n].upper().ljust(n, b"A"), dtype=np.uint8).copy() if n else np.zeros(0, dtype=np.uint8)
            hit = np.flatnonzero(rng.random(n) < sub)
            piece[hit] = np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, hit.shape[0])]
            out.append(piece.tobytes())
        elif op in (I, S):
            out.append(bytes(np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, n)]))
        if op in REF:
            p += n
    return b"".join(out)


def mrec(refs, ref_id, pos, cigar, seed=0, name="r", mapq=60, flag=0, seq=None, sub=0.05, **kw):
    if seq is None:
        seq = read_for(refs[ref_id][1] if 0 <= ref_id < len(refs) else b"", max(pos, 0), cigar, seed, sub)
    return bamfmt.encode_record(ref_id, pos, name, mapq, flag, cigar, len(seq), seq=seq, **kw)


def build(refs, records, ref_sel=None, runs=((EXCL, 0),), cut=0):
    """refs: [(name, sequence bytes)].  The code array is the statement's, of a FASTA text of width 60, 15 in the padding."""
    c = assemble([(n, len(s)) for n, s in refs], records, ref_sel=ref_sel, runs=list(runs), cut=cut)
    sel = c["ref_sel"].tolist()
    chosen = [refs[k] for k in sorted((k for k in range(len(refs)) if sel[k] >= 0), key=lambda k: sel[k])]
    offs, total = R.layout(c["lengths"])
    text = b"".join(b">" + n.encode() + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for n, s in chosen)
    spans = R.fasta_records(text)
    c["codes"] = R.fasta_codes(text, [(a, b) for _, a, b in spans], offs, total, fill=15)
    c["fasta"] = text
    return c


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------
def _phases():
    """An M that begins at an odd and at an even query position, behind a 1-base S and behind a 1-base I; l_seq odd."""
    refs = [("c", b"ACGTACGTACGTACGTACGT")]
    recs = [mrec(refs, 0, 2, [(S, 1), (M, 5)], seq=b"TGTCCG"),              # GTACG: base 4 reads C
            mrec(refs, 0, 2, [(M, 5)], seq=b"GTACC"),                       # base 6 reads C; l_seq odd
            mrec(refs, 0, 0, [(M, 2), (I, 1), (M, 3)], seq=b"ACTGTT"),      # AC | GTA: base 4 reads T; the M begins at q = 3
            mrec(refs, 0, 0, [(S, 1), (I, 1), (M, 4)], seq=b"TTCCGT"),      # ACGT: base 0 reads C; the M begins at q = 2
            mrec(refs, 0, 10, [(M, 5)], seq=b"GTACT")]                      # GTACG: base 14, the last (high) nibble of the last byte
    return build(refs, recs)


def _letters():
    """= and X whose bases contradict their letter: the bases decide.  Read nibble 0, 15 and an IUPAC code; reference N, lower case, R."""
    refs = [("c", b"ACGTACGTAC"), ("d", b"acgNRt")]
    recs = [mrec(refs, 0, 0, [(EQ, 3), (X, 3), (M, 2)], seq=b"AGGTACGA"),   # ACG TAC GT: base 1 under =, none under X, base 7
            mrec(refs, 0, 0, [(M, 4)], seq=b"=NRA"),                        # only A against T is compared
            mrec(refs, 1, 0, [(M, 6)], seq=b"AGGAAT")]                      # a = A, G against c, g = G, N and R never, t = T
    return build(refs, recs)


EXPECTED = {
    ("phases", (EXCL, 0)): ([(0, 4), (0, 6), (0, 4), (0, 0), (0, 14)], [5, 5, 24]),
    ("letters", (EXCL, 0)): ([(0, 1), (0, 7), (0, 3), (1, 1)], [3, 4, 13]),
    ("lseq", (EXCL, 0)): ([(0, 1)], [4, 1, 4]),
}


def _lseq():
    """l_seq == 0: counted, nothing compared, no status.  l_seq one more and one less than S + M + I: malformed, no event.  The record
    whose operations run one base past its SEQ is the last one and its SEQ is whole bytes: a walk that took it would read the high
    nibble of its first QUAL byte, 0x11 -- an A against the T of base 7, one more pair compared and one more event."""
    refs = [("c", b"ACGTACGTACGTACGTACGT")]
    recs = [mrec(refs, 0, 0, [(M, 4)], seq=b""),
            mrec(refs, 0, 0, [(M, 4)], seq=b"AAGT"),                        # the one event
            mrec(refs, 0, 8, [(M, 4)], seq=b"TTTTT"),                       # one more: record 2
            mrec(refs, 0, 4, [(S, 1), (M, 4)], seq=b"TTTT", qual_fill=0x11)]      # one less: base q = 4 would face base 7
    return build(refs, recs)


# ---- against the statement -------------------------------------------------------------------------------------------------------------
def _lanes():
    """Operations of 1, 0, 65 and 129 bases (the lanes' steps of 4 bases, the rounds of 256), H P N D between matches."""
    refs = [("c", contig_seq(3000, 1))]
    recs = [mrec(refs, 0, 10, [(H, 5), (M, 1), (D, 2), (M, 0), (P, 3), (M, 65), (N, 7), (M, 129), (I, 2), (M, 1), (H, 4)], 1, sub=0.3),
            mrec(refs, 0, 400, [(M, 255), (D, 1), (M, 256), (D, 1), (M, 257)], 2, sub=0.3),
            mrec(refs, 0, 1300, [(M, 3), (I, 1), (M, 4), (I, 1), (M, 5), (S, 3)], 3, sub=0.5),
            mrec(refs, 0, 1400, [(M, 1024)], 4, sub=1.0)]
    return build(refs, recs)


def _ops(n_ops, seed, sub=0.2):
    def make():
        refs = [("c", contig_seq(3 * n_ops + 500, seed))]
        body = [(o, l + (1 if o in (M, EQ, X) else 0)) for o, l in CC._pattern(n_ops, seed)]
        return build(refs, [mrec(refs, 0, 7, body, seed, sub=sub), mrec(refs, 0, 100, [(M, 1)] * n_ops, seed + 1, sub=0.5)])
    return make


def _cg():
    """A record of more than 65535 operations: the placeholder in the record, the operations in the CG array, SEQ behind the placeholder."""
    refs = [("c", contig_seq(150000, 5))]
    body = [(S, 30)] + [(M, 1), (I, 1)] * 32768 + [(M, 1), (H, 40)]
    return build(refs, [mrec(refs, 0, 1000, body, 5, sub=0.1), mrec(refs, 0, 50, [(M, 100)], 6)])


def _ends():
    """A read running over the contig's end; pos + reference length beyond 2^31; a contig of one base."""
    refs = [("a", contig_seq(100, 7)), ("b", b"G")]
    recs = [mrec(refs, 0, 90, [(M, 30)], 1, sub=0.5),
            mrec(refs, 0, 99, [(M, 1), (I, 2), (M, 5)], 2, sub=1.0),
            mrec(refs, 0, 100, [(M, 8)], 3, sub=1.0),
            mrec(refs, 1, 0, [(M, 3)], seq=b"TTT"),
            mrec(refs, 0, 50, [(M, 3)] + [(N, (1 << 28) - 1)] * 9 + [(M, 3)], 4, sub=1.0),
            mrec(refs, 0, 2 ** 31 - 10, [(M, 20)], 5, sub=1.0)]
    return build(refs, recs)


def _skip_rule():
    refs = [("a", contig_seq(300, 8)), ("b", contig_seq(300, 9))]
    body = [(M, 20), (D, 2), (M, 20)]
    recs = [mrec(refs, 0, 10 * k, body, k, flag=f, sub=0.5) for k, f in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0x1, 0x10 | 0x80))]
    recs += [mrec(refs, 0, 100, body, 20, mapq=10, sub=0.5), mrec(refs, 0, 105, body, 21, mapq=9, sub=0.5),
             mrec(refs, 1, 130, body, 22, sub=0.5), mrec(refs, 2, 130, body, 23, sub=0.5), mrec(refs, -1, 120, body, 24, sub=0.5),
             mrec(refs, 0, -1, body, 25, sub=0.5)]
    return build(refs, recs, ref_sel=[0, -1], runs=[(EXCL, 0), (EXCL & ~0x100, 0), (EXCL | 0x800, 0), (EXCL, 10), (0, 0)])


def _second_contig():
    """Only the second @SQ contig selected: its codes begin at element 0."""
    refs = [("a", contig_seq(300, 10)), ("b", contig_seq(5000, 11))]
    recs = [mrec(refs, 1, 4000, [(M, 500)], 1, sub=0.2), mrec(refs, 0, 10, [(M, 50)], 2, sub=0.5)]
    return build(refs, recs, ref_sel=[-1, 0])


def _many(n_rec, seed):
    def make():
        rng = np.random.default_rng(seed)
        refs = [("x", contig_seq(5000, seed)), ("y", contig_seq(4097, seed + 1)), ("z", contig_seq(12000, seed + 2))]
        recs = []
        for k in range(n_rec):
            c = int(rng.integers(-1, 3))
            L = len(refs[c][1]) if c >= 0 else 1000
            flag = int(rng.choice([0, 0, 0, 0x10, 0x800, 0x4, 0x100, 0x200, 0x400, 0x1 | 0x40]))
            body = [(o, l * 5) for o, l in CC._pattern(int(rng.integers(0, 14)), seed * 100000 + k)]
            recs.append(mrec(refs, c, int(rng.integers(0, L)), body, seed * 7 + k, "q%d" % k, int(rng.integers(0, 61)), flag, sub=0.1))
        return build(refs, recs, runs=[(EXCL, 0), (EXCL, 20)])
    return make


def _ont_hifi():
    """A record of short operations (every one at most 20 bases) beside one of long operations."""
    refs = [("c", contig_seq(40000, 12))]
    rng = np.random.default_rng(13)
    short = []
    for _ in range(700):
        short += [(M, int(rng.integers(1, 21))), (int(rng.choice([I, D])), int(rng.integers(1, 4)))]
    long_ = [(M, 9000), (D, 1), (M, 7000), (I, 2), (M, 3000)]
    return build(refs, [mrec(refs, 0, 100, short + [(M, 5)], 1, sub=0.04), mrec(refs, 0, 15000, long_, 2, sub=0.002)])


def _op9():
    """Codes 9 - 15 move nothing and are reported in a counted record only; the rest of the record is compared."""
    refs = [("c", contig_seq(200, 30))]
    recs = [mrec(refs, 0, 0, [(M, 10)], 1, sub=0.5), mrec(refs, 0, 5, [(9, 2), (M, 10)], 2, flag=0x4, sub=0.5),
            mrec(refs, 0, 20, [(M, 5), (9, 3), (M, 5)], 3, sub=0.5), mrec(refs, 0, 40, [(15, 1), (M, 4)], 4, sub=0.5)]
    return build(refs, recs)


def _cut_off():
    """The last record runs past the end of the stream: reported, not walked."""
    refs = [("c", contig_seq(200, 31))]
    recs = [mrec(refs, 0, 0, [(M, 10)], 1, sub=0.5), mrec(refs, 0, 5, [(M, 10)], 2, sub=0.5), mrec(refs, 0, 20, [(M, 30)], 3, sub=0.5)]
    return build(refs, recs, cut=3)


BUILDERS = {
    "phases": _phases, "letters": _letters, "lseq": _lseq, "lanes": _lanes, "ops_64": _ops(64, 20), "ops_65": _ops(65, 21),
    "ops_2048": _ops(CH, 22), "ops_2049": _ops(CH + 1, 23), "cg": _cg, "ends": _ends, "skip_rule": _skip_rule, "second_contig": _second_contig,
    "op9": _op9, "cut_off": _cut_off,
    "records_0": lambda: build([("a", b"ACGT")], []), "records_257": _many(257, 15), "records_4097": _many(4097, 16), "ont_hifi": _ont_hifi,
}
NAMES = list(BUILDERS)
MALFORMED = {"lseq": 2, "op9": 2, "cut_off": 2}          # the record the status word must name


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def want(name, run):
    c = case(name)
    return R.stream_events(c["stream"], c["offs"], c["lengths"], c["ref_sel"], c["codes"], *run)


def pairs():
    return [(name, run) for name in NAMES for run in case(name)["runs"]]


# ---- FASTA -----------------------------------------------------------------------------------------------------------------------------
def _fa(records, width=60, eol=b"\n", last_eol=True):
    out = b""
    for title, seq in records:
        out += b">" + title + eol + b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))
    return out if last_eol else out[:-len(eol)]


def _fasta(text, order, lengths=None):
    """order[r]: the index in the layout of record r, or -1 to leave it out; lengths: the layout (default: the records' own, in order)."""
    spans = R.fasta_records(text)
    seq_len = [R.seq_length(text, a, b) for _, a, b in spans]
    n = max(order) + 1
    if lengths is None:
        lengths = [0] * n
        for r, k in enumerate(order):
            if k >= 0:
                lengths[k] = seq_len[r]
    offs, total = R.layout(lengths)
    dst = [offs[k] if k >= 0 else -1 for k in order]
    return dict(text=np.frombuffer(text, dtype=np.uint8).copy(), bodies=np.array([(a, b) for _, a, b in spans], dtype=np.int64).reshape(-1, 2),
                dst=np.array(dst, dtype=np.int64), lengths=lengths, total=total)


_MIX = b"ACGTNacgtnRYKMSWBDHVUu*-=X"


def _mix(n, seed):
    return bytes(np.frombuffer(_MIX, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(_MIX), n)])


FASTA_BUILDERS = {
    "tiny": lambda: _fasta(b">a\nAC\nGT\n>b desc\nNNrY\n", [0, 1]),
    "width_60": lambda: _fasta(_fa([(b"a", _mix(10000, 1)), (b"b x", _mix(4097, 2))]), [0, 1]),
    "width_1": lambda: _fasta(_fa([(b"a", _mix(3000, 3)), (b"b", _mix(5, 4))], width=1), [0, 1]),
    "one_line": lambda: _fasta(_fa([(b"a", _mix(9000, 5))], width=10 ** 6), [0]),
    "crlf_blank": lambda: _fasta(_fa([(b"a", _mix(5000, 6)), (b"b", _mix(700, 7))], width=70, eol=b"\r\n").replace(b"\r\n", b"\r\n \r\n\r\n", 3), [0, 1]),
    "no_final_newline": lambda: _fasta(_fa([(b"a", _mix(4096 - 3, 8)), (b"b", _mix(4096, 9))], last_eol=False), [0, 1]),
    # the title line of b straddles byte 4096, that of c byte 8192; bodies run over tile edges
    "titles_on_edges": lambda: _fasta(_fa([(b"a", _mix(4020, 10)), (b"b " + b"t" * 200, _mix(3800, 11)), (b"c " + b"u" * 300, _mix(9000, 12))]),
                                      [0, 1, 2]),
    "other_order": lambda: _fasta(_fa([(b"a", _mix(5000, 13)), (b"b", _mix(100, 14)), (b"c", _mix(4097, 15))]), [2, 0, 1]),
    "left_out": lambda: _fasta(_fa([(b"a", _mix(500, 16)), (b"extra", _mix(6000, 17)), (b"b", _mix(4500, 18))]), [0, -1, 1]),
    "empty_record": lambda: _fasta(_fa([(b"a", _mix(50, 19)), (b"none", b""), (b"b", _mix(60, 20)), (b"last", b"")]), [0, -1, 1, -1]),
}
FASTA_NAMES = list(FASTA_BUILDERS)
FASTA_EXPECTED = {"tiny": {0: [1, 2, 4, 8], 4096: [15, 15, 5, 10]}}      # flat element -> the codes from there
FILL = 0xEE


@functools.lru_cache(maxsize=None)
def fasta_case(name):
    return FASTA_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def want_codes(name):
    c = fasta_case(name)
    return R.fasta_codes(c["text"].tobytes(), c["bodies"].tolist(), c["dst"].tolist(), c["total"], fill=FILL)


# ---- sites: tracks written by hand -----------------------------------------------------------------------------------------------------
def _site_runs():
    """Runs of 1, 64, 65 and 9000 elements, one across a tile edge, one from a wave's first lane (1024, in both thread mappings of the
    lister) and one across that edge (2047 - 2048); a run cut by a window edge and by two touching windows; a fraction
    exactly at the threshold and one part per million beside it; the maximum reached twice: the depth of the first."""
    lengths = [20000]
    offs, total = R.layout(lengths)
    mism, depth = np.zeros(total, dtype=np.int32), np.full(total, 8, dtype=np.int32)
    for a, n in ((100, 1), (300, 64), (500, 65), (1024, 64), (2047, 2), (4090, 10), (8192, 3)):
        mism[a:a + n] = 5
    mism[10000:19000] = 6
    mism[10500], depth[10500] = 9, 12
    mism[18999], depth[18999] = 9, 13                  # the maximum again: the depth stays 12
    # 3 of 6 is 500000 ppm exactly, the next base one part per million above a half, the third one below
    mism[1000:1003], depth[1000:1003] = [3, 500001, 499999], [6, 1000000, 1000000]
    depth[1100], mism[1100] = 0, 0                     # depth 0 and no mismatch: hot only with min_reads 0, which is refused
    runs = [(3, 500000, ()), (3, 500001, ()), (3, 499999, ()), (1, 0, ()), (6, 600000, ()), (3, 500000, ((0, 12000), (12000, 20000))),
            (3, 500000, ((4093, 4099),)), (3, 500000, ((250, 330), (330, 340), (500, 565))), (3, 1000000, ()), (7, 0, ((-5, 10 ** 9),))]
    return dict(lengths=lengths, mism=mism, depth=depth, runs=runs)


def _site_contigs():
    lengths = [4096, 5000, 100, 1]
    offs, total = R.layout(lengths)
    mism, depth = np.zeros(total, dtype=np.int32), np.full(total, 8, dtype=np.int32)
    mism[4090:4100] = 4                                # contig 0's last six bases, contig 1's first four
    mism[4096 + 4990:4096 + 5100] = 5                  # contig 1's last ten bases, then padding
    mism[4096 + 6000:4096 + 6010] = 8                  # padding only
    mism[12288 + 95:12288 + 300] = 4
    mism[16384:16390] = 6
    return dict(lengths=lengths, mism=mism, depth=depth, runs=[(3, 500000, ()), (3, 500000, ((-5, 10 ** 9),)), (5, 0, ((0, 20480),)), (7, 0, ())])


def _site_random():
    lengths = [5000, 4097, 3, 20000]
    offs, total = R.layout(lengths)
    rng = np.random.default_rng(6)
    depth = rng.integers(0, 40, total).astype(np.int32)
    mism = np.minimum(rng.integers(0, 60, total), depth).astype(np.int32)
    for a, n in zip(rng.integers(0, total, 100), rng.integers(1, 90, 100)):
        mism[a:a + n] = depth[a:a + n]
    return dict(lengths=lengths, mism=mism, depth=depth,
                runs=[(1, 0, ()), (3, 500000, ()), (5, 900000, ()), (2, 250000, ((17, 4100), (4100, 9000), (16384, 16390), (20000, 30001))), (30, 1000000, ())])


SITE_BUILDERS = {"runs": _site_runs, "contigs": _site_contigs, "random": _site_random}
SITE_NAMES = list(SITE_BUILDERS)
SITES_EXPECTED = {
    # at 500000 ppm 3 / 6 and 500001 / 1000000 are hot, 499999 / 1000000 is not: the run is 1000 - 1002 (exclusive)
    ("runs", 0): [(0, 100, 101, 5, 8), (0, 300, 364, 5, 8), (0, 500, 565, 5, 8), (0, 1000, 1002, 500001, 1000000), (0, 1024, 1088, 5, 8),
                  (0, 2047, 2049, 5, 8), (0, 4090, 4100, 5, 8), (0, 8192, 8195, 5, 8), (0, 10000, 19000, 9, 12)],
    # one part per million more: 3 / 6 is out, the run begins at 1001
    ("runs", 1): [(0, 100, 101, 5, 8), (0, 300, 364, 5, 8), (0, 500, 565, 5, 8), (0, 1001, 1002, 500001, 1000000), (0, 1024, 1088, 5, 8),
                  (0, 2047, 2049, 5, 8), (0, 4090, 4100, 5, 8), (0, 8192, 8195, 5, 8), (0, 10000, 19000, 9, 12)],
    # one less: all three
    ("runs", 2): [(0, 100, 101, 5, 8), (0, 300, 364, 5, 8), (0, 500, 565, 5, 8), (0, 1000, 1003, 500001, 1000000), (0, 1024, 1088, 5, 8),
                  (0, 2047, 2049, 5, 8), (0, 4090, 4100, 5, 8), (0, 8192, 8195, 5, 8), (0, 10000, 19000, 9, 12)],
    ("runs", 6): [(0, 4093, 4099, 5, 8)],
    ("runs", 7): [(0, 300, 330, 5, 8), (0, 330, 340, 5, 8), (0, 500, 565, 5, 8)],
    ("contigs", 0): [(0, 4090, 4096, 4, 8), (1, 0, 4, 4, 8), (1, 4990, 5000, 5, 8), (2, 95, 100, 4, 8), (3, 0, 1, 6, 8)],
}


@functools.lru_cache(maxsize=None)
def site_case(name):
    return SITE_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def want_sites(name, k):
    c = site_case(name)
    min_reads, frac, windows = c["runs"][k]
    return R.sites_of(c["mism"], c["depth"], c["lengths"], min_reads, frac, windows)
