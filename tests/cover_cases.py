"""Named inputs of the cover kernels (gci_bam_cover_*): a header plus records made with formats.bam.encode_record, the smallest shapes
at which the kernels can go wrong.  case(name) -> dict(stream, offs, lengths, ref_sel, runs); every run is (excl, min_mapq, count_del).
want(name, run) -> (depths per selected contig, status word) from tests/cover_ref.py, computed once."""
import functools
import struct

import numpy as np

import cover_ref as R
from gci_amd.formats import bam as bamfmt

CH = 2048                                              # GCI_COVER_CHUNK_OPS
M, I, D, N, S, H, P, EQ, X = range(9)
PLAIN = (R.EXCL_DEFAULT, 0, False)
WITH_DEL = (R.EXCL_DEFAULT, 0, True)


def rec(ref_id, pos, cigar, name="r", mapq=60, flag=0, l_seq=4, aux=b"", **kw):
    return bamfmt.encode_record(ref_id, pos, name, mapq, flag, cigar, l_seq, aux, **kw)


def assemble(refs, records, ref_sel=None, runs=(PLAIN, WITH_DEL), cut=0):
    """refs: [(name, length)]; ref_sel: per refID the index among the selected contigs or -1 (default: all, in order); cut: bytes
    taken off the end of the stream (the last record then runs past it)."""
    hdr = bamfmt.encode_header([n for n, _ in refs], [l for _, l in refs])
    offs, at = [], len(hdr)
    for r in records:
        offs.append(at)
        at += len(r)
    blob = hdr + b"".join(records)
    stream = np.frombuffer(blob[:len(blob) - cut] if cut else blob, dtype=np.uint8).copy()
    sel = np.arange(len(refs), dtype=np.int32) if ref_sel is None else np.asarray(ref_sel, dtype=np.int32)
    lengths = [l for (_, l), s in sorted(zip(refs, sel.tolist()), key=lambda x: x[1]) if s >= 0]
    return dict(stream=stream, offs=np.asarray(offs, dtype=np.uint64), lengths=lengths, ref_sel=sel, runs=list(runs))


def to_heads(stream, offs):
    """The heads form of a stream (gci_bam_heads): every record without its SEQ / QUAL bytes, block_size shortened, l_seq unchanged; a
    record whose lengths contradict its block_size (or that runs past the end) as its 36 fixed bytes with l_seq = -1."""
    first = int(offs[0]) if len(offs) else int(stream.shape[0])
    out, new_offs = [stream[:first].tobytes()], []
    at = first
    for off in np.asarray(offs).tolist():
        new_offs.append(at)
        if not R.bounds_ok(stream, off):
            core = bytearray(stream[off:off + 36].tobytes().ljust(36, b"\0"))
            struct.pack_into("<i", core, 0, 32)
            struct.pack_into("<i", core, 20, -1)
            piece = bytes(core)
        else:
            bs, l_rn, n_cig, l_seq = (struct.unpack_from("<i", stream, off)[0], int(stream[off + 12]), struct.unpack_from("<H", stream, off + 16)[0],
                                      struct.unpack_from("<i", stream, off + 20)[0])
            head = off + 36 + l_rn + 4 * n_cig
            aux = head + (l_seq + 1) // 2 + l_seq
            body = stream[off + 4:head].tobytes() + stream[aux:off + 4 + bs].tobytes()
            piece = struct.pack("<i", len(body)) + body
        out.append(piece)
        at += len(piece)
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy(), np.asarray(new_offs, dtype=np.uint64)


# ---- the example alignment of the SAM specification, section 1.1 -- the one answer here that does not come from this project's code
SAM_SPEC_DEPTH = np.array([0] * 6 + [1] * 2 + [3] * 6 + [2] + [3] * 3 + [1] + [2] * 2 + [1] + [0] * 6 + [1] * 5 + [0] * 2 + [1] + [2] * 4 + [1] * 5,
                          dtype=np.int64)             # 1-based 7-8: 1; 9-14: 3; 15: 2; 16-18: 3; 19: 1; 20-21: 2; 22: 1; 23-28: 0; 29-33: 1; 34-35: 0; 36: 1; 37-40: 2; 41-45: 1
SAM_SPEC_DEPTH_J = SAM_SPEC_DEPTH.copy()
SAM_SPEC_DEPTH_J[18] = 2                               # 1-based 19: r001's deletion


def _sam_spec():
    return assemble([("ref", 45)], [
        rec(0, 6, [(M, 8), (I, 2), (M, 4), (D, 1), (M, 3)], "r001", 30, 99, 17),
        rec(0, 8, [(S, 3), (M, 6), (P, 1), (I, 1), (M, 4)], "r002", 30, 0, 14),
        rec(0, 8, [(S, 5), (M, 6)], "r003", 30, 0, 11),
        rec(0, 15, [(M, 6), (N, 14), (M, 5)], "r004", 30, 0, 11),
        rec(0, 28, [(H, 6), (M, 5)], "r003", 17, 2064, 5),
        rec(0, 36, [(M, 9)], "r001", 30, 147, 9)])


def _operations():
    return assemble([("c", 200)], [
        rec(0, 3, [(M, 5), (I, 2), (D, 3), (N, 4), (S, 2), (H, 1), (P, 1), (EQ, 3), (X, 2)]),          # every operation code
        rec(0, 10, [(M, 0), (M, 4), (D, 0), (M, 3), (N, 0), (I, 0), (EQ, 0), (M, 2)]),                  # zero-length operations
        rec(0, 20, [(D, 3), (M, 4), (N, 2)]), rec(0, 30, [(N, 3), (M, 4), (D, 2)]),                    # leading and trailing D / N
        rec(0, 40, [(M, 3), (D, 2), (D, 1), (M, 3)]),                                                  # D D
        rec(0, 50, [(M, 4), (I, 3), (M, 4)]),                                                          # I between two M
        rec(0, 60, [(S, 5), (H, 3)]),                                                                  # only S / H
        rec(0, 70, []),                                                                                # n_cigar = 0
        rec(0, 80, [(D, 4)]), rec(0, 90, [(N, 4)]), rec(0, 100, [(D, 2), (N, 2), (D, 2)])])


def _excluded():
    refs = [("a", 300), ("b", 300)]
    recs = [rec(0, 10 * k, [(M, 20)], flag=f) for k, f in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0x1, 0x10 | 0x80))]
    recs += [rec(0, 100, [(M, 20)], mapq=10), rec(0, 105, [(M, 20)], mapq=9), rec(0, 110, [(M, 20)], mapq=0)]
    recs += [rec(-1, 120, [(M, 20)]), rec(1, 130, [(M, 20)]), rec(0, -1, [(M, 20)]), rec(0, 140, [(M, 20)], flag=0x100 | 0x400)]
    runs = [PLAIN, (R.EXCL_DEFAULT & ~0x100, 0, False), (R.EXCL_DEFAULT | 0x800, 0, False), (R.EXCL_DEFAULT, 10, False), (0, 0, True)]
    return assemble(refs, recs, ref_sel=[0, -1], runs=runs)


def _second_contig_selected():
    return assemble([("a", 300), ("b", 300), ("c", 50)], [rec(0, 5, [(M, 9)]), rec(1, 5, [(M, 9)]), rec(2, 5, [(M, 9)]), rec(2, 45, [(M, 9)])],
                    ref_sel=[-1, 1, 0])


def _contig_ends():
    lens = [1, 4095, 4096, 4097]
    refs = [("l%d" % l, l) for l in lens]
    recs = []
    for c, L in enumerate(lens):
        recs += [rec(c, 0, [(M, L)]), rec(c, max(L - 3, 0), [(M, min(3, L))]),                         # the whole contig; ending on its last base
                 rec(c, max(L - 2, 0), [(M, 2), (D, 1), (M, 6)]), rec(c, L - 1, [(M, 1), (N, 3), (M, 2)])]   # reaching beyond its end
    recs.append(rec(3, 4000, [(M, 50), (D, 60), (M, 40)]))
    # forged: reference lengths that sum past 2^31 (a covering run that begins beyond it too)
    recs.append(rec(3, 10, [(M, (1 << 28) - 1)] * 9 + [(D, 5), (M, 7), (N, (1 << 28) - 1), (M, 3)]))
    return assemble(refs, recs)


def _pattern(n, seed):
    rng = np.random.default_rng(seed)
    ops = rng.choice([M, M, M, I, D, N, EQ, X, S, P], size=n)
    lens = rng.integers(0, 4, size=n)
    return [(int(o), int(l)) for o, l in zip(ops, lens)]


def _chunks():
    refs = [("c", 60000)]
    recs = [rec(0, 100 * k, _pattern(n, n)) for k, n in enumerate((CH - 1, CH, CH + 1, 2 * CH + 1))]
    recs += [rec(0, 7000, [(M, 1)] * (CH + 5)),                                                        # a covering run straddling the boundary
             rec(0, 7100, [(M, 1)] * CH + [(D, 2)] + [(M, 1)] * 3),                                    # a D exactly on it: first of the next chunk
             rec(0, 7200, [(M, 1)] * (CH - 1) + [(D, 2)] + [(M, 1)] * 4),                              # ... last of this chunk
             rec(0, 7300, [(M, 1)] * (CH - 1) + [(I, 1), (I, 1)] + [(M, 1)] * 3),                      # the run goes on across I I on the boundary
             rec(0, 7400, [(M, 2)] * 63 + [(D, 1)] + [(M, 2)] * 64 + [(N, 1)] + [(M, 1)] * 10)]        # the same at the 64-lane rounds
    return assemble(refs, recs)


def _phases():
    """l_read_name of 1, 2, 3 and 4 (mod 4): the CIGAR begins at every byte phase (the stream's own phase varies with the records too)."""
    refs = [("c", 30000)]
    recs = []
    for k, name in enumerate(["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg"]):
        recs += [rec(0, 50 * k, _pattern(70, 100 + k), name), rec(0, 1000 * k + 3000, _pattern(CH + 1, 200 + k), name, l_seq=k)]
    return assemble(refs, recs)


def _long_cigar():
    refs = [("c", 300000)]
    big = _pattern(65536 + 1, 7)
    other = bamfmt.encode_aux([("NM", "i", 3), ("XS", "Z", "behind other tags"), ("XB", "B:C", [1, 2, 3])])
    small = [(M, 5), (D, 2), (M, 3), (N, 4), (M, 2)]
    cg_i = bamfmt.encode_aux([("CG", "B:i", [(l << 4) | o for o, l in small])])
    cg_z = bamfmt.encode_aux([("CG", "Z", "not an array")])
    recs = [rec(0, 1000, big, l_seq=10, aux=other),                                                   # encode_record: <l_seq>S<n>N + CG:B,I behind the tags
            rec(0, 50, [(S, 9), (N, 16)], l_seq=9, aux=other + cg_i),                                 # B,i
            rec(0, 100, [(S, 9), (N, 16)], l_seq=9, aux=other),                                       # the placeholder without a tag
            rec(0, 150, [(S, 9), (N, 16)], l_seq=9, aux=cg_z + cg_i),                                 # the FIRST CG tag counts
            rec(0, 200, [(S, 8), (M, 16)], l_seq=9, aux=cg_i)]                                        # not the placeholder: op0 is not <l_seq>S
    return assemble(refs, recs)


def _op9():
    # (operation code 9 in a skipped record -- an unselected contig, an excluded flag -- is not looked at)
    return assemble([("a", 300), ("b", 300)], [rec(1, 5, [(M, 4), (9, 3)]), rec(0, 5, [(9, 9)], flag=0x4), rec(0, 10, [(M, 4)]),
                                             rec(0, 20, [(M, 4), (9, 3), (M, 2)]), rec(0, 30, [(15, 1)])], ref_sel=[0, -1], runs=[PLAIN])


def _cut_off():
    return assemble([("a", 300)], [rec(0, 5, [(M, 9)]), rec(0, 10, [(M, 9)]), rec(0, 20, [(M, 9)], aux=bamfmt.encode_aux([("NM", "i", 1)]))], cut=5,
                    runs=[PLAIN])


def _op9_then_cut_off():
    return assemble([("a", 300)], [rec(0, 5, [(M, 9)]), rec(0, 10, [(10, 9)]), rec(0, 20, [(M, 9)])], cut=30, runs=[PLAIN])


def _random(n_rec, seed):
    rng = np.random.default_rng(seed)
    refs = [("x", 5000), ("y", 4097), ("z", 12000)]
    recs = []
    for k in range(n_rec):
        c = int(rng.integers(-1, 3))
        L = refs[c][1] if c >= 0 else 1000
        flag = int(rng.choice([0, 0, 0, 0x10, 0x800, 0x4, 0x100, 0x200, 0x400, 0x1 | 0x40]))
        recs.append(rec(c, int(rng.integers(0, L)), _pattern(int(rng.integers(0, 40)), seed * 100000 + k), "q%d" % k, int(rng.integers(0, 61)), flag,
                        int(rng.integers(0, 9))))
    return assemble(refs, recs, runs=[PLAIN, (R.EXCL_DEFAULT, 20, True)])


SCAN_BLOCK = 4096                                       # entries a workgroup of the device's exclusive scans takes


def _scan_blocks():
    """More than 4096 records AND more than 4096 chunks in every run, so that all three device scans (chunks per record, reference
    length and intervals per chunk) cross their blocks: 4095 kept records of one chunk each, then a record of three chunks -- chunks
    4095, 4096 and 4097, its own reference-length prefix crosses the block --, then 600 records of the random kind."""
    rng = np.random.default_rng(3)
    refs = [("x", 5000), ("y", 4097), ("z", 12000)]
    recs = []
    for k in range(SCAN_BLOCK - 1):
        c = int(rng.integers(0, 3))
        recs.append(rec(c, int(rng.integers(0, refs[c][1])), _pattern(int(rng.integers(1, 20)), 300000 + k), "s%d" % k, int(rng.integers(20, 61)),
                        int(rng.choice([0, 0x10, 0x800, 0x1 | 0x40])), int(rng.integers(0, 9))))
    recs.append(rec(2, 100, _pattern(2 * CH + 1, 9), "straddle"))
    tail = _random(600, 4)
    recs += [tail["stream"][int(a):int(b)].tobytes() for a, b in zip(tail["offs"], list(tail["offs"][1:]) + [tail["stream"].shape[0]])]
    return assemble(refs, recs, runs=[PLAIN, (R.EXCL_DEFAULT, 20, True)])


BUILDERS = {
    "sam_spec": _sam_spec, "operations": _operations, "excluded": _excluded, "second_contig_selected": _second_contig_selected,
    "contig_ends": _contig_ends, "chunks": _chunks, "phases": _phases, "long_cigar": _long_cigar, "op9": _op9, "cut_off": _cut_off,
    "op9_then_cut_off": _op9_then_cut_off, "no_records": lambda: assemble([("a", 100)], []),
    "one_record": lambda: assemble([("a", 100)], [rec(0, 3, [(M, 5), (D, 1), (M, 5)])]),
    "random_3000": lambda: _random(3000, 1),
    "scan_blocks": _scan_blocks,
}
NAMES = list(BUILDERS)
MALFORMED = {"op9": 3, "cut_off": 2, "op9_then_cut_off": 1}          # the record the status word must name


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def heads(name):
    c = case(name)
    return to_heads(c["stream"], c["offs"])


@functools.lru_cache(maxsize=None)
def want(name, run):
    c = case(name)
    return R.stream_depth(c["stream"], c["offs"], c["lengths"], c["ref_sel"], *run)


def chunks_per_record(name, run):
    """What k_cover_parse makes of the case: per record its chunks of CH operations, 0 for a skipped or malformed one."""
    c = case(name)
    out = []
    for off in c["offs"].tolist():
        n = 0
        if R.bounds_ok(c["stream"], off):
            rv = bamfmt.decode_record(c["stream"], off)
            if not R.is_skipped(rv, c["ref_sel"], run[0], run[1]):
                n = (len(rv.cigar) + CH - 1) // CH
        out.append(n)
    return np.asarray(out, dtype=np.int64)


def pairs():
    """(name, run) of every case."""
    return [(name, run) for name in NAMES for run in case(name)["runs"]]
