"""Inflated BAM streams for the record walk (gci_bam_record_offsets_device, k_records.hip), made with rec_bytes / op of
tests/test_bam_decode.py and patched field by field: the smallest shapes at which the walk can go wrong.  Every case is a Case --
stream, first (where the walk starts), n_ref, offs (the records from `first` on, by construction) and, for a reject case, the index
of the one record the strict test refuses.  All of it is deterministic: a case with random bytes names its seed.

TILE: the candidate kernel's tile (256 threads x 16 positions).  cases() -> every case by name; cut_span() -> the stream, the
three records and the cut lengths of the every-cut test; fuzz(seed, n_ref) -> one random mix with its own first / cut / skip."""
import functools
import struct
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from test_bam_decode import op, rec_bytes

TILE = 4096
BIG_REF = 2**31 - 1

# byte offset of every field the strict test reads, counted from the record's block_size word
FIELDS = {"block_size": (0, "<i"), "refID": (4, "<i"), "pos": (8, "<i"), "l_read_name": (12, "<B"), "n_cigar_op": (16, "<H"),
          "l_seq": (20, "<i"), "next_refID": (24, "<i"), "next_pos": (28, "<i")}


class Case(NamedTuple):
    stream: np.ndarray
    first: int
    n_ref: int
    offs: np.ndarray                 # int64: the true records from `first` on
    reject: Optional[int] = None     # index into offs of the record that fails the strict test


def patched(rec: bytes, **fields) -> bytes:
    """`rec` with some of its fixed fields overwritten in place (the layout stays as it was)."""
    b = bytearray(rec)
    for k, v in fields.items():
        at, fmt = FIELDS[k]
        struct.pack_into(fmt, b, at, v)
    return bytes(b)


def record(ref_id=0, pos=100, name=b"r", cigar: Sequence[int] = (), l_seq=0, aux=b"", fill: Optional[bytes] = None, **fields) -> bytes:
    """One record.  fill: the bytes of SEQ + QUAL (repeated / cut to their length) instead of rec_bytes' 0x11 / 0xff."""
    r = bytearray(rec_bytes(ref_id, pos, name, 30, 0, list(cigar), l_seq, aux))
    if fill is not None and l_seq:
        at, n_sq = 36 + len(name) + 1 + 4 * len(cigar), (l_seq + 1) // 2 + l_seq
        r[at:at + n_sq] = (fill * (n_sq // len(fill) + 1))[:n_sq]
    return patched(bytes(r), **fields)


MINIMAL = record(-1, -1, b"")                        # 37 bytes: unmapped, no name, no CIGAR, no bases
assert len(MINIMAL) == 37


def assemble(records: Sequence[bytes], n_ref: int, first_index: int = 0, reject: Optional[int] = None, front: bytes = b"") -> Case:
    """The records one after the other behind `front`; the walk starts at record `first_index`."""
    sizes = np.array([len(r) for r in records], dtype=np.int64)
    offs = len(front) + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    stream = np.frombuffer(front + b"".join(records), dtype=np.uint8).copy()
    return Case(stream, int(offs[first_index]), n_ref, offs[first_index:], reject)


def fake_head(block_size: int, ref_id=0, l_seq=0) -> bytes:
    """The 36 bytes of a record that is not there: they pass the strict test wherever they lie (n_ref > ref_id)."""
    return struct.pack("<iiiBBHHHiiii", block_size, ref_id, 7, 1, 0, 0, 0, 0, l_seq, -1, -1, 0)


# ---- assorted and limit-valued records ---------------------------------------------------------------------------------------------------
def _assorted() -> Case:
    rng = np.random.default_rng(11)
    recs = [MINIMAL, record(0, 0, b"a", [op(5, "M")], 5, b"NMC\x00"), record(-1, -1, b"unmapped", [], 40),
            record(2, 99, b"", [], 0, b"XYZabc\x00"), record(1, 5, b"q" * 30, [op(1, "M")] * 300, 1), MINIMAL,
            record(0, 7, b"long", [op(3000, "M"), op(5, "S")], 3005, b"NMC\x01"), record(2, 1 << 28, b"far", [op(9, "=")], 9)]
    for _ in range(30):
        l_seq = int(rng.choice([0, 1, 2, 17, 150, 3300]))
        n_cig = int(rng.integers(0, 5))
        recs.append(record(int(rng.integers(-1, 3)), int(rng.integers(-1, 1000)), b"n" * int(rng.integers(0, 40)),
                           [op(int(rng.integers(1, 500)), "M")] * n_cig, l_seq, b"NMC\x00" * int(rng.integers(0, 3))))
    return assemble(recs, 3)


def _limits() -> Dict[str, Case]:
    n_ref = 5
    at = [record(-1, -1, b"x"), record(n_ref - 1, 0, b"x", next_refID=n_ref - 1, next_pos=0), record(0, 0, b"x", next_refID=-1, next_pos=-1),
          record(0, 0, b""), record(0, 0, b"n" * 254), record(0, 0, b"e", [op(4, "M")], 0),
          record(3, 2**31 - 1, b"p", next_pos=2**31 - 1), record(0, 0, b"exact", [op(7, "M")], 7), MINIMAL]
    assert at[3][12] == 1 and at[4][12] == 255 and len(at[7]) - 4 == 32 + 6 + 4 + 4 + 7           # (block_size == what the fields need)
    out = {"limits": assemble(at, n_ref),
           "limits n_cigar 65535": assemble([MINIMAL, record(0, 0, b"c", [op(1, "M")] * 65535, 3), MINIMAL], 2),
           "limits n_ref 0": assemble([MINIMAL, record(-1, -1, b"u", [], 12), record(-1, 50, b"v"), MINIMAL], 0),
           "limits n_ref 1": assemble([record(0, 0, b"a"), record(-1, -1, b"b"), record(0, 3, b"c", next_refID=0)], 1)}
    return out


# ---- one field wrong, in the first, a middle and the last record ---------------------------------------------------------------------
N_REF_REJECT = 4
REJECTS = {"block_size 31": dict(block_size=31), "refID n_ref": dict(refID=N_REF_REJECT), "refID -2": dict(refID=-2), "pos -2": dict(pos=-2),
           "l_read_name 0": dict(l_read_name=0), "l_seq -1": dict(l_seq=-1), "next_refID n_ref": dict(next_refID=N_REF_REJECT),
           "next_refID -2": dict(next_refID=-2), "next_pos -2": dict(next_pos=-2),
           "need block_size + 1": dict(l_read_name=5)}                 # (a 3-byte name + NUL whose record holds nothing else: 4 -> 5)


def _rejects() -> Dict[str, Case]:
    good = [record(1, 10, b"abc", [op(6, "M")], 6), MINIMAL, record(0, 3, b"abc", [op(6, "M")], 6), record(2, 9, b"k" * 9, [], 50, b"NMC\x00"),
            record(1, 10, b"abc", [op(6, "M")], 6), MINIMAL, record(3, 10, b"abc", [op(6, "M")], 6)]
    out = {}
    for why, fields in REJECTS.items():
        for where, j in (("first", 0), ("middle", 4), ("last", 6)):
            recs = list(good)
            recs[j] = patched(recs[j], **fields)
            out["reject %s, %s record" % (why, where)] = assemble(recs, N_REF_REJECT, reject=j)
    return out


# ---- positions that pass the test and are no record ----------------------------------------------------------------------------------
PATTERN = struct.pack("<ii", 0x00100000, 1)           # every 8th byte of its repetition passes with n_ref > 0x100000
PATTERN_REF = 0x100000
DENSE = bytes([0, 0, 0, 0x10, 1, 1, 1, 1])            # four of every 8 bytes of its repetition pass with n_ref > 0x10000000
DENSE_REF = 0x10000000


def _false_candidates() -> Dict[str, Case]:
    out = {}
    carrier = record(0, 5, b"carrier", [op(4800, "M")], 4800)
    at = 36 + 8 + 4 + 2400                                                    # its QUAL bytes
    carrier = carrier[:at] + PATTERN * 600 + carrier[at + 4800:]
    out["pattern in QUAL"] = assemble([MINIMAL, carrier, MINIMAL], PATTERN_REF + 1)
    out["pattern in QUAL, n_ref at the pattern's value"] = assemble([MINIMAL, carrier, MINIMAL], PATTERN_REF)
    out["pattern, then 5000 minimal records"] = assemble([record(0, 5, b"p", [op(4096, "M")], 4096, fill=PATTERN)] + [MINIMAL] * 5000,
                                                         PATTERN_REF + 1)
    out["dense pattern"] = assemble([MINIMAL, record(0, 5, b"d", [op(9000, "M")], 9000, fill=DENSE), MINIMAL, MINIMAL], DENSE_REF + 1)
    # complete heads of records that are not there: in a name, in aux data, in SEQ
    fakes = [record(0, 1, fake_head(40) + b"tail"), record(1, 2, b"a", [op(3, "M")], 3, b"XXZ" + fake_head(33) * 3 + b"\x00"),
             record(2, 3, b"s", [op(90, "M")], 90, fill=b"\x00" * 5 + fake_head(1000, 2, 4)), MINIMAL]
    out["fake heads"] = assemble([MINIMAL] + fakes * 3, 3)
    # ... one whose block_size lands exactly on the end of the stream, one whose block_size lands exactly on a true record
    recs = [MINIMAL, record(0, 1, b"h", [], 0, b"XXZ" + fake_head(33) + b"\x00"), record(1, 2, b"i", [op(20, "M")], 20), MINIMAL, MINIMAL]
    c = assemble(recs, 2)
    fake_at = int(c.offs[1]) + 36 + 2 + 3
    to_end = c.stream.copy()
    to_end[fake_at:fake_at + 4] = np.frombuffer(struct.pack("<i", to_end.shape[0] - fake_at - 4), dtype=np.uint8)
    out["fake head that ends at the end of the stream"] = c._replace(stream=to_end)
    to_rec = c.stream.copy()
    to_rec[fake_at:fake_at + 4] = np.frombuffer(struct.pack("<i", int(c.offs[3]) - fake_at - 4), dtype=np.uint8)
    out["fake head that ends at a true record"] = c._replace(stream=to_rec)
    # valid records in front of the first one (a regional call starts inside a run of members)
    out["records in front"] = assemble([MINIMAL, record(0, 1, b"front"), MINIMAL, record(1, 2, b"here"), MINIMAL], 2, first_index=3)
    out["only the last record"] = assemble([record(0, 1, b"front", [], 70)] * 40 + [MINIMAL], 2, first_index=40)
    # a position 8 bytes in front of the first record that passes the test with the first record's own head behind it: block_size
    # and refID in the tail of the record before, then the head's block_size as pos, its refID (1) as l_read_name, ...
    lead = record(0, 1, b"lead", [], 0, b"XXZ" + b"\x00" * 20 + struct.pack("<ii", 0x7F000000, 0))
    out["candidate 8 bytes in front"] = assemble([MINIMAL, lead, record(1, 3, b"first"), MINIMAL], BIG_REF, first_index=2)
    return out


# ---- the second record at every byte around a tile border ----------------------------------------------------------------------------
PLACEMENTS = range(TILE - 40, TILE + 17)


def _placement(at: int) -> Case:
    base = len(record(0, 1, b"", [op(2600, "M")], 2600))                      # 3941 bytes with an empty name
    lead = record(0, 1, b"n" * (at - base), [op(2600, "M")], 2600)
    c = assemble([lead, record(1, 2, b"second", [op(10, "M")], 10, b"NMC\x00"), MINIMAL, record(2, 3, b"x" * 17), MINIMAL], 3)
    assert int(c.offs[1]) == at
    return c


# ---- chains of minimal records: the model's candidate count is the record count ------------------------------------------------------
COUNTS = sorted({1, 2, 3, 4095, 4096, 4097} | {(1 << k) + d for k in range(2, 14) for d in (-1, 0, 1)})


def _count(n_rec: int) -> Case:
    return assemble([MINIMAL] * n_rec, 0)


@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, Case]:
    out = {"assorted": _assorted()}
    out.update(_limits())
    out.update(_rejects())
    out.update(_false_candidates())
    for at in PLACEMENTS:
        out["second record at byte %d" % at] = _placement(at)
    for n_rec in COUNTS:
        out["%d minimal records" % n_rec] = _count(n_rec)
    return out


def valid_names() -> List[str]:
    return [k for k, c in cases().items() if c.reject is None]


def reject_names() -> List[str]:
    return [k for k, c in cases().items() if c.reject is not None]


# ---- every cut through three records across a tile border ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cut_span() -> Tuple[Case, range]:
    """-> (the stream, the cut lengths): three records of 37 .. 120 bytes, the middle one across byte TILE, and every length from 40
    bytes in front of the first of them to 40 bytes behind the last."""
    lead = record(0, 1, b"n" * 70, [op(2600, "M")], 2600)                      # 4011 bytes
    recs = [lead, record(1, 2, b"one", [op(10, "M")], 10), record(0, 9, b"two", [op(40, "M")], 40, b"NMC\x00"), MINIMAL,
            record(1, 50, b"behind", [op(30, "M")], 30), MINIMAL]
    c = assemble(recs, 2)
    assert c.offs[2] < TILE < c.offs[3]
    return c, range(int(c.offs[1]) - 40, int(c.offs[4]) + 40 + 1)


# ---- random mixes --------------------------------------------------------------------------------------------------------------------
def fuzz(seed: int, n_ref: int) -> Tuple[Case, int, int]:
    """-> (a stream of random records whose name, SEQ / QUAL and aux bytes are random -- walked from a random record boundary --,
    a cut length behind that boundary, a device address offset 0 .. 15)."""
    rng = np.random.default_rng(seed)
    hi_ref = min(n_ref, 1000)
    recs = []
    for _ in range(int(rng.integers(40, 120))):
        l_seq = int(rng.choice([0, 1, 9, 64, 700, 5000]))
        name = rng.integers(0, 256, int(rng.integers(0, 255)), dtype=np.uint8).tobytes()
        aux = rng.integers(0, 256, int(rng.choice([0, 3, 50, 400])), dtype=np.uint8).tobytes()
        fill = rng.integers(0, 256, max(1, (l_seq + 1) // 2 + l_seq), dtype=np.uint8).tobytes()
        recs.append(record(int(rng.integers(-1, hi_ref)), int(rng.integers(-1, 1 << 30)), name,
                           [int(w) for w in rng.integers(0, 1 << 32, int(rng.integers(0, 6)), dtype=np.uint64)], l_seq, aux, fill=fill,
                           next_refID=int(rng.integers(-1, hi_ref)), next_pos=int(rng.integers(-1, 1 << 30))))
    k = int(rng.integers(0, len(recs) // 2))
    c = assemble(recs, n_ref, first_index=k)
    cut = int(rng.integers(c.first, c.stream.shape[0] + 1))
    return c, cut, int(rng.integers(0, 16))


FUZZ = [(seed, n_ref) for seed in (1, 2, 3, 4, 5, 6) for n_ref in (3, BIG_REF)]
