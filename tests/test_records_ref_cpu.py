"""The model of the record walk (tests/records_ref.py) against the serial block_size walkers -- formats.bam.record_offsets,
hostio.bam_record_offsets, hostio.bam_chunk_offsets -- on the streams of tests/records_cases.py, its candidate test against a loop
over the positions, and the conditions the cases were built to meet.  No GPU: tests/test_gpu_record_walk.py holds the kernel
against this model."""
import struct

import numpy as np
import pytest

import records_cases as C
import records_ref as R
from gci_amd import hostio
from gci_amd.formats import bam as bamfmt

CASES = C.cases()


@pytest.mark.parametrize("name", C.valid_names())
def test_valid_streams_walk_like_the_serial_walkers(name):
    c = CASES[name]
    offs, used, ok = R.walk(c.stream, c.first, c.n_ref)
    assert ok is True and used == c.stream.shape[0]
    assert np.array_equal(np.asarray(offs, dtype=np.int64), c.offs)
    assert np.array_equal(bamfmt.record_offsets(c.stream, c.first).astype(np.int64), c.offs)
    hdr = bamfmt.encode_header([], [])                           # (the host walker finds the first record itself: behind a header)
    whole = np.concatenate([np.frombuffer(hdr, dtype=np.uint8), c.stream[c.first:]])
    got, first = hostio.bam_record_offsets(whole)
    assert first == len(hdr) and np.array_equal(got.astype(np.int64) - len(hdr) + c.first, c.offs)
    got, consumed = hostio.bam_chunk_offsets(c.stream, c.first)
    assert consumed == used and np.array_equal(got.astype(np.int64), c.offs)


def test_every_cut_through_three_records_walks_like_the_chunk_walker():
    c, cuts = C.cut_span()
    assert len(cuts) > 200
    seen = set()
    for cut in cuts:
        offs, used, ok = R.walk(c.stream[:cut], c.first, c.n_ref)
        want, consumed = hostio.bam_chunk_offsets(c.stream[:cut].copy(), c.first)
        assert ok is True, cut
        assert (offs, used) == (want.astype(np.int64).tolist(), consumed), cut
        seen.add("end" if used == cut else "head" if cut - used < R.HEAD else "tail")
    assert seen == {"end", "head", "tail"}                       # a cut on a boundary, inside a record's head and behind one


@pytest.mark.parametrize("name", C.reject_names())
def test_a_rejected_record_breaks_the_chain_behind_the_record_before_it(name):
    c = CASES[name]
    j = c.reject
    offs, used, ok = R.walk(c.stream, c.first, c.n_ref)
    assert ok is False
    assert offs == c.offs[:j].tolist() and used == (int(c.offs[j - 1]) if j else c.first)
    # the one record, and nothing else, fails the test
    cand = set(R.candidates(c.stream, c.first, c.n_ref).tolist())
    assert [int(o) in cand for o in c.offs] == [k != j for k in range(len(c.offs))]


def by_position(stream: np.ndarray, lo: int, n_ref: int):
    buf, out = stream.tobytes(), []
    for p in range(lo, len(buf) - 35):
        block_size, ref_id, pos, l_read_name, _, _, n_cigar, _, l_seq, next_ref, next_pos = struct.unpack_from("<iiiBBHHHiii", buf, p)
        if block_size < 32 or not -1 <= ref_id < n_ref or pos < -1 or l_read_name < 1 or l_seq < 0:
            continue
        if not -1 <= next_ref < n_ref or next_pos < -1:
            continue
        if 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq <= block_size:
            out.append(p)
    return out


@pytest.mark.parametrize("n_ref", [3, C.BIG_REF])
def test_candidates_against_a_loop_over_the_positions(n_ref):
    rng = np.random.default_rng(17)
    s = rng.integers(0, 256, 6000, dtype=np.uint8)
    s[1000:1036] = np.frombuffer(C.fake_head(40, 2), dtype=np.uint8)
    s[2001:2038] = np.frombuffer(C.MINIMAL, dtype=np.uint8)
    s[3003:3403] = np.frombuffer(C.PATTERN * 50, dtype=np.uint8)
    s[4000:4400] = np.frombuffer(C.DENSE * 50, dtype=np.uint8)
    s[-36:] = np.frombuffer(C.fake_head(33, 0), dtype=np.uint8)          # the last position there is
    want = by_position(s, 0, n_ref)
    assert R.candidates(s, 0, n_ref).tolist() == want
    assert {1000, 2001, len(s) - 36} <= set(want) and len(want) > (100 if n_ref > 3 else 2)
    for lo in (1, 1000, 1001, 5964, 5965, 6000):
        assert R.candidates(s, lo, n_ref).tolist() == [p for p in want if p >= lo]
    for n in (0, 35, 36, 37):
        assert R.candidates(s[-n:] if n else s[:0], 0, n_ref).tolist() == by_position(s[-n:] if n else s[:0], 0, n_ref)


def test_the_cases_are_what_they_were_built_to_be():
    # the 8-byte pattern: every 8th byte of 4 800 passes, none with n_ref at the pattern's value
    c = CASES["pattern in QUAL"]
    inside = R.candidates(c.stream, 0, c.n_ref)
    qual = int(c.offs[1]) + 36 + 8 + 4 + 2400
    inside = inside[(inside >= qual) & (inside < qual + 4800)]
    alone = np.frombuffer(C.PATTERN * 600, dtype=np.uint8)
    assert R.candidates(alone, 0, c.n_ref).tolist() == list(range(0, 4800 - 35, 8)) and len(range(0, 4800 - 35, 8)) == 596
    assert R.candidates(alone, 0, C.PATTERN_REF).shape[0] == 0
    assert inside.shape[0] >= 596 and np.all((inside - qual) % 8 == 0)         # (the last two read into the record behind)
    c = CASES["pattern in QUAL, n_ref at the pattern's value"]
    got = R.candidates(c.stream, 0, c.n_ref)
    assert not np.any((got >= qual) & (got + 32 <= qual + 4800)) and set(c.offs.tolist()) <= set(got.tolist())
    # more than 512 candidates inside one tile, more than 4096 in all
    per_tile = max(np.bincount(R.candidates(c.stream, 0, c.n_ref) // C.TILE).max() for c in
                   (CASES["dense pattern"], CASES["pattern, then 5000 minimal records"]))
    assert per_tile > 512
    c = CASES["pattern, then 5000 minimal records"]
    assert R.candidates(c.stream, 0, c.n_ref).shape[0] > 4096
    # more records than Engine.bam_record_offsets gives room for at first
    assert c.offs.shape[0] > max(1024, c.stream.shape[0] // 256)
    assert sum(1 for n in C.COUNTS if n > max(1024, 37 * n // 256)) >= 10
    # chains of minimal records: as many candidates as records
    for n_rec in C.COUNTS:
        c = CASES["%d minimal records" % n_rec]
        assert R.candidates(c.stream, 0, c.n_ref).tolist() == c.offs.tolist() and c.offs.shape[0] == n_rec
    # the fakes pass the test, where they were put
    for name, more in (("fake heads", 9), ("fake head that ends at the end of the stream", 1), ("fake head that ends at a true record", 1)):
        c = CASES[name]
        assert R.candidates(c.stream, 0, c.n_ref).shape[0] >= c.offs.shape[0] + more, name
    c = CASES["fake head that ends at the end of the stream"]
    fake = [p for p in R.candidates(c.stream, 0, c.n_ref).tolist() if p not in set(c.offs.tolist())]
    assert [p + 4 + R.block_size_at(c.stream, p) for p in fake] == [c.stream.shape[0]]
    c = CASES["fake head that ends at a true record"]
    fake = [p for p in R.candidates(c.stream, 0, c.n_ref).tolist() if p not in set(c.offs.tolist())]
    assert [p + 4 + R.block_size_at(c.stream, p) for p in fake] == [int(c.offs[3])]
    for name in ("records in front", "only the last record", "candidate 8 bytes in front"):
        c = CASES[name]
        assert R.candidates(c.stream, 0, c.n_ref)[0] < c.first, name
    c = CASES["candidate 8 bytes in front"]
    assert c.first - 8 in R.candidates(c.stream, 0, c.n_ref).tolist()
    # the placement sweep: every position of a thread's window and both sides of the tile's last thread
    at = [int(CASES["second record at byte %d" % p].offs[1]) for p in C.PLACEMENTS]
    assert at == list(range(C.TILE - 40, C.TILE + 17)) and {p % 16 for p in at} == set(range(16))
    # the limits that must pass
    c = CASES["limits n_cigar 65535"]
    assert struct.unpack_from("<H", c.stream, int(c.offs[1]) + 16)[0] == 65535
    assert CASES["limits n_ref 0"].n_ref == 0 and CASES["limits n_ref 1"].n_ref == 1
    assert len(C.reject_names()) == 3 * len(C.REJECTS) == 30
    assert max(c.stream.shape[0] for c in CASES.values()) < 320_000


@pytest.mark.parametrize("seed,n_ref", C.FUZZ)
def test_random_mixes_walk_like_the_chunk_walker(seed, n_ref):
    c, cut, _ = C.fuzz(seed, n_ref)
    s = c.stream[:cut].copy()
    offs, used, ok = R.walk(s, c.first, n_ref)
    want, consumed = hostio.bam_chunk_offsets(s, c.first)
    assert ok is True and (offs, used) == (want.astype(np.int64).tolist(), consumed)
    assert R.candidates(c.stream, 0, n_ref).shape[0] >= c.offs.shape[0] + (50 if n_ref > 3 else 0)
