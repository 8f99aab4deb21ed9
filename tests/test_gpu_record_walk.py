"""gci_bam_record_offsets_device (k_records.hip) through Engine.bam_record_offsets against the model of tests/records_ref.py, on
the streams of tests/records_cases.py: limit-valued fields, one-field rejects, positions that pass the test and are no record,
a record at every byte around a tile border at every address alignment, every cut through three records, tails shorter than a
record head, chains of 1 .. 8193 records (the doubling rounds, the scan blocks, the second call with more room), random mixes,
and a small stream behind a large one on the same context.  Every comparison is exact: the offsets, the bytes consumed, ok."""
import functools

import numpy as np
import pytest

import records_cases as C
import records_ref as R
from gci_amd import hostio

pytestmark = pytest.mark.gpu

CASES = C.cases()


@functools.lru_cache(maxsize=None)
def want(name):
    c = CASES[name]
    return R.walk(c.stream, c.first, c.n_ref)


def device_walk(engine, stream, first, n_ref, skip=0):
    """The walk over `stream` uploaded `skip` bytes behind a 16-byte address (a slice of a larger buffer) -> (offsets, used, ok)."""
    buf = np.zeros(skip + stream.shape[0] + 16, dtype=np.uint8)
    buf[skip:skip + stream.shape[0]] = stream
    d = engine.to_device(buf)
    assert d.data_ptr() % 16 == 0
    offs, used, ok = engine.bam_record_offsets(d[skip:skip + stream.shape[0]], first, n_ref)
    return offs.cpu().numpy().astype(np.int64).tolist(), used, ok


@pytest.mark.parametrize("name", C.valid_names())
def test_valid_streams(engine, name):
    c = CASES[name]
    offs, used, ok = device_walk(engine, c.stream, c.first, c.n_ref)
    assert ok is True
    assert (offs, used, ok) == want(name)
    assert offs == c.offs.tolist() and used == c.stream.shape[0]


@pytest.mark.parametrize("name", C.reject_names())
def test_rejects(engine, name):
    c = CASES[name]
    got = device_walk(engine, c.stream, c.first, c.n_ref)
    assert got == want(name) and got[2] is False
    assert len(got[0]) == c.reject


@pytest.mark.parametrize("skip", range(16))
def test_every_address_alignment_at_every_placement(engine, skip):
    for at in C.PLACEMENTS:
        name = "second record at byte %d" % at
        c = CASES[name]
        got = device_walk(engine, c.stream, c.first, c.n_ref, skip)
        assert got[2] is True and got == want(name), (skip, at)
    # ... and where a position in front of the first record passes the test, records lie in front, many candidates share a tile
    for name in ("candidate 8 bytes in front", "records in front", "only the last record", "dense pattern", "fake heads", "assorted",
                 "reject refID -2, middle record", "reject need block_size + 1, last record"):
        c = CASES[name]
        got = device_walk(engine, c.stream, c.first, c.n_ref, skip)
        assert got[2] is (c.reject is None) and got == want(name), (skip, name)


def test_every_cut_through_three_records(engine):
    c, cuts = C.cut_span()
    ends = set()
    for k, cut in enumerate(cuts):
        s = c.stream[:cut]
        got = device_walk(engine, s, c.first, c.n_ref, k % 16)
        assert got[2] is True and got == R.walk(s, c.first, c.n_ref), cut
        offs, consumed = hostio.bam_chunk_offsets(s.copy(), c.first)
        assert got[:2] == (offs.astype(np.int64).tolist(), consumed), cut
        ends.add("end" if got[1] == cut else "head" if cut - got[1] < R.HEAD else "tail")
    assert ends == {"end", "head", "tail"} and len(cuts) > 200


def test_tails(engine):
    c = CASES["assorted"]
    n = int(c.offs[3])                                                        # three records
    # 0 .. 35 bytes behind `first`: no record head to test, everything is tail -- behind records and at the start of the stream
    for left in range(36):
        for first, s in ((n, c.stream[:n + left]), (0, c.stream[:left])):
            got = device_walk(engine, s, first, c.n_ref, left % 16)
            assert got == ([], first, True) == R.walk(s, first, c.n_ref), (left, first)
    assert device_walk(engine, c.stream[:n], n, c.n_ref) == ([], n, True)        # first == n
    # one record longer than the chunk: no record, nothing consumed, ok
    big = CASES["limits n_cigar 65535"]
    for cut in (int(big.offs[1]) + 36, int(big.offs[1]) + 5000, int(big.offs[2]) - 1):
        s = big.stream[:cut]
        got = device_walk(engine, s, int(big.offs[1]), big.n_ref)
        assert got == ([], int(big.offs[1]), True) == R.walk(s, int(big.offs[1]), big.n_ref), cut
    # `first` is no candidate: one byte off a record, inside a name, on a rejected record
    for first in (1, int(c.offs[1]) - 1, int(c.offs[1]) + 1, int(c.offs[4]) + 40):
        got = device_walk(engine, c.stream, first, c.n_ref, first % 16)
        assert got == ([], first, False) == R.walk(c.stream, first, c.n_ref), first
    zeros = np.zeros(5000, dtype=np.uint8)                                    # no candidate at all
    assert device_walk(engine, zeros, 0, 3) == ([], 0, False) == R.walk(zeros, 0, 3)


@pytest.mark.parametrize("seed,n_ref", C.FUZZ)
def test_random_mixes(engine, seed, n_ref):
    c, cut, skip = C.fuzz(seed, n_ref)
    whole = device_walk(engine, c.stream, c.first, n_ref, skip)
    assert whole[2] is True and whole == R.walk(c.stream, c.first, n_ref) and whole[0] == c.offs.tolist()
    s = c.stream[:cut]
    got = device_walk(engine, s, c.first, n_ref, skip)
    assert got[2] is True and got == R.walk(s, c.first, n_ref)
    offs, consumed = hostio.bam_chunk_offsets(s.copy(), c.first)
    assert got[:2] == (offs.astype(np.int64).tolist(), consumed)


def test_a_small_stream_behind_a_large_one_on_the_same_context(engine):
    """The scratch of a call (tile counts, candidates, links, marks) is the context's and is used again: what a large stream with
    thousands of candidates left there must not show in the small one that follows."""
    large, dense = "pattern, then 5000 minimal records", "dense pattern"
    for small in ("limits", "1 minimal records", "reject pos -2, middle record", "fake head that ends at a true record", "3 minimal records"):
        for before in (large, dense):
            c = CASES[before]
            assert device_walk(engine, c.stream, c.first, c.n_ref) == want(before)
            c = CASES[small]
            assert device_walk(engine, c.stream, c.first, c.n_ref) == want(small), (before, small)
    c = CASES[large]
    assert device_walk(engine, c.stream, c.first, c.n_ref) == want(large)
    s = CASES["assorted"].stream[:20]                                         # ... and a call that tests no position at all
    assert device_walk(engine, s, 0, 3) == ([], 0, True)
