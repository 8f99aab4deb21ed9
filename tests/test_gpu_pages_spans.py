"""Record pages whose writer stages a page's source span in LDS (k_pages.hip, k_pg_write): byte for byte against the plain-Python
statement of the format (tests/pages_ref.py) on the inputs where a staged copy can go wrong -- pages whose records lie in one
window, pages where the window covers only the front of the records and the rest is gathered, offset tables that are not
ascending or skip records, junk between records, a stream cut inside its last core, a stream at an unaligned device address.

Which pages are which is computed here on the host (`_spans`), so that the test cannot pass on the gather alone: the plain HiFi
heads stream must have EVERY page's span within page_bytes, the spliced one at least three pages of each sort."""
import functools

import numpy as np
import pytest

from gci_amd import synth
from gci_amd.formats import bam
import pages_ref
from bam_util import heads_expected

pytestmark = pytest.mark.gpu

PAGE_DEFAULT = 24576
ALL_PAGE_BYTES = tuple(range(8192, 32768 + 1, 4096))


# ---- inputs (host only) -------------------------------------------------------------------------------------------------------

def _heads(stream, offs):
    h_bytes, h_offs = heads_expected(stream, offs, bam.parse_header(stream).first_record)
    return np.frombuffer(h_bytes, dtype=np.uint8).copy(), np.asarray(h_offs, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def odd_heads():
    """The records of test_gpu_pages.test_pages_of_odd_records (same seed, same draws) in heads form -> (stream, offsets,
    damaged stream cut 20 bytes into its last core).  Built once per session; nobody writes to what it returns."""
    rng = np.random.default_rng(3)
    recs = []
    for i in range(600):
        n_ops = int(rng.choice([0, 1, 3, 70, 150, 200, 230, 260, 700]))
        ops = [(int(rng.choice([0, 7, 8, 1, 2, 4])), int(rng.integers(1, 300))) for _ in range(n_ops)]
        qlen = sum(l for o, l in ops if (bam.QUERY_CONSUMING >> o) & 1)
        name = bytes(rng.integers(33, 127, int(rng.choice([1, 11, 12, 27, 28, 43, 44, 100, 254]))).astype(np.uint8)).decode()
        tags = [("NM", "C", 3)]
        if rng.random() < 0.3:
            tags.append(("XZ", "Z", "t" * int(rng.choice([1, 100, 600, 900, 990, 1100, 3000]))))
        if rng.random() < 0.1:
            tags.append(("XB", "B:I", list(range(int(rng.integers(0, 400))))))
        recs.append(bam.encode_record(int(rng.integers(0, 2)), int(rng.integers(0, 10_000)), name, 60, 0, ops, qlen, bam.encode_aux(tags)))
    hdr = bam.encode_header(["x", "y"], [100_000, 100_000])
    stream = np.frombuffer(hdr + b"".join(recs), dtype=np.uint8).copy()
    offs = bam.record_offsets(stream, bam.parse_header(stream).first_record)
    h, h_offs = _heads(stream, offs)
    # damage, in the heads form: a block_size beyond the stream, one below 32, a negative l_seq, an l_seq beyond everything
    s2 = h.copy()
    for k, (field, val) in enumerate(((0, 1 << 30), (0, 8), (20, -5), (20, 1 << 20))):
        o = int(h_offs[10 + 50 * k])
        s2[o + field:o + field + 4] = np.array([val], dtype="<i4").view(np.uint8)
    cut = int(h_offs[-1]) + 20                                             # the last record: fewer than 36 bytes of it
    return h, h_offs, s2[:cut].copy()


@functools.lru_cache(maxsize=None)
def hifi_heads(splice_every=0, repeat=1):
    """The suite's HiFi reads as a heads stream; with splice_every, a record that does not fit a page inline behind every
    splice_every-th record, in turn: a CIGAR of 300 operations (kind 1, 1.2 KB of source), one of 9000 (kind 1, 36 KB: longer
    than any page), a 3000-byte Z tag (kind 2).  The reads are 227 records, four pages of the default size: `repeat` writes them
    out that many times, one after the other, so that there are enough pages for three of each sort."""
    rs = synth.simulate_reads((("a", 300_000), ("b", 60_000)), 12, "hifi", seed=5)
    stream, offs = synth.to_bam_stream(rs)
    if splice_every:
        first = bam.parse_header(stream).first_record
        ends = list(offs[1:]) + [stream.shape[0]]
        rng = np.random.default_rng(11)
        parts, n_spliced = [stream[:first].tobytes()], 0
        for i, (o, e) in enumerate(list(zip(offs, ends)) * repeat):
            parts.append(stream[int(o):int(e)].tobytes())
            if (i + 1) % splice_every == 0:
                which = n_spliced % 3
                n_ops = (300, 9000, 70)[which]
                ops = [(int(rng.choice([7, 8, 1, 2])), int(rng.integers(1, 40))) for _ in range(n_ops)]
                qlen = sum(l for op, l in ops if (bam.QUERY_CONSUMING >> op) & 1)
                tags = [("NM", "C", 3)] + ([("XZ", "Z", "t" * 3000)] if which == 2 else [])
                parts.append(bam.encode_record(0, 1000 + i, "spliced_%d" % i, 60, 0, ops, qlen, bam.encode_aux(tags)))
                n_spliced += 1
        stream = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        offs = bam.record_offsets(stream, first)
    return _heads(stream, offs)


def with_junk(stream, offs, seed):
    """The same records with 1 .. 40 junk bytes in front of each -> (stream, offsets)."""
    rng = np.random.default_rng(seed)
    ends = [int(x) for x in offs[1:]] + [int(stream.shape[0])]
    parts, new_offs, w = [stream[:int(offs[0])].tobytes()], [], int(offs[0])
    for o, e in zip(offs.tolist(), ends):
        junk = rng.integers(0, 256, int(rng.integers(1, 41))).astype(np.uint8).tobytes()
        parts += [junk, stream[int(o):e].tobytes()]
        w += len(junk)
        new_offs.append(w)
        w += e - int(o)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.asarray(new_offs, dtype=np.uint64)


def tables(offs, seed):
    """Offset tables over the same stream that are not the ascending list of all records."""
    rng = np.random.default_rng(seed)
    offs = np.asarray(offs, dtype=np.uint64)
    keep = rng.random(offs.shape[0]) < 0.6
    keep[0] = True
    return {"reversed": offs[::-1].copy(), "permuted": offs[rng.permutation(offs.shape[0])], "skipping": offs[keep],
            "every_third": offs[::3].copy()}


def _spans(stream, offs, page_bytes):
    """-> one bool per page: its whole span -- from its first record's offset rounded down to 16, to the end of its last record
    -- is no longer than page_bytes (a window of the page's size holds everything the page takes)."""
    n_bytes = int(stream.shape[0])
    Q = page_bytes - pages_ref.MAX_REC - 48
    pages, s = {}, 0
    for o in offs.tolist():
        r = pages_ref._measure(stream, int(o), n_bytes, False)
        if r["kind"] == pages_ref.F_MALFORMED:
            end = min(int(o) + 36, n_bytes)
        else:
            end = int(o) + 36 + r["lrn"] + 4 * r["n_cig"] + r["aux_len"]
        lo, hi = pages.get(s // Q, (int(o) & ~15, 0))
        pages[s // Q] = (min(lo, int(o) & ~15), max(hi, end))
        s += r["size"] + 2
    return [hi - lo <= page_bytes for k, (lo, hi) in sorted(pages.items())]


# ---- the device against the statement -----------------------------------------------------------------------------------------

def _check(engine, stream, offs, page_bytes, shift=0):
    want, n_pages, blob_off = pages_ref.build_pages(stream, offs, False, page_bytes)
    if shift:                                                              # the stream at a device address that is base + shift
        d_stream = engine.to_device(np.concatenate([np.full(shift, 0xA5, dtype=np.uint8), stream]))[shift:]
        assert d_stream.data_ptr() % 16 == shift % 16
    else:
        d_stream = engine.to_device(stream)
    pg = engine.bam_pages(d_stream, engine.to_device(np.asarray(offs, dtype=np.uint64)), False, page_bytes)
    assert (pg.n_pages, pg.blob_off, pg.n_rec) == (n_pages, blob_off, len(offs))
    got = pg.buf.cpu().numpy()
    assert got.shape[0] == want.shape[0]
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError("pages differ at byte %d (page %d + %d; blob at %d)" % (bad, bad // page_bytes, bad % page_bytes, blob_off))


@pytest.mark.parametrize("page_bytes", ALL_PAGE_BYTES)
def test_odd_heads_records_at_every_page_size(engine, page_bytes):
    """Every record kind in heads form, whole and cut inside the last core: the input where a window holds only the front of a
    page's records."""
    h, h_offs, cut = odd_heads()
    kinds = [pages_ref._measure(h, int(o), int(h.shape[0]), False)["kind"] for o in h_offs]
    assert (kinds.count(0), kinds.count(pages_ref.F_EXT), kinds.count(pages_ref.F_OVERSIZE)) == (330, 156, 114)
    assert h.shape[0] == 732_759
    if page_bytes in (8192, 24576):
        assert not any(_spans(h, h_offs, page_bytes))
    _check(engine, h, h_offs, page_bytes)
    _check(engine, cut, h_offs, page_bytes)


@pytest.mark.parametrize("page_bytes", [8192, 24576, 32768])
def test_hifi_heads_pages_are_staged_whole(engine, page_bytes):
    h, h_offs = hifi_heads()
    whole = _spans(h, h_offs, page_bytes)
    assert len(whole) >= 2 and all(whole)
    _check(engine, h, h_offs, page_bytes)


SPLICE_EVERY, SPLICE_REPEAT = 60, 3        # chosen on the host: 13 pages of the default size, 6 whole and 7 mixed (asserted below)


def test_hifi_heads_with_spliced_records(engine):
    """Some pages staged whole, some mixed (a spliced record's bytes reach out of the window)."""
    h, h_offs = hifi_heads(SPLICE_EVERY, SPLICE_REPEAT)
    whole = _spans(h, h_offs, PAGE_DEFAULT)
    assert whole.count(True) >= 3 and whole.count(False) >= 3, whole
    for pb in (8192, PAGE_DEFAULT, 32768):
        _check(engine, h, h_offs, pb)


@pytest.mark.parametrize("which", ["odd", "odd_cut", "hifi_spliced"])
def test_offset_tables_that_are_not_ascending(engine, which):
    if which == "hifi_spliced":
        h, h_offs = hifi_heads(SPLICE_EVERY, SPLICE_REPEAT)
    else:
        h, h_offs, cut = odd_heads()
        if which == "odd_cut":
            h = cut
    for name, tab in tables(h_offs, seed=17).items():
        for pb in (8192, PAGE_DEFAULT):
            try:
                _check(engine, h, tab, pb)
            except AssertionError as e:
                raise AssertionError("%s table, page_bytes %d: %s" % (name, pb, e))


@pytest.mark.parametrize("which", ["odd", "hifi_spliced"])
def test_junk_between_records(engine, which):
    h, h_offs = hifi_heads(SPLICE_EVERY, SPLICE_REPEAT) if which == "hifi_spliced" else odd_heads()[:2]
    j, j_offs = with_junk(h, h_offs, seed=23)
    for pb in (8192, PAGE_DEFAULT):
        _check(engine, j, j_offs, pb)
    _check(engine, j, tables(j_offs, seed=29)["permuted"], PAGE_DEFAULT)


@pytest.mark.parametrize("shift", [1, 5, 15])
def test_stream_at_an_unaligned_device_address(engine, shift):
    h, h_offs = hifi_heads(SPLICE_EVERY, SPLICE_REPEAT)
    _check(engine, h, h_offs, PAGE_DEFAULT, shift)
    o, o_offs, cut = odd_heads()
    _check(engine, cut, o_offs, PAGE_DEFAULT, shift)
    _check(engine, o, o_offs, 8192, shift)
