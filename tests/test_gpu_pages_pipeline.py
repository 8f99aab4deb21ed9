"""Record pages through the two writers (k_pages.hip): k_pg_lean, which writes the pages it finds LEAN and lists the others,
and k_pg_write over that list -- byte for byte against the plain-Python statement of the format (tests/pages_ref.py).

Which pages are lean is computed here on the host (`lean_pages`, the rule of pgl_win_of() and of k_pg_lean's phase A) and
asserted before anything runs, so that no case passes on one kernel alone.  GCI_PAGES_GRID caps the persistent grids: without it
a test's few pages are one per workgroup and the steady state of the loops -- a page composed while the next one's loads are in
flight -- would run at genome size only.  The switch is read when a context is made, so every cap has a context of its own."""
import ctypes
import functools
import os

import numpy as np
import pytest

from gci_amd import synth
import pages_ref
from test_gpu_pages_spans import PAGE_DEFAULT, ALL_PAGE_BYTES, hifi_heads, odd_heads, tables, with_junk

pytestmark = pytest.mark.gpu

META_MAX = 128                                                             # PG_META_MAX


# ---- inputs (host only) -------------------------------------------------------------------------------------------------------

def compose(h, h_offs, order):
    """The records `order` (indices, any number of times) of a stream, behind its header -> (stream, offsets)."""
    ends = [int(x) for x in h_offs[1:]] + [int(h.shape[0])]
    parts, offs, w = [h[:int(h_offs[0])].tobytes()], [], int(h_offs[0])
    for i in order:
        offs.append(w)
        parts.append(h[int(h_offs[i]):ends[i]].tobytes())
        w += ends[i] - int(h_offs[i])
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.asarray(offs, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def steady():
    """The suite's HiFi heads, eight times over: 32 pages of the default size, 24 of the largest."""
    h, h_offs = hifi_heads()
    return compose(h, h_offs, list(range(len(h_offs))) * 8)


@functools.lru_cache(maxsize=None)
def mixed():
    """HiFi heads with records that do not fit a page inline (hifi_heads' spliced ones) put where the cases below need them:
    in the first page, in two neighbouring pages in the middle, in the last page."""
    h, h_offs = hifi_heads(60, 3)
    kinds = [pages_ref._measure(h, int(o), int(h.shape[0]), False)["kind"] for o in h_offs]
    dirty = [i for i, k in enumerate(kinds) if k != 0]
    clean = [i for i, k in enumerate(kinds) if k == 0][:220]
    assert len(dirty) >= 6
    order = (dirty[0:1] + clean + clean[:100] + dirty[1:2] + clean[100:119] + dirty[2:3] + clean[119:160] + dirty[3:4] + clean[160:]
             + clean + clean + clean[:30] + dirty[4:5])
    return compose(h, h_offs, order)


def lean_pages(stream, offs, page_bytes, has_seq=False, shift=0):
    """-> one bool per page: k_pg_lean writes it.  The page's span -- from its first record's ADDRESS (offset + shift) rounded
    down to 16, to the first record of the next page (the stream's end for the last) rounded up -- is whole 16-byte pieces inside
    the stream, no longer than the page; 1 .. 128 records at ascending offsets, each of kind 0 and inside the span."""
    n_bytes = int(stream.shape[0])
    Q = page_bytes - pages_ref.MAX_REC - 48
    recs = [pages_ref._measure(stream, int(o), n_bytes, has_seq) for o in offs]
    by_page, s = {}, 0
    for i, r in enumerate(recs):
        by_page.setdefault(s // Q, []).append(i)
        s += r["size"] + 2
    n_pages = (s - recs[-1]["size"] - 2) // Q + 1
    first = [by_page[k][0] if k in by_page else None for k in range(n_pages)]
    out = []
    for k in range(n_pages):
        idx = by_page.get(k, [])
        if has_seq or not (1 <= len(idx) <= META_MAX):
            out.append(False)
            continue
        nxt = next((first[j] for j in range(k + 1, n_pages) if first[j] is not None), None)
        off0 = int(offs[idx[0]])
        span_end = min(int(offs[nxt]) if nxt is not None else n_bytes, n_bytes)
        lo, hi = (off0 + shift) & ~15, (span_end + shift + 15) & ~15
        ok = off0 < span_end and lo >= shift and hi <= shift + n_bytes and hi - lo <= page_bytes
        prev = -1
        for i in idx:
            o, r = int(offs[i]), recs[i]
            ok = ok and r["kind"] == 0 and o > prev and o + shift >= lo and \
                o + shift + 36 + r.get("lrn", 0) + 4 * r.get("n_cig", 0) + r.get("aux_len", 0) <= hi
            prev = o
        out.append(bool(ok))
    return out


@functools.lru_cache(maxsize=None)
def _want(which, page_bytes):
    """The statement's pages of a named input: computed once, shared, never written to."""
    stream, offs = {"steady": steady, "mixed": mixed, "hifi": hifi_heads}[which]()
    return pages_ref.build_pages(stream, offs, False, page_bytes)


# ---- the device against the statement -----------------------------------------------------------------------------------------

_capped = {}


def capped(cap):
    """A context whose page writers run at most `cap` workgroups (0: as many as the device holds)."""
    if cap not in _capped:
        import torch
        if not torch.cuda.is_available():
            pytest.fail("gpu-marked test selected but no GPU is visible: the HIP path has no CPU fallback")
        from gci_amd.device import Engine
        old = os.environ.get("GCI_PAGES_GRID")
        os.environ["GCI_PAGES_GRID"] = str(cap)
        try:
            _capped[cap] = Engine(0)
        finally:
            if old is None:
                del os.environ["GCI_PAGES_GRID"]
            else:
                os.environ["GCI_PAGES_GRID"] = old
    return _capped[cap]


def _same(got, want, page_bytes, what=""):
    assert got.shape[0] == want.shape[0]
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%spages differ at byte %d (page %d + %d)" % (what, bad, bad // page_bytes, bad % page_bytes))


def _run(eng, stream, offs, page_bytes, want, has_seq=False, shift=0):
    buf, n_pages, blob_off = want
    if shift:                                                              # the stream at a device address that is base + shift
        d_stream = eng.to_device(np.concatenate([np.full(shift, 0xA5, dtype=np.uint8), stream]))[shift:]
        assert d_stream.data_ptr() % 16 == shift % 16
    else:
        d_stream = eng.to_device(stream)
    pg = eng.bam_pages(d_stream, eng.to_device(np.asarray(offs, dtype=np.uint64)), has_seq, page_bytes)
    assert (pg.n_pages, pg.blob_off, pg.n_rec) == (n_pages, blob_off, len(offs))
    _same(pg.buf.cpu().numpy(), buf, page_bytes)


@pytest.mark.parametrize("cap", [1, 2, 3, 5])
@pytest.mark.parametrize("page_bytes", ALL_PAGE_BYTES)
def test_lean_steady_state(cap, page_bytes):
    """Every workgroup of the lean writer composes at least four pages, one after the other; over the four caps a workgroup's
    share is odd and even, and its last page has none behind it.  Every page but the last is lean (the stream ends inside a
    16-byte piece, which no window load touches: that page goes through the list)."""
    stream, offs = steady()
    lean = lean_pages(stream, offs, page_bytes)
    n = len(lean)
    assert n >= 4 * cap and all(lean[:-1]), (n, lean)
    shares = {(n - w + c - 1) // c % 2 for c in (1, 2, 3, 5) for w in range(c)}
    assert shares == {0, 1}
    _run(capped(cap), stream, offs, page_bytes, _want("steady", page_bytes))


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("page_bytes", [8192, PAGE_DEFAULT])
def test_lean_and_listed_pages_mixed(cap, page_bytes):
    stream, offs = mixed()
    lean = lean_pages(stream, offs, page_bytes)
    assert lean.count(True) >= 3 and lean.count(False) >= 3, lean
    assert not lean[0] and not lean[-1], lean
    assert any(not a and not b for a, b in zip(lean[1:-1], lean[2:-1])), lean          # two listed neighbours in the middle
    _run(capped(cap), stream, offs, page_bytes, _want("mixed", page_bytes))


ALL_LISTED = ["odd", "odd_cut", "reversed", "permuted", "junk", "whole"]


@pytest.mark.parametrize("which", ALL_LISTED)
def test_all_pages_listed(which):
    """Inputs none of whose pages is lean: everything goes through the list (or, with SEQ / QUAL in the stream, through
    k_pg_write alone), with one workgroup and with as many as the device holds."""
    has_seq = which == "whole"
    if which == "whole":
        stream, offs = synth.to_bam_stream(synth.simulate_reads((("a", 300_000), ("b", 60_000)), 12, "hifi", seed=5))
        offs = np.asarray(offs, dtype=np.uint64)
    else:
        h, h_offs, cut = odd_heads()
        stream, offs = (cut if which == "odd_cut" else h), h_offs
        if which in ("reversed", "permuted"):
            offs = tables(h_offs, seed=17)[which]
        if which == "junk":
            stream, offs = with_junk(h, h_offs, seed=23)
    for pb in (8192, PAGE_DEFAULT):
        assert not any(lean_pages(stream, offs, pb, has_seq)), which
        want = pages_ref.build_pages(stream, offs, has_seq, pb)
        for cap in (1, 0):
            _run(capped(cap), stream, offs, pb, want, has_seq)


@pytest.mark.parametrize("shift", [1, 4, 15, 17])
def test_lean_pages_of_a_stream_at_an_unaligned_device_address(shift):
    stream, offs = hifi_heads()
    lean = lean_pages(stream, offs, PAGE_DEFAULT, shift=shift)
    assert sum(lean) >= 3, lean
    for cap in (1, 0):
        _run(capped(cap), stream, offs, PAGE_DEFAULT, _want("hifi", PAGE_DEFAULT), shift=shift)


def test_two_calls_on_one_context():
    """The list's counter is cleaned by the kernels: a call with listed pages, then one without on the same context; and
    gci_bam_pages_write twice after one gci_bam_pages_size gives the same bytes."""
    eng = capped(2)
    m_stream, m_offs = mixed()
    s_stream, s_offs = steady()
    assert not all(lean_pages(m_stream, m_offs, PAGE_DEFAULT)) and all(lean_pages(s_stream, s_offs, PAGE_DEFAULT)[:-1])
    for _ in range(2):
        _run(eng, m_stream, m_offs, PAGE_DEFAULT, _want("mixed", PAGE_DEFAULT))
        _run(eng, s_stream, s_offs, PAGE_DEFAULT, _want("steady", PAGE_DEFAULT))
    want = _want("mixed", PAGE_DEFAULT)[0]
    d_stream, d_offs = eng.to_device(m_stream), eng.to_device(m_offs)
    h = (ctypes.c_uint64 * 3)()
    args = (eng.ctx, eng._p(d_stream), int(m_stream.shape[0]), eng._p(d_offs), len(m_offs), 0)
    eng._chk(eng.lib.gci_bam_pages_size(*args, PAGE_DEFAULT, h), "gci_bam_pages_size")
    assert int(h[1]) == want.shape[0]
    for call in range(3):
        buf = eng.T.empty(int(h[1]), eng.T.uint8, eng.device)
        buf.fill_(0xEE)
        eng._chk(eng.lib.gci_bam_pages_write(*args, eng._p(buf), int(h[1])), "gci_bam_pages_write")
        _same(buf.cpu().numpy(), want, PAGE_DEFAULT, "write call %d: " % call)
