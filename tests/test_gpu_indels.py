"""indel_sites.py on the GPU: gci_bam_indel_size / _write and gci_indel_sites_size / _write (k_indels.hip) against the statement of
tests/indels_ref.py on every case of tests/indels_cases.py, in both stream forms, into pre-filled buffers with guard entries behind
them; the built tracks; pipeline.bam_indel_sites over a small synthetic file in one piece, in several and with forced flushes, against
pipeline.bam_raw_depth and file by file; and the command line once, its BED file handed on to filter_reads.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import indels_cases as C
import indels_ref as R
from cover_cases import D, I, M, rec
from gci_amd import _lib, pipeline, synth
from gci_amd.device import INDEL_SITE_DTYPE, IVL_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16                                             # entries behind the output that must stay
PATTERN = -0x5A5A5A5B
U64 = 2 ** 64 - 1
FIELDS = ("contig", "start", "end", "del", "ins", "depth")


def upload(engine, name, form):
    c = C.case(name)
    stream, offs = (c["stream"], c["offs"]) if form == "stream" else C.heads(name)
    up = lambda a: engine.to_device(a if a.shape[0] else np.zeros(1, dtype=a.dtype))      # noqa: E731
    return dict(stream=engine.to_device(stream), offs=up(offs), sel=engine.to_device(c["ref_sel"]), n_bytes=int(stream.shape[0]),
                n_rec=int(offs.shape[0]))


@pytest.fixture(scope="module")
def on_device(engine):
    cache = {}

    def get(name, form):
        if (name, form) not in cache:
            cache[(name, form)] = upload(engine, name, form)
        return cache[(name, form)]
    return get


def device_indel(engine, b, has_seq, run, cap=None):
    """-> (deletions, insertions, counts, status word, the write call's return, the whole buffer) of the exports as they are: the output
    pre-filled with a pattern, GUARD entries behind it."""
    p, lib = engine._p, engine.lib
    counts = (ctypes.c_uint64 * 3)()
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    st = lib.gci_bam_indel_size(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]) if b["n_rec"] else None, b["n_rec"], int(has_seq), p(b["sel"]),
                                int(b["sel"].shape[0]), run[0], run[1], run[2], counts, p(status))
    assert st == 0
    n_del, n_ins = int(counts[1]), int(counts[2])
    total = n_del + n_ins
    out = engine.to_device(np.full((total + GUARD, 4), PATTERN, dtype=np.int32))
    wr = lib.gci_bam_indel_write(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]) if b["n_rec"] else None, b["n_rec"], int(has_seq), p(out),
                                 total if cap is None else cap, p(status))
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 4)
    ivl = host.view(IVL_DTYPE).reshape(-1)
    return ivl[:n_del], ivl[n_del:total], [int(x) for x in counts], int(status.item()) & U64, wr, host


def dels_of(ivl):
    assert (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist(), ivl["end"].tolist()))


def inss_of(ivl):
    assert (ivl["start"] == ivl["end"]).all() and (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist()))


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name", C.NAMES)
def test_the_device_gives_the_events_of_the_statement(engine, on_device, name, form):
    """Both halves in (record, operation) order, status and counts as the statement's, the guard entries untouched; the tracks built from
    either half hold, per base, the events over it."""
    c, b = C.case(name), on_device(name, form)
    engine.set_layout(c["lengths"])
    for run in c["runs"]:
        want_dels, want_inss, want_counts, want_status = C.want(name, run)
        dels, inss, counts, status, wr, host = device_indel(engine, b, form == "stream", run)
        assert wr == 0 and status == want_status and counts == want_counts, run
        assert (host[counts[1] + counts[2]:] == PATTERN).all(), "entries behind the events were written"
        assert dels_of(dels) == want_dels and inss_of(inss) == want_inss, run
        for ivl, want in ((dels, want_dels), (inss, want_inss)):
            if not len(want):
                continue
            track = engine.depth_build(engine.to_device(np.ascontiguousarray(ivl).view(np.int32).reshape(-1, 4)), None, 0, engine.new_track())
            assert np.array_equal(track.cpu().numpy(), R.track_of(want, c["lengths"])), run


def test_two_runs_give_the_same_bytes(engine, on_device):
    c, b = C.case("records_4097"), on_device("records_4097", "stream")
    engine.set_layout(c["lengths"])
    first = device_indel(engine, b, True, c["runs"][1])[5]
    assert np.array_equal(first, device_indel(engine, b, True, c["runs"][1])[5])


def test_the_device_gives_the_hand_written_events(engine, on_device):
    for (name, run), (dels, inss, counted) in C.EXPECTED.items():
        engine.set_layout(C.case(name)["lengths"])
        got_dels, got_inss, counts, status, _, _ = device_indel(engine, on_device(name, "stream"), True, run)
        assert (dels_of(got_dels), inss_of(got_inss), counts[0], status) == (dels, inss, counted, U64), (name, run)


def test_engine_bam_indel_and_its_status(engine, on_device):
    c, b = C.case("random_2000"), on_device("random_2000", "heads")
    engine.set_layout(c["lengths"])
    run = c["runs"][0]
    dels, inss, counts = engine.bam_indel(b["stream"], b["offs"], False, b["sel"], *run)
    want = C.want("random_2000", run)
    assert counts == want[2]
    assert dels_of(dels.cpu().numpy().view(IVL_DTYPE).reshape(-1)) == want[0] and inss_of(inss.cpu().numpy().view(IVL_DTYPE).reshape(-1)) == want[1]
    for name, bad in C.MALFORMED.items():
        b = on_device(name, "stream")
        engine.set_layout(C.case(name)["lengths"])
        with pytest.raises(_lib.GciError) as e:
            engine.bam_indel(b["stream"], b["offs"], True, b["sel"], min_len=5)
        assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == bad, name


def test_argument_errors_of_the_record_calls(engine, on_device):
    c, b = C.case("thresholds"), on_device("thresholds", "stream")
    engine.set_layout(c["lengths"])
    p, lib = engine._p, engine.lib
    counts = (ctypes.c_uint64 * 3)()
    size = lambda e, min_len=5, h=counts: lib.gci_bam_indel_size(e.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"], 1, p(b["sel"]),      # noqa: E731
                                                                 int(b["sel"].shape[0]), 0x704, 0, min_len, h, p(engine._status))
    assert size(engine, min_len=0) == _lib.GCI_E_INVALID and size(engine, h=None) == _lib.GCI_E_INVALID
    _, _, counts_ok, _, wr, host = device_indel(engine, b, True, (C.EXCL, 0, 5), cap=5)          # six events: one entry too few
    assert counts_ok == [4, 4, 2] and wr == _lib.GCI_E_CAPACITY and (host == PATTERN).all()
    out = engine.T.empty((16, 4), engine.T.int32, engine.device)
    assert lib.gci_bam_indel_write(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"] - 1, 1, p(out), 16, p(engine._status)) == _lib.GCI_E_INVALID
    from gci_amd.device import Engine
    fresh = Engine(0)
    try:
        assert size(fresh) == _lib.GCI_E_NO_LAYOUT
        fresh.set_layout(c["lengths"])
        assert lib.gci_bam_indel_write(fresh.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"], 1, p(out), 16, p(engine._status)) == _lib.GCI_E_INVALID
    finally:
        fresh.close()


# ---- sites -----------------------------------------------------------------------------------------------------------------------------

def device_sites(engine, t, min_reads, windows, with_depth=True, cap=None):
    p, lib = engine._p, engine.lib
    arr, nw = engine._window_array(windows), len(windows)
    n = ctypes.c_uint64(0)
    head = (engine.ctx, p(t["dele"]), p(t["ins"]), p(t["depth"]) if with_depth else None, min_reads, arr, nw)
    assert lib.gci_indel_sites_size(*head, ctypes.byref(n)) == 0
    total = int(n.value)
    out = engine.to_device(np.full((total + GUARD, 6), PATTERN, dtype=np.int32))
    wr = lib.gci_indel_sites_write(*head, p(out), total if cap is None else cap)
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 6)
    return host[:total].view(INDEL_SITE_DTYPE).reshape(-1), wr, host


def site_rows(sites):
    return list(zip(*(sites[f].tolist() for f in FIELDS)))


@pytest.mark.parametrize("name", C.SITE_NAMES)
def test_the_device_gives_the_sites_of_the_statement(engine, name):
    c = C.site_case(name)
    engine.set_layout(c["lengths"])
    assert int(engine.total) == c["dele"].shape[0]
    t = {k: engine.to_device(c[k]) for k in ("dele", "ins", "depth")}
    for k, (min_reads, windows) in enumerate(c["runs"]):
        for with_depth in (True, False):
            got, wr, host = device_sites(engine, t, min_reads, windows, with_depth)
            assert wr == 0 and (host[got.shape[0]:] == PATTERN).all()
            assert site_rows(got) == C.want_sites(name, k, with_depth), (k, with_depth)
        if (name, k) in C.SITES_EXPECTED:
            assert [s[:5] for s in site_rows(got)] == C.SITES_EXPECTED[(name, k)], k
    sites = engine.indel_sites(t["dele"], t["ins"], t["depth"], *c["runs"][0])
    assert site_rows(sites) == C.want_sites(name, 0)


def test_argument_errors_of_the_site_calls(engine):
    c = C.site_case("random")
    engine.set_layout(c["lengths"])
    t = {k: engine.to_device(c[k]) for k in ("dele", "ins", "depth")}
    p, lib = engine._p, engine.lib
    n = ctypes.c_uint64(0)
    size = lambda l=t["dele"], m=3, w=None, nw=0: lib.gci_indel_sites_size(engine.ctx, p(l), p(t["ins"]), p(t["depth"]), m, w, nw, ctypes.byref(n))      # noqa: E731
    assert size(m=0) == _lib.GCI_E_INVALID and size(l=t["dele"][1:]) == _lib.GCI_E_INVALID                  # min_reads < 1; not 16-byte aligned
    assert size(w=engine._window_array([(0, 5000), (4999, 6000)]), nw=2) == _lib.GCI_E_INVALID              # windows that overlap
    got, wr, host = device_sites(engine, t, 3, (), cap=len(C.want_sites("random", 1)) - 1)
    assert wr == _lib.GCI_E_CAPACITY and (host == PATTERN).all()
    out = engine.T.empty((8192, 6), engine.T.int32, engine.device)
    assert lib.gci_indel_sites_write(engine.ctx, p(t["dele"]), p(t["ins"]), p(t["depth"]), 4, None, 0, p(out), 8192) == _lib.GCI_E_INVALID      # another min_reads
    assert size() == 0
    engine.depth_hist(t["depth"], [(0, 100)], 0)                                                            # ... something else set windows in between
    assert lib.gci_indel_sites_write(engine.ctx, p(t["dele"]), p(t["ins"]), p(t["depth"]), 3, None, 0, p(out), 8192) == _lib.GCI_E_INVALID


def test_a_size_call_of_another_lister_ends_what_the_clip_size_call_measured(engine):
    """Every *_sites_size call sets the context's windows anew, so a write call that follows the size call of ANOTHER lister is refused
    and the other lister's own write call gives its sites: what lets the three listers share one scratch and one memo."""
    engine.set_layout([100])
    a = np.zeros(int(engine.total), dtype=np.int32)
    a[10:13], a[40] = [3, 4, 3], 5
    t = engine.to_device(a)
    p, lib = engine._p, engine.lib
    n = ctypes.c_uint64(0)
    head = (engine.ctx, p(t), p(t), None, 3, None, 0)
    assert lib.gci_clip_sites_size(*head, ctypes.byref(n)) == 0 and n.value == 4
    assert lib.gci_indel_sites_size(*head, ctypes.byref(n)) == 0 and n.value == 2
    out = engine.to_device(np.full((4 + GUARD, 6), PATTERN, dtype=np.int32))
    assert lib.gci_clip_sites_write(*head, p(out), 4) == _lib.GCI_E_INVALID
    assert lib.gci_indel_sites_write(*head, p(out), 4) == 0
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 6)
    assert site_rows(host[:2].view(INDEL_SITE_DTYPE).reshape(-1)) == [(0, 10, 13, 4, 4, 0), (0, 40, 41, 5, 5, 0)] and (host[2:] == PATTERN).all()


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctgA", 300_000), ("ctgB", 200_000), ("ctgC", 6_000))          # no simulated read lies on ctgC: what is planted there is all there is
MIN_LEN, MIN_READS = 50, 3
NM0 = bamfmt.encode_aux([("NM", "i", 0)])
PLANTED_DEL = ["plantD%d" % k for k in range(4)]       # four reads with 300M 60D 300M at ctgC:1000: the bases 1300 - 1359 are deleted
PLANTED_INS = ["plantI%d" % k for k in range(3)]       # three with 300M 80I 300M at ctgC:2000, one of them supplementary: the site is 2299
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Two BAM files (BGZF) of about a hundred synthetic records each over ctgA and ctgB, the first with the planted records on ctgC
    behind them; their streams and record offsets.  Made once."""
    if not _FILES:
        d = tmp_path_factory.mktemp("indels")
        hdr = bamfmt.encode_header([n for n, _ in CONTIGS], [l for _, l in CONTIGS])
        for kind, seed in (("hifi", 41), ("ont", 42)):
            rs = synth.simulate_reads(CONTIGS[:2], 3, kind, seed=seed).sorted()
            stream, offs = synth.to_bam_stream(rs)
            body = stream[int(offs[0]):].tobytes()
            new_offs = [int(o) - int(offs[0]) + len(hdr) for o in offs]
            if kind == "hifi":
                planted = [rec(2, 1000, [(M, 300), (D, 60), (M, 300)], n, aux=NM0) for n in PLANTED_DEL]
                planted += [rec(2, 2000, [(M, 300), (I, 80), (M, 300)], n, flag=0x800 if k == 0 else 0, aux=NM0) for k, n in enumerate(PLANTED_INS)]
                planted += [rec(2, 3000, [(M, 300), (D, 49), (M, 300)], "short%d" % k, aux=NM0) for k in range(5)]      # one base short of -l
                planted += [rec(2, 4000, [(M, 300), (D, 60), (M, 300)], "few%d" % k, aux=NM0) for k in range(2)]        # one read short of -n
                for r in planted:
                    new_offs.append(len(hdr) + len(body))
                    body += r
            stream = np.frombuffer(hdr + body, dtype=np.uint8).copy()
            path = str(d / (kind + ".bam"))
            bamfmt.write_bam_stream(path, stream, level=1, threads=4)
            _FILES[kind] = dict(path=path, stream=stream, offs=np.asarray(new_offs, dtype=np.uint64))
    return _FILES


def host_tracks(res):
    return {k: getattr(res, k).track.cpu().numpy().copy() for k in ("dele", "ins", "depth")}


def test_the_pipeline_in_one_piece_in_several_and_with_forced_flushes(engine, files, monkeypatch):
    """All three give identical tracks and sites: those of the statement over the file's stream.  The depth track is bit-equal to
    pipeline.bam_raw_depth on the same file and options; what -J adds to that depth is the del track of a run at -l 1."""
    f = files["hifi"]
    lengths = [l for _, l in CONTIGS]
    sel = np.arange(len(CONTIGS), dtype=np.int32)
    opts = pipeline.CoverOpts()
    want_dels, want_inss, want_counts, status = R.stream_events(f["stream"], f["offs"], lengths, sel, opts.excl, opts.min_mapq, MIN_LEN)
    assert status == R.NO_STATUS and want_dels.count((2, 1300, 1359)) == 4 and want_inss.count((2, 2299)) == 3
    raw = pipeline.bam_raw_depth(engine, [f["path"]], [], opts, 4).track.cpu().numpy().copy()
    want = dict(dele=R.track_of(want_dels, lengths), ins=R.track_of(want_inss, lengths), depth=raw)
    want_sites = R.sites_of(want["dele"], want["ins"], raw, lengths, MIN_READS)
    on_c = [s for s in want_sites if s[0] == 2]
    assert on_c == [(2, 1300, 1360, 4, 0, 0), (2, 2299, 2300, 0, 3, 3)], on_c      # (the four reads do not count as depth over the bases they delete)
    pieces, visit = [], pipeline._ClipVisitor.visit
    monkeypatch.setattr(pipeline._ClipVisitor, "visit", lambda self, *a: (pieces.append(a[-1]), visit(self, *a))[1])      # (a[-1]: rec_idx_base)
    whole = (pipeline.GPU_INFLATE_MAX, pipeline.BAM_CHUNK_BYTES)
    for several, budget in ((False, None), (True, None), (True, 1)):
        monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0 if several else whole[0])
        monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", (1 << 20) if several else whole[1])
        del pieces[:]
        res = pipeline.bam_indel_sites(engine, [f["path"]], [], opts, 4, MIN_LEN, MIN_READS, None, budget)
        assert (len(pieces) > 1) == several and pieces[0] == 0 and sorted(pieces) == pieces, pieces
        assert (res.flushes > 0) == (budget == 1) and res.counts == [want_counts]
        got = host_tracks(res)
        for k in want:
            assert np.array_equal(got[k], want[k]), (several, budget, k)
        assert site_rows(res.sites) == want_sites, (several, budget)
    monkeypatch.undo()
    # counting deletions as covered (-J) adds to the depth exactly the del track of a run at -l 1
    with_del = pipeline.bam_raw_depth(engine, [f["path"]], [], pipeline.CoverOpts(opts.excl, opts.min_mapq, True), 4).track.cpu().numpy().copy()
    res = pipeline.bam_indel_sites(engine, [f["path"]], [], opts, 4, 1, MIN_READS)
    assert np.array_equal(with_del - raw, host_tracks(res)["dele"]) and int((with_del - raw).sum()) > 4 * 60
    # regions select sites, not tracks; --chrs selects contigs
    res = pipeline.bam_indel_sites(engine, [f["path"]], [], opts, 4, MIN_LEN, MIN_READS, [("ctgC", 1310, 1320), ("ctgC", 2300, 2400), ("nowhere", 0, 9)])
    assert site_rows(res.sites) == [(2, 1310, 1320, 4, 0, 0)] and np.array_equal(host_tracks(res)["ins"], want["ins"])
    res = pipeline.bam_indel_sites(engine, [f["path"]], ["ctgC"], opts, 4, MIN_LEN, MIN_READS)
    assert site_rows(res.sites) == [(0, 1300, 1360, 4, 0, 0), (0, 2299, 2300, 0, 3, 3)] and list(res.dele.keys()) == ["ctgC"]
    # supplementary alignments excluded (-G 0x800): the insertion site is one read short
    res = pipeline.bam_indel_sites(engine, [f["path"]], ["ctgC"], pipeline.CoverOpts(0x704 | 0x800), 4, MIN_LEN, MIN_READS)
    assert site_rows(res.sites) == [(0, 1300, 1360, 4, 0, 0)] and int(host_tracks(res)["ins"].sum()) == 2


def test_two_files_add(engine, files):
    paths = [files["hifi"]["path"], files["ont"]["path"]]
    both = pipeline.bam_indel_sites(engine, paths, [], None, 4, 2, 1)
    got, counts = host_tracks(both), both.counts
    alone = [pipeline.bam_indel_sites(engine, [p], [], None, 4, 2, 1) for p in paths]
    parts = [host_tracks(r) for r in alone]
    assert counts == [alone[0].counts[0], alone[1].counts[0]] and counts[1][1] > 0 and counts[1][2] > 0
    for k in got:
        assert np.array_equal(got[k], parts[0][k] + parts[1][k]), k
    assert int(got["ins"].sum()) == counts[0][2] + counts[1][2]
    assert site_rows(both.sites) == R.sites_of(got["dele"], got["ins"], got["depth"], [l for _, l in CONTIGS], 1)


def test_command_line(engine, files, tmp_path):
    out = str(tmp_path)
    f = files["hifi"]
    r = _run("indel_sites.py", ["-d", out, "-o", "s", "-t", "4", f["path"]], dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["s.indel.del.depth.gz", "s.indel.ins.depth.gz", "s.indel.sites.bed", "s.indel.txt"]
    res = pipeline.bam_indel_sites(engine, [f["path"]], [], None, 4)
    want = host_tracks(res)
    lengths = dict(CONTIGS)
    for side, key in (("del", "dele"), ("ins", "ins")):
        tracks, got_lengths = pipeline.read_depth_tracks(engine, os.path.join(out, "s.indel.%s.depth.gz" % side))
        assert dict(got_lengths) == lengths and np.array_equal(tracks.track.cpu().numpy(), want[key]), side
    bed = os.path.join(out, "s.indel.sites.bed")
    assert open(bed).read() == pipeline.indel_sites_bed(res.sites, [n for n, _ in CONTIGS])
    assert "ctgC\t1300\t1360\t4\t0\t0\n" in open(bed).read() and "ctgC\t2299\t2300\t0\t3\t3\n" in open(bed).read()
    text = open(os.path.join(out, "s.indel.txt")).read()
    assert text == pipeline.indel_summary_text([f["path"]], res.counts, int(res.sites.shape[0]),
                                               [("min_len", 50), ("min_reads", 3), ("excl_flags", "0x704"), ("min_mapq", 0), ("count_del", 0),
                                                ("chrs", "."), ("regions", ".")])
    # filter_reads.py -R on the written BED lists, for the planted sites, exactly the planted reads
    r = _run("filter_reads.py", ["-d", out, "-o", "fr", "-t", "4", "-R", bed, f["path"]])
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split("\t") for ln in open(os.path.join(out, "fr.reads.tsv")) if not ln.startswith("#")]
    on_c = [(row[1], int(row[3])) for row in rows if row[2] == "ctgC"]
    assert sorted(n for n, start in on_c if start == 1000) == PLANTED_DEL and sorted(n for n, start in on_c if start == 2000) == PLANTED_INS
    assert len(on_c) == len(PLANTED_DEL) + len(PLANTED_INS)
    r = _run("indel_sites.py", ["-d", out, "-o", "s", f["path"]])               # a second run without -f refuses
    assert r.returncode != 0 and r.stderr.strip().split("\n")[-1] == 'Please use "-f" or "--force" to rewrite'
    # a malformed record: bam_depth.py's message, and no output
    n = int(f["offs"].shape[0])
    stream = np.concatenate([f["stream"], np.frombuffer(rec(0, 5, [(M, 4), (9, 3)]), dtype=np.uint8)])
    path = str(tmp_path / "op9.bam")
    bamfmt.write_bam_stream(path, stream, level=1, threads=2)
    r = _run("indel_sites.py", ["-d", out, "-o", "bad", path])
    assert r.returncode != 0 and "Traceback" not in r.stderr
    assert r.stderr.strip().split("\n")[-1] == 'ERROR!!! The file "%s" holds a malformed BAM record (record %d)' % (path, n)
    assert not [x for x in os.listdir(out) if x.startswith("bad.")]
