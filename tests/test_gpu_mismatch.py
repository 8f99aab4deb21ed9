"""mismatch_sites.py on the GPU: gci_fasta_codes, gci_bam_mismatch_size / _write and gci_mismatch_sites_size / _write (k_mismatch.hip)
against the statement of tests/mismatch_ref.py on every case of tests/mismatch_cases.py, into pre-filled buffers with guard entries
behind them; the built track; pipeline.bam_mismatch_sites over a small synthetic file with real bases in one piece, in several and
with forced flushes, against the statement and pipeline.bam_raw_depth, and file by file; and the command line once, its BED file handed
on to filter_reads.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mismatch_cases as C
import mismatch_ref as R
from cover_cases import M
from gci_amd import _lib, pipeline, synth
from gci_amd.device import IVL_DTYPE, MISMATCH_SITE_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16                                             # entries behind the output that must stay
PATTERN = -0x5A5A5A5B
U64 = 2 ** 64 - 1
FIELDS = ("contig", "start", "end", "mismatch", "depth")
STREAM_GUARD = 64                                      # bytes behind the stream: 0x88, the base T in both nibbles


def upload(engine, name):
    c = C.case(name)
    stream, offs = c["stream"], c["offs"]
    padded = np.concatenate([stream, np.full(STREAM_GUARD, 0x88, dtype=np.uint8)])
    up = lambda a: engine.to_device(a if a.shape[0] else np.zeros(1, dtype=a.dtype))      # noqa: E731
    return dict(stream=engine.to_device(padded), offs=up(offs), sel=engine.to_device(c["ref_sel"]), n_bytes=int(stream.shape[0]),
                n_rec=int(offs.shape[0]), codes=engine.to_device(c["codes"]))


@pytest.fixture(scope="module")
def on_device(engine):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = upload(engine, name)
        return cache[name]
    return get


def device_mismatch(engine, b, run, cap=None, has_seq=1):
    """-> (events, counts, status word, the size call's return, the write call's return, the whole buffer) of the exports as they are:
    the output pre-filled with a pattern, GUARD entries behind it."""
    p, lib = engine._p, engine.lib
    counts = (ctypes.c_uint64 * 3)()
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    offs = p(b["offs"]) if b["n_rec"] else None
    st = lib.gci_bam_mismatch_size(engine.ctx, p(b["stream"]), b["n_bytes"], offs, b["n_rec"], has_seq, p(b["sel"]), int(b["sel"].shape[0]), run[0],
                                   run[1], p(b["codes"]), counts, p(status))
    if st:
        return None, None, None, st, None, None
    total = int(counts[1])
    out = engine.to_device(np.full((total + GUARD, 4), PATTERN, dtype=np.int32))
    wr = lib.gci_bam_mismatch_write(engine.ctx, p(b["stream"]), b["n_bytes"], offs, b["n_rec"], has_seq, p(b["codes"]), p(out),
                                    total if cap is None else cap, p(status))
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 4)
    return host.view(IVL_DTYPE).reshape(-1)[:total], [int(x) for x in counts], int(status.item()) & U64, st, wr, host


def events_of(ivl):
    assert (ivl["start"] == ivl["end"]).all() and (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist()))


@pytest.mark.parametrize("name", C.NAMES)
def test_the_device_gives_the_events_of_the_statement(engine, on_device, name):
    """The events in (record, reference position) order, status and counts as the statement's, the guard entries untouched; the track
    built from them holds, per base, the events over it."""
    c, b = C.case(name), on_device(name)
    engine.set_layout(c["lengths"])
    for run in c["runs"]:
        want_events, want_counts, want_status = C.want(name, run)
        ivl, counts, status, st, wr, host = device_mismatch(engine, b, run)
        assert st == 0 and wr == 0 and status == want_status and counts == want_counts, run
        assert (host[counts[1]:] == PATTERN).all(), "entries behind the events were written"
        assert events_of(ivl) == want_events, run
        if want_events:
            track = engine.depth_build(engine.to_device(np.ascontiguousarray(ivl).view(np.int32).reshape(-1, 4)), None, 0, engine.new_track())
            assert np.array_equal(track.cpu().numpy(), R.track_of(want_events, c["lengths"])), run


def test_the_device_gives_the_hand_written_events(engine, on_device):
    for (name, run), (events, counts) in C.EXPECTED.items():
        engine.set_layout(C.case(name)["lengths"])
        ivl, got, _, st, wr, _ = device_mismatch(engine, on_device(name), run)
        assert (st, wr, events_of(ivl), got) == (0, 0, events, counts), (name, run)


def test_two_runs_give_the_same_bytes(engine, on_device):
    c, b = C.case("records_4097"), on_device("records_4097")
    engine.set_layout(c["lengths"])
    first = device_mismatch(engine, b, c["runs"][0])[5]
    assert first.shape[0] > 3000 + GUARD and np.array_equal(first, device_mismatch(engine, b, c["runs"][0])[5])


def test_engine_bam_mismatch_and_its_status(engine, on_device):
    c, b = C.case("records_257"), on_device("records_257")
    engine.set_layout(c["lengths"])
    run = c["runs"][0]
    ivl, counts = engine.bam_mismatch(b["stream"][:b["n_bytes"]], b["offs"], True, b["sel"], b["codes"], *run)
    want = C.want("records_257", run)
    assert counts == want[1] and events_of(ivl.cpu().numpy().view(IVL_DTYPE).reshape(-1)) == want[0]
    for name, bad in C.MALFORMED.items():
        b = on_device(name)
        engine.set_layout(C.case(name)["lengths"])
        with pytest.raises(_lib.GciError) as e:
            engine.bam_mismatch(b["stream"][:b["n_bytes"]], b["offs"], True, b["sel"], b["codes"])
        assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == bad, name


def test_argument_errors_of_the_record_calls(engine, on_device):
    c, b = C.case("phases"), on_device("phases")
    engine.set_layout(c["lengths"])
    p, lib = engine._p, engine.lib
    assert device_mismatch(engine, b, (C.EXCL, 0), has_seq=0)[3] == _lib.GCI_E_INVALID          # a heads stream holds no SEQ
    _, counts, _, st, wr, host = device_mismatch(engine, b, (C.EXCL, 0), cap=4)                # five events: one entry too few
    assert st == 0 and counts == [5, 5, 24] and wr == _lib.GCI_E_CAPACITY and (host == PATTERN).all()
    out = engine.T.empty((16, 4), engine.T.int32, engine.device)
    write = lambda e, n_rec=b["n_rec"], codes=b["codes"]: lib.gci_bam_mismatch_write(e.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), n_rec, 1,      # noqa: E731
                                                                                     p(codes), p(out), 16, p(engine._status))
    assert write(engine, n_rec=b["n_rec"] - 1) == _lib.GCI_E_INVALID                           # not what the size call measured
    assert write(engine, codes=engine.to_device(c["codes"])) == _lib.GCI_E_INVALID
    assert write(engine) == 0
    from gci_amd.device import Engine
    fresh = Engine(0)
    try:
        assert device_mismatch(fresh, b, (C.EXCL, 0))[3] == _lib.GCI_E_NO_LAYOUT
        fresh.set_layout(c["lengths"])
        assert write(fresh) == _lib.GCI_E_INVALID                                               # no size call in front of it
    finally:
        fresh.close()


# ---- the assembly ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.FASTA_NAMES)
def test_the_device_gives_the_codes_of_the_statement(engine, name):
    """Into an array pre-filled with a pattern: every base once, the elements no base goes to untouched."""
    c = C.fasta_case(name)
    engine.set_layout(c["lengths"])
    assert int(engine.total) == c["total"]
    codes = engine.to_device(np.full(c["total"], C.FILL, dtype=np.uint8))
    got, kept = engine.fasta_codes(c["text"], c["bodies"], c["dst"], codes)
    want = C.want_codes(name)
    host = got.cpu().numpy()
    assert np.array_equal(host, want), np.flatnonzero(host != want)[:8]
    spans = R.fasta_records(c["text"].tobytes())
    assert int(kept.sum()) == sum(R.seq_length(c["text"], a, b) for _, a, b in spans)
    if name in C.FASTA_EXPECTED:
        for at, codes_at in C.FASTA_EXPECTED[name].items():
            assert host[at:at + len(codes_at)].tolist() == codes_at


def test_the_cases_code_arrays_are_the_devices(engine):
    """The code arrays the record cases are walked with come from the statement: the device makes the same from the same FASTA text."""
    from gci_amd.formats import fasta
    for name in ("letters", "second_contig", "records_257"):
        c = C.case(name)
        engine.set_layout(c["lengths"])
        text = np.frombuffer(c["fasta"], dtype=np.uint8).copy()
        bodies = np.array([s[1:] for s in fasta.record_spans(text)], dtype=np.int64)
        got, _ = engine.fasta_codes(text, bodies, np.asarray(engine.offsets, dtype=np.int64)[:bodies.shape[0]])
        assert np.array_equal(got.cpu().numpy(), c["codes"]), name


# ---- sites -----------------------------------------------------------------------------------------------------------------------------

def device_sites(engine, t, min_reads, frac, windows, cap=None):
    p, lib = engine._p, engine.lib
    arr, nw = engine._window_array(windows), len(windows)
    n = ctypes.c_uint64(0)
    head = (engine.ctx, p(t["mism"]), p(t["depth"]), min_reads, frac, arr, nw)
    assert lib.gci_mismatch_sites_size(*head, ctypes.byref(n)) == 0
    total = int(n.value)
    out = engine.to_device(np.full((total + GUARD, 5), PATTERN, dtype=np.int32))
    wr = lib.gci_mismatch_sites_write(*head, p(out), total if cap is None else cap)
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 5)
    return host[:total].view(MISMATCH_SITE_DTYPE).reshape(-1), wr, host


def site_rows(sites):
    return list(zip(*(sites[f].tolist() for f in FIELDS)))


@pytest.mark.parametrize("name", C.SITE_NAMES)
def test_the_device_gives_the_sites_of_the_statement(engine, name):
    c = C.site_case(name)
    engine.set_layout(c["lengths"])
    assert int(engine.total) == c["mism"].shape[0]
    t = {k: engine.to_device(c[k]) for k in ("mism", "depth")}
    for k, (min_reads, frac, windows) in enumerate(c["runs"]):
        got, wr, host = device_sites(engine, t, min_reads, frac, windows)
        assert wr == 0 and (host[got.shape[0]:] == PATTERN).all()
        assert site_rows(got) == C.want_sites(name, k), k
        if (name, k) in C.SITES_EXPECTED:
            assert site_rows(got) == C.SITES_EXPECTED[(name, k)], k
    sites = engine.mismatch_sites(t["mism"], t["depth"], *c["runs"][0])
    assert site_rows(sites) == C.want_sites(name, 0)


def test_argument_errors_of_the_site_calls(engine):
    c = C.site_case("random")
    engine.set_layout(c["lengths"])
    t = {k: engine.to_device(c[k]) for k in ("mism", "depth")}
    p, lib = engine._p, engine.lib
    n = ctypes.c_uint64(0)
    size = lambda m=t["mism"], d=t["depth"], r=3, f=500000, w=None, nw=0: lib.gci_mismatch_sites_size(engine.ctx, p(m), p(d), r, f, w, nw, ctypes.byref(n))      # noqa: E731
    assert size(r=0) == _lib.GCI_E_INVALID and size(m=t["mism"][1:]) == _lib.GCI_E_INVALID and size(d=None) == _lib.GCI_E_INVALID
    assert size(f=-1) == _lib.GCI_E_INVALID and size(f=1000001) == _lib.GCI_E_INVALID
    assert size(w=engine._window_array([(0, 5000), (4999, 6000)]), nw=2) == _lib.GCI_E_INVALID              # windows that overlap
    got, wr, host = device_sites(engine, t, 3, 500000, (), cap=len(C.want_sites("random", 1)) - 1)
    assert wr == _lib.GCI_E_CAPACITY and (host == PATTERN).all()
    out = engine.T.empty((8192, 5), engine.T.int32, engine.device)
    assert lib.gci_mismatch_sites_write(engine.ctx, p(t["mism"]), p(t["depth"]), 3, 500001, None, 0, p(out), 8192) == _lib.GCI_E_INVALID      # another fraction
    assert size() == 0
    engine.depth_hist(t["depth"], [(0, 100)], 0)                                                            # ... something else set windows in between
    assert lib.gci_mismatch_sites_write(engine.ctx, p(t["mism"]), p(t["depth"]), 3, 500000, None, 0, p(out), 8192) == _lib.GCI_E_INVALID


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctgA", 300_000), ("ctgB", 200_000), ("ctgC", 6_000))          # no simulated read lies on ctgC: what is planted there is all there is
MIN_READS, MIN_FRAC = 3, "0.5"
PLANTED = ["plant%d" % k for k in range(4)]            # four reads with 600M at ctgC:1000 that read another base at 1300, three of them at 1301 too
NM = bamfmt.encode_aux([("NM", "i", 2)])              # (filter_reads.py, run on the same file, asks for the tag)
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


def _other(base):
    return b"ACGT"[(b"ACGT".index(base) + 1) % 4]


def _planted(ref, name, pos, n, changed, flag=0):
    seq = bytearray(ref[pos:pos + n].tobytes())
    for p in changed:
        seq[p - pos] = _other(seq[p - pos])
    return bamfmt.encode_record(2, pos, name, 60, flag, [(M, n)], n, NM, seq=bytes(seq))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A random assembly as FASTA (its records in another order than @SQ, one extra) and two BAM files (BGZF) of about a hundred synthetic
    records each over ctgA and ctgB with 2 % substituted bases, the first with the planted records on ctgC behind them.  Made once."""
    if not _FILES:
        d = tmp_path_factory.mktemp("mismatch")
        ref = synth.random_reference(CONTIGS + (("extra", 5000),), seed=3)
        fa = str(d / "ref.fa")
        synth.write_fasta(fa, {k: ref[k] for k in ("ctgB", "extra", "ctgC", "ctgA")}, width=61)
        hdr = bamfmt.encode_header([n for n, _ in CONTIGS], [l for _, l in CONTIGS])
        for kind, seed in (("hifi", 41), ("ont", 42)):
            rs = synth.simulate_reads(CONTIGS[:2], 3, kind, seed=seed).sorted()
            stream, offs = synth.to_bam_stream(rs, seq_qual="reference", reference=ref, sub_rate=0.02, seed=seed)
            body = stream[int(offs[0]):].tobytes()
            new_offs = [int(o) - int(offs[0]) + len(hdr) for o in offs]
            if kind == "hifi":
                c = ref["ctgC"]
                planted = [_planted(c, n, 1000, 600, [1300, 1301] if k else [1300], flag=0x800 if k == 3 else 0) for k, n in enumerate(PLANTED)]
                planted += [_planted(c, "few%d" % k, 4000, 300, [4100]) for k in range(2)]                      # one read short of -n
                planted += [_planted(c, "part%d" % k, 5000, 300, [5100] if k < 3 else []) for k in range(7)]     # 3 of 7: below -F 0.5
                for r in planted:
                    new_offs.append(len(hdr) + len(body))
                    body += r
            stream = np.frombuffer(hdr + body, dtype=np.uint8).copy()
            path = str(d / (kind + ".bam"))
            bamfmt.write_bam_stream(path, stream, level=1, threads=4)
            _FILES[kind] = dict(path=path, stream=stream, offs=np.asarray(new_offs, dtype=np.uint64))
        offs, total = R.layout([l for _, l in CONTIGS])
        codes = np.full(total, 15, dtype=np.uint8)
        for (name, L), o in zip(CONTIGS, offs):
            codes[o:o + L] = synth._ACGT_CODE[ref[name]]
        _FILES.update(fasta=fa, codes=codes, ref=ref, dir=d)
    return _FILES


def host_tracks(res):
    return {k: getattr(res, k).track.cpu().numpy().copy() for k in ("mismatch", "depth")}


def test_the_pipeline_in_one_piece_in_several_and_with_forced_flushes(engine, files, monkeypatch):
    """All three give identical tracks and sites: those of the statement over the file's stream and the assembly's bases.  The depth
    track is bit-equal to pipeline.bam_raw_depth on the same file and options."""
    f = files["hifi"]
    lengths = [l for _, l in CONTIGS]
    sel = np.arange(len(CONTIGS), dtype=np.int32)
    opts = pipeline.CoverOpts()
    want_events, want_counts, status = R.stream_events(f["stream"], f["offs"], lengths, sel, files["codes"], opts.excl, opts.min_mapq)
    assert status == R.NO_STATUS and want_events.count((2, 1300)) == 4 and want_events.count((2, 1301)) == 3 and want_counts[1] > 10000
    raw = pipeline.bam_raw_depth(engine, [f["path"]], [], opts, 4).track.cpu().numpy().copy()
    want = dict(mismatch=R.track_of(want_events, lengths), depth=raw)
    assert (want["mismatch"] <= raw).all()
    want_sites = R.sites_of(want["mismatch"], raw, lengths, MIN_READS, 500000)
    assert [s for s in want_sites if s[0] == 2] == [(2, 1300, 1302, 4, 4)]
    pieces, visit = [], pipeline._ClipVisitor.visit
    monkeypatch.setattr(pipeline._ClipVisitor, "visit", lambda self, *a: (pieces.append(a[-1]), visit(self, *a))[1])      # (a[-1]: rec_idx_base)
    whole = (pipeline.GPU_INFLATE_MAX, pipeline.BAM_CHUNK_BYTES)
    for several, budget in ((False, None), (True, None), (True, 1)):
        monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0 if several else whole[0])
        monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", (1 << 20) if several else whole[1])
        del pieces[:]
        res = pipeline.bam_mismatch_sites(engine, files["fasta"], [f["path"]], [], opts, 4, MIN_READS, MIN_FRAC, None, budget)
        assert (len(pieces) > 1) == several and pieces[0] == 0 and sorted(pieces) == pieces, pieces
        assert (res.flushes > 0) == (budget == 1) and res.counts == [want_counts]
        got = host_tracks(res)
        for k in want:
            assert np.array_equal(got[k], want[k]), (several, budget, k)
        assert site_rows(res.sites) == want_sites, (several, budget)
    monkeypatch.undo()
    # the fraction: 3 of 7 reads is a site from -F 0.428571 down, not at 0.428572
    for frac, there in (("0.428571", True), ("0.428572", False), (428571, True)):
        res = pipeline.bam_mismatch_sites(engine, files["fasta"], [f["path"]], ["ctgC"], opts, 4, MIN_READS, frac)
        assert ((0, 5100, 5101, 3, 7) in site_rows(res.sites)) == there, frac
    # regions select sites, not tracks; supplementary alignments excluded (-G 0x800): base 1301 is one read short
    res = pipeline.bam_mismatch_sites(engine, files["fasta"], [f["path"]], [], opts, 4, MIN_READS, MIN_FRAC, [("ctgC", 1301, 1400), ("nowhere", 0, 9)])
    assert site_rows(res.sites) == [(2, 1301, 1302, 3, 4)] and np.array_equal(host_tracks(res)["mismatch"], want["mismatch"])
    res = pipeline.bam_mismatch_sites(engine, files["fasta"], [f["path"]], ["ctgC"], pipeline.CoverOpts(0x704 | 0x800), 4, MIN_READS, MIN_FRAC)
    assert site_rows(res.sites) == [(0, 1300, 1301, 3, 3)] and list(res.mismatch.keys()) == ["ctgC"]


def test_two_files_add(engine, files):
    paths = [files["hifi"]["path"], files["ont"]["path"]]
    both = pipeline.bam_mismatch_sites(engine, files["fasta"], paths, [], None, 4, 1, "0")
    got, counts = host_tracks(both), both.counts
    alone = [pipeline.bam_mismatch_sites(engine, files["fasta"], [p], [], None, 4, 1, "0") for p in paths]
    parts = [host_tracks(r) for r in alone]
    assert counts == [alone[0].counts[0], alone[1].counts[0]] and counts[1][1] > 0 and counts[1][2] > counts[1][1]
    for k in got:
        assert np.array_equal(got[k], parts[0][k] + parts[1][k]), k
    assert int(got["mismatch"].sum()) == counts[0][1] + counts[1][1]
    assert site_rows(both.sites) == R.sites_of(got["mismatch"], got["depth"], [l for _, l in CONTIGS], 1, 0)


def test_the_assembly_must_fit_the_sq_table(engine, files):
    ref, d = files["ref"], files["dir"]
    bad = str(d / "short.fa")
    synth.write_fasta(bad, {"ctgA": ref["ctgA"], "ctgB": ref["ctgB"][:-1], "ctgC": ref["ctgC"]})
    with pytest.raises(ValueError, match="`ctgB` has 199999 bases"):
        pipeline.bam_mismatch_sites(engine, bad, [files["hifi"]["path"]])
    synth.write_fasta(bad, {"ctgA": ref["ctgA"], "ctgB": ref["ctgB"]})
    with pytest.raises(ValueError, match="`ctgC` is not in"):
        pipeline.bam_mismatch_sites(engine, bad, [files["hifi"]["path"]])
    res = pipeline.bam_mismatch_sites(engine, bad, [files["hifi"]["path"]], ["ctgB"])          # ... which --chrs leaves out
    assert list(res.mismatch.keys()) == ["ctgB"]


def test_command_line(engine, files, tmp_path):
    out = str(tmp_path)
    f = files["hifi"]
    r = _run("mismatch_sites.py", ["-r", files["fasta"], "-d", out, "-o", "s", "-t", "4", f["path"]], dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["s.mismatch.depth.gz", "s.mismatch.sites.bed", "s.mismatch.txt"]
    res = pipeline.bam_mismatch_sites(engine, files["fasta"], [f["path"]], [], None, 4)
    tracks, got_lengths = pipeline.read_depth_tracks(engine, os.path.join(out, "s.mismatch.depth.gz"))
    assert dict(got_lengths) == dict(CONTIGS) and np.array_equal(tracks.track.cpu().numpy(), host_tracks(res)["mismatch"])
    bed = os.path.join(out, "s.mismatch.sites.bed")
    assert open(bed).read() == pipeline.mismatch_sites_bed(res.sites, [n for n, _ in CONTIGS])
    assert "ctgC\t1300\t1302\t4\t4\n" in open(bed).read()
    text = open(os.path.join(out, "s.mismatch.txt")).read()
    assert text == pipeline.mismatch_summary_text([f["path"]], res.counts, int(res.sites.shape[0]),
                                                  [("reference", files["fasta"]), ("min_reads", 3), ("min_frac_ppm", 500000), ("excl_flags", "0x704"),
                                                   ("min_mapq", 0), ("count_del", 0), ("chrs", "."), ("regions", ".")])
    # filter_reads.py -R on the written BED lists, for the planted site, exactly the planted reads
    r = _run("filter_reads.py", ["-d", out, "-o", "fr", "-t", "4", "-R", bed, f["path"]])
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split("\t") for ln in open(os.path.join(out, "fr.reads.tsv")) if not ln.startswith("#")]
    assert sorted(row[1] for row in rows if row[2] == "ctgC") == PLANTED
    r = _run("mismatch_sites.py", ["-r", files["fasta"], "-d", out, "-o", "s", f["path"]])          # a second run without -f refuses
    assert r.returncode != 0 and r.stderr.strip().split("\n")[-1] == 'Please use "-f" or "--force" to rewrite'
    r = _run("mismatch_sites.py", ["-r", files["fasta"], "-d", out, "-o", "h", f["path"]], dict(GCI_BAM_INGEST="heads"))
    assert r.returncode != 0 and "Traceback" not in r.stderr and "GCI_BAM_INGEST=heads" in r.stderr
    assert not [x for x in os.listdir(out) if x.startswith("h.")]
