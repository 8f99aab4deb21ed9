"""clip_sites.py on the GPU: gci_bam_clip_size / _write and gci_clip_sites_size / _write (k_clips.hip) against the statement of
tests/clips_ref.py on every case of tests/clips_cases.py, in both stream forms, into pre-filled buffers with guard entries behind them;
the built tracks; pipeline.bam_clip_sites over a small synthetic file in one piece, in several and with forced flushes, against
pipeline.bam_raw_depth and file by file; and the command line once, its BED file handed on to filter_reads.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import clips_cases as C
import clips_ref as R
from cover_cases import H, M, S, rec
from gci_amd import _lib, pipeline, synth
from gci_amd.device import IVL_DTYPE, SITE_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16                                             # entries behind the output that must stay
PATTERN = -0x5A5A5A5B
U64 = 2 ** 64 - 1


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


def device_clip(engine, b, has_seq, run, cap=None):
    """-> (left events, right events, counts, status word, the write call's return, the whole buffer) of the exports as they are: the
    output pre-filled with a pattern, GUARD entries behind it."""
    p, lib = engine._p, engine.lib
    counts = (ctypes.c_uint64 * 3)()
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    st = lib.gci_bam_clip_size(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]) if b["n_rec"] else None, b["n_rec"], int(has_seq), p(b["sel"]),
                               int(b["sel"].shape[0]), run[0], run[1], run[2], counts, p(status))
    assert st == 0
    n_left, n_right = int(counts[1]), int(counts[2])
    total = n_left + n_right
    out = engine.to_device(np.full((total + GUARD, 4), PATTERN, dtype=np.int32))
    wr = lib.gci_bam_clip_write(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]) if b["n_rec"] else None, b["n_rec"], int(has_seq), p(out),
                                total if cap is None else cap, p(status))
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 4)
    ivl = host.view(IVL_DTYPE).reshape(-1)
    return ivl[:n_left], ivl[n_left:total], [int(x) for x in counts], int(status.item()) & U64, wr, host


def pairs_of(ivl):
    assert (ivl["start"] == ivl["end"]).all() and (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist()))


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name", C.NAMES)
def test_the_device_gives_the_events_of_the_statement(engine, on_device, name, form):
    """Both halves in record order, status and counts as the statement's, the guard entries untouched; the tracks built from either half
    hold, per base, the events there."""
    c, b = C.case(name), on_device(name, form)
    engine.set_layout(c["lengths"])
    for run in c["runs"]:
        want_left, want_right, want_counts, want_status = C.want(name, run)
        left, right, counts, status, wr, host = device_clip(engine, b, form == "stream", run)
        assert wr == 0 and status == want_status and counts == want_counts, run
        assert (host[counts[1] + counts[2]:] == PATTERN).all(), "entries behind the events were written"
        assert pairs_of(left) == want_left and pairs_of(right) == want_right, run
        for ivl, want in ((left, want_left), (right, want_right)):
            if not len(want):
                continue
            track = engine.depth_build(engine.to_device(np.ascontiguousarray(ivl).view(np.int32).reshape(-1, 4)), None, 0, engine.new_track())
            got = track.cpu().numpy()
            assert np.array_equal(got, R.track_of(want, c["lengths"])) and int(got.sum(dtype=np.int64)) == len(want), run


def test_the_device_gives_the_hand_written_events(engine, on_device):
    for (name, run), (left, right, counted) in C.EXPECTED.items():
        engine.set_layout(C.case(name)["lengths"])
        got_left, got_right, counts, status, _, _ = device_clip(engine, on_device(name, "stream"), True, run)
        assert (pairs_of(got_left), pairs_of(got_right), counts[0], status) == (left, right, counted, U64), (name, run)


def test_engine_bam_clip_and_its_status(engine, on_device):
    c, b = C.case("random_2000"), on_device("random_2000", "heads")
    engine.set_layout(c["lengths"])
    run = c["runs"][0]
    left, right, counts = engine.bam_clip(b["stream"], b["offs"], False, b["sel"], *run)
    want = C.want("random_2000", run)
    assert counts == want[2]
    assert pairs_of(left.cpu().numpy().view(IVL_DTYPE).reshape(-1)) == want[0] and pairs_of(right.cpu().numpy().view(IVL_DTYPE).reshape(-1)) == want[1]
    b = on_device("op9", "stream")
    engine.set_layout(C.case("op9")["lengths"])
    with pytest.raises(_lib.GciError) as e:
        engine.bam_clip(b["stream"], b["offs"], True, b["sel"], min_clip=5)
    assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == C.MALFORMED["op9"]


def test_argument_errors_of_the_record_calls(engine, on_device):
    c, b = C.case("end_operations"), on_device("end_operations", "stream")
    engine.set_layout(c["lengths"])
    p, lib = engine._p, engine.lib
    counts = (ctypes.c_uint64 * 3)()
    size = lambda e, min_clip=5, h=counts: lib.gci_bam_clip_size(e.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"], 1, p(b["sel"]),      # noqa: E731
                                                                 int(b["sel"].shape[0]), 0x704, 0, min_clip, h, p(engine._status))
    assert size(engine, min_clip=0) == _lib.GCI_E_INVALID and size(engine, h=None) == _lib.GCI_E_INVALID
    run = c["runs"][0]
    _, _, counts_ok, _, wr, host = device_clip(engine, b, True, run, cap=8)          # nine events: one entry too few
    assert counts_ok == [9, 5, 4] and wr == _lib.GCI_E_CAPACITY and (host == PATTERN).all()
    out = engine.T.empty((16, 4), engine.T.int32, engine.device)
    assert lib.gci_bam_clip_write(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"] - 1, 1, p(out), 16, p(engine._status)) == _lib.GCI_E_INVALID
    from gci_amd.device import Engine
    fresh = Engine(0)
    try:
        assert size(fresh) == _lib.GCI_E_NO_LAYOUT
        fresh.set_layout(c["lengths"])
        assert lib.gci_bam_clip_write(fresh.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"], 1, p(out), 16, p(engine._status)) == _lib.GCI_E_INVALID
    finally:
        fresh.close()


# ---- sites -----------------------------------------------------------------------------------------------------------------------------

def device_sites(engine, t, min_reads, windows, with_depth=True, cap=None):
    p, lib = engine._p, engine.lib
    arr, nw = engine._window_array(windows), len(windows)
    n = ctypes.c_uint64(0)
    head = (engine.ctx, p(t["left"]), p(t["right"]), p(t["depth"]) if with_depth else None, min_reads, arr, nw)
    assert lib.gci_clip_sites_size(*head, ctypes.byref(n)) == 0
    total = int(n.value)
    out = engine.to_device(np.full((total + GUARD, 6), PATTERN, dtype=np.int32))
    wr = lib.gci_clip_sites_write(*head, p(out), total if cap is None else cap)
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 6)
    return host[:total].view(SITE_DTYPE).reshape(-1), wr, host


@pytest.mark.parametrize("name", C.SITE_NAMES)
def test_the_device_gives_the_sites_of_the_statement(engine, name):
    c = C.site_case(name)
    engine.set_layout(c["lengths"])
    assert int(engine.total) == c["left"].shape[0]
    t = {k: engine.to_device(c[k]) for k in ("left", "right", "depth")}
    for k, (min_reads, windows) in enumerate(c["runs"]):
        for with_depth in (True, False):
            got, wr, host = device_sites(engine, t, min_reads, windows, with_depth)
            assert wr == 0 and (host[got.shape[0]:] == PATTERN).all() and (got["pad"] == 0).all()
            assert list(zip(*(got[f].tolist() for f in ("contig", "pos", "left", "right", "depth")))) == C.want_sites(name, k, with_depth), (k, with_depth)
    sites = engine.clip_sites(t["left"], t["right"], t["depth"], *c["runs"][0])
    assert list(zip(*(sites[f].tolist() for f in ("contig", "pos", "left", "right", "depth")))) == C.want_sites(name, 0)


def test_argument_errors_of_the_site_calls(engine):
    c = C.site_case("tiles")
    engine.set_layout(c["lengths"])
    t = {k: engine.to_device(c[k]) for k in ("left", "right", "depth")}
    p, lib = engine._p, engine.lib
    n = ctypes.c_uint64(0)
    size = lambda l=t["left"], m=3, w=None, nw=0: lib.gci_clip_sites_size(engine.ctx, p(l), p(t["right"]), p(t["depth"]), m, w, nw, ctypes.byref(n))      # noqa: E731
    assert size(m=0) == _lib.GCI_E_INVALID and size(l=t["left"][1:]) == _lib.GCI_E_INVALID                  # min_reads < 1; not 16-byte aligned
    assert size(w=engine._window_array([(0, 5000), (4999, 6000)]), nw=2) == _lib.GCI_E_INVALID              # windows that overlap
    got, wr, host = device_sites(engine, t, 3, (), cap=len(C.want_sites("tiles", 0)) - 1)
    assert wr == _lib.GCI_E_CAPACITY and (host == PATTERN).all()
    out = engine.T.empty((8192, 6), engine.T.int32, engine.device)
    assert lib.gci_clip_sites_write(engine.ctx, p(t["left"]), p(t["right"]), p(t["depth"]), 4, None, 0, p(out), 8192) == _lib.GCI_E_INVALID      # another min_reads
    assert size() == 0
    engine.depth_hist(t["depth"], [(0, 100)], 0)                                                            # ... something else set windows in between
    assert lib.gci_clip_sites_write(engine.ctx, p(t["left"]), p(t["right"]), p(t["depth"]), 3, None, 0, p(out), 8192) == _lib.GCI_E_INVALID


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctgA", 300_000), ("ctgB", 200_000), ("ctgC", 6_000))          # no simulated read lies on ctgC: what is planted there is all there is
MIN_CLIP, MIN_READS = 100, 3
NM0 = bamfmt.encode_aux([("NM", "i", 0)])
PLANTED_LEFT = ["plantL%d" % k for k in range(4)]      # four alignments that begin at ctgC:1000 behind 150 clipped bases
PLANTED_RIGHT = ["plantR%d" % k for k in range(3)]     # three that end at ctgC:2299 in front of 150 hard clipped bases
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Two BAM files (BGZF) of about a hundred synthetic records each over ctgA and ctgB, the first with the planted records on ctgC
    behind them; their streams and record offsets.  Made once."""
    if not _FILES:
        d = tmp_path_factory.mktemp("clips")
        hdr = bamfmt.encode_header([n for n, _ in CONTIGS], [l for _, l in CONTIGS])
        for kind, seed in (("hifi", 41), ("ont", 42)):
            rs = synth.simulate_reads(CONTIGS[:2], 3, kind, seed=seed).sorted()
            stream, offs = synth.to_bam_stream(rs)
            body = stream[int(offs[0]):].tobytes()
            new_offs = [int(o) - int(offs[0]) + len(hdr) for o in offs]
            if kind == "hifi":
                planted = [rec(2, 1000, [(S, 100), (H, 50), (M, 300)], n, aux=NM0) for n in PLANTED_LEFT]
                planted += [rec(2, 2000, [(M, 300), (H, 150)], n, flag=0x800, aux=NM0) for n in PLANTED_RIGHT]
                planted += [rec(2, 3000, [(S, 99), (M, 300)], "short%d" % k, aux=NM0) for k in range(5)]      # one base short of -c
                planted += [rec(2, 4000, [(S, 150), (M, 300)], "few%d" % k, aux=NM0) for k in range(2)]      # one read short of -n
                for r in planted:
                    new_offs.append(len(hdr) + len(body))
                    body += r
            stream = np.frombuffer(hdr + body, dtype=np.uint8).copy()
            path = str(d / (kind + ".bam"))
            bamfmt.write_bam_stream(path, stream, level=1, threads=4)
            _FILES[kind] = dict(path=path, stream=stream, offs=np.asarray(new_offs, dtype=np.uint64))
    return _FILES


def host_tracks(res):
    return {k: getattr(res, k).track.cpu().numpy().copy() for k in ("left", "right", "depth")}


def site_rows(sites):
    return list(zip(*(sites[f].tolist() for f in ("contig", "pos", "left", "right", "depth"))))


def test_the_pipeline_in_one_piece_in_several_and_with_forced_flushes(engine, files, monkeypatch):
    """All three give identical tracks and sites: those of the statement over the file's stream.  The depth track is bit-equal to
    pipeline.bam_raw_depth on the same file and options."""
    f = files["hifi"]
    lengths = [l for _, l in CONTIGS]
    sel = np.arange(len(CONTIGS), dtype=np.int32)
    opts = pipeline.CoverOpts()
    want_left, want_right, want_counts, status = R.stream_events(f["stream"], f["offs"], lengths, sel, opts.excl, opts.min_mapq, MIN_CLIP)
    assert status == R.NO_STATUS and (2, 1000) in want_left and (2, 2299) in want_right
    raw = pipeline.bam_raw_depth(engine, [f["path"]], [], opts, 4).track.cpu().numpy().copy()
    want = dict(left=R.track_of(want_left, lengths), right=R.track_of(want_right, lengths), depth=raw)
    want_sites = R.sites_of(want["left"], want["right"], raw, lengths, MIN_READS)
    assert (2, 1000, 4, 0, 4) in want_sites and (2, 2299, 0, 3, 3) in want_sites and not [s for s in want_sites if s[0] == 2 and s[1] in (3000, 4000)]
    pieces, visit = [], pipeline._ClipVisitor.visit
    monkeypatch.setattr(pipeline._ClipVisitor, "visit", lambda self, *a: (pieces.append(a[-1]), visit(self, *a))[1])      # (a[-1]: rec_idx_base)
    whole = (pipeline.GPU_INFLATE_MAX, pipeline.BAM_CHUNK_BYTES)
    for several, budget in ((False, None), (True, None), (True, 1)):
        monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0 if several else whole[0])
        monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", (1 << 20) if several else whole[1])
        del pieces[:]
        res = pipeline.bam_clip_sites(engine, [f["path"]], [], opts, 4, MIN_CLIP, MIN_READS, None, budget)
        assert (len(pieces) > 1) == several and pieces[0] == 0 and sorted(pieces) == pieces, pieces
        assert (res.flushes > 0) == (budget == 1) and res.counts == [want_counts]
        got = host_tracks(res)
        for k in want:
            assert np.array_equal(got[k], want[k]), (several, budget, k)
        assert site_rows(res.sites) == want_sites, (several, budget)
    # regions select sites, not tracks; --chrs selects contigs
    res = pipeline.bam_clip_sites(engine, [f["path"]], [], opts, 4, MIN_CLIP, MIN_READS, [("ctgC", 900, 1001), ("ctgC", 2299, 2299), ("nowhere", 0, 9)])
    assert site_rows(res.sites) == [(2, 1000, 4, 0, 4)] and np.array_equal(host_tracks(res)["right"], want["right"])
    res = pipeline.bam_clip_sites(engine, [f["path"]], ["ctgC"], opts, 4, MIN_CLIP, MIN_READS)
    assert site_rows(res.sites) == [(0, 1000, 4, 0, 4), (0, 2299, 0, 3, 3)] and list(res.left.keys()) == ["ctgC"]
    # supplementary alignments excluded (-G 0x800): the right site goes
    res = pipeline.bam_clip_sites(engine, [f["path"]], ["ctgC"], pipeline.CoverOpts(0x704 | 0x800), 4, MIN_CLIP, MIN_READS)
    assert site_rows(res.sites) == [(0, 1000, 4, 0, 4)]


def test_two_files_add(engine, files):
    paths = [files["hifi"]["path"], files["ont"]["path"]]
    both = pipeline.bam_clip_sites(engine, paths, [], None, 4, 50, 1)
    got, counts = host_tracks(both), both.counts
    alone = [pipeline.bam_clip_sites(engine, [p], [], None, 4, 50, 1) for p in paths]
    parts = [host_tracks(r) for r in alone]
    assert counts == [alone[0].counts[0], alone[1].counts[0]]
    for k in got:
        assert np.array_equal(got[k], parts[0][k] + parts[1][k]), k
    assert int(got["left"].sum()) == counts[0][1] + counts[1][1] and int(got["right"].sum()) == counts[0][2] + counts[1][2]
    assert site_rows(both.sites) == R.sites_of(got["left"], got["right"], got["depth"], [l for _, l in CONTIGS], 1)


def test_command_line(engine, files, tmp_path):
    out = str(tmp_path)
    f = files["hifi"]
    r = _run("clip_sites.py", ["-d", out, "-o", "s", "-t", "4", f["path"]], dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["s.clip.left.depth.gz", "s.clip.right.depth.gz", "s.clip.sites.bed", "s.clip.txt"]
    res = pipeline.bam_clip_sites(engine, [f["path"]], [], None, 4)
    want = host_tracks(res)
    lengths = dict(CONTIGS)
    for side in ("left", "right"):
        tracks, got_lengths = pipeline.read_depth_tracks(engine, os.path.join(out, "s.clip.%s.depth.gz" % side))
        assert dict(got_lengths) == lengths and np.array_equal(tracks.track.cpu().numpy(), want[side]), side
    bed = os.path.join(out, "s.clip.sites.bed")
    assert open(bed).read() == pipeline.clip_sites_bed(res.sites, [n for n, _ in CONTIGS])
    assert "ctgC\t1000\t1001\t4\t0\t4\n" in open(bed).read() and "ctgC\t2299\t2300\t0\t3\t3\n" in open(bed).read()
    text = open(os.path.join(out, "s.clip.txt")).read()
    assert text == pipeline.clip_summary_text([f["path"]], res.counts, int(res.sites.shape[0]),
                                              [("min_clip", 100), ("min_reads", 3), ("excl_flags", "0x704"), ("min_mapq", 0), ("count_del", 0),
                                               ("chrs", "."), ("regions", ".")])
    # filter_reads.py -R on the written BED lists, for the planted sites, exactly the planted reads
    r = _run("filter_reads.py", ["-d", out, "-o", "fr", "-t", "4", "-R", bed, f["path"]])
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split("\t") for ln in open(os.path.join(out, "fr.reads.tsv")) if not ln.startswith("#")]
    on_c = [(row[1], int(row[3])) for row in rows if row[2] == "ctgC"]
    assert sorted(n for n, start in on_c if start == 1000) == PLANTED_LEFT and sorted(n for n, start in on_c if start == 2000) == PLANTED_RIGHT
    assert len(on_c) == len(PLANTED_LEFT) + len(PLANTED_RIGHT)
    r = _run("clip_sites.py", ["-d", out, "-o", "s", f["path"]])                # a second run without -f refuses
    assert r.returncode != 0 and r.stderr.strip().split("\n")[-1] == 'Please use "-f" or "--force" to rewrite'
    # a malformed record: bam_depth.py's message, and no output
    n = int(f["offs"].shape[0])
    stream = np.concatenate([f["stream"], np.frombuffer(rec(0, 5, [(M, 4), (9, 3)]), dtype=np.uint8)])
    path = str(tmp_path / "op9.bam")
    bamfmt.write_bam_stream(path, stream, level=1, threads=2)
    r = _run("clip_sites.py", ["-d", out, "-o", "bad", path])
    assert r.returncode != 0 and "Traceback" not in r.stderr
    assert r.stderr.strip().split("\n")[-1] == 'ERROR!!! The file "%s" holds a malformed BAM record (record %d)' % (path, n)
    assert not [x for x in os.listdir(out) if x.startswith("bad.")]
