"""bam_depth.py on the GPU: gci_bam_cover_size / _write (k_cover.hip) against the statement of tests/cover_ref.py on every case of
tests/cover_cases.py in both stream forms -- the intervals written into a 0xA5-filled buffer whose bytes behind them must stay --,
gci_track_add against numpy, pipeline.bam_raw_depth with a tiny interval budget, and the command line over small synthetic HiFi and
ONT files in every ingest mode against what convert_samtools_depth.py writes from the statement's depths."""
import ctypes
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import cover_cases as C
import cover_ref as R
from gci_amd import _lib, pipeline, synth
from gci_amd.device import IVL_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 5                                                # guard intervals behind the output


def device_cover(engine, c, stream, offs, has_seq, run):
    """-> (depths per contig, status word, intervals): the two exports as they are, the output 0xA5-filled with PAD intervals behind
    it that must stay so, built with gci_depth_build at flank 0."""
    engine.set_layout(c["lengths"])
    d_stream, d_off, d_sel = engine.to_device(stream), engine.to_device(offs), engine.to_device(c["ref_sel"])
    n, n_rec = ctypes.c_uint64(0), int(offs.shape[0])
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    args = (engine.ctx, engine._p(d_stream), int(stream.shape[0]), engine._p(d_off) if n_rec else None, n_rec, int(has_seq))
    assert engine.lib.gci_bam_cover_size(*args, engine._p(d_sel), int(d_sel.shape[0]), run[0], run[1], int(run[2]), ctypes.byref(n),
                                         engine._p(status)) == 0
    size_status = int(status.item()) & (2 ** 64 - 1)
    total = int(n.value)
    out = engine.T.empty((total + PAD, 4), engine.T.int32, engine.device)
    assert engine.lib.gci_memset(engine.ctx, engine._p(out), 0xA5, (total + PAD) * 16) == 0
    assert engine.lib.gci_bam_cover_write(*args, engine._p(out), total, engine._p(status)) == 0
    engine.sync()
    assert int(status.item()) & (2 ** 64 - 1) == size_status
    h = out.cpu().numpy()
    assert (h[total:].view(np.uint8) == 0xA5).all(), "intervals behind the output were written"
    track = engine.new_track()
    engine.depth_build(out[:total], None, 0, track)
    host = track.cpu().numpy()
    depths = [host[o:o + L].astype(np.int64) for o, L in zip(engine.offsets, c["lengths"])]
    return depths, size_status, np.ascontiguousarray(h[:total]).view(IVL_DTYPE).reshape(-1)


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name, run", C.pairs())
def test_the_device_equals_the_statement(engine, name, run, form):
    c = C.case(name)
    stream, offs = (c["stream"], c["offs"]) if form == "stream" else C.heads(name)
    want, want_status = C.want(name, run)
    got, status, ivl = device_cover(engine, c, stream, offs, form == "stream", run)
    assert status == want_status                       # a malformed record is an answer in the status word
    if name in C.MALFORMED:
        return
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    L = np.asarray(c["lengths"], dtype=np.int64)[ivl["contig"]] if ivl.shape[0] else np.zeros(0, np.int64)
    inside = np.maximum(np.minimum(ivl["end"].astype(np.int64) + 1, L) - ivl["start"].astype(np.int64), 0)
    assert int(inside.sum()) == sum(int(w.sum()) for w in want)                  # the covered-base total, interval by interval
    assert (ivl["contig"] >= 0).all() and (ivl["start"] >= 0).all() and (ivl["end"] >= ivl["start"]).all() and (ivl["pad"] == 0).all()


def test_the_device_gives_the_hand_written_depths(engine):
    c = C.case("sam_spec")
    assert np.array_equal(device_cover(engine, c, c["stream"], c["offs"], True, C.PLAIN)[0][0], C.SAM_SPEC_DEPTH)
    assert np.array_equal(device_cover(engine, c, c["stream"], c["offs"], True, C.WITH_DEL)[0][0], C.SAM_SPEC_DEPTH_J)


def test_a_malformed_record_raises_with_its_index(engine):
    c = C.case("op9")
    engine.set_layout(c["lengths"])
    with pytest.raises(_lib.GciError) as e:
        engine.bam_cover(engine.to_device(c["stream"]), engine.to_device(c["offs"]), True, engine.to_device(c["ref_sel"]))
    assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == 3


def test_argument_errors(engine):
    c = C.case("sam_spec")
    engine.set_layout(c["lengths"])
    d_stream, d_off, d_sel = engine.to_device(c["stream"]), engine.to_device(c["offs"]), engine.to_device(c["ref_sel"])
    n, n_rec = ctypes.c_uint64(0), int(c["offs"].shape[0])
    args = (engine.ctx, engine._p(d_stream), int(c["stream"].shape[0]), engine._p(d_off), n_rec, 1)
    out = engine.T.zeros((64, 4), engine.T.int32, engine.device)
    st = engine._p(engine._status)
    assert engine.lib.gci_bam_cover_size(*args, engine._p(d_sel), 1, 0x704, 0, 0, None, st) == _lib.GCI_E_INVALID
    assert engine.lib.gci_bam_cover_size(*args, engine._p(d_sel), 1, 0x704, 0, 0, ctypes.byref(n), None) == _lib.GCI_E_INVALID
    assert engine.lib.gci_bam_cover_write(*args, engine._p(out), 64, st) == _lib.GCI_E_INVALID         # no size call in front of it
    assert engine.lib.gci_bam_cover_size(*args, engine._p(d_sel), 1, 0x704, 0, 0, ctypes.byref(n), st) == 0 and n.value > 1
    assert engine.lib.gci_bam_cover_write(*args[:4], n_rec - 1, 1, engine._p(out), 64, st) == _lib.GCI_E_INVALID
    assert engine.lib.gci_bam_cover_write(*args, engine._p(out), n.value - 1, st) == _lib.GCI_E_CAPACITY
    engine.sync()
    assert not out.cpu().numpy().any()                                                                  # ... and nothing was written
    assert engine.lib.gci_track_add(engine.ctx, None, engine._p(out)) == _lib.GCI_E_INVALID
    from gci_amd.device import Engine
    fresh = Engine(0)
    assert fresh.lib.gci_track_add(fresh.ctx, engine._p(out), engine._p(out)) == _lib.GCI_E_NO_LAYOUT
    assert fresh.lib.gci_bam_cover_size(fresh.ctx, *args[1:], engine._p(d_sel), 1, 0x704, 0, 0, ctypes.byref(n), st) == _lib.GCI_E_NO_LAYOUT
    fresh.close()


def test_track_add(engine):
    engine.set_layout([1, 4095, 4096, 4097])
    rng = np.random.default_rng(5)
    a, b = (rng.integers(-1000, 1000, engine.total).astype(np.int32) for _ in range(2))
    d_a, d_b = engine.to_device(a), engine.to_device(b)
    engine.track_add(d_a, d_b)
    engine.sync()
    assert np.array_equal(d_a.cpu().numpy(), a + b) and np.array_equal(d_b.cpu().numpy(), b)
    # whole, 16-byte aligned tracks only: a pointer one element into a buffer is refused and nothing is added
    big = engine.T.zeros(engine.total + 4, engine.T.int32, engine.device)
    assert engine.lib.gci_track_add(engine.ctx, engine._p(big[1:]), engine._p(d_b)) == _lib.GCI_E_INVALID
    assert engine.lib.gci_track_add(engine.ctx, engine._p(d_a), engine._p(big[1:])) == _lib.GCI_E_INVALID
    engine.sync()
    assert not big.cpu().numpy().any() and np.array_equal(d_a.cpu().numpy(), a + b)


def test_a_pass_that_starts_over_discards_the_one_before(engine):
    """The visitor's rule for a file whose device walk gives up part-way (the next ingest path reads it again from record 0)."""
    c = C.case("operations")
    engine.set_layout(c["lengths"])
    v = pipeline._CoverVisitor(engine, pipeline.CoverOpts(), 4)             # (a budget the first call exceeds: a flushed track is dropped too)
    d = engine.to_device(c["stream"]), engine.to_device(c["offs"]), True, engine.to_device(c["ref_sel"])
    v.begin_file()
    assert v(engine, *d, 0).recs.shape[0] == 0 and v.track is not None
    v(engine, *d, 0)
    track = v.file_done().cpu().numpy()
    assert np.array_equal(track[:c["lengths"][0]], C.want("operations", C.PLAIN)[0][0])


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctgA", 600_000), ("ctgB", 400_000))
KINDS = {"hifi": dict(coverage=4, seed=11), "ont": dict(coverage=4, seed=12, long_cigar_frac=0.05)}
MODES = {"gpu": dict(GCI_BAM_INGEST="gpu"),
         "gpu_runs": dict(GCI_BAM_INGEST="gpu", GCI_GPU_INFLATE_MAX=str(1 << 16), GCI_BAM_CHUNK_BYTES=str(1 << 20)),
         "heads": dict(GCI_BAM_INGEST="heads"),
         "full": dict(GCI_BAM_INGEST="full"),
         "full_chunks": dict(GCI_BAM_INGEST="full", GCI_BAM_CHUNK_BYTES="700000")}
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per kind: the BAM file, the statement's depths of its stream, and the text of the .depth.gz convert_samtools_depth.py writes from
    synth.samtools_depth_text of those depths.  Made once."""
    if not _FILES:
        d = tmp_path_factory.mktemp("cover")
        for kind, kw in KINDS.items():
            rs = synth.simulate_reads(CONTIGS, kw["coverage"], kind, seed=kw["seed"], **{k: v for k, v in kw.items() if k == "long_cigar_frac"}).sorted()
            stream, offs = synth.to_bam_stream(rs)
            path = str(d / (kind + ".bam"))
            bamfmt.write_bam_stream(path, stream, level=1, threads=4)
            want, status = R.stream_depth(stream, offs, [l for _, l in CONTIGS], np.arange(len(CONTIGS), dtype=np.int32))
            assert status == R.NO_STATUS and sum(int(w.sum()) for w in want) > 0
            text = str(d / (kind + ".samtools.depth"))
            synth.samtools_depth_text([(n, w) for (n, _), w in zip(CONTIGS, want)]).tofile(text)
            r = _run("convert_samtools_depth.py", [text, str(d / (kind + "_converted"))])
            assert r.returncode == 0, r.stderr[-2000:]
            with gzip.open(str(d / (kind + "_converted.depth.gz")), "rb") as f:
                _FILES[kind] = dict(path=path, want=want, text=f.read(), n_ops=int(np.diff(rs.cigar_off).max()))
        _FILES["dir"] = d
    return _FILES


def test_the_files_hold_what_the_modes_need(files):
    assert files["ont"]["n_ops"] > 65535 and files["hifi"]["n_ops"] < 65535     # the CG:B,I placeholder travels through every mode


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_command_line_in_every_ingest_mode(engine, files, kind, mode):
    f, out = files[kind], str(files["dir"])
    r = _run("bam_depth.py", ["-d", out, "-o", "%s_%s" % (kind, mode), "-t", "4", f["path"]], dict(MODES[mode], GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    path = os.path.join(out, "%s_%s.depth.gz" % (kind, mode))
    with gzip.open(path, "rb") as g:
        assert g.read() == f["text"]
    if mode == "gpu":                                  # ... and back through the project's own reader, in the compressed domain
        tracks, lengths = pipeline.read_depth_tracks(engine, path)
        assert lengths == dict(CONTIGS)
        for (name, _), w in zip(CONTIGS, f["want"]):
            assert np.array_equal(tracks[name], w)


def test_a_tiny_interval_budget_changes_nothing(engine, files, monkeypatch):
    f = files["ont"]
    whole = pipeline.bam_raw_depth(engine, [f["path"]], threads=4)
    assert whole.cover_flushes == 0
    for (name, _), w in zip(CONTIGS, f["want"]):
        assert np.array_equal(whole[name], w)
    few = pipeline.bam_raw_depth(engine, [f["path"]], threads=4, ivl_budget=64)
    assert few.cover_flushes == 1
    monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0)
    monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", 1 << 20)
    runs = pipeline.bam_raw_depth(engine, [f["path"]], threads=4, ivl_budget=64)          # run by run: the walk engine flushes
    assert runs.cover_flushes > 2
    for (name, _), w in zip(CONTIGS, f["want"]):
        assert np.array_equal(few[name], w) and np.array_equal(runs[name], w)


def test_two_files_add_chrs_select_and_another_sq_table_is_refused(engine, files, tmp_path):
    paths = [files["hifi"]["path"], files["ont"]["path"]]
    both = pipeline.bam_raw_depth(engine, paths, threads=4)
    for k, (name, _) in enumerate(CONTIGS):
        assert np.array_equal(both[name], files["hifi"]["want"][k] + files["ont"]["want"][k])
    only = pipeline.bam_raw_depth(engine, paths, chrs=["ctgB"], opts=pipeline.CoverOpts(), threads=4, ivl_budget=1000)
    assert list(only.keys()) == ["ctgB"] and np.array_equal(only["ctgB"], files["hifi"]["want"][1] + files["ont"]["want"][1])
    other = str(tmp_path / "other.bam")
    bamfmt.write_bam(other, ["ctgA", "ctgB"], [600_000, 400_001], [])
    with pytest.raises(pipeline.SqMismatch):
        pipeline.bam_raw_depth(engine, [paths[0], other])
    r = _run("bam_depth.py", ["-d", str(tmp_path), paths[0], other])
    assert r.returncode != 0 and "Traceback" not in r.stderr
    assert r.stderr.strip().split("\n")[-1] == 'ERROR!!! The @SQ table of "%s" differs from that of "%s"' % (other, paths[0])


def test_command_line_chrs_and_a_file_without_records(files, tmp_path):
    out = str(tmp_path)
    r = _run("bam_depth.py", ["-d", out, "-o", "b", "--chrs", "ctgB", files["hifi"]["path"], files["ont"]["path"]])
    assert r.returncode == 0, r.stderr[-2000:]
    want = pipeline_text([("ctgB", files["hifi"]["want"][1] + files["ont"]["want"][1])])
    with gzip.open(os.path.join(out, "b.depth.gz"), "rb") as g:
        assert g.read() == want
    empty = str(tmp_path / "empty.bam")                 # a header and no record: every base of every contig at depth 0
    bamfmt.write_bam(empty, ["e1", "e2"], [5000, 1], [])
    for mode in ("gpu", "heads", "full"):
        r = _run("bam_depth.py", ["-f", "-d", out, "-o", "e", empty], MODES[mode])
        assert r.returncode == 0, (mode, r.stderr[-2000:])
        with gzip.open(os.path.join(out, "e.depth.gz"), "rb") as g:
            assert g.read() == b">e1\n" + b"0\n" * 5000 + b">e2\n0\n", mode


def pipeline_text(items):
    """The payload of a .depth.gz: '>name' then one decimal per line."""
    return b"".join(b">" + n.encode() + b"\n" + b"".join(b"%d\n" % v for v in d.tolist()) for n, d in items)


def test_a_malformed_record_is_named_by_its_index_in_the_file(engine, tmp_path, monkeypatch):
    """Whole and run by run: GciError.rec and the message agree on the record of the FILE; the command line says it in one line."""
    c = C.case("scan_blocks")
    n = int(c["offs"].shape[0])
    stream = np.concatenate([c["stream"], np.frombuffer(C.rec(0, 5, [(C.M, 4), (9, 3)]), dtype=np.uint8)])
    path = str(tmp_path / "op9.bam")
    bamfmt.write_bam_stream(path, stream, level=1, threads=2)
    from gci_amd import hostio
    pos, isz = hostio.bgzf_blocks(np.fromfile(path, dtype=np.uint8))
    assert len(pipeline._Members(engine, 1 << 17, pos, isz).run_bytes()) >= 3         # not vacuous: the record lies behind several runs
    for knobs in ({}, {"GPU_INFLATE_MAX": 0, "BAM_CHUNK_BYTES": 1 << 17}):
        with monkeypatch.context() as m:
            for k, v in knobs.items():
                m.setattr(pipeline, k, v)
            with pytest.raises(_lib.GciError) as e:
                pipeline.bam_raw_depth(engine, [path], threads=2)
        assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == n and "(record %d of the file)" % n in str(e.value), knobs
    r = _run("bam_depth.py", ["-d", str(tmp_path), path])
    assert r.returncode != 0 and "Traceback" not in r.stderr
    assert r.stderr.strip().split("\n")[-1] == 'ERROR!!! The file "%s" holds a malformed BAM record (record %d)' % (path, n)


def test_the_output_feeds_the_depth_tools_without_conversion(files, tmp_path):
    """depth_dist.py and plot_depth.py read bam_depth.py's file as they read GCI.py's."""
    out = str(tmp_path)
    r = _run("bam_depth.py", ["-d", out, "-o", "raw", "-J", "-Q", "1", files["hifi"]["path"]])
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run("depth_dist.py", [os.path.join(out, "raw.depth.gz"), os.path.join(out, "raw")])
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split("\t") for ln in open(os.path.join(out, "raw.depth.summary.txt")).read().splitlines()]
    assert [row[0] for row in rows[1:]] == ["ctgA", "ctgB", "total"] and [int(row[3]) for row in rows[1:]] == [600_000, 400_000, 1_000_000]
    mean = rows[-1][5]                                 # (the `total` row's mean is the -dmean plot_depth.py asks for)
    r = _run("plot_depth.py", ["-r", _fai(tmp_path), "--hifi", os.path.join(out, "raw.depth.gz"), "-dmean", mean, "-d", out, "-o", "rawplot"])
    assert r.returncode == 0, r.stderr[-2000:]


def _fai(tmp_path):
    p = str(tmp_path / "ref.fa")
    synth.write_reference_fasta(p, CONTIGS)
    return p
