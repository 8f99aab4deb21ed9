"""filter_depth.py on the GPU: gci_bam_fate (k_fate.hip) against the statement of tests/fate_ref.py on every case of
tests/fate_cases.py in both stream forms -- classes, counts, status word -- and against gci_bam_filter on the same buffers; the
per-class depth through gci_bam_cover_size_sel + gci_depth_build; pipeline.bam_filter_depth with a tiny interval budget over small
synthetic HiFi and ONT files; and the command line once."""
import ctypes
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import cover_cases as C
import fate_cases as FC
import fate_ref as F
from gci_amd import _lib, pipeline, synth
from gci_amd.device import IVL_DTYPE, REC_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64                                               # guard bytes behind the class bytes
U64 = 2 ** 64 - 1


def form_of(name, form):
    c = FC.case(name)
    return (c["stream"], c["offs"]) if form == "stream" else FC.heads(name)


@pytest.fixture(scope="module")
def on_device(engine):
    """The buffers of every (case, form), uploaded once."""
    cache = {}

    def get(name, form):
        if (name, form) not in cache:
            stream, offs = form_of(name, form)
            cache[(name, form)] = (engine.to_device(stream), engine.to_device(offs), engine.to_device(FC.case(name)["ref_sel"]), int(stream.shape[0]),
                                   int(offs.shape[0]))
        return cache[(name, form)]
    return get


def device_fate(engine, bufs, has_seq, run):
    """-> (classes, counts, status word): the export as it is, the class bytes 0xA5-filled with PAD bytes behind them that must stay."""
    d_stream, d_off, d_sel, n_bytes, n_rec = bufs
    cls = engine.T.empty(n_rec + PAD, engine.T.uint8, engine.device)
    assert engine.lib.gci_memset(engine.ctx, engine._p(cls), 0xA5, n_rec + PAD) == 0
    counts = (ctypes.c_uint64 * 8)(*([7] * 8))
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    assert engine.lib.gci_bam_fate(engine.ctx, engine._p(d_stream), n_bytes, engine._p(d_off) if n_rec else None, n_rec, int(has_seq), engine._p(d_sel),
                                   int(d_sel.shape[0]), run[0], run[1], run[2], engine._p(cls), counts, engine._p(status)) == 0
    h = cls.cpu().numpy()
    assert (h[n_rec:] == 0xA5).all(), "bytes behind the classes were written"
    return h[:n_rec], np.array(list(counts), dtype=np.uint64), int(status.item()) & U64


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name, run", FC.pairs())
def test_the_device_gives_the_classes_of_the_statement(engine, on_device, name, run, form):
    want_cls, want_counts, want_status = FC.want(name, run)
    cls, counts, status = device_fate(engine, on_device(name, form), form == "stream", run)
    assert status == want_status
    assert np.array_equal(cls, want_cls), np.flatnonzero(cls != want_cls)[:10]
    assert np.array_equal(counts, want_counts)


@pytest.mark.parametrize("form", ["stream", "heads"])
def test_the_device_on_and_around_every_quotient(engine, on_device, form):
    """Thresholds on, one ulp beside and +- 1e-7 .. 1e-3 around every record's two f64 quotients: inside and outside the band in which
    ratio_cmp lets single precision decide."""
    bufs, seen = on_device("threshold_band", form), set()
    for run in FC.case("threshold_band")["runs"]:
        want_cls, want_counts, want_status = FC.want("threshold_band", run)
        cls, counts, status = device_fate(engine, bufs, form == "stream", run)
        assert status == want_status == F.NO_STATUS
        assert np.array_equal(cls, want_cls) and np.array_equal(counts, want_counts), run
        seen |= set(cls.tolist())
    assert seen == {F.CLIP, F.IDENTITY, F.KEPT}


@pytest.mark.parametrize("name", FC.NAMES)
def test_kept_is_the_filters_pass_and_the_status_word_is_the_filters(engine, on_device, name):
    """gci_bam_filter on the same buffers and thresholds (it reads whole streams only).  none_op9 holds records with pos = -1 and no NM:
    the filter meets them, the classes do not (include/gci_hip.h)."""
    d_stream, d_off, d_sel, _, n_rec = bufs = on_device(name, "stream")
    runs = FC.case(name)["runs"]
    for run in (runs if name != "threshold_band" else runs[::5]):
        recs = engine.bam_filter(d_stream, d_off, d_sel, run[0], 50, run[1], run[2], check=False)
        filter_status = int(engine._status.item()) & U64
        passed = (np.ascontiguousarray(recs.cpu().numpy()).view(REC_DTYPE).reshape(-1)["flags"][:n_rec] & _lib.REC_PASS) != 0
        cls, counts, status = device_fate(engine, bufs, True, run)
        assert np.array_equal(cls == F.KEPT, passed), run
        assert int(counts[F.KEPT]) == int(passed.sum())
        if name != "none_op9":
            assert status == filter_status, run


def test_a_status_raises_with_its_record(engine, on_device):
    d_stream, d_off, d_sel, _, _ = on_device("zero_div_identity", "stream")
    with pytest.raises(_lib.GciError) as e:
        engine.bam_fate(d_stream, d_off, True, d_sel, *FC.case("zero_div_identity")["runs"][0])
    assert e.value.status == _lib.GCI_E_ZERO_DIV and e.value.rec == 2


def device_class_depth(engine, c, bufs, has_seq, d_cls, mask, count_del, excl=0):
    """-> (depths per contig, intervals) of gci_bam_cover_size_sel + gci_bam_cover_write + gci_depth_build at flank 0."""
    d_stream, d_off, d_sel, n_bytes, n_rec = bufs
    n, status = ctypes.c_uint64(0), engine.T.zeros(1, engine.T.int64, engine.device)
    args = (engine.ctx, engine._p(d_stream), n_bytes, engine._p(d_off) if n_rec else None, n_rec, int(has_seq))
    assert engine.lib.gci_bam_cover_size_sel(*args, engine._p(d_sel), int(d_sel.shape[0]), excl, 0, int(count_del), None if d_cls is None else engine._p(d_cls),
                                             mask, ctypes.byref(n), engine._p(status)) == 0
    total = int(n.value)
    out = engine.T.empty((total + 4, 4), engine.T.int32, engine.device)
    assert engine.lib.gci_memset(engine.ctx, engine._p(out), 0xA5, (total + 4) * 16) == 0
    assert engine.lib.gci_bam_cover_write(*args, engine._p(out), total, engine._p(status)) == 0
    h = out.cpu().numpy()
    assert (h[total:].view(np.uint8) == 0xA5).all(), "intervals behind the output were written"
    track = engine.new_track()
    engine.depth_build(out[:total], None, 0, track)
    host = track.cpu().numpy()
    ivl = np.ascontiguousarray(h[:total]).view(IVL_DTYPE).reshape(-1)
    return [host[o:o + L].astype(np.int64) for o, L in zip(engine.offsets, c["lengths"])], ivl


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name, run", FC.depth_pairs())
def test_the_selected_cover_gives_the_depth_of_every_class(engine, on_device, name, run, form):
    """With the class bytes the device itself wrote; every class with and without deletions; all classes at once against the call
    without classes (the same multiset of intervals)."""
    c, bufs = FC.case(name), on_device(name, form)
    engine.set_layout(c["lengths"])
    d_cls, _ = engine.bam_fate(bufs[0], bufs[1], form == "stream", bufs[2], *run, check=False)
    n_ivl = 0
    for k in range(1, _lib.FATE_CLASSES):
        for count_del in (False, True):
            got, ivl = device_class_depth(engine, c, bufs, form == "stream", d_cls, 1 << k, count_del)
            for j, w in enumerate(FC.want_depth(name, run, k, count_del)):
                assert np.array_equal(got[j], w), (k, count_del, j)
        n_ivl += ivl.shape[0]
    order = list(IVL_DTYPE.names)
    every = device_class_depth(engine, c, bufs, form == "stream", d_cls, 0xFE, True, excl=0x4)[1]
    plain = device_class_depth(engine, c, bufs, form == "stream", None, 0, True, excl=0x4)[1]
    assert every.shape[0] == plain.shape[0] == n_ivl and np.array_equal(np.sort(every, order=order), np.sort(plain, order=order))
    assert device_class_depth(engine, c, bufs, form == "stream", d_cls, 0, True)[1].shape[0] == 0


def test_argument_errors(engine, on_device):
    d_stream, d_off, d_sel, n_bytes, n_rec = on_device("one_per_class", "stream")
    cls = engine.T.zeros(n_rec, engine.T.uint8, engine.device)
    counts, n, st = (ctypes.c_uint64 * 8)(), ctypes.c_uint64(0), engine._p(engine._status)
    head = (engine._p(d_stream), n_bytes, engine._p(d_off), n_rec, 1, engine._p(d_sel), int(d_sel.shape[0]))
    lib = engine.lib
    assert lib.gci_bam_fate(engine.ctx, *head, 30, 0.1, 0.9, None, counts, st) == _lib.GCI_E_INVALID
    assert lib.gci_bam_fate(engine.ctx, *head, 30, 0.1, 0.9, engine._p(cls), None, st) == _lib.GCI_E_INVALID
    assert lib.gci_bam_fate(engine.ctx, *head, 30, 0.1, 0.9, engine._p(cls), counts, None) == _lib.GCI_E_INVALID
    assert lib.gci_bam_fate(None, *head, 30, 0.1, 0.9, engine._p(cls), counts, st) == _lib.GCI_E_INVALID
    engine.set_layout(FC.case("one_per_class")["lengths"])
    assert lib.gci_bam_cover_size_sel(engine.ctx, *head, 0, 0, 0, engine._p(cls), 1, None, st) == _lib.GCI_E_INVALID
    assert lib.gci_bam_cover_size_sel(engine.ctx, *head, 0, 0, 0, engine._p(cls), 1, ctypes.byref(n), None) == _lib.GCI_E_INVALID
    from gci_amd.device import Engine
    fresh = Engine(0)
    assert fresh.lib.gci_bam_cover_size_sel(fresh.ctx, *head, 0, 0, 0, engine._p(cls), 1, ctypes.byref(n), st) == _lib.GCI_E_NO_LAYOUT
    assert fresh.lib.gci_bam_fate(fresh.ctx, *head, 30, 0.1, 0.9, engine._p(cls), counts, st) == 0                  # the classes need no layout
    assert list(counts) == FC.want("one_per_class", FC.DEFAULT)[1].tolist()
    fresh.close()


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctgA", 600_000), ("ctgB", 400_000))
KINDS = {"hifi": dict(coverage=4, seed=21, filt=(30, 0.1, 0.995)), "ont": dict(coverage=4, seed=22, long_cigar_frac=0.05, filt=(30, 0.1, 0.9))}
FILT = (30, 0.1, 0.9)                                   # the command line's defaults; `filt` above: thresholds at which every class occurs
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per kind: the BAM file (BGZF) of a few hundred synthetic records, its stream and record offsets.  Made once."""
    if not _FILES:
        d = tmp_path_factory.mktemp("fate")
        for kind, kw in KINDS.items():
            rs = synth.simulate_reads(CONTIGS, kw["coverage"], kind, seed=kw["seed"], **{k: v for k, v in kw.items() if k == "long_cigar_frac"}).sorted()
            stream, offs = synth.to_bam_stream(rs)
            path = str(d / (kind + ".bam"))
            bamfmt.write_bam_stream(path, stream, level=1, threads=4)
            _FILES[kind] = dict(path=path, stream=stream, offs=offs)
        _FILES["dir"] = d
    return _FILES


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_pipeline_with_a_tiny_interval_budget(engine, files, kind, monkeypatch):
    """The six tracks add up exactly to bam_raw_depth with excl = 0x4, the record counts are the statement's, `kept` is the filter's PASS
    count; a budget of a few dozen intervals makes the collectors build in parts -- whole, and run by run on the walk engine, where
    later parts are added to a class's track."""
    f, filt = files[kind], KINDS[kind]["filt"]
    sel = np.arange(len(CONTIGS), dtype=np.int32)
    want_cls, want_counts, want_status = F.stream_classes(f["stream"], f["offs"], sel, *filt)
    assert want_status == F.NO_STATUS and (want_counts[1:7] > 0).all(), want_counts
    for count_del in (False, True):
        if count_del:
            monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0)
            monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", 1 << 20)
        res = pipeline.bam_filter_depth(engine, [f["path"]], [], pipeline.FateOpts(*filt, count_del), 4, pipeline.FATE_WANTED, ivl_budget=48)
        assert res.flushes > (len(pipeline.FATE_WANTED) if count_del else 0)
        assert res.counts == [[int(x) for x in want_counts]]
        raw = pipeline.bam_raw_depth(engine, [f["path"]], opts=pipeline.CoverOpts(0x4, 0, count_del), threads=4)
        lengths = [l for _, l in CONTIGS]
        for j, (name, _) in enumerate(CONTIGS):
            total = sum(res.tracks[c][name].astype(np.int64) for c in pipeline.FATE_WANTED)
            assert np.array_equal(total, raw[name])
            for c in pipeline.FATE_WANTED:
                want = F.class_depth(f["stream"], f["offs"], lengths, sel, want_cls, F.NAMES.index(c), count_del)[j]
                assert np.array_equal(res.tracks[c][name], want), (c, name)
    d_sel = engine.to_device(sel)
    recs = engine.bam_filter(engine.to_device(f["stream"]), engine.to_device(f["offs"]), d_sel, filt[0], 50, filt[1], filt[2])
    passed = int((np.ascontiguousarray(recs.cpu().numpy()).view(REC_DTYPE).reshape(-1)["flags"] & _lib.REC_PASS != 0).sum())
    assert res.counts[0][F.KEPT] == passed


def test_two_files_add_per_class_and_chrs_select(engine, files):
    paths = [files["hifi"]["path"], files["ont"]["path"]]
    one = [pipeline.bam_filter_depth(engine, [p], ["ctgB"], None, 4, ["clip", "kept"], ivl_budget=1000) for p in paths]
    both = pipeline.bam_filter_depth(engine, paths, ["ctgB"], None, 4, ["clip", "kept"])
    assert both.counts == one[0].counts + one[1].counts and list(both.tracks) == ["clip", "kept"]
    for c in ("clip", "kept"):
        assert list(both.tracks[c].keys()) == ["ctgB"]
        assert np.array_equal(both.tracks[c]["ctgB"], one[0].tracks[c]["ctgB"] + one[1].tracks[c]["ctgB"])


def test_tracks_that_do_not_fit_are_refused_before_anything_is_read(engine, files, monkeypatch):
    monkeypatch.setattr(pipeline, "device_memory_free", lambda e: 7 * 4 * 1_000_000 - 1)
    monkeypatch.setattr(pipeline, "bam_join_input", lambda *a, **k: pytest.fail("a file was read"))
    with pytest.raises(pipeline.TracksDoNotFit) as e:
        pipeline.bam_filter_depth(engine, [files["hifi"]["path"]], [], None, 1, pipeline.FATE_WANTED)
    assert e.value.n_tracks == 7 and e.value.track_bytes >= 4 * 1_000_000


def test_command_line(files, tmp_path):
    out = str(tmp_path)
    argv = ["-d", out, "-o", "x", "-t", "4", "-J", files["hifi"]["path"], files["ont"]["path"]]
    r = _run("filter_depth.py", argv, dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    sums = {}
    for c in pipeline.FATE_WANTED:
        with gzip.open(os.path.join(out, "x.%s.depth.gz" % c), "rb") as g:
            lines = g.read().split(b"\n")
        assert lines[-1] == b"" and lines[0] == b">ctgA" and lines[600_001] == b">ctgB" and len(lines) == 1_000_003
        a, b = np.array(lines[1:600_001], dtype="S").astype(np.int64), np.array(lines[600_002:-1], dtype="S").astype(np.int64)
        sums[c] = [int(a.sum()), int(b.sum()), int(a.sum() + b.sum())]
    rows = [ln.split("\t") for ln in open(os.path.join(out, "x.filter.txt")).read().splitlines()]
    assert rows[0] == ["#records"] and rows[1] == ["file"] + list(F.NAMES[:7]) and [r[0] for r in rows[2:4]] == argv[-2:]
    sel = np.arange(len(CONTIGS), dtype=np.int32)
    for row, kind in zip(rows[2:4], ("hifi", "ont")):
        assert [int(x) for x in row[1:]] == F.stream_classes(files[kind]["stream"], files[kind]["offs"], sel, *FILT)[1][:7].tolist()
    assert rows[4] == ["#covered_bases"] and rows[5] == ["contig"] + list(pipeline.FATE_WANTED) and [r[0] for r in rows[6:]] == ["ctgA", "ctgB", "total"]
    for k, row in enumerate(rows[6:]):
        assert [int(x) for x in row[1:]] == [sums[c][k] for c in pipeline.FATE_WANTED]
    assert sum(sums[c][2] for c in pipeline.FATE_WANTED) > 0
    # a second run without -f refuses; the output feeds depth_dist.py as GCI.py's does
    r = _run("filter_depth.py", argv)
    assert r.returncode != 0 and r.stderr.strip().split("\n")[-2:] == ['ERROR!!! The file "%s/x.secondary.depth.gz" exists' % out,
                                                                       'Please use "-f" or "--force" to rewrite']
    r = _run("depth_dist.py", [os.path.join(out, "x.mapq.depth.gz"), os.path.join(out, "x.mapq")])
    assert r.returncode == 0, r.stderr[-2000:]


def test_command_line_names_the_record_without_nm(tmp_path):
    c = FC.case("scan_blocks")
    ok = np.flatnonzero(FC.want("scan_blocks", FC.DEFAULT)[0] != F.ERROR)
    offs = list(c["offs"].tolist()) + [int(c["stream"].shape[0])]
    blob = c["stream"][:offs[0]].tobytes() + b"".join(c["stream"][offs[i]:offs[i + 1]].tobytes() for i in ok.tolist())
    blob += C.rec(0, 5, [(C.S, 30), (C.M, 10)])                                    # clipped, and no NM: KeyError in the reference
    path = str(tmp_path / "no_nm.bam")
    bamfmt.write_bam_stream(path, np.frombuffer(blob, dtype=np.uint8), level=1, threads=2)
    r = _run("filter_depth.py", ["-d", str(tmp_path), "--classes", "kept", path])
    assert r.returncode != 0 and "Traceback" not in r.stderr
    assert r.stderr.strip().split("\n")[-1] == ('ERROR!!! The file "%s" holds a record without an NM tag (record %d): GCI.py would have raised KeyError'
                                                % (path, ok.shape[0]))
    assert not os.path.exists(str(tmp_path / "GCI_fate.kept.depth.gz"))
