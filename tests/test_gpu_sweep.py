"""filter_sweep.py on the GPU: gci_bam_sweep (k_sweep.hip) against the statement of tests/sweep_ref.py on every case of
tests/sweep_cases.py in both stream forms and for K = 1, 2, 3, into a pre-filled table with guard entries behind it; against
gci_bam_fate on the same buffers; with the workgroups capped; pipeline.bam_filter_sweep over small synthetic files in one piece and in
several, and against filter_reads.py's row counts; and the command line once."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fate_ref as F
import sweep_cases as SC
import sweep_ref as SR
from gci_amd import _lib, pipeline, synth
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16                                             # entries behind the table that must stay
PATTERN = 0xA5A5A5A5A5A5A5A5
U64 = 2 ** 64 - 1


def form_of(name, form):
    c = SC.case(name)
    return (c["stream"], c["offs"]) if form == "stream" else SC.heads(name)


def upload(engine, name, form):
    """The buffers of a (case, form): stream, offsets, ref_sel, windows."""
    c = SC.case(name)
    stream, offs = form_of(name, form)
    up = lambda a: engine.to_device(a if a.shape[0] else np.zeros(1, dtype=a.dtype))      # noqa: E731
    return dict(stream=engine.to_device(stream), offs=up(offs), sel=engine.to_device(c["ref_sel"]),
                win=None if c["win0"] is None else up(np.ascontiguousarray(c["win"]).reshape(-1)),
                win0=None if c["win0"] is None else engine.to_device(c["win0"]), n_bytes=int(stream.shape[0]), n_rec=int(offs.shape[0]))


@pytest.fixture(scope="module")
def on_device(engine):
    cache = {}

    def get(name, form):
        if (name, form) not in cache:
            cache[(name, form)] = upload(engine, name, form)
        return cache[(name, form)]
    return get


def device_sweep(engine, b, has_seq, run, digits):
    """-> (the table, the status word) of the export as it is: the table pre-filled with a pattern, guard entries behind it checked."""
    cells = 4 * SR.Rows(digits).rows
    table = np.full(cells + GUARD, PATTERN, dtype=np.uint64)
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    p = engine._p
    st = engine.lib.gci_bam_sweep(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]) if b["n_rec"] else None, b["n_rec"], int(has_seq), p(b["sel"]),
                                  int(b["sel"].shape[0]), p(b["win"]), p(b["win0"]), run[0], run[1], run[2], digits, table.ctypes.data_as(ctypes.c_void_p),
                                  p(status))
    assert st == 0
    assert (table[cells:] == PATTERN).all(), "entries behind the table were written"
    return table[:cells].reshape(-1, 4), int(status.item()) & U64


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name", SC.NAMES)
def test_the_device_gives_the_tables_of_the_statement(engine, on_device, name, form):
    c, b = SC.case(name), on_device(name, form)
    engine.set_layout(c["lengths"])
    for run in c["runs"]:
        for digits in SC.DIGITS:
            want, want_status = SC.want(name, run, digits)
            got, status = device_sweep(engine, b, form == "stream", run, digits)
            assert status == want_status, (run, digits)
            assert np.array_equal(got, want), (run, digits, np.argwhere(got != want)[:5])


def on_the_grid(x: float, digits: int) -> bool:
    return abs(x * 10 ** digits - round(x * 10 ** digits)) < 1e-9


@pytest.mark.parametrize("name", [n for n in SC.NAMES if SC.case(n)["win0"] is None])
def test_a_thresholds_own_row_keeps_what_gci_bam_fate_keeps(engine, on_device, name):
    """The same buffers and thresholds through gci_bam_fate: wherever it reports no status, its `kept` count is kept_at of the run's own
    threshold in all three tables (thresholds that are multiples of 10^-K)."""
    c, b = SC.case(name), on_device(name, "stream")
    for run in c["runs"] if b["n_rec"] else []:
        _, counts = engine.bam_fate(b["stream"], b["offs"][:b["n_rec"]], True, b["sel"], *run, check=False)
        if (int(engine._status.item()) & U64) != U64:
            continue
        for digits in SC.DIGITS:
            table, _ = device_sweep(engine, b, True, run, digits)
            rows, kept = SR.Rows(digits), SR.kept_at(table, digits)
            assert kept[rows.mapq0 + run[0]][0] == counts[F.KEPT], (run, digits)
            if on_the_grid(run[1], digits):
                assert kept[rows.clip0 + round(run[1] * rows.bins)][0] == counts[F.KEPT], (run, digits)
            if on_the_grid(run[2], digits):
                assert kept[rows.iden0 + round(run[2] * rows.bins)][0] == counts[F.KEPT], (run, digits)
            assert int(table[:256, 0].sum()) == sum(counts[k] for k in (F.MAPQ, F.CLIP, F.IDENTITY, F.KEPT))


def test_gci_bam_fate_reports_nothing_where_it_is_compared(engine, on_device):
    """... and the comparison above is not empty: most cases, the random set and the many-operation CIGARs among them, go through it."""
    clean = []
    for name in SC.NAMES:
        c = SC.case(name)
        if c["win0"] is None and all(F.stream_classes(c["stream"], c["offs"], c["ref_sel"], *run)[2] == F.NO_STATUS for run in c["runs"]):
            clean.append(name)
    assert {"edges", "all_clip_rows", "identical_3000", "wave_rows", "big_operations", "chunks", "placeholder", "records_257"} <= set(clean)


@pytest.mark.parametrize("cap", ["1", "2"])
def test_capped_workgroups_give_the_same_tables(engine, on_device, cap, monkeypatch):
    """GCI_SWEEP_GRID=1, 2: a workgroup goes round its loop more than once (769 records: four blocks of 256), and twelve times for 3000."""
    from gci_amd.device import Engine
    monkeypatch.setenv("GCI_SWEEP_GRID", cap)
    capped = Engine(0)
    try:
        for name in (SC.GRID_CASE, "random_3000", "identical_3000", "wave_rows"):
            c = SC.case(name)
            assert name != SC.GRID_CASE or int(c["offs"].shape[0]) == 3 * SC.GROUP + 1
            engine.set_layout(c["lengths"])
            capped.set_layout(c["lengths"])
            b = upload(capped, name, "heads")
            for run in c["runs"]:
                free, status = device_sweep(engine, on_device(name, "heads"), False, run, 3)
                got, status2 = device_sweep(capped, b, False, run, 3)
                assert status == status2 and np.array_equal(got, free) and np.array_equal(got, SC.want(name, run, 3)[0]), (name, run)
    finally:
        capped.close()


def test_argument_errors(engine, on_device):
    c, b = SC.case("window_edges"), on_device("window_edges", "stream")
    p, lib = engine._p, engine.lib
    table = np.full(4 * SR.Rows(3).rows, PATTERN, dtype=np.uint64)

    def call(e, digits=3, win=b["win"], win0=b["win0"], h_table=table.ctypes.data_as(ctypes.c_void_p)):
        return lib.gci_bam_sweep(e.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"], 1, p(b["sel"]), int(b["sel"].shape[0]), p(win), p(win0), 30,
                                 0.1, 0.9, digits, h_table, p(engine._status))

    engine.set_layout(c["lengths"])
    for digits in (0, 4):
        assert call(engine, digits=digits) == _lib.GCI_E_INVALID
    assert call(engine, h_table=None) == _lib.GCI_E_INVALID and call(engine, win=None) == _lib.GCI_E_INVALID
    assert (table == PATTERN).all()
    from gci_amd.device import Engine
    fresh = Engine(0)
    try:
        assert call(fresh) == _lib.GCI_E_NO_LAYOUT and call(fresh, win=None, win0=None) == 0
    finally:
        fresh.close()


def test_a_status_raises_with_its_record(engine, on_device):
    b = on_device("op9", "stream")
    with pytest.raises(_lib.GciError) as e:
        engine.bam_sweep(b["stream"], b["offs"], True, b["sel"], 30, 0.1, 0.9)
    assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == SC.STATUS["op9"][0]


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctgA", 300_000), ("ctgB", 200_000))
KINDS = {"hifi": dict(coverage=3, seed=31, filt=(30, 0.1, 0.995)), "ont": dict(coverage=3, seed=32, long_cigar_frac=0.05, filt=(30, 0.1, 0.9))}
FILT = (30, 0.1, 0.9)                                   # the command line's defaults
REGIONS = [("ctgA", 100_000, 100_500), ("ctgA", 100_400, 101_000), ("ctgB", 0, 50), ("ctgB", 150_000, 150_001), ("nowhere", 0, 10)]
WIDE = [("ctgA", 50_000, 150_000), ("ctgB", 20_000, 60_000)]
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per kind: the BAM file (BGZF) of about a hundred synthetic records, its stream and record offsets.  Made once."""
    if not _FILES:
        d = tmp_path_factory.mktemp("sweep")
        for kind, kw in KINDS.items():
            rs = synth.simulate_reads(CONTIGS, kw["coverage"], kind, seed=kw["seed"], **{k: v for k, v in kw.items() if k == "long_cigar_frac"}).sorted()
            stream, offs = synth.to_bam_stream(rs)
            path = str(d / (kind + ".bam"))
            bamfmt.write_bam_stream(path, stream, level=1, threads=4)
            _FILES[kind] = dict(path=path, stream=stream, offs=offs)
    return _FILES


def statement_of(f, filt, regions, digits=3):
    sel = np.arange(len(CONTIGS), dtype=np.int32)
    win = (None, None) if regions is None else pipeline.merge_windows(regions, dict(CONTIGS))
    table, status = SR.stream_table(f["stream"], f["offs"], sel, filt, digits, win[0], win[1])
    assert status == SR.NO_STATUS
    return table


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_pipeline_in_one_piece_and_in_several(engine, files, kind, monkeypatch):
    """The file in several pieces (run by run on the walk engine) == the file in one piece == the statement, with and without regions."""
    f, filt = files[kind], KINDS[kind]["filt"]
    pieces, visit = [], pipeline._SweepVisitor.visit
    monkeypatch.setattr(pipeline._SweepVisitor, "visit", lambda self, *a: (pieces.append(a[-1]), visit(self, *a))[1])      # (a[-1]: rec_idx_base)
    whole = (pipeline.GPU_INFLATE_MAX, pipeline.BAM_CHUNK_BYTES)
    for regions in (None, REGIONS):
        want = statement_of(f, filt, regions)
        assert 0 < int(want[:256, 0].sum()) and ((regions is None) or int(want[:256, 0].sum()) < len(f["offs"]))
        for several in (False, True):
            monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0 if several else whole[0])
            monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", (1 << 20) if several else whole[1])
            del pieces[:]
            res = pipeline.bam_filter_sweep(engine, [f["path"]], [], pipeline.FateOpts(*filt), 4, 3, regions)
            assert (len(pieces) > 1) == several and pieces[0] == 0 and sorted(pieces) == pieces, pieces
            assert res.files == [f["path"]] and res.digits == 3 and np.array_equal(res.tables[0], want), (regions is not None, several)


def test_with_windows_the_tables_count_filter_reads_rows(engine, files, tmp_path):
    """Two files, each its own table; over the same windows every table counts the rows filter_reads.py lists for the classes mapq, clip,
    identity and kept; --chrs selects; fewer digits give the same records."""
    paths = [files["hifi"]["path"], files["ont"]["path"]]
    res = pipeline.bam_filter_sweep(engine, paths, [], None, 4, 2, WIDE)
    out = str(tmp_path / "rows.tsv")
    reads = pipeline.bam_filter_reads(engine, paths, [], None, 4, ["mapq", "clip", "identity", "kept"], WIDE, out)
    rows, per_class = SR.Rows(2), {}
    for line in open(out):
        if not line.startswith("#"):
            cols = line.rstrip("\n").split("\t")
            per_class[(int(cols[0]), cols[-1])] = per_class.get((int(cols[0]), cols[-1]), 0) + 1
    for k, kind in enumerate(("hifi", "ont")):
        assert np.array_equal(res.tables[k], statement_of(files[kind], FILT, WIDE, 2))
        for a, b in ((rows.mapq0, rows.clip0), (rows.clip0, rows.iden_below), (rows.iden_below, rows.rows)):
            assert int(res.tables[k][a:b, 0].sum()) == reads.rows[k] > 0
        kept, listed = SR.kept_at(res.tables[k], 2), per_class.get((k + 1, "kept"), 0)
        assert kept[rows.mapq0 + 30][0] == kept[rows.clip0 + 10][0] == kept[rows.iden0 + 90][0] == listed > 0
    only_b = pipeline.bam_filter_sweep(engine, paths[:1], ["ctgB"], None, 4, 1, None)
    sel_b = np.array([-1, 0], dtype=np.int32)
    want, status = SR.stream_table(files["hifi"]["stream"], files["hifi"]["offs"], sel_b, FILT, 1)
    assert status == SR.NO_STATUS and np.array_equal(only_b.tables[0], want) and 0 < int(want[:256, 0].sum()) < int(statement_of(files["hifi"], FILT, None)[:256, 0].sum())
    with pytest.raises(ValueError):
        pipeline.bam_filter_sweep(engine, paths[:1], [], None, 4, 4, None)


def test_command_line(files, tmp_path):
    out = str(tmp_path)
    bed = tmp_path / "r.bed"
    bed.write_text("".join("%s\t%d\t%d\n" % r for r in WIDE))
    argv = ["-d", out, "-o", "s", "-t", "4", "-R", str(bed), "-ip", "0.85", files["hifi"]["path"], files["ont"]["path"]]
    r = _run("filter_sweep.py", argv, dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["r.bed", "s.sweep.txt"]
    text = open(os.path.join(out, "s.sweep.txt")).read()
    want = "#filter_sweep\tdigits=3\tmq=30\tcp=0.1\tip=0.85\tregions=%s\n" % bed
    for k, kind in enumerate(("hifi", "ont")):
        want += SR.file_text(k + 1, files[kind]["path"], statement_of(files[kind], (30, 0.1, 0.85), WIDE), 3)
    assert text == want
    r = _run("filter_sweep.py", argv)                     # a second run without -f refuses
    assert r.returncode != 0 and r.stderr.strip().split("\n")[-2:] == ['ERROR!!! The file "%s/s.sweep.txt" exists' % out,
                                                                       'Please use "-f" or "--force" to rewrite']
    # a malformed record: filter_depth.py's message, and no table
    f = files["hifi"]
    n = int(f["offs"].shape[0])
    from cover_cases import M, rec
    from fate_cases import nm
    stream = np.concatenate([f["stream"], np.frombuffer(rec(0, 5, [(M, 4), (9, 3)], aux=nm(0)), dtype=np.uint8)])
    path = str(tmp_path / "op9.bam")
    bamfmt.write_bam_stream(path, stream, level=1, threads=2)
    r = _run("filter_sweep.py", ["-d", out, "-o", "bad", path])
    assert r.returncode != 0 and "Traceback" not in r.stderr
    assert r.stderr.strip().split("\n")[-1] == 'ERROR!!! The file "%s" holds a malformed BAM record (record %d)' % (path, n)
    assert not os.path.exists(os.path.join(out, "bad.sweep.txt"))
