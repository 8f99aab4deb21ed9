"""filter_reads.py on the GPU: gci_bam_reads_size / _write (k_reads.hip) against the statement of tests/reads_ref.py on every case of
tests/reads_cases.py in both stream forms, byte for byte, with guard bytes behind the text; pipeline.bam_filter_reads over small
synthetic files in one piece and in several, against filter_depth.py's record counts, and with --join; and the command line once."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fate_ref as F
import joinfate_ref as J
import reads_cases as RC
import reads_ref as RR
from gci_amd import _lib, filterdepth_cli, pipeline, synth
from gci_amd.device import REC_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64                                               # guard bytes behind the rows
U64 = 2 ** 64 - 1


def form_of(name, form):
    c = RC.case(name)
    return (c["stream"], c["offs"]) if form == "stream" else RC.heads(name)


@pytest.fixture(scope="module")
def on_device(engine):
    """The buffers of every (case, form), uploaded once: stream, offsets, ref_sel, class bytes, contig names, windows."""
    cache = {}

    def get(name, form):
        if (name, form) not in cache:
            c = RC.case(name)
            stream, offs = form_of(name, form)
            up = lambda a: engine.to_device(a if a.shape[0] else np.zeros(1, dtype=a.dtype))      # noqa: E731
            cache[(name, form)] = dict(
                stream=engine.to_device(stream), offs=up(offs), sel=engine.to_device(c["ref_sel"]), cls=up(RC.classes(name)),
                names=engine.to_device(np.frombuffer(b"".join(c["names"]) + b"\0", dtype=np.uint8)),
                win=None if c["win0"] is None else up(np.ascontiguousarray(c["win"]).reshape(-1)),
                win0=None if c["win0"] is None else engine.to_device(c["win0"]), n_bytes=int(stream.shape[0]), n_rec=int(offs.shape[0]))
        return cache[(name, form)]
    return get


def name_tables(c):
    name_len = np.array([len(x) for x in c["names"]], dtype=np.uint32)
    name_off = np.concatenate(([0], np.cumsum(name_len[:-1]))).astype(np.uint64)
    return name_off, name_len


def device_size(engine, b, c, has_seq, mask=None, file_no=1):
    """-> (rows, bytes, status word) of the size export as it is."""
    _, name_len = name_tables(c)
    rows, size, status = ctypes.c_uint64(7), ctypes.c_uint64(7), engine.T.zeros(1, engine.T.int64, engine.device)
    p = engine._p
    st = engine.lib.gci_bam_reads_size(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]) if b["n_rec"] else None, b["n_rec"], int(has_seq), p(b["sel"]),
                                       int(b["sel"].shape[0]), p(b["cls"]), c["mask"] if mask is None else mask, p(b["win"]), p(b["win0"]),
                                       name_len.ctypes.data_as(ctypes.c_void_p), file_no, ctypes.byref(rows), ctypes.byref(size), p(status))
    assert st == 0
    return int(rows.value), int(size.value), int(status.item()) & U64


def device_write(engine, b, c, total, cap):
    """-> (return value, the bytes [0, total + PAD) of a 0xA5-filled buffer after the write export)."""
    name_off, name_len = name_tables(c)
    out = engine.T.empty(total + PAD, engine.T.uint8, engine.device)
    assert engine.lib.gci_memset(engine.ctx, engine._p(out), 0xA5, total + PAD) == 0
    p = engine._p
    st = engine.lib.gci_bam_reads_write(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]) if b["n_rec"] else None, b["n_rec"], p(b["names"]),
                                        name_off.ctypes.data_as(ctypes.c_void_p), name_len.ctypes.data_as(ctypes.c_void_p), p(out), cap)
    engine.sync()
    return st, out.cpu().numpy()


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name", RC.NAMES)
def test_the_device_gives_the_rows_of_the_statement(engine, on_device, name, form):
    c, b = RC.case(name), on_device(name, form)
    want_rows, want_status = RC.want(name)
    want = RR.text(want_rows)
    engine.set_layout(c["lengths"])
    rows, size, status = device_size(engine, b, c, form == "stream")
    assert status == want_status
    assert (rows, size) == (len(want_rows), len(want))
    st, h = device_write(engine, b, c, size, size)
    assert st == 0
    assert (h[size:] == 0xA5).all(), "bytes behind the rows were written"
    assert h[:size].tobytes() == want


def test_too_little_room_writes_nothing(engine, on_device):
    for name in ("window_edges", "stage_overflow"):        # (rows through the stage, rows straight to memory)
        c, b = RC.case(name), on_device(name, "stream")
        engine.set_layout(c["lengths"])
        rows, size, _ = device_size(engine, b, c, True)
        assert size > 0
        st, h = device_write(engine, b, c, size, size - 1)
        assert st == _lib.GCI_E_CAPACITY and (h == 0xA5).all()


def test_argument_errors(engine, on_device):
    c, b = RC.case("window_edges"), on_device("window_edges", "stream")
    other = on_device("no_reference", "stream")
    engine.set_layout(c["lengths"])
    p, lib = engine._p, engine.lib
    _, name_len = name_tables(c)
    rows, size = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for mask in (1 << 0, 1 << 7, 1 << 13, 1 << 31):
        assert lib.gci_bam_reads_size(engine.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"], 1, p(b["sel"]), int(b["sel"].shape[0]), p(b["cls"]), mask,
                                      p(b["win"]), p(b["win0"]), name_len.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(rows), ctypes.byref(size),
                                      p(engine._status)) == _lib.GCI_E_INVALID
    # the write call takes the input of the size call in front of it alone
    device_size(engine, b, c, True)
    device_size(engine, other, RC.case("no_reference"), True)
    st, h = device_write(engine, b, c, 4096, 4096)
    assert st == _lib.GCI_E_INVALID and (h == 0xA5).all()
    from gci_amd.device import Engine
    fresh = Engine(0)
    assert fresh.lib.gci_bam_reads_size(fresh.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), b["n_rec"], 1, p(b["sel"]), int(b["sel"].shape[0]), p(b["cls"]),
                                        c["mask"], p(b["win"]), p(b["win0"]), name_len.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(rows),
                                        ctypes.byref(size), p(engine._status)) == _lib.GCI_E_NO_LAYOUT
    fresh.close()


def test_a_status_raises_with_its_record(engine, on_device):
    c, b = RC.case("op9"), on_device("op9", "stream")
    engine.set_layout(c["lengths"])
    with pytest.raises(_lib.GciError) as e:
        engine.bam_reads(b["stream"], b["offs"], True, b["sel"], b["cls"], c["mask"], c["names"], b["names"])
    assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == 3


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctgA", 300_000), ("ctgB", 200_000))
KINDS = {"hifi": dict(coverage=3, seed=31, filt=(30, 0.1, 0.995)), "ont": dict(coverage=3, seed=32, long_cigar_frac=0.05, filt=(30, 0.1, 0.9))}
FILT = (30, 0.1, 0.9)                                   # the command line's defaults
REGIONS = [("ctgA", 100_000, 100_500), ("ctgA", 100_400, 101_000), ("ctgB", 0, 50), ("ctgB", 150_000, 150_001), ("nowhere", 0, 10)]
JOIN_REGIONS = [("ctgA", 50_000, 150_000), ("ctgB", 20_000, 60_000)]
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per kind: the BAM file (BGZF) of about a hundred synthetic records, its stream and record offsets.  Made once."""
    if not _FILES:
        d = tmp_path_factory.mktemp("reads")
        for kind, kw in KINDS.items():
            rs = synth.simulate_reads(CONTIGS, kw["coverage"], kind, seed=kw["seed"], **{k: v for k, v in kw.items() if k == "long_cigar_frac"}).sorted()
            stream, offs = synth.to_bam_stream(rs)
            path = str(d / (kind + ".bam"))
            bamfmt.write_bam_stream(path, stream, level=1, threads=4)
            _FILES[kind] = dict(path=path, stream=stream, offs=offs)
        _FILES["dir"] = d
    return _FILES


def statement_of(f, filt, regions, file_no=1, classes=None, mask=RC.ALL):
    sel = np.arange(len(CONTIGS), dtype=np.int32)
    cls = F.stream_classes(f["stream"], f["offs"], sel, *filt)[0] if classes is None else classes
    win = (None, None) if regions is None else pipeline.merge_windows(regions, dict(CONTIGS))
    rows, status = RR.stream_rows(f["stream"], f["offs"], sel, [n.encode() for n, _ in CONTIGS], cls, mask, win[0], win[1], file_no)
    assert status == RR.NO_STATUS
    return rows


def table_of(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b""
    head = [ln for ln in lines[:-1] if ln.startswith(b"#")]
    assert head[-1] == b"#" + "\t".join(RR.COLUMNS).encode() and lines[:len(head)] == head
    return head[:-1], b"".join(ln + b"\n" for ln in lines[len(head):-1])


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_pipeline_in_one_piece_and_in_several(engine, files, kind, tmp_path, monkeypatch):
    """The file in several pieces (run by run on the walk engine) == the file in one piece == the statement, with and without regions."""
    f, filt = files[kind], KINDS[kind]["filt"]
    pieces, visit = [], pipeline._ReadsVisitor.visit
    monkeypatch.setattr(pipeline._ReadsVisitor, "visit", lambda self, *a: (pieces.append(a[-1]), visit(self, *a))[1])      # (a[-1]: rec_idx_base)
    whole = (pipeline.GPU_INFLATE_MAX, pipeline.BAM_CHUNK_BYTES)
    for regions in (None, REGIONS):
        want = RR.text(statement_of(f, filt, regions))
        assert (regions is None) or 0 < want.count(b"\n") < len(f["offs"])
        for several in (False, True):
            monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0 if several else whole[0])
            monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", (1 << 20) if several else whole[1])
            del pieces[:]
            out = str(tmp_path / ("%s_%d_%d.tsv" % (kind, regions is not None, several)))
            res = pipeline.bam_filter_reads(engine, [f["path"]], [], pipeline.FateOpts(*filt), 4, pipeline.FATE_WANTED, regions, out)
            assert (len(pieces) > 1) == several and pieces[0] == 0 and sorted(pieces) == pieces, pieces
            head, text = table_of(out)
            assert head == [b"#file\t1\t" + f["path"].encode()] and res.rows == [text.count(b"\n")] and res.files == [f["path"]]
            assert text == want, (regions is not None, several)


def test_the_rows_per_class_are_filter_depths_record_counts(engine, files, tmp_path):
    """Without regions: two files, listed one after the other; the rows per file and class equal the #records rows of filter_depth.py's table."""
    paths = [files["hifi"]["path"], files["ont"]["path"]]
    out = str(tmp_path / "both.tsv")
    res = pipeline.bam_filter_reads(engine, paths, [], None, 4, pipeline.FATE_WANTED, None, out)
    head, text = table_of(out)
    assert head == [b"#file\t%d\t%s" % (k + 1, p.encode()) for k, p in enumerate(paths)]
    assert text == RR.text(statement_of(files["hifi"], FILT, None, 1)) + RR.text(statement_of(files["ont"], FILT, None, 2))
    depth = pipeline.bam_filter_depth(engine, paths, [], None, 4, ["kept"])
    table = str(tmp_path / "x.filter.txt")
    filterdepth_cli.write_table(table, paths, depth.counts, ["kept"], depth.tracks["kept"].targets, {"kept": engine.depth_sum(depth.tracks["kept"].track)})
    records = [ln.split("\t") for ln in open(table).read().split("#covered_bases")[0].splitlines()[2:]]
    assert [r[0] for r in records] == paths and res.counts == depth.counts
    per = {}
    for row in text.split(b"\n")[:-1]:
        cols = row.decode().split("\t")
        per[(int(cols[0]), cols[-1])] = per.get((int(cols[0]), cols[-1]), 0) + 1
    for k, r in enumerate(records):
        for name, cell in zip(F.NAMES[1:7], r[2:]):
            assert per.get((k + 1, name), 0) == int(cell), (k, name)
    # --chrs and --classes select
    res = pipeline.bam_filter_reads(engine, paths[:1], ["ctgB"], None, 4, ["kept", "mapq"], None, out)
    _, text = table_of(out)
    assert {r.split(b"\t")[2] for r in text.split(b"\n")[:-1]} == {b"ctgB"} and {r.split(b"\t")[-1] for r in text.split(b"\n")[:-1]} <= {b"kept", b"mapq"}
    assert res.rows[0] == res.counts[0][F.KEPT] + res.counts[0][F.MAPQ]


def test_a_record_the_reference_raises_on_leaves_no_table(engine, files, tmp_path):
    f = files["hifi"]
    blob = f["stream"].tobytes() + bamfmt.encode_record(0, 5, "no_nm", 60, 0, [(4, 30), (0, 10)], 4)       # clipped, and no NM
    path, out = str(tmp_path / "no_nm.bam"), str(tmp_path / "no_nm.tsv")
    bamfmt.write_bam_stream(path, np.frombuffer(blob, dtype=np.uint8), level=1, threads=2)
    with pytest.raises(_lib.GciError) as e:
        pipeline.bam_filter_reads(engine, [path], [], None, 2, ["kept"], None, out)
    assert e.value.status == _lib.GCI_E_NO_NM and e.value.path == path and "record %d of the file" % len(f["offs"]) in str(e.value)
    assert not os.path.exists(out)


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """One read set as a BAM file and as a PAF file, with reads planted so that the join shadows some records of the BAM file and leaves
    one unpaired; and the statement's class per BAM record (fate_ref refined with joinfate_ref)."""
    from dataclasses import replace
    from gci_amd import cpu, hostio
    d = tmp_path_factory.mktemp("reads_join")
    base = synth.simulate_reads(CONTIGS, 3.0, "hifi", seed=41)
    moved = base.take(np.arange(2, len(base), max(len(base) // 5, 1))[:4])
    moved = replace(moved, ref_id=(1 - moved.ref_id).astype(np.int32), pos=np.minimum(moved.pos, 100_000).astype(np.int32))
    lonely = base.names[len(base) // 2 + 1]
    rs = synth.concat(synth.perturb(base, 42), moved).sorted()
    rs = replace(rs, mapq=np.where(rs.names == lonely, 40, rs.mapq).astype(np.uint8))
    targets, sel = [n for n, _ in CONTIGS], np.arange(len(CONTIGS), dtype=np.int32)
    paf = str(d / "reads.paf")
    open(paf, "w").write("".join(synth.to_paf_lines(base.take(np.flatnonzero(base.names != lonely)), 43)))
    recs, names, off = hostio.paf_filter([paf], targets, FILT[0], 50, FILT[2])[0]
    joined = [(np.ascontiguousarray(recs).reshape(-1).view(REC_DTYPE), [bytes(names[int(off[i]):int(off[i + 1])]) for i in range(off.shape[0] - 1)])]
    stream, offs = synth.to_bam_stream(rs)
    bam = str(d / "reads.bam")
    bamfmt.write_bam_stream(bam, stream, level=1, threads=4)
    r = cpu.CpuEngine(threads=4).bam_filter(stream, offs, sel, FILT[0], 50, FILT[1], FILT[2])
    joined.append((r, [bytes(stream[int(o) + 36:int(o) + 36 + int(n)]) for o, n in zip(offs.tolist(), r["name_len"].tolist())]))
    fate, counts, status, _ = J.statement(joined, 0.9)
    assert status == J.NO_STATUS
    cls, _, status = F.stream_classes(stream, offs, sel, *FILT)
    refined, status2 = J.refine(cls, fate[1])
    assert status == F.NO_STATUS and status2 == J.NO_STATUS
    return dict(bam=bam, paf=paf, stream=stream, offs=offs, cls=refined, counts=counts)


def test_with_join_the_class_column_is_the_joins(engine, pair, tmp_path):
    assert len(set(pair["cls"].tolist()) & set(range(J.SHADOWED, J.JOINED + 1))) >= 3, np.bincount(pair["cls"])     # the condition
    out = str(tmp_path / "join.tsv")
    join = pipeline.JoinFateOpts([pair["paf"]], 50, 0.9, 0)
    res = pipeline.bam_filter_reads(engine, [pair["bam"]], [], pipeline.FateOpts(*FILT), 4, pipeline.FATE_WANTED[:5] + pipeline.JOIN_FATE_NAMES, JOIN_REGIONS, out,
                                    join=join)
    head, text = table_of(out)
    want = statement_of(pair, FILT, JOIN_REGIONS, classes=pair["cls"], mask=_lib.READS_CLASS_MASK)
    assert head == [b"#file\t1\t" + pair["bam"].encode()] and text == RR.text(want) and 0 < len(want) < len(pair["offs"])
    assert res.counts[0][J.SHADOWED:J.JOINED + 1] == [int(x) for x in pair["counts"][1][J.SHADOWED:J.JOINED + 1]]
    # `kept` with the join is the five of them; without regions every record that belongs to a class is listed
    pipeline.bam_filter_reads(engine, [pair["bam"]], [], pipeline.FateOpts(*FILT), 4, ["kept"], None, out, join=join)
    _, text = table_of(out)
    join_mask = sum(1 << k for k in range(J.SHADOWED, J.JOINED + 1))
    assert text == RR.text(statement_of(pair, FILT, None, classes=pair["cls"], mask=join_mask))
    with pytest.raises(ValueError):
        pipeline.bam_filter_reads(engine, [pair["bam"]], [], None, 4, ["joined"], None, out)


def test_command_line(files, tmp_path):
    out = str(tmp_path)
    bed = tmp_path / "r.bed"
    bed.write_text("".join("%s\t%d\t%d\n" % r for r in REGIONS))
    argv = ["-d", out, "-o", "x", "-t", "4", "-R", str(bed), "--classes", "kept,clip,identity", files["hifi"]["path"], files["ont"]["path"]]
    r = _run("filter_reads.py", argv, dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["r.bed", "x.reads.tsv"]
    head, text = table_of(os.path.join(out, "x.reads.tsv"))
    mask = (1 << F.KEPT) | (1 << F.CLIP) | (1 << F.IDENTITY)
    want = RR.text(statement_of(files["hifi"], FILT, REGIONS, 1, mask=mask)) + RR.text(statement_of(files["ont"], FILT, REGIONS, 2, mask=mask))
    assert head == [b"#file\t%d\t%s" % (k + 1, files[kind]["path"].encode()) for k, kind in enumerate(("hifi", "ont"))]
    assert text == want and want
    r = _run("filter_reads.py", argv)                     # a second run without -f refuses
    assert r.returncode != 0 and r.stderr.strip().split("\n")[-2:] == ['ERROR!!! The file "%s/x.reads.tsv" exists' % out,
                                                                       'Please use "-f" or "--force" to rewrite']
