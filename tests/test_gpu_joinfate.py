"""filter_depth.py --join on the GPU: gci_name_join_fate (k_join.hip) against the statement of tests/joinfate_ref.py on every case of
tests/joinfate_cases.py -- bytes, counts, status word, guard bytes -- and against gci_name_join on the same inputs; the join tables
left clean between the two; gci_fate_refine; pipeline.bam_filter_depth(join=...) over three small synthetic files and a PAF in every
ingest mode; and the command line once."""
import ctypes
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import fate_ref as F
import joinfate_cases as JC
import joinfate_ref as J
from gci_amd import _lib, pipeline, synth
from gci_amd.device import Engine, JoinInput, REC_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64                                               # guard bytes behind every file's verdicts
U64 = 2 ** 64 - 1


def upload(engine, name):
    """The files of a case as device join inputs."""
    out = []
    for recs, blob, off, delta in JC.inputs(name):
        if recs.shape[0] == 0:
            out.append(pipeline._concat_parts(engine, []))
            continue
        out.append(JoinInput(engine.to_device(recs.view(np.uint8).reshape(-1, 32)), engine.to_device(blob),
                             engine.to_device(off.astype(np.int64) if off.shape[0] else np.zeros(1, np.int64)), delta))
    return out


@pytest.fixture(scope="module")
def on_device(engine):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = upload(engine, name)
        return cache[name]
    return get


def device_join_fate(engine, files, op):
    """-> (bytes per file, counts [n, 16], status word): the export as it is, the outputs 0xA5-filled with PAD bytes behind them."""
    n = len(files)
    sizes = [int(f.recs.shape[0]) for f in files]
    bufs = [engine.T.empty(k + PAD, engine.T.uint8, engine.device) for k in sizes]
    for b, k in zip(bufs, sizes):
        assert engine.lib.gci_memset(engine.ctx, engine._p(b), 0xA5, k + PAD) == 0
    ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
    counts = (ctypes.c_uint64 * ((n + 1) * J.ROW))(*([7] * ((n + 1) * J.ROW)))
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    assert engine.lib.gci_name_join_fate(engine.ctx, engine._join_files(files), n, float(op), ptrs, counts, engine._p(status)) == 0
    host = [b.cpu().numpy() for b in bufs]
    for h, k in zip(host, sizes):
        assert (h[k:] == 0xA5).all(), "bytes behind the verdicts were written"
    c = np.array(list(counts), dtype=np.uint64).reshape(n + 1, J.ROW)
    assert (c[n] == 7).all(), "counts behind the last file's row were written"
    return [h[:k] for h, k in zip(host, sizes)], c[:n], int(status.item()) & U64


def device_join(engine, files, op):
    """gci_name_join -> (sorted (contig, start, end), the count it reports, status word)."""
    ivl, count = engine.name_join(files, op, check=False)
    n = int(count.item())
    h = ivl.cpu().numpy()[:n]
    return sorted(map(tuple, h[:, :3].tolist())), n, int(engine._status.item()) & U64


@pytest.mark.parametrize("name, op", JC.pairs())
def test_the_device_gives_the_bytes_of_the_statement(engine, on_device, name, op):
    want_fate, want_counts, want_status, _ = JC.want(name, op)
    fate, counts, status = device_join_fate(engine, on_device(name), op)
    assert status == want_status
    for f, (got, want) in enumerate(zip(fate, want_fate)):
        assert np.array_equal(got, want), (f, np.flatnonzero(got != want)[:10])
    assert np.array_equal(counts, want_counts)


@pytest.mark.parametrize("name, op", JC.pairs())
def test_the_join_emits_the_joined_names(engine, on_device, name, op):
    """gci_name_join on the same inputs, before and after the verdicts on the same context: the statement's intervals, one per
    distinct `joined` name; where the statement reports a status, the same word."""
    _, _, want_status, kept = JC.want(name, op)
    for _ in range(2):
        ivl, n, status = device_join(engine, on_device(name), op)
        assert status == want_status
        if want_status == J.NO_STATUS:
            assert n == len(kept) and ivl == sorted(kept.values())
        device_join_fate(engine, on_device(name), op)


def test_the_tables_are_left_clean(engine, on_device):
    """One context, calls of both kinds with different numbers of files and table sizes in both orders: every answer is what a fresh
    context gives (one per call, closed here)."""
    order = ["max_files", "one_file", "slots_2048", "three_records", "random_3_files", "one_file", "zero_qlen_reached", "random_5_files",
             "empty_file_of_three"]
    want = {}
    for name in set(order):
        got = []
        for call in (device_join_fate, device_join):
            fresh = Engine(0)
            try:
                got.append(call(fresh, upload(fresh, name), 0.9))
            finally:
                fresh.close()
        want[name] = (got[0], got[1][:2])
    for k, name in enumerate(order + order[::-1]):
        files = on_device(name)
        calls = (device_join_fate, device_join) if k % 2 else (device_join, device_join_fate)
        for call in calls:
            got = call(engine, files, 0.9)
            if call is device_join:
                assert got[:2] == want[name][1], (k, name)
            else:
                w = want[name][0]
                assert got[2] == w[2] and np.array_equal(got[1], w[1]) and all(np.array_equal(a, b) for a, b in zip(got[0], w[0])), (k, name)


def test_join_mode_does_not_change_the_verdicts(engine, on_device):
    """The export takes the classic table whatever gci_join_mode says."""
    want = JC.want("random_4_files", 0.9)
    try:
        engine.set_join_mode("partition")
        fate, counts, status = device_join_fate(engine, on_device("random_4_files"), 0.9)
    finally:
        engine.set_join_mode("auto")
    assert status == want[2] and np.array_equal(counts, want[1]) and all(np.array_equal(a, b) for a, b in zip(fate, want[0]))


def test_a_zero_qlen_raises_with_its_record_and_the_file_is_found(engine, on_device):
    files = on_device("zero_qlen_reached")
    with pytest.raises(_lib.GciError) as e:
        engine.name_join_fate(files, 0.9)
    assert e.value.status == _lib.GCI_E_ZERO_DIV and e.value.rec == 7
    assert pipeline._zero_qlen_file(files, 7) == 1 and pipeline._zero_qlen_file(files, 40) == -1
    fate, counts = engine.name_join_fate(on_device("zero_qlen_not_reached"), 0.9)
    want = JC.want("zero_qlen_not_reached", 0.9)
    assert [c[:J.ROW] for c in counts] == [[int(x) for x in row] for row in want[1]]
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(fate, want[0]))


HAND = np.array([0, 1, 6, 6, 3, 6, 6, 6, 5, 7, 6], dtype=np.uint8)
HAND_JOIN = np.array([0, 0, 12, 8, 0, 9, 10, 11, 0, 0, 12], dtype=np.uint8)


def device_refine(engine, cls, join):
    n = cls.shape[0]
    d_cls = engine.to_device(np.concatenate([cls, np.full(PAD, 0xA5, np.uint8)]))
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    assert engine.lib.gci_fate_refine(engine.ctx, engine._p(d_cls), engine._p(engine.to_device(join)), n, engine._p(status)) == 0
    h = d_cls.cpu().numpy()
    assert (h[n:] == 0xA5).all(), "bytes behind the classes were written"
    return h[:n], int(status.item()) & U64


def test_refine_on_a_hand_array(engine):
    want, want_status = J.refine(HAND, HAND_JOIN)
    assert want.tolist() == [0, 1, 12, 8, 3, 9, 10, 11, 5, 7, 12] and want_status == J.NO_STATUS
    got, status = device_refine(engine, HAND, HAND_JOIN)
    assert status == want_status and np.array_equal(got, want)
    for at, cls_byte, join_byte in ((3, 6, 0), (3, 6, 7), (3, 6, 13), (4, 3, 12), (0, 0, 9)):       # both misalignments, the smaller word wins
        cls, join = HAND.copy(), HAND_JOIN.copy()
        cls[at], join[at] = cls_byte, join_byte
        cls[9], join[9] = 6, 0
        want, want_status = J.refine(cls, join)
        assert want_status == J.word(at, J.E_INVALID)
        got, status = device_refine(engine, cls, join)
        assert status == want_status and np.array_equal(got, want)
    with pytest.raises(_lib.GciError) as e:
        engine.fate_refine(engine.to_device(np.array([6, 6], np.uint8)), engine.to_device(np.array([12, 0], np.uint8)), rec_idx_base=100)
    assert e.value.status == _lib.GCI_E_INVALID and e.value.rec == 101
    lib, st = engine.lib, engine._p(engine._status)
    d = engine.to_device(HAND)
    assert lib.gci_fate_refine(None, engine._p(d), engine._p(d), 1, st) == _lib.GCI_E_INVALID
    assert lib.gci_fate_refine(engine.ctx, None, engine._p(d), 1, st) == _lib.GCI_E_INVALID
    assert lib.gci_fate_refine(engine.ctx, engine._p(d), engine._p(d), 1, None) == _lib.GCI_E_INVALID
    assert lib.gci_fate_refine(engine.ctx, None, None, 0, st) == 0


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctgA", 600_000), ("ctgB", 400_000))
FILT = (30, 0.1, 0.9)                                   # the command line's defaults
MQ_CUTOFF, OP = 50, 0.9
CLASSES = pipeline.FATE_WANTED[:5] + pipeline.JOIN_FATE_NAMES
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """One read set aligned three times (BAM) and once more as PAF, with a few reads planted so that the join does every one of its five
    things to records of the first BAM file; and the statement's answer.  Made once.
      shadowed: a few reads of the first file a second time under the same names, on the other contig
      unpaired: one read below the cutoff wherever it is, missing from the PAF and from the third file"""
    if _FILES:
        return _FILES
    from dataclasses import replace
    from gci_amd import cpu, hostio
    d = tmp_path_factory.mktemp("joinfate")
    base = synth.simulate_reads(CONTIGS, 3.0, "hifi", seed=11)
    sets = [base, synth.perturb(base, 12), synth.perturb(base, 13)]
    moved = base.take(np.arange(2, len(base), max(len(base) // 5, 1))[:4])
    moved = replace(moved, ref_id=(1 - moved.ref_id).astype(np.int32), pos=np.minimum(moved.pos, 300_000).astype(np.int32))
    sets[0] = synth.concat(base, moved).sorted()
    lonely = base.names[len(base) // 2 + 1]
    for k, rs in enumerate(sets):
        sets[k] = replace(rs, mapq=np.where(rs.names == lonely, 40, rs.mapq).astype(np.uint8))
    sets[2] = sets[2].take(np.flatnonzero(sets[2].names != lonely))
    targets, sel = [n for n, _ in CONTIGS], np.arange(len(CONTIGS), dtype=np.int32)
    paf = str(d / "first.paf")
    open(paf, "w").write("".join(synth.to_paf_lines(base.take(np.flatnonzero(base.names != lonely)), 14)))
    recs, names, off = hostio.paf_filter([paf], targets, FILT[0], MQ_CUTOFF, FILT[2])[0]
    joined = [(np.ascontiguousarray(recs).reshape(-1).view(REC_DTYPE), [bytes(names[int(off[i]):int(off[i + 1])]) for i in range(off.shape[0] - 1)])]
    eng, bams = cpu.CpuEngine(threads=4), []
    for k, rs in enumerate(sets):
        stream, offs = synth.to_bam_stream(rs)
        path = str(d / ("aligner%d.bam" % k))
        bamfmt.write_bam_stream(path, stream, level=1, threads=4)
        r = eng.bam_filter(stream, offs, sel, FILT[0], MQ_CUTOFF, FILT[1], FILT[2])
        joined.append((r, [bytes(stream[int(o) + 36:int(o) + 36 + int(n)]) for o, n in zip(offs.tolist(), r["name_len"].tolist())]))
        bams.append(dict(path=path, stream=stream, offs=offs))
    fate, counts, status, kept = J.statement(joined, OP)
    assert status == J.NO_STATUS
    _FILES.update(dir=d, paf=paf, bams=bams, fate=fate, counts=counts, sel=sel)
    return _FILES


@pytest.fixture(scope="module")
def plain(engine, files):
    """Per BAM file (made on first use): the record classes of the statement refined with the join's bytes, and what the device says
    without `join` -- the `kept` track, and bam_raw_depth with excl = 0x4."""
    cache = {}

    def get(k):
        if k not in cache:
            b = files["bams"][k]
            cls, counts, status = F.stream_classes(b["stream"], b["offs"], files["sel"], *FILT)
            assert status == F.NO_STATUS
            refined, status = J.refine(cls, files["fate"][1 + k])
            assert status == J.NO_STATUS
            kept = pipeline.bam_filter_depth(engine, [b["path"]], [], pipeline.FateOpts(*FILT), 4, ["kept"])
            raw = pipeline.bam_raw_depth(engine, [b["path"]], opts=pipeline.CoverOpts(0x4, 0, False), threads=4)
            cache[k] = dict(cls=refined, counts=counts, kept={n: kept.tracks["kept"][n].astype(np.int64) for n, _ in CONTIGS},
                            raw={n: np.asarray(raw[n]).astype(np.int64) for n, _ in CONTIGS})
        return cache[k]
    return get


@pytest.mark.parametrize("mode", ["whole", "runs", "heads", "full"])
def test_the_pipeline_with_join(engine, files, plain, mode, monkeypatch):
    """Every class track against the statement's bytes; the ten tracks add up to bam_raw_depth with excl = 0x4, the five of the join to
    the `kept` track of a run without it.  whole: the file in one piece; runs: run by run on the walk engine with a budget of a few
    dozen intervals (slices of the join's bytes by rec_idx_base); heads, full: the ingest modes of the host."""
    cover = 0                                          # (the file the reads were planted in)
    want_row = files["counts"][1 + cover]
    assert (want_row[J.SHADOWED:J.JOINED + 1] > 0).all(), want_row         # the condition, before the device is asked
    budget = None
    if mode == "runs":
        monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0)
        monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", 1 << 20)
        budget = 48
    elif mode != "whole":
        monkeypatch.setenv("GCI_BAM_INGEST", mode)
    paths = [b["path"] for b in files["bams"]]
    res = pipeline.bam_filter_depth(engine, paths, [], pipeline.FateOpts(*FILT), 4, CLASSES, ivl_budget=budget,
                                    join=pipeline.JoinFateOpts([files["paf"]], MQ_CUTOFF, OP, cover))
    p, b = plain(cover), files["bams"][cover]
    if mode == "runs":
        assert res.flushes > 1                              # (later parts were added to a class's track)
    assert res.cover_file == 1 + cover and res.join_files == [files["paf"]] + paths
    assert res.counts == [[int(x) for x in p["counts"]] + [int(x) for x in want_row[J.SHADOWED:J.JOINED + 1]]]
    assert [[int(x) for x in row] for row in res.join_counts] == [[int(x) for x in row] for row in files["counts"]]
    lengths = [l for _, l in CONTIGS]
    for j, (name, _) in enumerate(CONTIGS):
        assert np.array_equal(sum(res.tracks[c][name].astype(np.int64) for c in CLASSES), p["raw"][name])
        assert np.array_equal(sum(res.tracks[c][name].astype(np.int64) for c in pipeline.JOIN_FATE_NAMES), p["kept"][name])
        for c in CLASSES:
            want = F.class_depth(b["stream"], b["offs"], lengths, files["sel"], p["cls"], pipeline.ALL_FATE_NAMES.index(c))[j]
            assert np.array_equal(res.tracks[c][name], want), (c, name)


def test_kept_with_join_is_the_five_together_and_tracks_are_counted(engine, files, plain, monkeypatch):
    paths = [b["path"] for b in files["bams"]]
    res = pipeline.bam_filter_depth(engine, paths, ["ctgB"], None, 4, ["kept", "joined"], join=pipeline.JoinFateOpts([], MQ_CUTOFF, OP, 0))
    assert list(res.tracks) == ["kept", "joined"] and np.array_equal(res.tracks["kept"]["ctgB"], plain(0)["kept"]["ctgB"])
    with pytest.raises(ValueError):
        pipeline.bam_filter_depth(engine, paths, [], None, 4, ["joined"])
    with pytest.raises(ValueError):
        pipeline.bam_filter_depth(engine, paths, [], None, 4, ["joined"], join=pipeline.JoinFateOpts([], MQ_CUTOFF, OP, 3))
    monkeypatch.setattr(pipeline, "device_memory_free", lambda e: 11 * 4 * 1_000_000 - 1)
    monkeypatch.setattr(pipeline, "bam_join_input", lambda *a, **k: pytest.fail("a file was read"))
    with pytest.raises(pipeline.TracksDoNotFit) as e:
        pipeline.bam_filter_depth(engine, paths, [], None, 4, CLASSES, join=pipeline.JoinFateOpts([files["paf"]], MQ_CUTOFF, OP, 0))
    assert e.value.n_tracks == len(CLASSES) + 1


def _depth_lines(path):
    with gzip.open(path, "rb") as g:
        lines = g.read().split(b"\n")
    assert lines[-1] == b"" and lines[0] == b">ctgA" and lines[600_001] == b">ctgB" and len(lines) == 1_000_003
    return np.concatenate([np.array(lines[1:600_001], dtype="S").astype(np.int64), np.array(lines[600_002:-1], dtype="S").astype(np.int64)])


def test_command_line(files, tmp_path):
    out = str(tmp_path)
    paths = [b["path"] for b in files["bams"]]
    argv = ["-d", out, "-o", "x", "-t", "4", "--join", paths[0], files["paf"], paths[1], paths[2]]
    r = _run("filter_depth.py", argv, dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == sorted(["x.%s.depth.gz" % c for c in CLASSES] + ["x.filter.txt"])
    rows = [ln.split("\t") for ln in open(os.path.join(out, "x.filter.txt")).read().splitlines()]
    order = [files["paf"]] + paths                                             # the reference's order: PAF files first
    assert rows[0] == ["#records"] and rows[1] == ["file"] + list(F.NAMES[:7]) + list(J.NAMES) and [r[0] for r in rows[2:6]] == order
    counts = files["counts"]
    for k, row in enumerate(rows[2:6]):
        join_cells = [str(int(x)) for x in counts[k][J.SHADOWED:J.JOINED + 1]]
        if k == 1:                                                             # the covered file: the first BAM
            cls_counts = F.stream_classes(files["bams"][0]["stream"], files["bams"][0]["offs"], files["sel"], *FILT)[1]
            assert row[1:] == [str(int(x)) for x in cls_counts[:7]] + join_cells
        else:
            assert row[1:] == ["-"] * 6 + [str(int(counts[k][J.SHADOWED:J.JOINED + 1].sum()))] + join_cells
    assert rows[6] == ["#covered_bases"] and rows[7] == ["contig"] + list(CLASSES) and [r[0] for r in rows[8:]] == ["ctgA", "ctgB", "total"]
    tracks = {c: _depth_lines(os.path.join(out, "x.%s.depth.gz" % c)) for c in J.NAMES}
    five = sum(tracks.values())
    assert [int(x) for x in rows[10][6:]] == [int(tracks[c].sum()) for c in J.NAMES] and min(int(x) for x in rows[10][6:]) > 0
    # a second run without -f refuses
    r = _run("filter_depth.py", argv)
    assert r.returncode != 0 and r.stderr.strip().split("\n")[-2:] == ['ERROR!!! The file "%s/x.secondary.depth.gz" exists' % out,
                                                                       'Please use "-f" or "--force" to rewrite']
    # --cover 2: the second BAM of the command line gives the depth
    r = _run("filter_depth.py", ["-d", out, "-o", "y", "-t", "4", "--join", "--cover", "2", "--classes", "joined", "--chrs", "ctgB"] + argv[7:])
    assert r.returncode == 0, r.stderr[-2000:]
    rows2 = [ln.split("\t") for ln in open(os.path.join(out, "y.filter.txt")).read().splitlines()]
    assert [r[0] for r in rows2[2:6]] == order and "-" not in rows2[4] and rows2[3][1:7] == ["-"] * 6 and rows2[7] == ["contig", "joined"]
    assert [r[0] for r in rows2[8:]] == ["ctgB", "total"]
    # without --join: what the tool wrote before -- six classes, seven columns -- and its `kept` is the five classes of the join together
    r = _run("filter_depth.py", ["-d", out, "-o", "z", "-t", "4", paths[0]], dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(n for n in os.listdir(out) if n.startswith("z.")) == sorted(["z.%s.depth.gz" % c for c in pipeline.FATE_WANTED] + ["z.filter.txt"])
    rows3 = [ln.split("\t") for ln in open(os.path.join(out, "z.filter.txt")).read().splitlines()]
    assert rows3[1] == ["file"] + list(F.NAMES[:7]) and rows3[2] == rows[3][:8] and rows3[4] == ["contig"] + list(pipeline.FATE_WANTED)
    assert np.array_equal(_depth_lines(os.path.join(out, "z.kept.depth.gz")), five)
    for c in pipeline.FATE_WANTED[:5]:
        assert open(os.path.join(out, "z.%s.depth.gz" % c), "rb").read() == open(os.path.join(out, "x.%s.depth.gz" % c), "rb").read()
