"""depth_dist.py off the GPU: the numpy statement (tests/hist_ref.py) against a per-base loop, the CPU twin of gci_depth_hist against
the statement on the shapes the device is tested on, the arguments the export checks, pipeline.depth_distribution's batching, and the
command line through the CPU twin on the reference's own MH63.depth.gz: both files against the statement's text computed from the
gunzipped lines, --chrs, -R, --max-depth, -q, the refusals and -f."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hist_cases as C
import hist_ref as R
from bedgraph_ref import clip
from gci_amd import _lib, cpu, pipeline
from gci_amd.formats import depthfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH63 = os.path.join(ROOT, "tests", "golden", "MH63", "MH63.depth.gz")
A5 = 0xA5A5A5A5A5A5A5A5


def loop_hist(seg, n_bins):
    """The definition, base by base."""
    h, total, lo, hi = [0] * (n_bins + 2), 0, R.I32_MAX, R.I32_MIN
    for d in (int(x) for x in seg):
        h[n_bins + 1 if d < 0 else n_bins if d >= n_bins else d] += 1
        total, lo, hi = total + d, min(lo, d), max(hi, d)
    return h, [total, lo, hi, len(seg)]


@pytest.mark.parametrize("name, n_bins", [("extremes", 2), ("window_edges", 5), ("last_bin", 64)])
def test_the_statement_equals_a_loop_over_the_bases(name, n_bins):
    c = C.case(name, n_bins)
    H, S = C.want(name, n_bins)
    for k, w in enumerate(c["windows"]):
        a, b = clip(w, c["track"].shape[0])
        h, s = loop_hist(c["track"][a:b], n_bins)
        assert H[k].tolist() == h and S[k].tolist() == s
        assert int(H[k].sum()) == b - a                          # every element lands in exactly one column
    assert R.quantile(np.array([2, 0, 1, 1]), 4, "1/2", 3) == "0" and R.quantile(np.array([2, 0, 1, 1]), 4, "3/4", 3) == "2"
    x = np.sort(np.random.default_rng(31).integers(0, 9, 101))
    for q in ("0", "1/3", "0.5", "0.99", "1"):
        k = max(1, -(-R.Fraction(q).numerator * 101 // R.Fraction(q).denominator))
        assert R.quantile(np.bincount(x, minlength=9), 101, q, 8) == str(x[k - 1])
    assert R.quantile(np.array([3]), 5, "1", 0) == ">0"          # two of the five bases lie in the over class


def test_the_constants_are_the_header_s():
    from gci_amd.device import Engine
    hdr = open(os.path.join(ROOT, "include", "gci_hip.h")).read()
    hip = open(os.path.join(ROOT, "gci_amd", "csrc", "k_hist.hip")).read()
    assert int(re.search(r"#define GCI_HIST_MAX_BINS\s+(\d+)", hdr).group(1)) == _lib.HIST_MAX_BINS == 65536
    assert int(re.search(r"#define GCI_HIST_CHUNK_TILES\s+(\d+)", hdr).group(1)) == _lib.HIST_CHUNK_TILES == C.CT
    assert int(re.search(r"#define GCI_HIST_LDS_BINS\s+(\d+)", hip).group(1)) == Engine.HIST_LDS_BINS == cpu.CpuEngine.HIST_LDS_BINS == C.LDS
    assert C.CT * C.TILE < 2 ** 32 and 2 < C.LDS < _lib.HIST_MAX_BINS


@pytest.mark.parametrize("name, n_bins", C.PAIRS)
def test_the_cpu_twin_equals_the_statement(name, n_bins):
    c = C.case(name, n_bins)
    e = cpu.CpuEngine()
    e.set_layout(c["lengths"])
    want_hist, want_stats = C.want(name, n_bins)
    hist, stats = e.depth_hist(c["track"], c["windows"], n_bins)
    assert hist.dtype == np.uint64 and stats.dtype == np.int64
    assert np.array_equal(stats, want_stats)
    assert np.array_equal(hist, want_hist)


def test_the_twin_checks_its_arguments():
    p, W = cpu._p, cpu._Window
    t = np.array([1, 1, 2, -2, 2, 3, 0, 0], dtype=np.int32)
    w = (W * 3)(W(-5, 4), W(4, 1 << 40), W(6, 2))                # clamped to [0, 4), [4, total) and empty
    hist, stats = np.full(3 * 4, A5, dtype=np.uint64), np.full(3 * 4, A5, dtype=np.uint64)
    e = cpu.CpuEngine()
    assert e.lib.gci_depth_hist(e.ctx, p(t), w, 3, 2, p(hist), p(stats)) == _lib.GCI_E_NO_LAYOUT
    e.set_layout([8])
    t = np.concatenate([t, np.zeros(e.total - 8, np.int32)])
    for args in ((None, p(t), w, 3, 2, p(hist), p(stats)), (e.ctx, None, w, 3, 2, p(hist), p(stats)), (e.ctx, p(t), None, 3, 2, p(hist), p(stats)),
                 (e.ctx, p(t), w, 3, 2, p(hist), None), (e.ctx, p(t), w, 3, 2, None, p(stats)), (e.ctx, p(t), w, 3, 65537, p(hist), p(stats)),
                 (e.ctx, p(t), w, 1 << 31, 2, p(hist), p(stats))):
        assert e.lib.gci_depth_hist(*args) == _lib.GCI_E_INVALID
        assert (hist == A5).all() and (stats == A5).all()       # a refused call writes nothing
    assert e.lib.gci_depth_hist(e.ctx, p(t), w, 3, 2, p(hist), p(stats)) == 0
    assert hist.reshape(3, 4).tolist() == [[0, 2, 1, 1], [e.total - 6, 0, 2, 0], [0, 0, 0, 0]]
    assert stats.view(np.int64).reshape(3, 4).tolist() == [[2, -2, 2, 4], [5, 0, 3, e.total - 4], [0, R.I32_MAX, R.I32_MIN, 0]]
    stats[:] = A5                                                # statistics only: over / under, or no histogram at all
    assert e.lib.gci_depth_hist(e.ctx, p(t), w, 3, 0, p(hist), p(stats)) == 0
    assert hist[:6].reshape(3, 2).tolist() == [[3, 1], [e.total - 4, 0], [0, 0]]
    hist[:] = A5
    assert e.lib.gci_depth_hist(e.ctx, p(t), w, 3, 0, None, p(stats)) == 0 and (hist == A5).all()
    assert stats.view(np.int64).reshape(3, 4)[:, 0].tolist() == [2, 5, 0]
    assert e.lib.gci_depth_hist(e.ctx, p(t), None, 0, 2, None, None) == 0          # no windows: nothing to write


# ---- pipeline.depth_distribution and the command line through the CPU twin -----------------------------------------------------------

_HostEngine = C.HostEngine


def _host_reader(engine, path, ref_lengths=None, plotter_v2=False):
    """pipeline.read_depth_tracks by the reference's own statements, into the twin's memory."""
    with gzip.open(path, "rb") as f:
        depths = depthfile.parse_depth_lines(f)
    return pipeline._upload_depths(engine, depths)


DEPTHS = {"chrA": [3] * 10 + [0] * 5 + [7], "chrB": [1, 2, 2], "chrC": [9] * 4, "chrD": [70000, 1]}


@pytest.fixture()
def depth_gz(tmp_path):
    path = str(tmp_path / "in.depth.gz")
    with gzip.open(path, "wb") as f:
        for name, d in DEPTHS.items():
            f.write(b">%s\n" % name.encode() + b"".join(b"%d\n" % x for x in d))
    return path


def test_depth_distribution_in_batches_equals_one_round(depth_gz, monkeypatch):
    tracks, _ = _host_reader(_HostEngine(), depth_gz)
    items = [("chrA", 0, 16), ("chrB", 1, 3), ("chrA", 8, 16), ("chrC", 2, 2), ("chrD", 0, 2), ("chrA", 0, 5), ("chrC", 0, 4)]
    depths = {k: np.array(v) for k, v in DEPTHS.items()}
    whole_h, whole_s = pipeline.depth_distribution(tracks, items)
    want_h, want_s = R.distribution(depths, items)
    assert whole_h.shape == (7, 65536 + 2) and np.array_equal(whole_h, want_h) and np.array_equal(whole_s, want_s)
    calls = []
    real = tracks.engine.depth_hist
    monkeypatch.setattr(tracks.engine, "depth_hist", lambda t, w, n: calls.append((len(w), n)) or real(t, w, n), raising=False)
    monkeypatch.setattr(pipeline, "DIST_HIST_BUDGET", 3 * 65538 * 8)             # three items' histogram a round
    h, s = pipeline.depth_distribution(tracks, items)
    assert np.array_equal(h, whole_h) and np.array_equal(s, whole_s)
    assert calls == [(7, 0), (3, 65536), (3, 65536), (1, 65536)]
    monkeypatch.setattr(pipeline, "DIST_HIST_BUDGET", 1)                         # never less than one item a round
    calls.clear()
    h, s = pipeline.depth_distribution(tracks, items[:2], max_depth=2)
    assert calls == [(1, 0), (1, 0), (1, 3), (1, 3)] and np.array_equal(h, R.distribution(depths, items[:2], 2)[0])
    # None: every contig whole; every item empty: one bin; items outside their contig
    h, s = pipeline.depth_distribution(tracks)
    assert np.array_equal(h, R.distribution(depths, [(k, 0, len(v)) for k, v in DEPTHS.items()])[0])
    h, s = pipeline.depth_distribution(tracks, [("chrB", 3, 3)])
    assert h.tolist() == [[0, 0, 0]] and s.tolist() == [[0, R.I32_MAX, R.I32_MIN, 0]]
    h, s = pipeline.depth_distribution(tracks, [])
    assert h.shape == (0, 3) and s.shape == (0, 4)
    with pytest.raises(ValueError):
        pipeline.depth_distribution(tracks, [("chrB", 0, 4)])
    with pytest.raises(ValueError):
        pipeline.depth_distribution(tracks, max_depth=65536)


@pytest.fixture(scope="module")
def mh63(oracle):
    """The reference's own MH63.depth.gz, read once: the per-base arrays from its gunzipped lines (the oracle's parser) for the
    statement, and the same text through the CPU twin's reader (gci_depth_text_index / _parse) for the command."""
    e, tracks, text = C.host_tracks(MH63)
    depths = oracle.parse_depth_text(text)
    names, lengths = tracks.targets, tracks.lengths
    assert names == list(depths) and lengths == [int(v.shape[0]) for v in depths.values()]
    return e, tracks, depths


@pytest.fixture()
def cli(monkeypatch, mh63):
    from gci_amd import dist_cli
    e, tracks, _ = mh63

    def reader(engine, path, ref_lengths=None, plotter_v2=False):
        if path == MH63:
            return tracks, dict(tracks.targets_length)
        return _host_reader(engine, path)
    monkeypatch.setattr(pipeline, "default_engine", lambda: e)
    monkeypatch.setattr(pipeline, "read_depth_tracks", reader)
    return dist_cli


def _files(prefix):
    return open(prefix + ".depth.summary.txt").read(), open(prefix + ".depth.hist.txt").read()


def _want_files(depths, items, with_total, quantiles=("0.25", "0.5", "0.75"), at_least=(1,), max_depth=65535):
    H, S = R.distribution(depths, items, max_depth)
    return R.summary(items, H, S, list(quantiles), list(at_least), max_depth, with_total), R.histogram(items, H, S, max_depth, with_total)


def test_mh63_whole_and_its_total_mean(cli, mh63, tmp_path):
    _, _, depths = mh63
    prefix = str(tmp_path / "mh63")
    assert cli.main(["depth_dist.py", MH63, prefix]) == (prefix + ".depth.summary.txt", prefix + ".depth.hist.txt")
    items = [(k, 0, int(v.shape[0])) for k, v in depths.items()]
    summary, hist = _files(prefix)
    assert (summary, hist) == _want_files(depths, items, True)
    rows = [ln.split("\t") for ln in summary.split("\n")[:-1]]
    assert rows[0] == ["#name", "start", "end", "bases", "covered", "mean", "min", "q0.25", "q0.5", "q0.75", "max", "ge1"] and len(rows) == 14
    total, bases = sum(int(v.sum()) for v in depths.values()), sum(int(v.shape[0]) for v in depths.values())
    assert rows[-1][:4] == ["total", "0", str(bases), str(bases)] and rows[-1][5] == "%.4f" % (total / bases)      # the value for plot_depth.py -dmean
    assert hist.startswith("#name\tstart\tend\tdepth\tbases\tat_least\nChr01_MH63\t0\t") and all(re.fullmatch(r"[^\t]+(\t\d+){5}", ln) for ln in hist.split("\n")[1:-1])


def test_mh63_chrs_regions_max_depth_and_quantiles(cli, mh63, tmp_path):
    _, _, depths = mh63
    prefix = str(tmp_path / "o")
    L = {k: int(v.shape[0]) for k, v in depths.items()}
    cli.main(["depth_dist.py", "--chrs", "Chr07_MH63,Chr02_MH63", MH63, prefix])             # the file's order, not the option's
    assert _files(prefix) == _want_files(depths, [("Chr02_MH63", 0, L["Chr02_MH63"]), ("Chr07_MH63", 0, L["Chr07_MH63"])], True)
    regions = [("Chr03_MH63", 1000, 2_000_000), ("Chr01_MH63", 0, 4097), ("Chr03_MH63", 1_500_000, 2_500_001), ("Chr12_MH63", 5, 5),
               ("Chr03_MH63", 1000, 2_000_000), ("Chr12_MH63", L["Chr12_MH63"] - 3, L["Chr12_MH63"])]      # overlapping, repeated, empty
    bed = str(tmp_path / "r.bed")
    with open(bed, "w") as f:
        f.write("".join("%s\t%d\t%d\n" % r for r in regions))
    cli.main(["depth_dist.py", "-f", "-R", bed, "--at-least", "1,5,10", MH63, prefix])
    assert _files(prefix) == _want_files(depths, regions, False, at_least=(1, 5, 10))
    assert "total" not in _files(prefix)[0] and "\nChr12_MH63\t5\t5\t0\t0\tnan\tnan\tnan\tnan\tnan\tnan\t0\t0\t0\n" in _files(prefix)[0]
    cli.main(["depth_dist.py", "-f", "--max-depth", "20", "-q", "0.5,0.9999999", "--at-least", "0,21", "--chrs", "Chr05_MH63", MH63, prefix])
    items = [("Chr05_MH63", 0, L["Chr05_MH63"])]
    got = _files(prefix)
    assert got == _want_files(depths, items, True, quantiles=("0.5", "0.9999999"), at_least=(0, 21), max_depth=20)
    assert "\t>20\t" in got[0] and re.search(r"\nChr05_MH63\t0\t\d+\t>20\t(\d+)\t\1\ntotal\t", got[1])
    cli.main(["depth_dist.py", "--force", "-q", "0,1/3,1", "--chrs", "Chr09_MH63", MH63, prefix])
    got = _files(prefix)
    assert got == _want_files(depths, [("Chr09_MH63", 0, L["Chr09_MH63"])], True, quantiles=("0", "1/3", "1"))
    x = depths["Chr09_MH63"]
    row = got[0].split("\n")[1].split("\t")
    assert got[0].split("\n")[0].split("\t")[7:10] == ["q0", "q1/3", "q1"]
    assert row[6] == row[7] == str(int(x.min())) and row[9] == row[10] == str(int(x.max()))
    assert row[8] == str(int(np.partition(x, -(-x.shape[0] // 3) - 1)[-(-x.shape[0] // 3) - 1]))            # np.sort(x)[k - 1], k = ceil(n / 3)


def _run(cli, argv):
    with pytest.raises(SystemExit) as e:
        cli.main(["depth_dist.py"] + argv)
    return e.value.code


def test_the_refusals_and_force(cli, depth_gz, tmp_path):
    prefix = str(tmp_path / "out")
    cli.main(["depth_dist.py", depth_gz, prefix])
    depths = {k: np.array(v) for k, v in DEPTHS.items()}
    assert _files(prefix) == _want_files(depths, [(k, 0, len(v)) for k, v in DEPTHS.items()], True)
    for gone in (".depth.summary.txt", ".depth.hist.txt"):                        # either file in the way refuses
        keep = open(prefix + gone).read()
        other = prefix + (".depth.hist.txt" if gone == ".depth.summary.txt" else ".depth.summary.txt")
        os.remove(other)
        assert _run(cli, [depth_gz, prefix]) == 'ERROR!!! The file "%s%s" exists\nPlease use "-f" or "--force" to rewrite' % (prefix, gone)
        assert not os.path.exists(other) and open(prefix + gone).read() == keep
        cli.main(["depth_dist.py", "-f", depth_gz, prefix])
    fresh = str(tmp_path / "fresh")
    bed = str(tmp_path / "r.bed")
    open(bed, "w").write("chrA\t0\t17\n")
    for argv, message in [
        (["--chrs", "chrA,chrZ"], 'ERROR!!! The chromosome "chrZ" is not in the depth file'),
        (["-R", bed], "ERROR!!! The region chrA:0-17 of the bed file ends beyond the contig (16 bases)"),
        (["-q", "0.5,x"], 'ERROR!!! The quantile "x" is not a number'),
        (["-q", "3/2"], 'ERROR!!! The quantile "3/2" is not in [0, 1]'),
        (["--at-least", "1.5"], 'ERROR!!! The depth "1.5" of --at-least is not an integer'),
        (["--max-depth", "20", "--at-least", "22"], 'ERROR!!! The depth "22" of --at-least is not in [0, 21] (--max-depth + 1)'),
        (["--max-depth", "65536"], "ERROR!!! --max-depth 65536 is not in [0, 65535]"),
    ]:
        assert _run(cli, argv + [depth_gz, fresh]) == message
        assert not os.path.exists(fresh + ".depth.summary.txt") and not os.path.exists(fresh + ".depth.hist.txt")


def test_a_negative_depth_is_refused(cli, tmp_path, monkeypatch):
    e = _HostEngine()
    tracks, lengths = pipeline._upload_depths(e, {"c1": np.array([1, 2, 3]), "c2": np.array([4, -1, 4]), "c3": np.array([-5])})
    monkeypatch.setattr(pipeline, "default_engine", lambda: e)
    monkeypatch.setattr(pipeline, "read_depth_tracks", lambda engine, path, **kw: (tracks, lengths))
    prefix = str(tmp_path / "neg")
    assert _run(cli, ["any.depth.gz", prefix]) == 'ERROR!!! The depth file holds a negative depth on "c2"'
    assert not os.path.exists(prefix + ".depth.summary.txt") and not os.path.exists(prefix + ".depth.hist.txt")
    cli.main(["depth_dist.py", "--chrs", "c1", "any.depth.gz", prefix])           # (the items alone are looked at)
    assert _files(prefix)[1] == "#name\tstart\tend\tdepth\tbases\tat_least\nc1\t0\t3\t1\t1\t3\nc1\t0\t3\t2\t1\t2\nc1\t0\t3\t3\t1\t1\ntotal\t0\t3\t1\t1\t3\ntotal\t0\t3\t2\t1\t2\ntotal\t0\t3\t3\t1\t1\n"


def test_entry_point_exists_and_imports_no_torch(tmp_path):
    script = os.path.join(ROOT, "depth_dist.py")
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1")
    (tmp_path / "there.depth.hist.txt").write_bytes(b"")
    r = subprocess.run([sys.executable, script, "x.depth.gz", "there"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=env)
    assert r.returncode == 1 and r.stderr.startswith('ERROR!!! The file "there.depth.hist.txt" exists\nPlease use "-f" or "--force" to rewrite')
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=env)
    assert r.returncode == 2 and "the following arguments are required: input.depth.gz, output_prefix" in r.stderr
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=env)
    assert r.returncode == 0 and "-dmean" in r.stdout
