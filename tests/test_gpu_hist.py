"""depth_dist.py on the GPU: gci_depth_hist (k_hist.hip) against the numpy statement (tests/hist_ref.py) for every byte of the
histogram and the statistics -- the outputs filled with 0xA5 beforehand, the bytes behind them untouched --, one larger case for the
flush path, the argument checks, and the command line on the reference's own MH63.depth.gz against the files the CPU twin's run
writes."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hist_cases as C
import hist_ref as R
from gci_amd import _lib, cpu, phases, pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH63 = os.path.join(ROOT, "tests", "golden", "MH63", "MH63.depth.gz")
PAD = 80                                                     # guard bytes behind every output


class Filled:
    """A device buffer of n + PAD bytes, every byte 0xA5."""

    def __init__(self, engine, n):
        self.engine, self.n = engine, int(n)
        self.buf = engine.T.empty(self.n + PAD, engine.T.uint8, engine.device)
        assert engine.lib.gci_memset(engine.ctx, engine._p(self.buf), 0xA5, self.n + PAD) == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr())

    def host(self, used):
        """-> the first `used` bytes; what lies behind them must still be 0xA5."""
        self.engine.sync()
        h = self.buf.cpu().numpy()
        assert (h[used:] == 0xA5).all(), "bytes outside the output were written"
        return h[:used]


def one_call(engine, c, n_bins, null_hist=False):
    """The export over a case -> (hist, stats) as it left them in 0xA5-filled buffers."""
    engine.set_layout(c["lengths"])
    assert engine.offsets == C.B.offsets(c["lengths"])[0]
    d_track = engine.to_device(c["track"])
    nw = len(c["windows"])
    arr = engine._window_array(c["windows"])
    hist, stats = Filled(engine, nw * (n_bins + 2) * 8), Filled(engine, nw * 32)
    assert engine.lib.gci_depth_hist(engine.ctx, engine._p(d_track), arr, nw, n_bins, None if null_hist else hist.ptr, stats.ptr) == 0
    h = hist.host(0 if null_hist else nw * (n_bins + 2) * 8).view(np.uint64).reshape(-1, n_bins + 2)
    return h, stats.host(nw * 32).view(np.int64).reshape(nw, 4)


@pytest.mark.parametrize("name, n_bins", C.PAIRS)
def test_the_device_equals_the_statement(engine, name, n_bins):
    want_hist, want_stats = C.want(name, n_bins)
    hist, stats = one_call(engine, C.case(name, n_bins), n_bins)
    assert np.array_equal(stats, want_stats)
    assert np.array_equal(hist, want_hist)
    assert (hist.sum(axis=1) == want_stats[:, 3].astype(np.uint64)).all()          # every element in exactly one column


def test_the_flush_path(engine):
    """4224 tiles in three windows (a third, the rest, the last 4099 elements): 68 chunks, each flushed once; depths reach 299, so
    n_bins = 256 leaves an over class."""
    c = C.case("flush_path", 256)
    want_hist, want_stats = C.want("flush_path", 256)
    hist, stats = one_call(engine, c, 256)
    assert np.array_equal(stats, want_stats) and np.array_equal(hist, want_hist) and (want_hist[:, 256] > 0).all()


def test_statistics_alone(engine):
    for name in ("extremes", "layout25", "chunk_run"):
        want_hist, want_stats = C.want(name, 0)
        hist, stats = one_call(engine, C.case(name, 0), 0, null_hist=True)      # no histogram: nothing is counted, the statistics stand
        assert hist.shape[0] == 0 and np.array_equal(stats, want_stats)


def test_the_engine_methods_the_cpu_twin_and_the_statement_agree(engine):
    assert engine.HIST_LDS_BINS == C.LDS == cpu.CpuEngine.HIST_LDS_BINS
    c = C.case("layout25", 64)
    twin = cpu.CpuEngine()
    twin.set_layout(c["lengths"])
    engine.set_layout(c["lengths"])
    d = engine.to_device(c["track"])
    for n_bins in (0, 64, C.LDS + 1):
        want_hist, want_stats = C.want("layout25", n_bins)
        for e, t in ((engine, d), (twin, c["track"])):
            hist, stats = e.depth_hist(t, c["windows"], n_bins)
            assert hist.dtype == np.uint64 and stats.dtype == np.int64
            assert np.array_equal(hist, want_hist) and np.array_equal(stats, want_stats)
    hist, stats = engine.depth_hist(d, [], 5)
    assert hist.shape == (0, 7) and stats.shape == (0, 4)
    hist, stats = engine.depth_hist(d, [(5, 5)], 3)
    assert hist.tolist() == [[0] * 5] and stats.tolist() == [[0, R.I32_MAX, R.I32_MIN, 0]]


def test_arguments(engine):
    from gci_amd.device import Engine
    lib, p = engine.lib, engine._p
    engine.set_layout([8])
    d = engine.to_device(np.zeros(engine.total, dtype=np.int32))
    arr = engine._window_array([(0, 8), (2, 1 << 40)])
    hist, stats = Filled(engine, 2 * 4 * 8), Filled(engine, 2 * 32)
    for args in ((None, p(d), arr, 2, 2, hist.ptr, stats.ptr), (engine.ctx, None, arr, 2, 2, hist.ptr, stats.ptr),
                 (engine.ctx, p(d), None, 2, 2, hist.ptr, stats.ptr), (engine.ctx, p(d), arr, 2, 2, hist.ptr, None),
                 (engine.ctx, p(d), arr, 2, 2, None, stats.ptr), (engine.ctx, p(d), arr, 2, _lib.HIST_MAX_BINS + 1, hist.ptr, stats.ptr),
                 (engine.ctx, p(d), arr, 1 << 31, 2, hist.ptr, stats.ptr)):
        assert lib.gci_depth_hist(*args) == _lib.GCI_E_INVALID
    bare = Engine(0)
    with pytest.raises(_lib.GciError) as err:
        bare.depth_hist(d, [(0, 4)], 2)
    assert err.value.status == _lib.GCI_E_NO_LAYOUT
    assert lib.gci_depth_hist(bare.ctx, p(d), arr, 2, 2, hist.ptr, stats.ptr) == _lib.GCI_E_NO_LAYOUT
    hist.host(0)                                                                  # a refused call writes nothing
    stats.host(0)
    assert lib.gci_depth_hist(engine.ctx, p(d), None, 0, 2, None, None) == 0     # no windows: nothing to write
    # a window pass like every other: the run writer's count call is no longer the last one that set windows
    run0, runs = Filled(engine, 3 * 8), Filled(engine, 64)
    assert lib.gci_depth_runs_count(engine.ctx, p(d), arr, 2, run0.ptr) == 0
    assert lib.gci_depth_hist(engine.ctx, p(d), arr, 2, 2, hist.ptr, stats.ptr) == 0
    assert lib.gci_depth_runs_write(engine.ctx, p(d), runs.ptr, 8) == _lib.GCI_E_INVALID
    assert hist.host(64).view(np.uint64).reshape(2, 4).tolist() == [[8, 0, 0, 0], [engine.total - 2, 0, 0, 0]]
    assert stats.host(64).view(np.int64).reshape(2, 4).tolist() == [[0, 0, 0, 8], [0, 0, 0, engine.total - 2]]


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def _files(prefix):
    return open(prefix + ".depth.summary.txt").read(), open(prefix + ".depth.hist.txt").read()


VARIANTS = {
    "whole": [],
    "chrs": ["--chrs", "Chr11_MH63,Chr03_MH63", "-q", "0,1/3,1"],
    "regions": ["-R", "{BED}", "--at-least", "1,5,10", "--max-depth", "20"],
}
REGIONS = [("Chr03_MH63", 1000, 2_000_000), ("Chr01_MH63", 0, 4097), ("Chr03_MH63", 1_500_000, 2_500_001), ("Chr12_MH63", 5, 5),
           ("Chr03_MH63", 1000, 2_000_000), ("Chr02_MH63", 4095, 35_000_000)]


@pytest.fixture(scope="module")
def cpu_files(tmp_path_factory):
    """What the command writes through the CPU twin (tests/test_hist_cpu.py holds those files to the statement)."""
    from gci_amd import dist_cli
    d = tmp_path_factory.mktemp("dist")
    bed = str(d / "r.bed")
    with open(bed, "w") as f:
        f.write("".join("%s\t%d\t%d\n" % r for r in REGIONS))
    e, tracks, _ = C.host_tracks(MH63)
    mp = pytest.MonkeyPatch()
    mp.setattr(pipeline, "default_engine", lambda: e)
    mp.setattr(pipeline, "read_depth_tracks", lambda engine, path, **kw: (tracks, dict(tracks.targets_length)))
    try:
        out = {}
        for name, argv in VARIANTS.items():
            dist_cli.main(["depth_dist.py"] + [a.replace("{BED}", bed) for a in argv] + [MH63, str(d / name)])
            out[name] = _files(str(d / name))
    finally:
        mp.undo()
    return bed, out


def _main(engine, argv):
    from gci_amd import dist_cli
    pipeline._ENGINE = engine
    phases.start()
    try:
        dist_cli.main(["depth_dist.py"] + argv)
        return phases.report()
    finally:
        phases.stop()


def test_the_command_on_mh63_writes_what_the_cpu_twin_s_run_writes(engine, cpu_files, tmp_path):
    bed, want = cpu_files
    for name, argv in VARIANTS.items():
        prefix = str(tmp_path / name)
        log = _main(engine, [a.replace("{BED}", bed) for a in argv] + [MH63, prefix])
        assert {"dist_stats", "dist_hist", "dist_write_files"} <= set(log["wall_s"])
        assert _files(prefix) == want[name], name
    rows = [ln.split("\t") for ln in want["whole"][0].split("\n")[:-1]]
    assert len(rows) == 14 and rows[-1][0] == "total" and rows[-1][3] == "395765488" and float(rows[-1][5]) > 0


def test_the_entry_point_on_the_native_provider(cpu_files, tmp_path):
    """`python depth_dist.py ...` as a user starts it: the library's own HBM buffers (no torch in the process), GCI_PHASES."""
    _, want = cpu_files
    log = str(tmp_path / "phases.json")
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1", GCI_PHASES=log)
    env.pop("GCI_HBM", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_dist.py"), MH63, str(tmp_path / "e")], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and r.stdout == "", r.stderr[-3000:]
    assert _files(str(tmp_path / "e")) == want["whole"]
    assert "dist_hist" in json.load(open(log))["wall_s"]
