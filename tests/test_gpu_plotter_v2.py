"""depth_plotter_v2.py on the GPU: gci_depth_classes against the CPU twin field for field, the command line against the files and
transcripts of the UNMODIFIED reference utility (tests/golden/dpv2_*, tools/make_golden_plotter_v2.py) -- file names, stdout and
stderr, the PNG figures pixel for pixel, and which path ran --, a file of this project's own writer through the compressed-domain
read, and the entry point as a user starts it."""
import gzip
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import plotter_v2_cases as V
from gci_amd import cpu, phases, pipeline
from test_plotter_v2_cpu import SCENARIOS, run_scenario

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    e = cpu.CpuEngine()
    e.set_layout(V.LENGTHS)
    return e


@pytest.mark.parametrize("low_below", V.LOW_BELOW)
@pytest.mark.parametrize("kind", V.TRACKS)
def test_depth_classes_equals_the_cpu_twin(engine, twin, kind, low_below):
    """The alternating track has more keys per class than the first key buffer holds: the grow-and-retry runs."""
    engine.set_layout(V.LENGTHS)
    assert engine.total == V.TOTAL
    t = V.track(kind)
    wins = V.windows()
    zero, low, stats = engine.depth_classes(engine.to_device(t), wins, low_below)
    want_zero, want_low, want_stats = twin.depth_classes(t, wins, low_below)
    assert len(zero) == len(low) == len(wins)
    for k in range(len(wins)):
        assert np.array_equal(zero[k], want_zero[k]), (k, wins[k])
        assert np.array_equal(low[k], want_low[k]), (k, wins[k])
    assert stats.dtype == np.int64 and np.array_equal(stats, want_stats)


def test_depth_classes_without_windows_and_without_a_layout(engine):
    from gci_amd.device import Engine
    from gci_amd._lib import GciError, GCI_E_NO_LAYOUT
    engine.set_layout(V.LENGTHS)
    d = engine.to_device(V.track("random"))
    zero, low, stats = engine.depth_classes(d, [], 5)
    assert zero == [] and low == [] and stats.shape == (0, 2)
    zero, low, stats = engine.depth_classes(d, [(700, 700)], 5)                   # windows, but no tile to read
    assert zero[0].shape == (0, 2) and low[0].shape == (0, 2) and stats.tolist() == [[0, 0]]
    bare = Engine(0)
    with pytest.raises(GciError) as e:
        bare.depth_classes(d, [(0, 4)], 5)
    assert e.value.status == GCI_E_NO_LAYOUT


@pytest.mark.parametrize("window_size", [4, 100])
@pytest.mark.parametrize("kind", ["alternating", "random"])
def test_depth_profile_v2_follows_the_utility_rules(engine, kind, window_size):
    t = V.track(kind)
    engine.set_layout(V.LENGTHS)
    names = ["c%d" % c for c in range(len(V.LENGTHS))]
    tracks = pipeline.DepthTracks(engine, dict(zip(names, V.LENGTHS)), engine.to_device(t))
    its = V.items()
    got = pipeline.depth_profile_v2(tracks, [(names[c], s, e) for c, s, e in its], window_size, 5)
    for g, (c, s, e) in zip(got, its):
        V.same_profile(g, t[V.OFFSETS[c] + s:V.OFFSETS[c] + e + 1], window_size, 5)


# ---- the command line against the reference utility's files ---------------------------------------------------------------------

def _manifest(case):
    with open(os.path.join(V.GOLDEN, case, "manifest.json")) as f:
        return json.load(f)


def _pixels(path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.image as mpimg
    return mpimg.imread(path)


def _same_outputs(out, case, m):
    want_dir = os.path.join(V.GOLDEN, case, "expected")
    assert sorted(os.listdir(out)) == m["files"]
    kept = sorted(os.listdir(want_dir)) if os.path.isdir(want_dir) else []
    assert kept == [fn for fn in m["files"] if fn.endswith(".png")]              # every PNG of the reference is held, nothing else
    for fn in kept:
        a, b = _pixels(os.path.join(out, fn)), _pixels(os.path.join(want_dir, fn))
        assert a.shape == b.shape and np.array_equal(a, b), fn
    for fn in m["files"]:
        assert os.path.getsize(os.path.join(out, fn)) > 0, fn            # (PDF figures: only that they are there)


def _run_logged(argv):
    """plotter_v2_cli.main with the phase log on -> its notes."""
    from gci_amd import plotter_v2_cli
    phases.start()
    try:
        plotter_v2_cli.main(argv)
        return phases.report()["notes"]
    finally:
        phases.stop()


@pytest.mark.parametrize("case", V.CASES)
def test_plotter_v2_reproduces_the_reference_utility(engine, case, tmp_path, capsys):
    out = str(tmp_path / "out")
    m = _manifest(case)
    pipeline._ENGINE = engine
    notes = _run_logged(["depth_plotter_v2.py"] + [V.sub(a, out) for a in m["argv"]])
    cap = capsys.readouterr()
    assert V.norm(cap.out, out) == m["stdout"] and V.norm(cap.err, out) == m["stderr"]
    _same_outputs(out, case, m)
    assert notes["plotter_v2"] == V.PATH_OF.get(case, "device")
    if case == "dpv2_text_regions":                                      # a name without .gz: the bytes are the text
        assert notes["depth_read:" + os.path.join(V.DIN, "hifi.depth")] == "text"


def test_the_ignored_flags_are_ignored(engine, tmp_path, capsys):
    """--min-safe-depth and --max-depth-ratio change nothing: the case that gives them, run without them, draws the same pixels."""
    case = "dpv2_ont_region_ignored_flags"
    out = str(tmp_path / "out")
    m = _manifest(case)
    argv = [V.sub(a, out) for a in m["argv"]]
    for flag in ("--min-safe-depth", "--max-depth-ratio"):
        del argv[argv.index(flag):argv.index(flag) + 2]
    pipeline._ENGINE = engine
    _run_logged(["depth_plotter_v2.py"] + argv)
    _same_outputs(out, case, m)
    capsys.readouterr()


@pytest.mark.parametrize("sc", [s for s in SCENARIOS if s["gpu"]], ids=lambda s: s["name"])
def test_scenarios_that_reach_the_device(engine, sc, tmp_path, monkeypatch):
    pipeline._ENGINE = engine
    assert run_scenario(sc, str(tmp_path / "out"), monkeypatch, tmp_path) == sc["files"]


def test_a_file_of_this_projects_writer_is_read_in_the_compressed_domain(engine, tmp_path):
    """The HiFi input written again by Engine.depth_deflate: read as members, and every number equal to the text path's."""
    src = os.path.join(V.DIN, "hifi.depth.gz")
    pipeline._ENGINE = engine
    phases.start()
    try:
        text_tracks, lengths = pipeline.read_depth_tracks(engine, src, None, plotter_v2=True)
        assert list(lengths.items()) == [("s1", 13000), ("s2", 4096), ("s3", 700)]
        own = str(tmp_path / "own.depth.gz")
        with open(own, "wb") as f:
            for name, blob in zip(text_tracks.targets, engine.depth_deflate(text_tracks.track)):
                c = zlib.compressobj(1, zlib.DEFLATED, 31)
                f.write(c.compress(b">%s\n" % name.encode()) + c.flush() + bytes(blob))
        assert gzip.open(own, "rb").read() == gzip.open(src, "rb").read()
        own_tracks, own_lengths = pipeline.read_depth_tracks(engine, own, None, plotter_v2=True)
        notes = phases.report()["notes"]
    finally:
        phases.stop()
    assert notes["depth_read:" + src] == "text" and notes["depth_read:" + own] == "members"
    assert own_lengths == lengths
    items = [("s1", 0, 12999), ("s1", 4095, 4096), ("s2", 0, 4095), ("s3", 600, 699)]
    a = pipeline.depth_profile_v2(text_tracks, items, 100)
    b = pipeline.depth_profile_v2(own_tracks, items, 100)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for key in x:
            assert np.array_equal(x[key], y[key]), key
    assert sum(p["n_pos"] for p in a) > 0 and all(p["means"].shape[0] for p in a)


def test_the_other_depth_tools_still_go_by_the_bytes_not_the_name(engine, tmp_path):
    """Only depth_plotter_v2.py takes a name without `.gz` for plain text.  For GCI_score.py and plot_depth.py (read_depth_tracks
    without plotter_v2) a gzip file is read whatever it is called, and plain text raises gzip's own exception, as their utilities do."""
    import shutil
    odd = str(tmp_path / "hifi.depth")                                          # gzip bytes behind a name without .gz
    shutil.copy(os.path.join(V.DIN, "hifi.depth.gz"), odd)
    tracks, lengths = pipeline.read_depth_tracks(engine, odd)
    assert list(lengths.items()) == [("s1", 13000), ("s2", 4096), ("s3", 700)]
    want, _ = pipeline.read_depth_tracks(engine, os.path.join(V.DIN, "hifi.depth.gz"))
    for t in lengths:
        assert np.array_equal(tracks[t], want[t])
    with pytest.raises(gzip.BadGzipFile):
        pipeline.read_depth_tracks(engine, os.path.join(V.DIN, "hifi.depth"))    # plain text
    # ... and for depth_plotter_v2.py the same gzip bytes are "text" outside the grammar: not the device path's
    assert pipeline.read_depth_tracks(engine, odd, None, plotter_v2=True) == (None, {})


def test_the_entry_point_on_the_native_provider(tmp_path):
    """`python depth_plotter_v2.py ...` as a user starts it: the library's own HBM buffers (no torch in the process), same files."""
    case = "dpv2_text_regions"
    out = str(tmp_path / "out")
    log = str(tmp_path / "phases.json")
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1", GCI_PHASES=log)
    env.pop("GCI_HBM", None)
    m = _manifest(case)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_plotter_v2.py")] + [V.sub(a, out) for a in m["argv"]],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert V.norm(r.stdout, out) == m["stdout"]
    _same_outputs(out, case, m)
    assert json.load(open(log))["notes"]["plotter_v2"] == "device"
