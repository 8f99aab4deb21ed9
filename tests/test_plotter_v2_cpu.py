"""depth_plotter_v2.py off the GPU: gci_depth_classes of the CPU twin (+ gci_range_sums) against the utility's rules stated in
numpy, the lock-step reader and the parsers against the transcripts of the UNMODIFIED reference utility (tests/golden/dpv2_*,
tools/make_golden_plotter_v2.py), its refusals that end before any device work, and the entry point."""
import contextlib
import gzip
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plotter_v2_cases as V
from gci_amd import cpu, pipeline
from gci_amd.formats import depthfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = json.load(open(os.path.join(V.GOLDEN, "dpv2_errors.json")))


@pytest.fixture(scope="module")
def eng():
    e = cpu.CpuEngine()
    e.set_layout(V.LENGTHS)
    assert e.total == V.TOTAL and e.offsets.tolist() == V.OFFSETS
    return e


def test_the_window_rule_on_a_small_example():
    d = np.array([0, 1, 2, 3, 0, 0, 5, 5, 5, 5, 5, 5, 5, 5, 5, 0, 7])
    _, _, (means, starts, ends), _ = V.rules(d, 4, 5)
    assert means.tolist() == [2, 5, 5, 5, 7] and starts.tolist() == [1, 6, 10, 14, 16] and ends.tolist() == [3, 9, 13, 14, 16]


@pytest.mark.parametrize("low_below", V.LOW_BELOW)
@pytest.mark.parametrize("kind", V.TRACKS)
def test_depth_classes_of_the_cpu_twin(eng, kind, low_below):
    t = V.track(kind)
    wins = V.windows()
    zero, low, stats = eng.depth_classes(t, wins, low_below)
    assert len(zero) == len(low) == len(wins) and stats.shape == (len(wins), 2)
    for k, w in enumerate(wins):
        a, b = V.clip(w)
        want_zero, want_low, _, want_stats = V.rules(t[a:b], 1 << 30, low_below)
        incl = np.array([0, -1])
        assert np.array_equal(zero[k] + incl, want_zero), (k, w)
        assert np.array_equal(low[k] + incl, want_low), (k, w)
        assert tuple(stats[k].tolist()) == want_stats, (k, w)


def test_the_alternating_track_outgrows_the_first_key_buffer(eng):
    zero, _, _ = eng.depth_classes(V.track("alternating"), V.windows(), 5)
    assert 2 * sum(z.shape[0] for z in zero) > (1 << 16)      # (two keys a run: more than the device's first buffer holds, too)


def test_depth_classes_checks_its_arguments():
    e = cpu.CpuEngine()
    t = np.zeros(8, dtype=np.int32)
    with pytest.raises(cpu.CpuError) as err:
        e.depth_classes(t, [(0, 4)], 5)
    assert err.value.status == -10                              # GCI_E_NO_LAYOUT
    e.set_layout([8])
    keys, n, stats = np.zeros(4, np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.int64)
    w = (cpu._Window * 1)(cpu._Window(0, 4))
    p = cpu._p
    assert e.lib.gci_depth_classes(e.ctx, None, w, 1, 5, p(keys), 2, p(n), p(stats)) == -1
    assert e.lib.gci_depth_classes(e.ctx, p(t), None, 1, 5, p(keys), 2, p(n), p(stats)) == -1
    assert e.lib.gci_depth_classes(e.ctx, p(t), w, 1, 5, None, 2, p(n), p(stats)) == -1
    assert e.lib.gci_depth_classes(e.ctx, p(t), w, 1, 5, p(keys), 2, None, p(stats)) == -1
    assert e.lib.gci_depth_classes(e.ctx, p(t), w, 1, 5, p(keys), 2, p(n), None) == -1
    # a cap too small is reported through the counters: four zero bases are one run, two keys; cap 1 holds one
    assert e.lib.gci_depth_classes(e.ctx, p(t), w, 1, 5, p(keys), 1, p(n), p(stats)) == 0 and n.tolist() == [2, 0]
    assert e.lib.gci_depth_classes(e.ctx, p(t), w, 0, 5, None, 0, p(n), None) == 0 and n.tolist() == [0, 0]


@pytest.mark.parametrize("window_size", [1, 4, 100, 5000])
@pytest.mark.parametrize("kind", V.TRACKS)
def test_depth_profile_v2_on_the_cpu_twin(eng, kind, window_size):
    """pipeline.depth_profile_v2 over the twin: the window means bit-equal to np.mean of the int64 slices."""
    t = V.track(kind)
    names = ["c%d" % c for c in range(len(V.LENGTHS))]
    tracks = pipeline.DepthTracks(eng, dict(zip(names, V.LENGTHS)), t)
    its = V.items()
    got = pipeline.depth_profile_v2(tracks, [(names[c], s, e) for c, s, e in its], window_size, 5)
    assert len(got) == len(its)
    for g, (c, s, e) in zip(got, its):
        V.same_profile(g, t[V.OFFSETS[c] + s:V.OFFSETS[c] + e + 1], window_size, 5)
    assert pipeline.depth_profile_v2(tracks, [], window_size) == []


# ---- the host path's reader and the parsers ----------------------------------------------------------------------------------------

def _manifest(case):
    with open(os.path.join(V.GOLDEN, case, "manifest.json")) as f:
        return json.load(f)


def _reader_lines(stdout: str):
    """The lines of a transcript that the utility's reader prints."""
    keep = ("Processing last sequence: ", "All target sequences", "File reading ended")
    return [ln for ln in stdout.splitlines() if ln.startswith(keep) or (ln.startswith("Processing sequence: ") and ", remaining" in ln)]


def _arg(argv, flag):
    return V.sub(argv[argv.index(flag) + 1], "") if flag in argv else None


def test_the_cases_are_there():
    assert len(V.CASES) >= 6 and any(fn.endswith(".pdf") for c in V.CASES for fn in _manifest(c)["files"])
    assert all(0 < len(_manifest(c)["files"]) <= 4 for c in V.CASES)
    one_short = _manifest("dpv2_one_base_short")["stdout"]
    assert "Warning: No depth data for sequence s3" in one_short and "Successful: 2, Failed: 1" in one_short


@pytest.mark.parametrize("case", V.CASES)
def test_the_lockstep_reader_gives_the_reference_transcript(case):
    from gci_amd import plotter_v2_cli as cli
    m = _manifest(case)
    argv = m["argv"]
    targets = set(cli.parse_fai(_arg(argv, "-r")))
    if "--region" in argv:
        targets = {argv[argv.index("--region") + 1].split(":")[0]}
    elif "--regions" in argv:
        targets = set(cli.parse_bed(_arg(argv, "--regions")))
    said, seen = [], []
    files = [depthfile.open_depth_lines(p) if p else None for p in (_arg(argv, "--hifi"), _arg(argv, "--nano"))]
    for name, h, o in depthfile.lockstep_sequences(files[0], files[1], lambda nm: nm in targets, len(targets), said.append):
        seen.append((name, len(h), len(o)))
    assert said == _reader_lines(m["stdout"])
    # the figures' names carry the lengths the reader found
    whole = [fn for fn in m["files"] if "--region" not in argv and "--regions" not in argv]
    for fn in whole:
        name, span = fn.rsplit(".", 1)[0].rsplit("_", 1)
        assert (name, int(span.split("-")[1]) + 1) in [(nm, nh or no) for nm, nh, no in seen]
    if case not in V.PATH_OF and files[0] is not None:
        # headers that line up: the header sequence alone gives the same transcript
        with depthfile.open_depth_lines(_arg(argv, "--hifi")) as f:
            names = [ln.strip()[1:] for ln in f if ln.startswith(">")]
        said2 = []
        assert list(depthfile.conforming_sequences(names, lambda nm: nm in targets, len(targets), said2.append)) == [s[0] for s in seen]
        assert said2 == said


def test_lockstep_reader_quirks():
    """A header beside a data line drops that line; a bare '>' opens nothing and counts as nothing; what int() refuses is 0; the
    file that ends first ends the read; a name met again after it was yielded is not yielded twice at the end."""
    hifi = [">a\n", "1\n", "x\n", " 3 \n", ">b\n", "7\n", ">\n", "8\n", "9\n"]
    ont = [">a\n", "4\n", "5\n", ">b\n", "6\n", "6\n", "6\n", "6\n"]
    said = []
    got = list(depthfile.lockstep_sequences(iter(hifi), iter(ont), lambda nm: True, 5, said.append))
    #  step 4: ont's '>b' beside hifi ' 3 ' closes a; step 5: hifi's '>b' beside ont '6' closes the empty b and opens b again
    assert got == [("a", [1, 0], [4, 5]), ("b", [], [])]
    assert said == ["Processing sequence: a, remaining target sequences: 4", "Processing sequence: b, remaining target sequences: 3",
                    "File reading ended, processed 2 sequences in total"]
    said = []
    assert list(depthfile.lockstep_sequences(None, iter([">q\n", "2\n", ">r\n", "3\n"]), lambda nm: nm == "q", 1, said.append)) == [("q", [], [2])]
    assert said == ["Processing sequence: q, remaining target sequences: 0", "All target sequences have been processed, stopping reading",
                    "File reading ended, processed 1 sequences in total"]


def test_a_depth_beyond_int32_is_refused():
    """The stated deviation: such a line is outside the strict grammar, the lock-step read takes the file, and the upload refuses."""
    from gci_amd import plotter_v2_cli as cli
    (name, h, o), = depthfile.lockstep_sequences(iter([">s\n", "7\n", "2147483648\n"]), None, lambda nm: True, 1, lambda line: None)
    assert (name, h, o) == ("s", [7, 2147483648], [])
    with pytest.raises(SystemExit) as e:
        cli._upload(None, name, h)                                   # (refused before anything goes to an engine)
    assert str(e.value) == 'ERROR!!! The depth file holds a depth of "s" outside the 32-bit range (-2^31 .. 2^31 - 1), which is not supported'
    with pytest.raises(SystemExit) as e:
        cli._upload(None, name, [0, -2147483649])
    assert str(e.value).startswith("ERROR!!! The depth file holds a depth")
    assert cli._upload(None, name, o).length == 0                    # (no lines: nothing to upload)


class _HostEngine(cpu.CpuEngine):
    """The CPU twin where the command line expects an engine that uploads."""

    def to_device(self, a):
        return np.ascontiguousarray(a)


def test_figures_drawn_before_a_region_fails_stay_counted(monkeypatch, tmp_path, capsys):
    """Two regions of a sequence whose ONT depths are one base short: the first lies inside both and is drawn, the second meets the
    length mismatch.  The utility has counted the first by then: Successful 1, and the caller adds the one failure."""
    from gci_amd import plot_v2, plotter_v2_cli as cli
    drawn = []
    monkeypatch.setattr(plot_v2, "render", lambda spec: drawn.append((spec.path, spec.length, [l.kind for l in spec.layers])))
    e = _HostEngine()
    hifi, ont = cli._upload(e, "s", [3] * 100), cli._upload(e, "s", [0, 2] * 49 + [9])
    tally = {"successful": 0, "failed": 0}
    with pytest.raises(ValueError) as err:
        cli._plot_sequence("s", hifi, ont, [(0, 50), (10, 99), (20, 30)], 10, str(tmp_path), "png", tally)
    assert str(err.value) == ("Error: HiFi and ONT data length mismatch for sequence s. HiFi length: 90, ONT length: 89. "
                              "Both datasets must have the same length.")
    assert tally == {"successful": 1, "failed": 0}
    assert drawn == [(os.path.join(str(tmp_path), "s_0-50.png"), 51, ["hifi", "ont"])]
    assert capsys.readouterr().out == "  Generated: %s\n" % os.path.join(str(tmp_path), "s_0-50.png")
    # a sequence without depths is one failure and no exception
    cli._plot_sequence("t", cli._Side(), cli._Side(), None, 10, str(tmp_path), "png", tally)
    assert tally == {"successful": 1, "failed": 1} and capsys.readouterr().out == "Warning: No depth data for sequence t\n"


def test_the_parsers():
    from gci_amd import plotter_v2_cli as cli
    assert cli.parse_fai(os.path.join(V.DIN, "ref.fa.fai")) == {"s1": 13000, "s2": 4096, "s3": 700, "s4": 500}
    # sorted per sequence; the `#` line and the two-column row are skipped; ends are kept as written
    assert cli.parse_bed(os.path.join(V.DIN, "regions.bed")) == {"s1": [(2000, 5000), (4000, 7000), (4095, 4096)], "s3": [(600, 9999)]}
    args = cli.build_parser("depth_plotter_v2.py").parse_args(["-r", "x.fai"])
    assert (args.output_dir, args.output_format, args.window_size, args.max_depth_ratio, args.min_safe_depth) == ("images", "pdf", 1000, 3.0, 5)


def test_header_names_of_the_two_utilities():
    assert depthfile.header_name(b">a>b \n") == "b" and depthfile.header_name_v2(b">a>b \n") == "a>b"
    text = np.frombuffer(b">s\n1\n>s\n2\n", dtype=np.uint8)
    e = cpu.CpuEngine()
    counts, keys, bad = e.depth_text_index(text)
    line0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)          # first line of every tile, then the number of lines
    assert bad == (1 << 64) - 1
    assert depthfile.header_segments(text, keys, line0) is not None
    assert depthfile.header_segments(text, keys, line0, plotter_v2=True) is None          # a name twice: the lock-step read's


def test_the_inputs_sit_where_a_tile_ends():
    with gzip.open(os.path.join(V.DIN, "hifi.depth.gz"), "rt") as f:
        lines = f.read().split("\n")
    s1 = np.array([int(x) for x in lines[1:13001]])
    assert lines[0] == ">s1" and lines[13001] == ">s2"
    assert s1[4095] == 0 and 0 < s1[4096] < 5 and 0 < s1[8191] < 5 and s1[8192] == 0 and s1[4094] >= 5 and s1[4097] >= 5
    assert (s1[1000:1010] == 0).all() and ((s1[1010:1020] > 0) & (s1[1010:1020] < 5)).all() and s1[1020] == 5
    assert s1[0] == 0 and 0 < s1[-1] < 5 and (s1[6000:6350] == 0).all() and (s1[6350:6380] > 0).all() and s1[6380] == 0
    assert open(os.path.join(V.DIN, "hifi.depth"), "rb").read() == gzip.open(os.path.join(V.DIN, "hifi.depth.gz"), "rb").read()


# ---- refusals that need no device, and the entry point -------------------------------------------------------------------------------

def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, fn), root) for d, _, fns in os.walk(root) for fn in fns) if os.path.isdir(root) else []


def run_scenario(sc, out, monkeypatch, tmp_path):
    from gci_amd import plotter_v2_cli as cli
    monkeypatch.setenv("COLUMNS", "100")
    monkeypatch.chdir(tmp_path)
    so, se = io.StringIO(), io.StringIO()
    code, exc = "completed", None
    try:
        with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
            cli.main(["depth_plotter_v2.py"] + [V.sub(a, out) for a in sc["argv"]])
    except SystemExit as e:
        code = e.code
    except Exception as e:                                 # noqa: BLE001
        code, exc = "exception", {"type": type(e).__name__, "message": V.norm(str(e), out)}
    got = {"exit": code, "exception": exc, "stdout": V.norm(so.getvalue(), out), "stderr": V.norm(se.getvalue(), out),
           "made_out": os.path.isdir(out)}
    assert got == {k: sc[k] for k in got}, sc["name"]
    return _tree(out)


@pytest.mark.parametrize("sc", [s for s in SCENARIOS if not s["gpu"]], ids=lambda s: s["name"])
def test_refused_before_any_gpu_work(sc, tmp_path, monkeypatch):
    assert run_scenario(sc, str(tmp_path / "out"), monkeypatch, tmp_path) == sc["files"]


def test_the_scenarios_cover_the_ways_the_utility_ends_early():
    by = {s["name"]: s for s in SCENARIOS}
    assert set(by) == {"no_depth_file", "bad_region", "fai_missing", "depth_file_missing", "text_named_gz", "svg"}
    assert by["no_depth_file"]["exit"] == "completed" and by["bad_region"]["exit"] == "completed"        # messages, exit code 0
    assert by["text_named_gz"]["exception"]["type"] == "BadGzipFile" and by["svg"]["files"] == ["s3_0-699.svg"]


def test_entry_point_exists_and_imports_no_torch(tmp_path):
    script = os.path.join(ROOT, "depth_plotter_v2.py")
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1")                 # (main() ends with an error if the run imported torch)
    r = subprocess.run([sys.executable, script, "-r", "x.fai"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=env)
    assert r.returncode == 0 and r.stdout == "Error: Must provide at least one depth file (--hifi or --nano)\n", r.stderr
    assert not os.path.exists(tmp_path / "images")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=env)
    assert r.returncode == 2 and "the following arguments are required: -r/--fai" in r.stderr
