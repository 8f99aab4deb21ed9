"""GCI_score.py on the GPU: the re-scoring command line against files and transcripts of the UNMODIFIED reference utility
(tests/golden/score_*, tools/make_golden_score.py), its refusals that get as far as device work, the device parse
(k_depth_parse.hip) against its CPU twin, and a genome-size round trip through this project's own `.depth.gz` writer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLDEN
from gci_amd import pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_IN = os.path.join(GOLDEN, "score_inputs")
CASES = sorted(d for d in os.listdir(GOLDEN) if d.startswith("score_") and os.path.isdir(os.path.join(GOLDEN, d, "expected")))
NONE = (1 << 64) - 1


def _manifest(case):
    with open(os.path.join(GOLDEN, case, "manifest.json")) as f:
        return json.load(f)


def _sub(argv, out):
    return [a.replace("{GOLDEN}", GOLDEN).replace("{IN}", SCORE_IN).replace("{OUT}", out) for a in argv]


def _norm(text, out):
    return text.replace(out, "{OUT}").replace(SCORE_IN, "{IN}").replace(GOLDEN, "{GOLDEN}")


def _files(d):
    return {fn: open(os.path.join(d, fn), "rb").read() for fn in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, fn))}


@pytest.mark.parametrize("case", CASES)
def test_score_cli_reproduces_the_reference_utility(engine, case, tmp_path, capsys):
    from gci_amd import score_cli
    out = str(tmp_path / "out")
    m = _manifest(case)
    pipeline._ENGINE = engine
    score_cli.main(["GCI_score.py"] + _sub(m["argv"], out))
    got, want = _files(out), _files(os.path.join(GOLDEN, case, "expected"))
    assert sorted(got) == sorted(want) == m["files"]
    for fn in want:
        assert got[fn] == want[fn], fn
    cap = capsys.readouterr()
    assert _norm(cap.out, out) == m["stdout"] and _norm(cap.err, out) == m["stderr"]
    # refuses to overwrite without -f, like the reference; -f writes the same files again
    plain = [a for a in m["argv"] if a != "-f"]
    with pytest.raises(SystemExit) as e:
        score_cli.main(["GCI_score.py"] + _sub(plain, out))
    assert "exists" in str(e.value) and "--force" in str(e.value)
    score_cli.main(["GCI_score.py"] + _sub(plain, out) + ["-f"])
    assert _files(out) == got
    capsys.readouterr()


def test_score_refusals_after_device_work(engine, tmp_path, monkeypatch):
    """The scenarios of score_errors.json that get as far as the device, in their order (one of them finds the files the one before
    it wrote): the exit message, or the reference's uncaught exception, and the transcript up to it."""
    from test_score_cpu import SCENARIOS, run_score_scenario
    pipeline._ENGINE = engine
    out = str(tmp_path / "out")
    for sc in [s for s in SCENARIOS if s["gpu"]]:
        run_score_scenario(sc, out, monkeypatch)


def test_the_entry_point_on_the_native_provider(tmp_path):
    """`python GCI_score.py ...` as a user starts it: the library's own HBM buffers (no torch in the process), same files."""
    case = "score_c5_three_types"
    out = str(tmp_path / "out")
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1")
    env.pop("GCI_HBM", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "GCI_score.py")] + _sub(_manifest(case)["argv"], out),
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _norm(r.stdout, out) == _manifest(case)["stdout"]
    assert _files(out) == _files(os.path.join(GOLDEN, case, "expected"))


# ---- the device parse against its CPU twin ----------------------------------------------------------------------------------------

def _random_text(rng, n_contigs, max_len, final_newline=True) -> bytes:
    parts = []
    for k in range(n_contigs):
        L = int(rng.integers(0, max_len))
        vals = np.repeat(rng.choice([0, 1, 35, 999_999, 2_147_483_647, 1_000_000_000], int(L // 50 + 1)), 50)[:L]
        name = b"c%d" % k + (b"y" * 6000 if k == 2 else b"")
        parts.append(b">" + name + b"\n" + b"".join(b"%d\n" % v for v in vals.tolist()))
    t = b"".join(parts)
    return t if final_newline else t[:-1]


@pytest.mark.parametrize("seed", range(4))
def test_device_parse_matches_the_cpu_twin(engine, seed):
    from gci_amd import cpu
    from gci_amd.formats import depthfile
    rng = np.random.default_rng(100 + seed)
    text = _random_text(rng, 6, 300_000, final_newline=seed != 1)
    if seed == 3:                                                     # a repeated header
        text = text + b">c0\n" + b"5\n" * 12345
    arr = np.frombuffer(text, dtype=np.uint8)
    twin = cpu.CpuEngine(threads=4)
    c_tiles, c_keys, c_bad = twin.depth_text_index(arr)
    d_text = engine.to_device(arr)
    d_line0, line0, keys, bad = engine.depth_text_index(d_text)
    assert bad == c_bad == NONE
    assert np.array_equal(keys, c_keys)
    assert np.array_equal(line0, np.concatenate([[0], np.cumsum(c_tiles.astype(np.uint64))]).astype(np.uint64))
    names, lengths, segs = depthfile.header_segments(arr, keys, line0)
    engine.set_layout(lengths)
    twin.set_layout(lengths)
    track = engine.T.zeros(max(engine.total, 1), engine.T.int32, engine.device)
    engine.depth_text_parse(d_text, d_line0, segs(engine.offsets), track)
    want = twin.depth_text_parse(arr, line0, segs(twin.offsets), twin.new_track())
    assert np.array_equal(track.cpu().numpy()[:engine.total], want)


def test_device_parse_of_more_lines_in_a_tile_than_the_grammar_allows(engine):
    """The by-rank store's overflow branch: a tile with more lines than its staging arrays hold (test_score_cpu.CROWDED)."""
    from gci_amd import cpu
    from gci_amd.formats import depthfile
    from test_score_cpu import CROWDED, CROWDED_BAD, CROWDED_TILES, CROWDED_WANT
    arr = np.frombuffer(CROWDED, dtype=np.uint8)
    twin = cpu.CpuEngine(threads=2)
    c_tiles, c_keys, c_bad = twin.depth_text_index(arr)
    d_text = engine.to_device(arr)
    d_line0, line0, keys, bad = engine.depth_text_index(d_text)
    assert bad == c_bad == CROWDED_BAD
    assert np.array_equal(keys, c_keys) and keys.shape[0] == 2
    assert np.diff(line0.astype(np.int64)).tolist() == c_tiles.tolist() == CROWDED_TILES
    names, lengths, segs = depthfile.header_segments(arr, keys, line0)
    assert list(names) == ["a", "b"] and list(lengths) == [6200, 10]
    engine.set_layout(lengths)
    twin.set_layout(lengths)
    track = engine.T.zeros(max(engine.total, 1), engine.T.int32, engine.device)
    engine.depth_text_parse(d_text, d_line0, segs(engine.offsets), track)
    got = track.cpu().numpy()[:engine.total]
    assert np.array_equal(got, twin.depth_text_parse(arr, line0, segs(twin.offsets), twin.new_track()))
    for c, nm in enumerate(names):
        assert np.array_equal(twin.contig(got, c), CROWDED_WANT[nm]), nm


def test_device_grammar_check_reports_the_first_bad_line(engine):
    from gci_amd import cpu
    rng = np.random.default_rng(7)
    base = bytearray(_random_text(rng, 3, 50_000))
    twin = cpu.CpuEngine(threads=2)
    for at in rng.integers(0, len(base), 40).tolist():
        t = bytearray(base)
        t[at] = ord(" ") if at % 3 else ord("x")
        arr = np.frombuffer(bytes(t), dtype=np.uint8)
        _, _, _, bad = engine.depth_text_index(engine.to_device(arr))
        assert bad == twin.depth_text_index(arr)[2]


def test_slow_path_and_damaged_files_end_as_the_reference(engine, tmp_path):
    import gzip
    text = b">ctgA\r\n1\r\n2\r\n>ctgB\n+3\n 4 \n"
    p = str(tmp_path / "crlf.depth.gz")
    with open(p, "wb") as f:
        f.write(gzip.compress(text))
    depths, tl = pipeline.read_depth_tracks(engine, p)
    assert tl == {"ctgA": 2, "ctgB": 2} and depths["ctgA"].tolist() == [1, 2] and depths["ctgB"].tolist() == [3, 4]
    with open(p, "wb") as f:
        f.write(gzip.compress(b">a\n%d\n" % (1 << 31)))
    with pytest.raises(SystemExit) as e:
        pipeline.read_depth_tracks(engine, p)
    assert str(e.value).startswith("ERROR!!!")
    whole = gzip.compress(b">a\n" + b"12\n" * 5000)
    for bad, exc in ((whole[:len(whole) // 2], EOFError), (b"nonsense" * 4, gzip.BadGzipFile)):
        with open(p, "wb") as f:
            f.write(bad)
        with pytest.raises(exc):
            pipeline.read_depth_tracks(engine, p)


# ---- genome size: this project's writer, then the new reader ------------------------------------------------------------------

def test_chr1_size_round_trip_through_the_projects_own_depth_gz(engine, tmp_path):
    rng = np.random.default_rng(11)
    lengths = [248_956_422] + [int(x) for x in rng.integers(1_000, 3_000_000, 120)]
    targets_length = {("chr1" if k == 0 else "ctg%03d" % k): L for k, L in enumerate(lengths)}
    engine.set_layout(lengths)
    host = np.zeros(engine.total, dtype=np.int32)
    for o, L in zip(engine.offsets, lengths):
        runs = rng.integers(1, 60_000, L // 20_000 + 2)
        vals = rng.choice([0, 1, 2, 17, 38, 41, 250, 123_456], runs.shape[0]).astype(np.int32)
        host[o:o + L] = np.repeat(vals, runs)[:L] if runs.sum() >= L else np.resize(np.repeat(vals, runs), L)
    track = engine.to_device(host)
    orig = pipeline.DepthTracks(engine, targets_length, track)
    d = str(tmp_path)
    pipeline.write_depth(d, "RT", orig)
    back, tl = pipeline.read_depth_tracks(engine, os.path.join(d, "RT.depth.gz"), targets_length)
    assert tl == targets_length and back.lengths == lengths
    assert np.array_equal(back.track.cpu().numpy()[:engine.total], host)
    bed_a = pipeline.merge_depth(orig, "A", 2, 15, d, True, "HiFi")
    bed_b = pipeline.merge_depth(back, "B", 2, 15, d, True, "HiFi")
    assert bed_a == bed_b and open(os.path.join(d, "A.2.depth.bed")).read() == open(os.path.join(d, "B.2.depth.bed")).read()
