"""convert_samtools_depth.py on the GPU: the device parse of `samtools depth` text (k_sdepth.hip) against its CPU twin, the command
line against the payloads, transcripts and failures of the UNMODIFIED reference utility (tests/golden/convert_*,
tools/make_golden_convert.py) -- resident and in pieces, with the path each run took --, and a chromosome-size round trip through
the project's own reader of the format."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLDEN
from gci_amd import pipeline
from test_convert_cpu import CASES, CONVERT_IN, ERRORS, NONE, line0_of, random_text, run_convert_scenario, strict_bad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _manifest(case):
    with open(os.path.join(GOLDEN, case, "manifest.json")) as f:
        return json.load(f)


def _sub(argv, out):
    return [a.replace("{IN}", CONVERT_IN).replace("{OUT}", out) for a in argv]


# ---- the device kernels against the CPU twin --------------------------------------------------------------------------------------

def device_equals_twin(engine, text: bytes, prev: bytes = b"", cap: int = 1 << 12, line_base: int = 0):
    """Tile counts, keys and bad offset of gci_sdepth_index, then the track of gci_sdepth_parse over segments made from those keys."""
    from gci_amd import cpu
    from gci_amd.formats import depthfile
    twin = cpu.CpuEngine(threads=4)
    arr = np.frombuffer(text, dtype=np.uint8)
    c_tiles, c_keys, c_bad = twin.sdepth_index(arr, prev)
    d_text = engine.to_device(arr)
    d_line0, line0, keys, bad = engine.sdepth_index(d_text, prev, cap=cap)
    assert bad == c_bad
    assert np.array_equal(line0, line0_of(c_tiles))
    if bad != NONE:
        return bad
    assert np.array_equal(keys, c_keys)
    found = depthfile.sdepth_segments(arr, keys, line0, 0, line_base)
    if not found:
        return bad
    first = np.array([g for _, g in found] + [line_base + int(line0[-1])], dtype=np.int64)
    lengths = np.diff(first)
    engine.set_layout(lengths.tolist())
    twin.set_layout(lengths.tolist())
    track = engine.T.zeros(max(engine.total, 1), engine.T.int32, engine.device)
    engine.sdepth_parse(d_text, d_line0, np.stack([first[:-1], lengths, np.asarray(engine.offsets, dtype=np.int64)], axis=1), track, line_base)
    want = twin.sdepth_parse(arr, line0, np.stack([first[:-1], lengths, np.asarray(twin.offsets, dtype=np.int64)], axis=1), twin.new_track(),
                             line_base)
    assert np.array_equal(track.cpu().numpy()[:engine.total], want)
    return bad


@pytest.mark.parametrize("seed", range(8))
def test_device_matches_the_cpu_twin_on_random_texts(engine, seed):
    rng = np.random.default_rng(seed)                                  # (the texts of test_convert_cpu's twin test)
    text = random_text(rng, int(rng.integers(1, 12)), 400, final_newline=bool(seed % 2))
    assert device_equals_twin(engine, text) == NONE


def test_device_matches_the_cpu_twin_at_tile_edges_bounds_and_seams(engine):
    def line(name, k):
        return b"%s\t%010d\t%d\n" % (name, k, k % 10)
    for change_at in ({256, 512}, {255, 511}, {255, 256, 257}, {1, 1023}, set(range(250, 262))):
        names, cur, out = [b"aa", b"ab", b"ba", b"bb"], 0, []
        for k in range(1024):
            cur += k in change_at
            out.append(line(names[cur % 4], k))
        text = b"".join(out)
        assert device_equals_twin(engine, text) == NONE
        assert device_equals_twin(engine, text[:-1]) == NONE
        assert device_equals_twin(engine, text, prev=b"aa", line_base=12345) == NONE      # a later piece of a file
    long_a, long_b = b"A" * 250, b"A" * 249 + b"B"
    text = b"".join(b"%s\t%d\t%d\n" % (long_a if (k // 5) % 2 else long_b, k % 10, k % 10) for k in range(300))
    text += b"".join(b"%s\t%d\t%d\n" % (b"C" * 249, k % 10, (k * 7) % 10) for k in range(300))
    assert device_equals_twin(engine, text) == NONE
    assert device_equals_twin(engine, text, prev=long_b) == NONE
    at = 255 * 17
    assert device_equals_twin(engine, text[:at] + b"A" + text[at:]) == at
    # depths 0 / INT32_MAX / INT32_MAX + 1
    base = b"".join(b"c\t%d\t%d\n" % (k + 1, (0, 2147483647, 1000000000, 7)[k % 4]) for k in range(3000))
    assert device_equals_twin(engine, base) == NONE
    bad_text = base.replace(b"\t2147483647\n", b"\t2147483648\n", 1)
    assert device_equals_twin(engine, bad_text) == strict_bad(bad_text) != NONE


def test_device_parse_of_more_lines_in_a_tile_than_the_grammar_allows(engine):
    """The by-rank store's overflow branch: a tile with more lines than its staging arrays hold (test_convert_cpu.CROWDED)."""
    from gci_amd import cpu
    from test_convert_cpu import CROWDED, CROWDED_BAD, CROWDED_KEYS, CROWDED_LINES, CROWDED_WANT
    arr = np.frombuffer(CROWDED, dtype=np.uint8)
    twin = cpu.CpuEngine(threads=2)
    c_tiles, c_keys, c_bad = twin.sdepth_index(arr)
    d_text = engine.to_device(arr)
    d_line0, line0, keys, bad = engine.sdepth_index(d_text)
    assert bad == c_bad == CROWDED_BAD
    assert np.array_equal(keys, c_keys) and keys.shape[0] == CROWDED_KEYS
    assert np.array_equal(line0, line0_of(c_tiles)) and int(line0[-1]) == CROWDED_LINES
    engine.set_layout([CROWDED_LINES])
    twin.set_layout([CROWDED_LINES])
    segs = np.array([[0, CROWDED_LINES, 0]], dtype=np.int64)
    track = engine.T.zeros(max(engine.total, 1), engine.T.int32, engine.device)
    engine.sdepth_parse(d_text, d_line0, segs, track)
    got = track.cpu().numpy()[:engine.total]
    assert np.array_equal(got, twin.sdepth_parse(arr, line0, segs, twin.new_track()))
    assert np.array_equal(twin.contig(got, 0), CROWDED_WANT)


def test_device_key_overflow_and_retry(engine):
    text = b"".join(b"%s\t%d\t%d\n" % (b"x" if k % 2 else b"y", k, k % 9) for k in range(30_000))
    assert device_equals_twin(engine, text, cap=4) == NONE


def test_device_grammar_check_reports_the_first_bad_line(engine):
    rng = np.random.default_rng(11)
    text = random_text(rng, 4, 60)[:3 * 4096 + 100]
    text = text[:text.rfind(b"\n") + 1]
    damage = [b"\t", b"\n", b"\r", b" ", b"x", b"0", b"\x00", b"\x7f", b"\xc2", b"+"]
    for _ in range(150):
        p = int(rng.integers(0, len(text)))
        t = text[:p] + damage[int(rng.integers(0, len(damage)))] + text[p + 1:]
        assert device_equals_twin(engine, t) == strict_bad(t), p


# ---- the command line against the reference utility -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_convert_cli_reproduces_the_reference_utility(engine, case, tmp_path, capsys, monkeypatch):
    from gci_amd import convert_cli
    m = _manifest(case)
    want = open(os.path.join(GOLDEN, case, "expected.depth"), "rb").read()
    pipeline._ENGINE = engine
    monkeypatch.delenv("GCI_SDEPTH_RESIDENT_MAX", raising=False)
    out = str(tmp_path / "resident")
    os.makedirs(out)
    taken = convert_cli.main(["convert_samtools_depth.py"] + _sub(m["argv"], out))
    assert taken == ("device" if m["strict"] else "host")           # (everything on the host would pass the payload check too)
    assert sorted(os.listdir(out)) == m["files"]
    assert gzip.decompress(open(os.path.join(out, "GCI.depth.gz"), "rb").read()) == want
    cap = capsys.readouterr()
    assert cap.out == m["stdout"] and cap.err == m["stderr"]
    # no overwrite guard: a second run replaces the file
    assert convert_cli.main(["convert_samtools_depth.py"] + _sub(m["argv"], out)) == taken
    assert gzip.decompress(open(os.path.join(out, "GCI.depth.gz"), "rb").read()) == want
    # the same file in pieces cut at line ends
    monkeypatch.setenv("GCI_SDEPTH_RESIDENT_MAX", "0")
    for chunk in (4096, 4097):
        monkeypatch.setenv("GCI_SDEPTH_CHUNK_BYTES", str(chunk))
        out = str(tmp_path / ("pieces%d" % chunk))
        os.makedirs(out)
        taken = convert_cli.main(["convert_samtools_depth.py"] + _sub(m["argv"], out))
        assert taken == ("device-chunked" if m["strict"] else "host")
        assert gzip.decompress(open(os.path.join(out, "GCI.depth.gz"), "rb").read()) == want
    capsys.readouterr()


def test_our_own_reader_takes_what_the_converter_wrote(engine, tmp_path):
    from gci_amd import convert_cli
    pipeline._ENGINE = engine
    m = _manifest("convert_three")
    convert_cli.main(["convert_samtools_depth.py"] + _sub(m["argv"], str(tmp_path)))
    depths, tl = pipeline.read_depth_tracks(engine, str(tmp_path / "GCI.depth.gz"))
    assert tl == {"chr1": 2600, "chr2_hap1": 1200, "chrM": 90}
    want = open(os.path.join(GOLDEN, "convert_three", "expected.depth"), "rb").read().split(b">chr2_hap1\n")[0].split(b"\n")[1:-1]
    assert depths["chr1"].tolist() == [int(v) for v in want]


@pytest.mark.parametrize("sc", [s for s in ERRORS if s["gpu"]], ids=lambda s: s["name"])
def test_convert_failures_after_device_work(engine, sc, tmp_path):
    pipeline._ENGINE = engine
    run_convert_scenario(sc, str(tmp_path / "out"))


def test_an_empty_input_takes_the_host_path(engine, tmp_path):
    from gci_amd import convert_cli
    pipeline._ENGINE = engine
    open(str(tmp_path / "empty.depth"), "wb").close()
    assert convert_cli.main(["convert_samtools_depth.py", str(tmp_path / "empty.depth"), str(tmp_path / "E")]) == "host"
    assert gzip.decompress(open(str(tmp_path / "E.depth.gz"), "rb").read()) == b""


def test_the_entry_point_on_the_native_provider(tmp_path):
    """`python convert_samtools_depth.py ...` as a user starts it: the library's own HBM buffers (no torch in the process), the
    reference's payload, and the device path by the run's own phase log."""
    case = "convert_returns"
    out = str(tmp_path / "out")
    os.makedirs(out)
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1", GCI_PHASES=str(tmp_path / "phases.json"))
    for k in ("GCI_HBM", "GCI_SDEPTH_RESIDENT_MAX", "GCI_SDEPTH_CHUNK_BYTES"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "convert_samtools_depth.py")] + _sub(_manifest(case)["argv"], out),
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == _manifest(case)["stdout"]
    assert gzip.decompress(open(os.path.join(out, "GCI.depth.gz"), "rb").read()) == open(os.path.join(GOLDEN, case, "expected.depth"), "rb").read()
    assert json.load(open(str(tmp_path / "phases.json")))["notes"]["convert_samtools_depth_path"] == "device"


# ---- chromosome size: the converter, then the project's reader --------------------------------------------------------------------

def test_chromosome_size_round_trip_through_the_depth_gz_reader(engine, tmp_path):
    from gci_amd import synth
    rng = np.random.default_rng(23)
    lengths = [50_000_000] + [int(x) for x in rng.integers(1_000, 200_000, 100)]
    names = ["chr1"] + ["ctg%03d_hap%d" % (k, k % 2 + 1) for k in range(1, 101)]
    targets_length = dict(zip(names, lengths))
    engine.set_layout(lengths)
    host = np.zeros(engine.total, dtype=np.int32)
    items = []
    for nm, o, L in zip(names, engine.offsets, lengths):
        runs = rng.integers(10_000, 60_000, L // 20_000 + 2)
        vals = rng.choice([0, 1, 2, 17, 38, 41, 250, 123_456], runs.shape[0]).astype(np.int32)
        host[o:o + L] = np.repeat(vals, runs)[:L]
        items.append((nm, host[o:o + L]))
    text = synth.samtools_depth_text(items)
    assert text.shape[0] >= (256 << 20)                                # (the staged upload)
    d = str(tmp_path)
    text.tofile(os.path.join(d, "big.depth"))
    del text, items
    assert pipeline.convert_samtools_depth(engine, os.path.join(d, "big.depth"), os.path.join(d, "RT")) == "device"
    os.remove(os.path.join(d, "big.depth"))
    back, tl = pipeline.read_depth_tracks(engine, os.path.join(d, "RT.depth.gz"), targets_length)
    assert tl == targets_length and back.lengths == lengths
    assert np.array_equal(back.track.cpu().numpy()[:engine.total], host)
    orig = pipeline.DepthTracks(engine, targets_length, engine.to_device(host))
    bed_a = pipeline.merge_depth(orig, "A", 2, 15, d, True, "HiFi")
    bed_b = pipeline.merge_depth(back, "B", 2, 15, d, True, "HiFi")
    assert bed_a == bed_b and open(os.path.join(d, "A.2.depth.bed")).read() == open(os.path.join(d, "B.2.depth.bed")).read()
