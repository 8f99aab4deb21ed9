"""convert_samtools_depth.py off the GPU: the CPU twin of the three-column parse (libgci_cpu.so: gci_sdepth_index / _parse, the same
tiles, grammar, keys and status word as k_sdepth.hip) against a statement of the grammar and of the segmenting in Python, the
chunk cutting of a file too large to stay in HBM, the host slow path (formats.depthfile.convert_samtools_host) against the
payloads and failures of the reference utility (tests/golden/convert_*), and the command line's refusals that need no device."""
import contextlib
import gzip
import io
import json
import os
import re

import numpy as np
import pytest

from golden_util import GOLDEN

INT32_MAX = (1 << 31) - 1
NONE = (1 << 64) - 1
LINE_MAX = 255                                 # bytes of a line with its '\n' (k_sdepth.hip: SD_LINE_MAX)
STRICT = re.compile(rb"[\x21-\x7e]+\t[0-9]{1,10}\t(0|[1-9][0-9]{0,9})")

CONVERT_IN = os.path.join(GOLDEN, "convert_inputs")
CASES = sorted(d for d in os.listdir(GOLDEN) if d.startswith("convert_") and os.path.isdir(os.path.join(GOLDEN, d)) and d != "convert_inputs")
ERRORS = json.load(open(os.path.join(GOLDEN, "convert_errors.json")))


# ---- the grammar and the segmenting, stated in Python -----------------------------------------------------------------------------

def lines_of(text: bytes):
    """[(offset, line without its '\\n', closed by '\\n')]"""
    out, at = [], 0
    parts = text.split(b"\n")
    for k, part in enumerate(parts):
        last = k == len(parts) - 1
        if last and part == b"":
            break
        out.append((at, part, not last))
        at += len(part) + 1
    return out


def strict_bad(text: bytes) -> int:
    """Smallest offset of a line outside the strict grammar, or NONE."""
    for at, line, closed in lines_of(text):
        m = STRICT.fullmatch(line)
        if not (m and int(m.group(1)) <= INT32_MAX and len(line) + (1 if closed else 0) <= LINE_MAX):
            return at
    return NONE


def segments_of(text: bytes, prev: bytes = b""):
    """The reference's line loop over valid text: [(name, offset of the first line, its line index, [depths])]."""
    segs = []
    for g, (at, line, _) in enumerate(lines_of(text)):
        name, _, depth = line.split(b"\t")
        if name != prev:
            segs.append((name, at, g, []))
            prev = name
        if segs:
            segs[-1][3].append(int(depth))
    return segs


def line0_of(tiles) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(tiles.astype(np.uint64))]).astype(np.uint64)


def cpu_convert(eng, text: bytes, chunk_bytes=None, cap=1 << 10):
    """pipeline.convert_samtools_depth with the CPU twin in place of the device -> ([(name, int32 depths)], keys as (offset, line
    index) in the file, smallest bad offset)."""
    from gci_amd.formats import depthfile
    raw = np.frombuffer(text, dtype=np.uint8)
    pieces = [(0, len(text), b"")] if chunk_bytes is None else depthfile.sdepth_chunks(raw, chunk_bytes)
    found, per_piece, line_base, first_bad = [], [], 0, NONE
    for a, b, prev in pieces:
        tiles, keys, bad = eng.sdepth_index(raw[a:b], prev, cap=cap)
        if bad != NONE:
            first_bad = min(first_bad, a + bad)
        line0 = line0_of(tiles)
        found += [(nm, g, a + int(k >> np.uint64(12))) for (nm, g), k in zip(depthfile.sdepth_segments(raw, keys, line0, a, line_base), keys)]
        per_piece.append((line0, line_base))
        line_base += int(line0[-1])
    if first_bad != NONE:
        return None, [(o, g) for _, g, o in found], first_bad
    first = np.array([g for _, g, _ in found] + [line_base], dtype=np.int64)
    lengths = np.diff(first)
    eng.set_layout(lengths.tolist())
    segs = np.stack([first[:-1], lengths, np.asarray(eng.offsets, dtype=np.int64)], axis=1).reshape(-1, 3)
    track = eng.new_track()
    track[:] = -7
    for (a, b, _), (line0, base) in zip(pieces, per_piece):
        eng.sdepth_parse(raw[a:b], line0, segs, track, base)
    return ([(nm, eng.contig(track, c).copy()) for c, (nm, _, _) in enumerate(found)], [(o, g) for _, g, o in found], NONE)


@pytest.fixture(scope="module")
def cpu_engine():
    from gci_amd import cpu
    return cpu.CpuEngine(threads=4)


def check_against_statement(eng, text: bytes, **kw):
    got, keys, bad = cpu_convert(eng, text, **kw)
    assert bad == strict_bad(text) == NONE
    want = segments_of(text)
    assert keys == [(at, g) for _, at, g, _ in want]
    assert [nm for nm, _ in got] == [nm for nm, _, _, _ in want]
    for (nm, d), (_, _, _, w) in zip(got, want):
        assert np.array_equal(d, np.asarray(w, dtype=np.int64).astype(np.int32)), nm


# ---- texts ------------------------------------------------------------------------------------------------------------------------

def random_text(rng, n_names: int, max_run: int, final_newline: bool = True) -> bytes:
    """Runs of lines under random names of 1 .. 250 bytes (a name may return), positions of 1 .. 10 digits, depths with the corner
    values among them."""
    alphabet = np.frombuffer(bytes(range(0x21, 0x7F)), dtype=np.uint8)
    names = []
    for _ in range(n_names):
        L = int(rng.choice([1, 2, 5, 12, 40, 250, int(rng.integers(1, 251))]))
        names.append(alphabet[rng.integers(0, alphabet.shape[0], L)].tobytes())
    out = []
    for _ in range(n_names * 2):
        name = names[int(rng.integers(0, n_names))]
        for _ in range(int(rng.integers(1, max_run))):
            pos = int(rng.choice([1, 9999999999, int(rng.integers(0, 10 ** 10))]))
            dep = int(rng.choice([0, INT32_MAX, 10 ** 9, int(rng.integers(0, 100)), int(rng.integers(0, INT32_MAX))]))
            if len(name) + 2 + len(str(pos)) + len(str(dep)) + 1 > LINE_MAX:
                pos = 7
            if len(name) + 2 + len(str(pos)) + len(str(dep)) + 1 > LINE_MAX:
                dep = 3
            out.append(b"%s\t%d\t%d\n" % (name, pos, dep))
    t = b"".join(out)
    return t if final_newline else t[:-1]


@pytest.mark.parametrize("seed", range(8))
def test_cpu_twin_matches_the_python_statement_on_random_texts(cpu_engine, seed):
    rng = np.random.default_rng(seed)
    text = random_text(rng, int(rng.integers(1, 12)), 400, final_newline=bool(seed % 2))
    assert len(text) > 3 * 4096
    check_against_statement(cpu_engine, text)


# More lines in a tile than text inside the grammar can have (empty lines: a byte each).  The product never parses such text --
# the index pass reports it -- but the exports take it, and a parse that stages a tile's lines by rank must still place every one.
CROWDED = b"x\t1\t5\n" + b"\n" * 5000 + b"".join(b"x\t%d\t%d\n" % (k, k % 1000) for k in range(600))
CROWDED_LINES, CROWDED_BAD, CROWDED_KEYS = 5601, 6, 3
CROWDED_WANT = np.concatenate([[5], np.zeros(5000, dtype=np.int32), np.arange(600, dtype=np.int32) % 1000]).astype(np.int32)


def test_more_lines_in_a_tile_than_the_grammar_allows(cpu_engine):
    assert len(CROWDED) == 10786
    arr = np.frombuffer(CROWDED, dtype=np.uint8)
    tiles, keys, bad = cpu_engine.sdepth_index(arr)
    assert tiles.shape[0] == 3 and int(tiles.sum()) == CROWDED_LINES == len(lines_of(CROWDED))
    assert bad == CROWDED_BAD == strict_bad(CROWDED) and keys.shape[0] == CROWDED_KEYS
    cpu_engine.set_layout([CROWDED_LINES])
    segs = np.array([[0, CROWDED_LINES, 0]], dtype=np.int64)
    track = cpu_engine.sdepth_parse(arr, line0_of(tiles), segs, cpu_engine.new_track())
    assert np.array_equal(cpu_engine.contig(track, 0), CROWDED_WANT)


def test_name_changes_on_the_first_and_the_last_line_of_a_tile(cpu_engine):
    # every line 16 bytes: 256 lines fill a tile exactly, line 256 k is a tile's first and line 256 k - 1 a tile's last
    def line(name, k):
        return b"%s\t%010d\t%d\n" % (name, k, k % 10)
    for change_at in ({256, 512}, {255, 511}, {255, 256, 257}, {1, 1023}, set(range(250, 262))):
        names, cur, out = [b"aa", b"ab", b"ba", b"bb"], 0, []
        for k in range(1024):
            if k in change_at:
                cur += 1
            out.append(line(names[cur % 4], k))
        text = b"".join(out)
        assert len(text) == 4 * 4096
        check_against_statement(cpu_engine, text)
        check_against_statement(cpu_engine, text[:-1])


def test_lines_that_straddle_tiles_at_every_phase_and_names_up_to_the_bound(cpu_engine):
    # 255-byte lines (the bound) and 254-byte ones: the tile boundary falls on every byte of a line in turn
    long_a, long_b = b"A" * 250, b"A" * 249 + b"B"
    text = b"".join(b"%s\t%d\t%d\n" % (long_a if (k // 5) % 2 else long_b, k % 10, k % 10) for k in range(300))
    text += b"".join(b"%s\t%d\t%d\n" % (b"C" * 249, k % 10, (k * 7) % 10) for k in range(300))
    check_against_statement(cpu_engine, text)
    # one byte more: outside the grammar, at that line's offset
    at = 255 * 17
    bad_text = text[:at] + b"A" + text[at:]
    assert cpu_convert(cpu_engine, bad_text)[2] == strict_bad(bad_text) == at
    # a last line of 255 bytes without its '\n' is inside, of 256 outside
    tail = b"x\t1\t5\n" + b"D" * 251 + b"\t1\t5"
    assert len(tail) - 6 == 255 and cpu_convert(cpu_engine, tail)[2] == strict_bad(tail) == NONE
    tail = b"x\t1\t5\n" + b"D" * 252 + b"\t1\t5"
    assert cpu_convert(cpu_engine, tail)[2] == strict_bad(tail) == 6


def test_depth_corner_values(cpu_engine):
    base = b"".join(b"c\t%d\t%d\n" % (k + 1, k % 50) for k in range(2000))
    lines = lines_of(base)
    for dep, ok in ((b"0", True), (b"2147483647", True), (b"2147483648", False), (b"9999999999", False), (b"10000000000", False),
                    (b"00", False), (b"01", False), (b"+1", False), (b"", False), (b"-0", False)):
        at, line, _ = lines[1234]
        text = base[:at] + b"c\t1235\t" + dep + base[at + len(line):]
        _, _, bad = cpu_convert(cpu_engine, text)
        assert bad == strict_bad(text) == (NONE if ok else at), dep
        if ok:
            check_against_statement(cpu_engine, text)
    for pos, ok in ((b"0123456789", True), (b"12345678901", False), (b"", False), (b"1 ", False)):
        at, line, _ = lines[700]
        text = base[:at] + b"c\t" + pos + b"\t9" + base[at + len(line):]
        assert cpu_convert(cpu_engine, text)[2] == strict_bad(text) == (NONE if ok else at), pos


def test_alternating_names_overflow_the_key_buffer_and_the_retry_finds_them_all(cpu_engine):
    text = b"".join(b"%s\t%d\t%d\n" % (b"x" if k % 2 else b"y", k, k % 9) for k in range(3000))
    check_against_statement(cpu_engine, text, cap=4)
    check_against_statement(cpu_engine, text)


def test_first_bad_offset_for_single_byte_damage(cpu_engine):
    rng = np.random.default_rng(11)
    text = random_text(rng, 4, 60)[:3 * 4096 + 100]
    text = text[:text.rfind(b"\n") + 1]
    assert strict_bad(text) == NONE
    damage = [b"\t", b"\n", b"\r", b" ", b"x", b"0", b"\x00", b"\x7f", b"\xc2", b"+"]
    for _ in range(600):
        p = int(rng.integers(0, len(text)))
        c = damage[int(rng.integers(0, len(damage)))]
        t = text[:p] + c + text[p + 1:]
        tiles, _, bad = cpu_engine.sdepth_index(np.frombuffer(t, dtype=np.uint8))
        assert bad == strict_bad(t), (p, c)
        assert int(tiles.sum()) == len(lines_of(t))


def test_first_bad_offset_at_every_byte_of_a_small_text(cpu_engine):
    text = b"ab\t1\t7\nab\t2\t0\nc\t10\t123\nc\t11\t45"
    for p in range(len(text)):
        for c in (b"x", b" ", b"\r", b"\n", b"\t", b"0"):
            t = text[:p] + c + text[p + 1:]
            assert cpu_engine.sdepth_index(np.frombuffer(t, dtype=np.uint8))[2] == strict_bad(t), (p, c, t)


def test_prev_name_decides_the_first_line(cpu_engine):
    text = np.frombuffer(b"chr1\t1\t5\nchr1\t2\t6\nchr2\t1\t7\n", dtype=np.uint8)
    for prev, n_keys in ((b"", 2), (b"chr1", 1), (b"chr", 2), (b"chr11", 2), (b"chr2", 2)):
        assert cpu_engine.sdepth_index(text, prev)[1].shape[0] == n_keys, prev


# ---- a file that goes through in pieces -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(3))
def test_pieces_cut_at_line_ends_give_the_one_shot_result(cpu_engine, seed):
    from gci_amd.formats import depthfile
    rng = np.random.default_rng(100 + seed)
    text = random_text(rng, 5, 40, final_newline=bool(seed % 2))[:40_000]
    text = text[:text.rfind(b"\n") + (1 if seed % 2 else 0)]
    whole, keys, bad = cpu_convert(cpu_engine, text)
    assert bad == NONE
    raw = np.frombuffer(text, dtype=np.uint8)
    for chunk in (1, 7, 100, 255, 256, 4095, 4096, 4097, 10_000, len(text) - 1, len(text), len(text) + 1):
        pieces = depthfile.sdepth_chunks(raw, chunk)
        assert pieces[0][0] == 0 and pieces[-1][1] == len(text) and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
        assert all(text[b - 1:b] == b"\n" for _, b, _ in pieces[:-1])
        got, got_keys, bad = cpu_convert(cpu_engine, text, chunk_bytes=chunk)
        assert bad == NONE and got_keys == keys, chunk
        assert [nm for nm, _ in got] == [nm for nm, _ in whole]
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(got, whole)), chunk


# ---- the host slow path against the reference utility's payloads and failures -----------------------------------------------------

def _sub(t, out_root):
    return t.replace("{IN}", CONVERT_IN).replace("{OUT}", out_root)


@pytest.mark.parametrize("case", CASES)
def test_host_path_writes_the_reference_payload(case, tmp_path):
    from gci_amd.formats import depthfile
    m = json.load(open(os.path.join(GOLDEN, case, "manifest.json")))
    out = str(tmp_path / "x.depth.gz")
    depthfile.convert_samtools_host(_sub(m["argv"][0], str(tmp_path)), out)
    assert gzip.open(out, "rb").read() == open(os.path.join(GOLDEN, case, "expected.depth"), "rb").read()


@pytest.mark.parametrize("case", CASES)
def test_goldens_are_inside_the_strict_grammar_exactly_when_their_manifest_says_so(cpu_engine, case):
    m = json.load(open(os.path.join(GOLDEN, case, "manifest.json")))
    text = open(_sub(m["argv"][0], ""), "rb").read()
    got, _, bad = cpu_convert(cpu_engine, text)
    assert (bad == NONE) == m["strict"] and bad == strict_bad(text)
    if m["strict"]:
        payload = b"".join(b">" + nm + b"\n" + b"".join(b"%d\n" % v for v in d.tolist()) for nm, d in got)
        assert payload == open(os.path.join(GOLDEN, case, "expected.depth"), "rb").read()


class _HostBuffers:
    int32 = np.int32

    @staticmethod
    def zeros(n, dtype, device):
        return np.zeros(n, dtype=dtype)


def _stand_in_engine():
    """The CPU twin with the few Engine methods pipeline.convert_samtools_depth calls: the host side of the converter -- pieces,
    segments, layout, members, the file -- runs off the GPU with it."""
    from gci_amd import cpu

    class StandIn(cpu.CpuEngine):
        T, device = _HostBuffers, None

        def upload_staged(self, a):
            return np.ascontiguousarray(a)

        to_device = upload_staged

        def sdepth_index(self, text, prev_name=b"", cap=1 << 12):
            tiles, keys, bad = cpu.CpuEngine.sdepth_index(self, text, prev_name, cap=cap)
            return line0_of(tiles), line0_of(tiles), keys, bad
    return StandIn(threads=2)


@pytest.mark.parametrize("case", CASES)
def test_the_host_side_of_the_converter_over_the_cpu_twin(case, tmp_path, monkeypatch):
    from gci_amd import pipeline
    m = json.load(open(os.path.join(GOLDEN, case, "manifest.json")))
    want = open(os.path.join(GOLDEN, case, "expected.depth"), "rb").read()
    eng = _stand_in_engine()
    for k, env in enumerate(({}, {"GCI_SDEPTH_RESIDENT_MAX": "0", "GCI_SDEPTH_CHUNK_BYTES": "4096"},
                             {"GCI_SDEPTH_RESIDENT_MAX": "0", "GCI_SDEPTH_CHUNK_BYTES": "300"})):
        monkeypatch.delenv("GCI_SDEPTH_RESIDENT_MAX", raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        taken = pipeline.convert_samtools_depth(eng, _sub(m["argv"][0], ""), str(tmp_path / ("x%d" % k)))
        assert taken == (("device-chunked" if env else "device") if m["strict"] else "host")
        assert gzip.decompress(open(str(tmp_path / ("x%d.depth.gz" % k)), "rb").read()) == want


@pytest.mark.parametrize("sc", [s for s in ERRORS if len(s["argv"]) == 2], ids=lambda s: s["name"])
def test_host_path_raises_what_the_reference_raises(sc, tmp_path):
    from gci_amd.formats import depthfile
    out = str(tmp_path / "x.depth.gz")
    with pytest.raises(Exception) as e:
        depthfile.convert_samtools_host(_sub(sc["argv"][0], str(tmp_path)), out)
    assert {"type": type(e.value).__name__, "message": str(e.value).replace(CONVERT_IN, "{IN}")} == sc["exception"]
    assert os.path.exists(out) == sc["output_exists"]


def run_convert_scenario(sc, out_root):
    """convert_cli.main as the utility's transcript records it: exit, exception, stdout, stderr, and whether the output exists."""
    from gci_amd import convert_cli
    os.makedirs(out_root, exist_ok=True)
    norm = lambda t: t.replace(out_root, "{OUT}").replace(CONVERT_IN, "{IN}")      # noqa: E731
    so, se = io.StringIO(), io.StringIO()
    code, exc = "completed", None
    try:
        with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
            convert_cli.main(["convert_samtools_depth.py"] + [_sub(a, out_root) for a in sc["argv"]])
    except SystemExit as e:
        code = e.code
    except Exception as e:                                 # noqa: BLE001
        code, exc = "exception", {"type": type(e).__name__, "message": norm(str(e))}
    made = os.path.exists(_sub(sc["argv"][-1], out_root) + ".depth.gz") if len(sc["argv"]) == 2 else None
    got = {"exit": code, "exception": exc, "stdout": norm(so.getvalue()), "stderr": norm(se.getvalue()), "output_exists": made}
    assert got == {k: sc[k] for k in got}, sc["name"]


@pytest.mark.parametrize("sc", [s for s in ERRORS if not s["gpu"]], ids=lambda s: s["name"])
def test_convert_refused_before_any_gpu_work(sc, tmp_path):
    run_convert_scenario(sc, str(tmp_path / "out"))


def test_entry_point_exists_and_imports_no_torch():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, runpy; sys.argv = ['convert_samtools_depth.py', 'x.depth']\n"
            "try:\n    runpy.run_path(%r, run_name='__main__')\nexcept SystemExit as e:\n    print(repr(e.code))\n"
            "print('torch' in sys.modules)\n") % os.path.join(root, "convert_samtools_depth.py")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=120)
    assert r.stdout.strip().splitlines()[-2:] == ["1", "False"], r.stderr
    assert r.stdout.startswith("Usage: python ") and "convert_samtools_depth.py input.depth output_prefix\n" in r.stdout      # (runpy names the path)
