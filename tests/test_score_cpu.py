"""GCI_score.py off the GPU: the CPU twin of the depth-text parse (libgci_cpu.so: gci_depth_text_index / _parse, the same tiles,
keys and status word as k_depth_parse.hip) against the project's own reader of the format, the host halves of the read
(formats.depthfile), the multi-member gzip inflate (host_io.cpp through gci_amd.hostio) against Python's gzip on files of both
writers and on damaged ones, and the utility's refusals that end before any device work (tests/golden/score_errors.json)."""
import contextlib
import gzip
import io
import json
import os
import re
import zlib

import numpy as np
import pytest

from golden_util import GOLDEN

INT32_MAX = (1 << 31) - 1
NONE = (1 << 64) - 1


# ---- the depth text and its parse ------------------------------------------------------------------------------------------------

def _text(items, final_newline=True) -> bytes:
    t = b"".join(b">" + name.encode() + b"\n" + b"".join(b"%d\n" % v for v in d.tolist()) for name, d in items)
    return t if final_newline else t[:-1]


def _strict_bad(text: bytes) -> int:
    """Smallest offset of a data line outside [0-9]{1,10} ('\\n' | end), value <= INT32_MAX -- the grammar's statement in Python."""
    at = 0
    for line in text.split(b"\n")[:-1] + ([text.rsplit(b"\n", 1)[-1]] if not text.endswith(b"\n") else []):
        if not line.startswith(b">") and not (re.fullmatch(rb"[0-9]{1,10}", line) and int(line) <= INT32_MAX):
            return at
        at += len(line) + 1
    return NONE


def _cpu_parse(eng, text: bytes):
    """The read of pipeline.read_depth_tracks with the CPU twin in place of the device: -> ({name: int32 array}, bad offset)."""
    from gci_amd.formats import depthfile
    arr = np.frombuffer(text, dtype=np.uint8)
    tiles, keys, bad = eng.depth_text_index(arr)
    line0 = np.concatenate([[0], np.cumsum(tiles.astype(np.uint64))]).astype(np.uint64)
    if bad != NONE:
        return None, bad
    found = depthfile.header_segments(arr, keys, line0)
    assert found is not None
    names, lengths, segs = found
    eng.set_layout(lengths)
    track = eng.new_track()
    eng.depth_text_parse(arr, line0, segs(eng.offsets), track)
    return {nm: eng.contig(track, c).copy() for c, nm in enumerate(names)}, bad


@pytest.fixture(scope="module")
def cpu_engine():
    from gci_amd import cpu
    return cpu.CpuEngine(threads=4)


def _random_items(rng, n_contigs, max_len):
    items = []
    for k in range(n_contigs):
        L = int(rng.integers(0, max_len))
        runs = []
        while sum(len(r) for r in runs) < L:
            v = int(rng.choice([0, rng.integers(1, 100), rng.integers(10 ** 9, INT32_MAX + 1), rng.integers(0, 10 ** 6)]))
            runs.append(np.full(int(rng.integers(1, 3000)), v, dtype=np.int64))
        d = np.concatenate(runs)[:L] if runs else np.zeros(0, dtype=np.int64)
        name = "c%d_" % k + ("x" * int(rng.integers(5000, 9000)) if k % 5 == 3 else "")     # headers longer than a tile
        items.append((name, d))
    return items


@pytest.mark.parametrize("seed", range(6))
def test_cpu_twin_parses_like_the_reader(cpu_engine, seed, tmp_path):
    from gci_amd.formats import depthfile
    rng = np.random.default_rng(seed)
    items = _random_items(rng, int(rng.integers(1, 9)), 40_000)
    items.append(("empty", np.zeros(0, dtype=np.int64)))
    text = _text(items, final_newline=bool(seed % 2))
    p = str(tmp_path / "x.depth.gz")
    with open(p, "wb") as f:
        f.write(gzip.compress(text, 1))
    want = depthfile.read_depth_gz(p) if seed % 2 else {nm: d for nm, d in items}
    got, bad = _cpu_parse(cpu_engine, text)
    assert bad == NONE
    assert list(got) == list(want)
    for nm in want:
        assert np.array_equal(got[nm], want[nm].astype(np.int32)), nm


def test_repeated_header_last_segment_wins_first_place_kept(cpu_engine):
    from gci_amd.formats import depthfile
    a, b, a2 = np.arange(5000) % 7, np.arange(300) + 3, np.arange(9000) % 11
    text = _text([("A", a), ("B", b), ("A", a2)])
    got, _ = _cpu_parse(cpu_engine, text)
    want = depthfile.parse_depth_lines(io.BytesIO(text))
    assert list(got) == list(want) == ["A", "B"]
    for nm in want:
        assert np.array_equal(got[nm], want[nm])


def test_tile_straddling_lines_and_ten_digit_values(cpu_engine):
    # every data line 11 bytes: lines straddle every tile boundary at every phase
    d = np.full(20_000, INT32_MAX, dtype=np.int64)
    d[::3] = 10 ** 9
    text = _text([("big", d)])
    got, bad = _cpu_parse(cpu_engine, text)
    assert bad == NONE and np.array_equal(got["big"], d.astype(np.int32))
    # one more than INT32_MAX, and eleven digits: outside the strict grammar, at their line's offset
    for v in (INT32_MAX + 1, 10 ** 10):
        t = bytearray(text)
        at = len(b">big\n") + 11 * 777
        t[at:at + 11] = b"%d\n" % v if v < 10 ** 10 else b"%d" % v
        _, bad = _cpu_parse(cpu_engine, bytes(t))
        assert bad == _strict_bad(bytes(t)) == at


def test_grammar_violation_at_every_byte_offset_is_reported_where_its_line_begins(cpu_engine):
    text = _text([("ab", np.array([7, 0, 123, 45])), ("c", np.array([9, 10]))])
    for p in range(len(text)):
        for c in (b"x", b" ", b"\r", b"\n", b">"):
            t = text[:p] + c + text[p + 1:]
            tiles, keys, bad = cpu_engine.depth_text_index(np.frombuffer(t, dtype=np.uint8))
            assert bad == _strict_bad(t), (p, c, t)
            assert int(tiles.sum()) == len(t.split(b"\n")) - (1 if t.endswith(b"\n") else 0)


# More lines in a tile than text inside the grammar can have (empty lines: a byte each).  The product never parses such text --
# the index pass reports it -- but the exports take it, and a parse that stages a tile's lines by rank must still place every one.
CROWDED = b">a\n" + b"\n" * 5000 + b"".join(b"%d\n" % (k % 1000) for k in range(1200)) + b">b\n" + b"3\n" * 10
CROWDED_TILES = [4094, 1732, 386]
CROWDED_BAD = 3
CROWDED_WANT = {"a": np.concatenate([np.zeros(5000, dtype=np.int32), np.arange(1200, dtype=np.int32) % 1000]),
                "b": np.full(10, 3, dtype=np.int32)}


def test_more_lines_in_a_tile_than_the_grammar_allows(cpu_engine):
    from gci_amd.formats import depthfile
    assert len(CROWDED) == 9606
    arr = np.frombuffer(CROWDED, dtype=np.uint8)
    tiles, keys, bad = cpu_engine.depth_text_index(arr)
    assert tiles.tolist() == CROWDED_TILES and bad == CROWDED_BAD == _strict_bad(CROWDED) and keys.shape[0] == 2
    line0 = np.concatenate([[0], np.cumsum(tiles.astype(np.uint64))]).astype(np.uint64)
    names, lengths, segs = depthfile.header_segments(arr, keys, line0)
    assert list(names) == ["a", "b"] and list(lengths) == [6200, 10]
    cpu_engine.set_layout(lengths)
    track = cpu_engine.depth_text_parse(arr, line0, segs(cpu_engine.offsets), cpu_engine.new_track())
    for c, nm in enumerate(names):
        assert np.array_equal(cpu_engine.contig(track, c), CROWDED_WANT[nm]), nm


def test_header_segments_send_odd_texts_to_the_slow_path():
    from gci_amd.formats import depthfile
    from gci_amd import cpu
    eng = cpu.CpuEngine(threads=1)
    for text in (b"", b"5\n>a\n1\n", b">\n1\n>b\n2\n"):
        arr = np.frombuffer(text, dtype=np.uint8)
        tiles, keys, bad = eng.depth_text_index(arr)
        line0 = np.concatenate([[0], np.cumsum(tiles.astype(np.uint64))]).astype(np.uint64)
        assert bad != NONE or depthfile.header_segments(arr, keys, line0) is None, text


def test_slow_path_is_the_reference_statement_for_statement():
    from gci_amd.formats import depthfile
    d = depthfile.parse_depth_lines(io.BytesIO(b">a\r\n+7\r\n  3 \n-2\n>b>c\n0_1\n"))
    assert list(d) == ["a", "c"] and d["a"].tolist() == [7, 3, -2] and d["c"].tolist() == [1]
    for bad, exc in ((b"1\n", KeyError), (b">a\n\n", ValueError), (b">a\n1.5\n", ValueError), (b"", KeyError)):
        with pytest.raises(exc):
            depthfile.parse_depth_lines(io.BytesIO(bad))


# ---- the multi-member gzip inflate (host_io.cpp; reached through gci_amd.hostio for tools/asan_host.sh) --------------------------

def _project_style(text_items) -> bytes:
    """This project's layout: a '>name\\n' member, then members of ~0.8 MB of text each (here: fixed-Huffman members of zlib)."""
    out = b""
    for name, body in text_items:
        out += gzip.compress(b">" + name + b"\n", 1)
        for k in range(0, len(body), 800_000):
            c = zlib.compressobj(1, zlib.DEFLATED, 31, 9, zlib.Z_FIXED)
            out += c.compress(body[k:k + 800_000]) + c.flush()
    return out


def _reference_style(text_items, chunk=50_000) -> bytes:
    """The reference's layout: one member per (contig, chunk), Python's gzip at level 9 with FNAME set."""
    f = io.BytesIO()
    for name, body in text_items:
        for k in range(0, len(body), chunk):
            with gzip.GzipFile(filename="GCI.depth.gz", mode="wb", compresslevel=9, fileobj=f, mtime=0) as g:
                g.write((b">" + name + b"\n" if k == 0 else b"") + body[k:k + chunk])
    return f.getvalue()


def _bodies(seed):
    rng = np.random.default_rng(seed)
    return [(b"ctg%d" % k, b"".join(b"%d\n" % v for v in np.repeat(rng.integers(0, 60, 400), rng.integers(1, 200, 400)).tolist()))
            for k in range(4)]


@pytest.mark.parametrize("writer", [_project_style, _reference_style])
def test_inflate_matches_python_gzip_on_both_writers(writer):
    from gci_amd import hostio
    raw = writer(_bodies(1))
    g = hostio.GzipText(raw, threads=4)
    assert g.members > 4 and not g.serial
    assert g.export().tobytes() == gzip.decompress(raw)
    half = g.nbytes // 3
    assert g.export(half, 1000).tobytes() == gzip.decompress(raw)[half:half + 1000]
    g.close()


def test_inflate_single_member_padding_and_empty_file():
    from gci_amd import hostio
    body = b"".join(b for _, b in _bodies(2))
    raw = gzip.compress(body, 6)
    assert hostio.gzip_inflate(raw).tobytes() == body
    padded = raw + b"\0" * 7 + raw + b"\0\0"
    assert hostio.gzip_inflate(padded).tobytes() == gzip.decompress(padded)
    assert hostio.gzip_inflate(b"").tobytes() == b""


def test_inflate_ignores_false_magic_inside_member_payloads():
    """Stored blocks carry their bytes as they are: plant member headers -- and a whole valid member -- inside payloads.  The
    speculative inflate decodes those candidates too; the chain from offset 0 must not take them."""
    from gci_amd import hostio
    fake = gzip.compress(b">fake\n1\n2\n", 9)
    body = (b"12\n" * 1000 + b"\x1f\x8b\x08\x00" + b"7\n" * 50 + fake + b"\x1f\x8b\x08\x08abc\0" + b"3\n" * 4000)
    raw = b""
    for level in (0, 0, 1):
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        raw += c.compress(body) + c.flush()
    g = hostio.GzipText(raw, threads=3)
    assert g.members == 3 and g.export().tobytes() == gzip.decompress(raw)
    g.close()


def test_inflate_refuses_damaged_files_where_python_gzip_raises():
    from gci_amd import hostio
    from gci_amd._lib import GciError
    raw = _reference_style(_bodies(3))
    rng = np.random.default_rng(4)
    cases = [raw[:n] for n in (5, 10, 30, len(raw) // 2, len(raw) - 4, len(raw) - 1)]
    cases += [raw + b"x", b"junk" + raw, raw + b"\x1f\x8b"]
    for _ in range(12):
        b = bytearray(raw)
        b[int(rng.integers(0, len(raw)))] ^= 1 << int(rng.integers(0, 8))
        cases.append(bytes(b))
    for bad in cases:
        try:
            want = gzip.decompress(bad)
        except (gzip.BadGzipFile, EOFError, zlib.error, OSError):
            want = None
        if want is None:
            with pytest.raises(GciError):
                hostio.gzip_inflate(bad, threads=2)
        else:
            assert hostio.gzip_inflate(bad, threads=2).tobytes() == want


# ---- the utility's refusals before any device work (tests/golden/score_errors.json) -------------------------------------------

SCENARIOS = json.load(open(os.path.join(GOLDEN, "score_errors.json")))
SCORE_IN = os.path.join(GOLDEN, "score_inputs")


def run_score_scenario(sc, out_root, monkeypatch):
    from gci_amd import score_cli
    monkeypatch.setenv("COLUMNS", "100")
    sub = lambda t: t.replace("{GOLDEN}", GOLDEN).replace("{IN}", SCORE_IN).replace("{OUT}", out_root)       # noqa: E731
    norm = lambda t: t.replace(out_root, "{OUT}").replace(SCORE_IN, "{IN}").replace(GOLDEN, "{GOLDEN}")      # noqa: E731
    so, se = io.StringIO(), io.StringIO()
    code, exc = "completed", None
    try:
        with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
            score_cli.main(["GCI_score.py"] + [sub(a) for a in sc["argv"]])
    except SystemExit as e:
        code = e.code
    except Exception as e:                                 # noqa: BLE001
        code, exc = "exception", {"type": type(e).__name__, "message": str(e)}
    got = {"exit": norm(code) if isinstance(code, str) else code, "exception": exc, "stdout": norm(so.getvalue()),
           "stderr": norm(se.getvalue())}
    assert got == {k: sc[k] for k in ("exit", "exception", "stdout", "stderr")}, sc["name"]


@pytest.mark.parametrize("sc", [s for s in SCENARIOS if not s["gpu"]], ids=lambda s: s["name"])
def test_score_refused_before_any_gpu_work(sc, tmp_path, monkeypatch):
    run_score_scenario(sc, str(tmp_path / "out"), monkeypatch)


def test_entry_point_exists_and_imports_no_torch():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, runpy; sys.argv = ['GCI_score.py', '-r', 'x.fa']\n"
            "try:\n    runpy.run_path(%r, run_name='__main__')\nexcept SystemExit as e:\n    print(repr(e.code))\n"
            "print('torch' in sys.modules)\n") % os.path.join(root, "GCI_score.py")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=120)
    assert r.stdout.strip().splitlines() == [repr('ERROR!!! Please input at least one depth file\n'
                                                  'Please read the help message using "-h" or "--help"'), "False"], r.stderr
