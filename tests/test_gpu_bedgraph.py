"""depth_to_bedgraph.py on the GPU: gci_depth_runs_* / gci_bedgraph_* (k_bedgraph.hip) against the numpy statement
(tests/bedgraph_ref.py) for every byte of the runs, the offsets and the text -- the outputs filled with 0xA5 beforehand, the bytes
behind the totals untouched --, the capacity and argument checks, and the command line: the reference's own MH63.depth.gz expanded
back to its text, a file of this project's writer against the same payload from Python's gzip, --chrs and -R, the entry point."""
import ctypes
import gzip
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bedgraph_cases as C
import bedgraph_ref as R
from gci_amd import _lib, cpu, phases, pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH63 = os.path.join(ROOT, "tests", "golden", "MH63", "MH63.depth.gz")
PAD = 80                                                     # guard bytes behind every output


class Filled:
    """A device buffer of n + PAD bytes, every byte 0xA5, `shift` bytes into an allocation."""

    def __init__(self, engine, n, shift=0):
        self.engine, self.n, self.shift = engine, int(n), shift
        self.buf = engine.T.empty(self.n + PAD + shift, engine.T.uint8, engine.device)
        assert engine.lib.gci_memset(engine.ctx, engine._p(self.buf), 0xA5, self.n + PAD + shift) == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + shift)

    def host(self, used):
        """-> the first `used` bytes; what lies behind them, and in front of the buffer, must still be 0xA5."""
        engine = self.engine
        engine.sync()
        h = self.buf.cpu().numpy()
        assert (h[:self.shift] == 0xA5).all() and (h[self.shift + used:] == 0xA5).all(), "bytes outside the output were written"
        return h[self.shift:self.shift + used]


def blob_of(names):
    """The names with non-zero bytes behind every one of them -> (blob, offsets, lengths)."""
    parts, off = [], []
    for k, nm in enumerate(names):
        off.append(sum(len(x) for x in parts))
        parts += [nm, bytes([0xF0 + k % 15]) * (1 + k % 3)]
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.asarray(off, dtype=np.uint64), np.asarray([len(x) for x in names], dtype=np.uint32)


def four_calls(engine, c, out_shift=0, run_cap=None, byte_cap=None):
    """The four exports over a case -> (runs, run0, text, byte0); a cap given: -> the status of that write call."""
    lib, p = engine.lib, engine._p
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731
    engine.set_layout(c["lengths"])
    assert engine.offsets == C.offsets(c["lengths"])[0]
    d_track = engine.to_device(c["track"])
    nw = len(c["windows"])
    arr = engine._window_array(c["windows"])
    run0 = Filled(engine, (nw + 1) * 8)
    assert lib.gci_depth_runs_count(engine.ctx, p(d_track), arr, nw, run0.ptr) == 0
    h_run0 = run0.host((nw + 1) * 8).view(np.uint64).copy()
    n_runs = int(h_run0[nw])
    runs = Filled(engine, n_runs * 8)
    if run_cap is not None:
        st = lib.gci_depth_runs_write(engine.ctx, p(d_track), runs.ptr, run_cap)
        runs.host(0)
        return st
    assert lib.gci_depth_runs_write(engine.ctx, p(d_track), runs.ptr, n_runs) == 0
    h_runs = runs.host(n_runs * 8).view(R.RUN_DTYPE).copy()
    blob, name_off, name_len = blob_of(c["names"])
    coord = np.asarray(c["coord0"], dtype=np.int64)
    byte0 = Filled(engine, (nw + 1) * 8)
    assert lib.gci_bedgraph_size(engine.ctx, runs.ptr, run0.ptr, arr, nw, vp(coord), vp(name_len), byte0.ptr) == 0
    h_byte0 = byte0.host((nw + 1) * 8).view(np.uint64).copy()
    total = int(h_byte0[nw])
    out = Filled(engine, total, out_shift)
    d_blob = engine.to_device(blob)
    st = lib.gci_bedgraph_write(engine.ctx, runs.ptr, run0.ptr, arr, nw, vp(coord), p(d_blob), vp(name_off), vp(name_len), out.ptr,
                                total if byte_cap is None else byte_cap)
    if byte_cap is not None:
        out.host(0)
        return st
    assert st == 0
    return h_runs, h_run0, out.host(total).tobytes(), h_byte0


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_the_device_equals_the_statement(engine, name):
    want_runs, want_run0, want_text, want_byte0 = C.want(name)
    runs, run0, text, byte0 = four_calls(engine, C.case(name))
    assert np.array_equal(run0, want_run0)
    assert np.array_equal(runs, want_runs)
    assert np.array_equal(byte0, want_byte0)
    assert text == want_text
    if name in ("all_zero", "all_37"):
        assert text.count(b"\n") == 1


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_an_output_that_begins_at_any_byte(engine, shift):
    for name in ("names", "window_edges"):
        assert four_calls(engine, C.case(name), out_shift=shift)[2] == C.want(name)[2]


def test_capacity(engine):
    c = C.case("window_edges")
    _, run0, text, _ = C.want("window_edges")
    for cap in (int(run0[-1]) - 1, 0):
        assert four_calls(engine, c, run_cap=cap) == _lib.GCI_E_CAPACITY
    for cap in (len(text) - 1, 0):
        assert four_calls(engine, c, byte_cap=cap) == _lib.GCI_E_CAPACITY


def test_the_engine_methods_the_cpu_twin_and_the_statement_agree(engine):
    c = C.case("layout25")
    want_runs, want_run0, want_text, want_byte0 = C.want("layout25")
    twin = cpu.CpuEngine()
    twin.set_layout(c["lengths"])
    engine.set_layout(c["lengths"])
    d = engine.to_device(c["track"])
    for e, t in ((engine, d), (twin, c["track"])):
        runs, run0 = e.depth_runs(t, c["windows"])
        assert np.array_equal(run0, want_run0) and np.array_equal(runs, want_runs)
        text, byte0 = e.bedgraph(t, c["windows"], c["names"], c["coord0"])
        assert bytes(text) == want_text and np.array_equal(byte0, want_byte0)
    runs, run0 = engine.depth_runs(d, [])
    assert runs.shape == (0,) and run0.tolist() == [0]
    text, byte0 = engine.bedgraph(d, [(5, 5)], [b"x"], [5])
    assert bytes(text) == b"" and byte0.tolist() == [0, 0]


def test_arguments(engine):
    from gci_amd.device import Engine
    lib, p = engine.lib, engine._p
    engine.set_layout([8])
    d = engine.to_device(np.zeros(engine.total, dtype=np.int32))
    arr = engine._window_array([(0, 8)])
    run0 = Filled(engine, 16)
    runs = Filled(engine, 8)
    assert lib.gci_depth_runs_write(engine.ctx, p(d), runs.ptr, 8) == _lib.GCI_E_INVALID          # no count call in front
    assert lib.gci_depth_runs_count(engine.ctx, None, arr, 1, run0.ptr) == _lib.GCI_E_INVALID
    assert lib.gci_depth_runs_count(engine.ctx, p(d), None, 1, run0.ptr) == _lib.GCI_E_INVALID
    assert lib.gci_depth_runs_count(engine.ctx, p(d), arr, 1, None) == _lib.GCI_E_INVALID
    assert lib.gci_depth_runs_count(engine.ctx, p(d), arr, 1, run0.ptr) == 0
    assert lib.gci_depth_runs_write(engine.ctx, None, runs.ptr, 8) == _lib.GCI_E_INVALID
    engine.issue_scan_windows(d, [(0, 4)], -1.0, 0.0)                                          # other windows since the count
    assert lib.gci_depth_runs_write(engine.ctx, p(d), runs.ptr, 8) == _lib.GCI_E_INVALID
    runs.host(0)
    one, name_len, name_off = np.zeros(1, np.int64), np.ones(1, np.uint32), np.zeros(1, np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731
    assert lib.gci_bedgraph_size(engine.ctx, runs.ptr, None, arr, 1, vp(one), vp(name_len), run0.ptr) == _lib.GCI_E_INVALID
    assert lib.gci_bedgraph_write(engine.ctx, runs.ptr, run0.ptr, arr, 1, vp(one), p(d), vp(name_off), vp(name_len), runs.ptr, 8) == _lib.GCI_E_INVALID
    bare = Engine(0)
    with pytest.raises(_lib.GciError) as err:
        bare.depth_runs(d, [(0, 4)])
    assert err.value.status == _lib.GCI_E_NO_LAYOUT
    engine.set_layout([0x7FFFFFFF] * 3)                              # (nothing of that size is allocated: the window is refused first)
    assert lib.gci_depth_runs_count(engine.ctx, p(d), engine._window_array([(0, 1 << 33)]), 1, run0.ptr) == _lib.GCI_E_INVALID


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def _main(engine, argv):
    from gci_amd import bedgraph_cli
    pipeline._ENGINE = engine
    phases.start()
    try:
        bedgraph_cli.main(["depth_to_bedgraph.py"] + argv)
        return phases.report()
    finally:
        phases.stop()


def test_the_reference_s_own_file_comes_back_line_for_line(engine, tmp_path):
    """The bedGraph of MH63.depth.gz, every line expanded to `end - start` lines of `depth` under its name, is the gunzipped input:
    the text is walked run by run (a run of n bases of width w is n times the same w + 1 bytes)."""
    prefix = str(tmp_path / "mh63")
    log = _main(engine, [MH63, prefix])
    assert {"bedgraph_runs", "bedgraph_text", "bedgraph_write_file"} <= set(log["wall_s"])
    raw, parts = open(MH63, "rb").read(), []
    while raw:
        d = zlib.decompressobj(31)
        parts.append(d.decompress(raw))
        raw = d.unused_data.lstrip(b"\0")
    text = np.frombuffer(b"".join(parts), dtype=np.uint8)
    rows = [ln.split(b"\t") for ln in open(prefix + ".bedgraph", "rb").read().split(b"\n")[:-1]]
    at, k = 0, 0
    while k < len(rows):
        name = rows[k][0]
        head = b">" + name + b"\n"
        assert text[at:at + len(head)].tobytes() == head
        at += len(head)
        pos = 0
        while k < len(rows) and rows[k][0] == name:
            _, a, b, d = rows[k]
            n, line = int(b) - int(a), np.frombuffer(d + b"\n", dtype=np.uint8)
            assert int(a) == pos and n > 0 and (k == 0 or rows[k - 1][0] != name or rows[k - 1][3] != d)      # maximal runs, no gap
            assert (text[at:at + n * line.shape[0]].reshape(n, line.shape[0]) == line).all(), (name, a, b, d)
            at += n * line.shape[0]
            pos, k = int(b), k + 1
    assert at == text.shape[0] and len({r[0] for r in rows}) == 12


@pytest.fixture(scope="module")
def two_files(engine, tmp_path_factory):
    """The layout25 track as this project's writer writes it, and the same payload through Python's gzip."""
    d = tmp_path_factory.mktemp("bg")
    c = C.case("layout25")
    engine.set_layout(c["lengths"])
    own, plain = str(d / "own.depth.gz"), str(d / "plain.depth.gz")
    with open(own, "wb") as f:
        for name, blob in zip(c["names"], engine.depth_deflate(engine.to_device(c["track"]))):
            z = zlib.compressobj(1, zlib.DEFLATED, 31)
            f.write(z.compress(b">%s\n" % name) + z.flush() + bytes(blob))
    with gzip.open(plain, "wb", compresslevel=1) as f:
        f.write(gzip.open(own, "rb").read())
    return own, plain


def test_both_readers_give_the_same_bytes(engine, two_files, tmp_path):
    own, plain = two_files
    a = _main(engine, [own, str(tmp_path / "a")])
    b = _main(engine, [plain, str(tmp_path / "b")])
    assert a["notes"]["depth_read:" + own] == "members" and b["notes"]["depth_read:" + plain] == "text"
    got = open(str(tmp_path / "a.bedgraph"), "rb").read()
    assert got == open(str(tmp_path / "b.bedgraph"), "rb").read() == C.want("layout25")[2]


def test_chrs_and_regions(engine, two_files, tmp_path):
    own, _ = two_files
    c = C.case("layout25")
    off = C.offsets(c["lengths"])[0]
    prefix = str(tmp_path / "o")
    _main(engine, ["--chrs", "contig_9,contig_3,contig_24", own, prefix])
    keep = [3, 9, 24]
    want, _ = R.text(c["track"], [c["windows"][k] for k in keep], [c["names"][k] for k in keep], [0] * 3)
    assert open(prefix + ".bedgraph", "rb").read() == want
    rng = np.random.default_rng(15)
    regions = []
    for k in rng.integers(0, 25, 40):
        a, b = sorted(int(x) for x in rng.integers(0, c["lengths"][k] + 1, 2))
        regions.append((int(k), a, b))
    regions += [(3, 4095, 4097), (3, 0, 0), (9, 8191, 8191), (9, 0, c["lengths"][9])]
    bed = str(tmp_path / "r.bed")
    with open(bed, "w") as f:
        f.write("".join("contig_%d\t%d\t%d\n" % r for r in regions))
    _main(engine, ["-f", "-R", bed, own, prefix])
    want, _ = R.text(c["track"], [(off[k] + a, off[k] + b) for k, a, b in regions], [c["names"][k] for k, _, _ in regions], [a for _, a, _ in regions])
    assert open(prefix + ".bedgraph", "rb").read() == want
    _main(engine, ["-f", "-R", bed, "--chrs", "contig_3", own, prefix])
    kept = [r for r in regions if r[0] == 3]
    want, _ = R.text(c["track"], [(off[k] + a, off[k] + b) for k, a, b in kept], [b"contig_3"] * len(kept), [a for _, a, _ in kept])
    assert open(prefix + ".bedgraph", "rb").read() == want


def test_the_entry_point_on_the_native_provider(two_files, tmp_path):
    """`python depth_to_bedgraph.py ...` as a user starts it: the library's own HBM buffers (no torch in the process), GCI_PHASES."""
    own, _ = two_files
    log = str(tmp_path / "phases.json")
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1", GCI_PHASES=log)
    env.pop("GCI_HBM", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_to_bedgraph.py"), own, str(tmp_path / "e")], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and r.stdout == "", r.stderr[-3000:]
    assert open(str(tmp_path / "e.bedgraph"), "rb").read() == C.want("layout25")[2]
    ph = json.load(open(log))
    assert ph["notes"]["depth_read:" + own] == "members" and "bedgraph_text" in ph["wall_s"]
