"""depth_to_bedgraph.py off the GPU: the numpy statement (tests/bedgraph_ref.py) against a per-base loop, the CPU twins of
gci_depth_runs_* / gci_bedgraph_* against the statement on the shapes the device is tested on, the arguments the exports check, and
the command line through the CPU twin: every refusal, --chrs, -R, -f and the file's bytes."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bedgraph_cases as C
import bedgraph_ref as R
from gci_amd import _lib, cpu, pipeline
from gci_amd.formats import depthfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loop_text(seg, name, coord0):
    """The format, base by base."""
    out, k = [], 0
    seg = [int(x) for x in seg]
    while k < len(seg):
        j = k
        while j < len(seg) and seg[j] == seg[k]:
            j += 1
        out.append(name + b"\t" + str(coord0 + k).encode() + b"\t" + str(coord0 + j).encode() + b"\t" + str(seg[k]).encode() + b"\n")
        k = j
    return b"".join(out)


@pytest.mark.parametrize("name", ["tile_edges", "window_edges", "decimal_widths", "names", "chunk_257_split"])
def test_the_statement_equals_a_loop_over_the_bases(name):
    c = C.case(name)
    runs, run0, text, byte0 = C.want(name)
    parts = []
    for k, (w, nm, c0) in enumerate(zip(c["windows"], c["names"], c["coord0"])):
        a, b = R.clip(w, c["track"].shape[0])
        parts.append(loop_text(c["track"][a:b], nm, c0))
        assert int(byte0[k + 1] - byte0[k]) == len(parts[-1])
        assert int(run0[k + 1] - run0[k]) == parts[-1].count(b"\n")
    assert b"".join(parts) == text
    assert R.window_text(np.array([2, 2, -1]), b"x", 7) == b"x\t7\t9\t2\nx\t9\t10\t-1\n" and R.window_text(np.zeros(0, np.int32), b"x", 0) == b""


def test_the_block_size_is_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "gci_hip.h")).read()
    assert int(re.search(r"#define GCI_BG_RUNS_PER_BLOCK (\d+)", hdr).group(1)) == C.RPB == _lib.BG_RUNS_PER_BLOCK


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_the_cpu_twin_equals_the_statement(name):
    c = C.case(name)
    e = cpu.CpuEngine()
    e.set_layout(c["lengths"])
    assert e.offsets.tolist() == C.offsets(c["lengths"])[0]
    want_runs, want_run0, want_text, want_byte0 = C.want(name)
    runs, run0 = e.depth_runs(c["track"], c["windows"])
    assert np.array_equal(run0, want_run0) and np.array_equal(runs, want_runs)
    text, byte0 = e.bedgraph(c["track"], c["windows"], c["names"], c["coord0"])
    assert np.array_equal(byte0, want_byte0) and bytes(text) == want_text


def test_the_twin_checks_its_arguments():
    p = cpu._p
    W = cpu._Window
    t = np.array([1, 1, 2, 2, 2, 3, 0, 0], dtype=np.int32)
    w = (W * 2)(W(-5, 4), W(4, 1 << 40))                       # clamped to [0, 4) and [4, total)
    run0, runs = np.zeros(3, np.uint64), np.full(8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    e = cpu.CpuEngine()
    assert e.lib.gci_depth_runs_count(e.ctx, p(t), w, 2, p(run0)) == _lib.GCI_E_NO_LAYOUT
    e.set_layout([8])
    t = np.concatenate([t, np.zeros(e.total - 8, np.int32)])
    assert e.lib.gci_depth_runs_write(e.ctx, p(t), p(runs), 8) == _lib.GCI_E_INVALID          # no count call in front
    assert e.lib.gci_depth_runs_count(e.ctx, None, w, 2, p(run0)) == _lib.GCI_E_INVALID
    assert e.lib.gci_depth_runs_count(e.ctx, p(t), None, 2, p(run0)) == _lib.GCI_E_INVALID
    assert e.lib.gci_depth_runs_count(e.ctx, p(t), w, 2, None) == _lib.GCI_E_INVALID
    assert e.lib.gci_depth_runs_count(e.ctx, p(t), w, 2, p(run0)) == 0 and run0.tolist() == [0, 2, 5]
    assert e.lib.gci_depth_runs_write(e.ctx, p(t), p(runs), 4) == _lib.GCI_E_CAPACITY
    assert e.lib.gci_depth_runs_write(e.ctx, p(t), None, 0) == _lib.GCI_E_CAPACITY
    assert (runs == 0xA5A5A5A5A5A5A5A5).all()
    assert e.lib.gci_depth_runs_write(e.ctx, p(t), p(runs), 5) == 0
    assert runs[:5].view(R.RUN_DTYPE).tolist() == [(0, 1), (2, 2), (0, 2), (1, 3), (2, 0)] and (runs[5:] == 0xA5A5A5A5A5A5A5A5).all()
    coord, nlen, noff, blob = np.array([0, 4], np.int64), np.array([1, 2], np.uint32), np.array([0, 2], np.uint64), np.frombuffer(b"a#bc#", np.uint8)
    byte0, out = np.zeros(3, np.uint64), np.full(64, 0xA5, np.uint8)
    r = runs.view(R.RUN_DTYPE)
    assert e.lib.gci_bedgraph_write(e.ctx, p(r), p(run0), w, 2, p(coord), p(blob), p(noff), p(nlen), p(out), 64) == _lib.GCI_E_INVALID   # no size call
    assert e.lib.gci_bedgraph_size(e.ctx, p(r), None, w, 2, p(coord), p(nlen), p(byte0)) == _lib.GCI_E_INVALID
    assert e.lib.gci_bedgraph_size(e.ctx, p(r), p(run0), w, 2, p(coord), p(nlen), None) == _lib.GCI_E_INVALID
    assert e.lib.gci_bedgraph_size(e.ctx, p(r), p(run0), w, 2, p(np.array([0, -1], np.int64)), p(nlen), p(byte0)) == _lib.GCI_E_INVALID
    assert e.lib.gci_bedgraph_size(e.ctx, p(r), p(run0), w, 2, p(coord), p(nlen), p(byte0)) == 0
    want = b"a\t0\t2\t1\na\t2\t4\t2\nbc\t4\t5\t2\nbc\t5\t6\t3\nbc\t6\t%d\t0\n" % e.total
    assert byte0.tolist() == [0, 16, len(want)]
    assert e.lib.gci_bedgraph_write(e.ctx, p(r), p(run0), w, 2, p(coord), p(blob), p(noff), p(nlen), p(out), len(want) - 1) == _lib.GCI_E_CAPACITY
    assert (out == 0xA5).all()
    assert e.lib.gci_bedgraph_write(e.ctx, p(r), p(run0), w, 2, p(coord), p(blob), p(noff), p(nlen), p(out), len(want)) == 0
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()
    # a window an uint32 start cannot span
    big = cpu.CpuEngine()
    big.set_layout([0x7FFFFFFF] * 3)
    assert big.lib.gci_depth_runs_count(big.ctx, p(t), (W * 1)(W(0, 1 << 33)), 1, p(run0)) == _lib.GCI_E_INVALID


# ---- the command line through the CPU twin ------------------------------------------------------------------------------------------

class _HostEngine(cpu.CpuEngine):
    def to_device(self, a):
        return np.ascontiguousarray(a)


def _host_reader(engine, path, ref_lengths=None, plotter_v2=False):
    """pipeline.read_depth_tracks by the reference's own statements, into the twin's memory."""
    with gzip.open(path, "rb") as f:
        depths = depthfile.parse_depth_lines(f)
    return pipeline._upload_depths(engine, depths)


@pytest.fixture()
def cli(monkeypatch):
    from gci_amd import bedgraph_cli
    e = _HostEngine()
    monkeypatch.setattr(pipeline, "default_engine", lambda: e)
    monkeypatch.setattr(pipeline, "read_depth_tracks", _host_reader)
    return bedgraph_cli


DEPTHS = {"chrA": [3] * 10 + [0] * 5 + [7], "chrB": [1, 2, 2], "chrC": [9] * 4}


@pytest.fixture()
def depth_gz(tmp_path):
    path = str(tmp_path / "in.depth.gz")
    with gzip.open(path, "wb") as f:
        for name, d in DEPTHS.items():
            f.write(b">%s\n" % name.encode() + b"".join(b"%d\n" % x for x in d))
    return path


def _run(cli, argv):
    with pytest.raises(SystemExit) as e:
        cli.main(["depth_to_bedgraph.py"] + argv)
    return e.value.code


def test_the_whole_file(cli, depth_gz, tmp_path):
    prefix = str(tmp_path / "out")
    assert cli.main(["depth_to_bedgraph.py", depth_gz, prefix]) == prefix + ".bedgraph"
    got = open(prefix + ".bedgraph", "rb").read()
    assert got == (b"chrA\t0\t10\t3\nchrA\t10\t15\t0\nchrA\t15\t16\t7\nchrB\t0\t1\t1\nchrB\t1\t3\t2\nchrC\t0\t4\t9\n")
    assert R.expand(got) == {k.encode(): v for k, v in DEPTHS.items()}


def test_chrs_regions_and_force(cli, depth_gz, tmp_path):
    prefix = str(tmp_path / "out")
    cli.main(["depth_to_bedgraph.py", "--chrs", "chrC,chrA", depth_gz, prefix])              # the file's order, not the option's
    assert open(prefix + ".bedgraph", "rb").read() == b"chrA\t0\t10\t3\nchrA\t10\t15\t0\nchrA\t15\t16\t7\nchrC\t0\t4\t9\n"
    code = _run(cli, [depth_gz, prefix])
    assert code == 'ERROR!!! The file "%s.bedgraph" exists\nPlease use "-f" or "--force" to rewrite' % prefix
    bed = str(tmp_path / "r.bed")
    with open(bed, "w") as f:                                   # the bed file's order; overlapping; cut inside a run; empty; extra columns
        f.write("chrB\t1\t3\tx\nchrA\t2\t12\nchrA\t8\t16\n\nchrC\t2\t2\nchrA\t0\t5\nchrA\t5\t10\n")
    cli.main(["depth_to_bedgraph.py", "-f", "-R", bed, depth_gz, prefix])
    assert open(prefix + ".bedgraph", "rb").read() == (b"chrB\t1\t3\t2\nchrA\t2\t10\t3\nchrA\t10\t12\t0\nchrA\t8\t10\t3\nchrA\t10\t15\t0\n"
                                                        b"chrA\t15\t16\t7\nchrA\t0\t5\t3\nchrA\t5\t10\t3\n")
    cli.main(["depth_to_bedgraph.py", "--force", "--regions", bed, "--chrs", "chrB,chrC", depth_gz, prefix])
    assert open(prefix + ".bedgraph", "rb").read() == b"chrB\t1\t3\t2\n"


@pytest.mark.parametrize("bed, chrs, message", [
    (None, "chrA,chrZ", 'ERROR!!! The chromosome "chrZ" is not in the depth file'),
    ("chrZ\t0\t1\n", "", 'ERROR!!! The chromosome "chrZ" of the bed file is not in the depth file'),
    ("chrA\t5\t4\n", "", "ERROR!!! The region chrA:5-4 of the bed file does not have 0 <= start <= end"),
    ("chrA\t-1\t4\n", "", "ERROR!!! The region chrA:-1-4 of the bed file does not have 0 <= start <= end"),
    ("chrA\t0\t17\n", "", "ERROR!!! The region chrA:0-17 of the bed file ends beyond the contig (16 bases)"),
    ("chrA\t0\t4\nchrA\t3\n", "", 'ERROR!!! Line 2 of the bed file "{BED}" has fewer than three columns'),
    ("chrA\t0\tx\n", "", 'ERROR!!! Line 1 of the bed file "{BED}" has a coordinate that is not an integer'),
    ("chrA\t0.5\t3\n", "", 'ERROR!!! Line 1 of the bed file "{BED}" has a coordinate that is not an integer'),
])
def test_the_refusals(cli, depth_gz, tmp_path, bed, chrs, message):
    prefix = str(tmp_path / "out")
    argv = []
    path = str(tmp_path / "r.bed")
    if bed is not None:
        open(path, "w").write(bed)
        argv += ["-R", path]
    if chrs:
        argv += ["--chrs", chrs]
    code = _run(cli, argv + [depth_gz, prefix])
    assert isinstance(code, str) and code == message.replace("{BED}", path)       # (sys.exit with a string: the line goes to stderr)
    assert not os.path.exists(prefix + ".bedgraph")


def test_depth_bedgraph_returns_bytes_and_checks_its_items(cli, depth_gz):
    tracks, _ = _host_reader(_HostEngine(), depth_gz)
    assert pipeline.depth_bedgraph(tracks, [("chrB", 0, 3), ("chrB", 3, 3)]) == b"chrB\t0\t1\t1\nchrB\t1\t3\t2\n"
    assert pipeline.depth_bedgraph(tracks, []) == b""
    with pytest.raises(ValueError):
        pipeline.depth_bedgraph(tracks, [("chrB", 0, 4)])


def test_entry_point_exists_and_imports_no_torch(tmp_path):
    script = os.path.join(ROOT, "depth_to_bedgraph.py")
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1")
    (tmp_path / "there.bedgraph").write_bytes(b"")
    r = subprocess.run([sys.executable, script, "x.depth.gz", "there"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=env)
    assert r.returncode == 1 and r.stderr.startswith('ERROR!!! The file "there.bedgraph" exists\nPlease use "-f" or "--force" to rewrite')
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, cwd=str(tmp_path), timeout=120, env=env)
    assert r.returncode == 2 and "the following arguments are required: input.depth.gz, output_prefix" in r.stderr
