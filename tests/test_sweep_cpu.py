"""filter_sweep.py off the GPU: the CPU twin of gci_bam_sweep (gci_amd/csrc/cpu/gci_cpu.cpp) against the statement of tests/sweep_ref.py on
every case of tests/sweep_cases.py, in both stream forms and for K = 1, 2, 3, the status word included; the argument checks; the row
numbers against the header's macros; the command line's text against the statement's rendering; and the command line's error messages
that need no device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cover_cases as C
import fate_cases as FC
import sweep_cases as SC
import sweep_ref as SR
from gci_amd import _lib, cpu, filtersweep_cli, pipeline
from gci_amd.formats import bam as bamfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    return cpu.CpuEngine(threads=4)


def form_of(name, form):
    c = SC.case(name)
    return (c["stream"], c["offs"]) if form == "stream" else SC.heads(name)


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name", SC.NAMES)
def test_the_twin_gives_the_tables_of_the_statement(twin, name, form):
    c = SC.case(name)
    stream, offs = form_of(name, form)
    twin.set_layout(c["lengths"])
    for run in c["runs"]:
        for digits in SC.DIGITS:
            want, status = SC.want(name, run, digits)
            got = twin.bam_sweep(stream, offs, c["ref_sel"], *run, digits=digits, win=c["win"], win0=c["win0"], has_seq=form == "stream", check=False,
                                 guard=16)
            assert int(twin.last_status[0]) == status, (run, digits)
            assert got.shape == want.shape and np.array_equal(got, want), (run, digits, np.argwhere(got != want)[:5])


def test_a_status_raises_with_its_record(twin):
    c = SC.case("op9")
    with pytest.raises(cpu.CpuError) as e:
        twin.bam_sweep(c["stream"], c["offs"], c["ref_sel"], *FC.DEFAULT)
    assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == SC.STATUS["op9"][0]


def test_argument_errors():
    c = SC.case("window_edges")
    stream, offs, sel = c["stream"], c["offs"], c["ref_sel"]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    table, st = np.zeros(4 * SR.Rows(3).rows, np.uint64), np.zeros(1, np.uint64)
    fresh = cpu.CpuEngine(threads=1)

    def call(ctx, digits=3, win=p(c["win"]), win0=p(c["win0"]), h_table=p(table), status=p(st), d_sel=p(sel)):
        return fresh.lib.gci_bam_sweep(ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1, d_sel, sel.shape[0], win, win0, 30, 0.1, 0.9, digits,
                                       h_table, status)

    assert call(None) == _lib.GCI_E_INVALID
    assert call(fresh.ctx) == _lib.GCI_E_NO_LAYOUT             # windows index the layout's contigs
    assert call(fresh.ctx, win=None, win0=None) == 0           # ... without windows no layout is needed
    fresh.set_layout(c["lengths"])
    for digits in (0, 4, -1, 10):
        assert call(fresh.ctx, digits=digits) == _lib.GCI_E_INVALID, digits
    for kw in (dict(h_table=None), dict(status=None), dict(d_sel=None), dict(win=None)):
        assert call(fresh.ctx, **kw) == _lib.GCI_E_INVALID, kw
    assert call(fresh.ctx) == 0 and np.array_equal(table.reshape(-1, 4), SC.want("window_edges", FC.DEFAULT, 3)[0])


def test_the_row_numbers_are_the_headers():
    """_lib.SweepRows against the GCI_SWEEP_* macros of include/gci_hip.h, evaluated from the header's own text."""
    text = open(os.path.join(ROOT, "include", "gci_hip.h")).read()
    macros = {m.group(1): (m.group(2), m.group(3)) for m in re.finditer(r"#define (GCI_SWEEP_\w+)\(([\w, ]*)\) (.*?)\s*(?:/\*.*)?$", text, re.M)}
    assert set(macros) == {"GCI_SWEEP_BINS", "GCI_SWEEP_MAPQ", "GCI_SWEEP_CLIP", "GCI_SWEEP_CLIP_UNDEF", "GCI_SWEEP_IDEN_BELOW", "GCI_SWEEP_IDEN",
                           "GCI_SWEEP_IDEN_ABOVE", "GCI_SWEEP_IDEN_UNDEF", "GCI_SWEEP_ROWS"}

    def ev(name, *args):
        params, body = macros[name]
        env = dict(zip([x.strip() for x in params.split(",")], args))
        body = re.sub(r"(GCI_SWEEP_\w+)\(([^()]*)\)", lambda m: str(ev(m.group(1), *[eval(a, {}, env) for a in m.group(2).split(",")])), body)
        body = re.sub(r"\(digits\) == 1 \? 10 : \(digits\) == 2 \? 100 : 1000", "(10 if (digits) == 1 else 100 if (digits) == 2 else 1000)", body)
        return eval(body, {}, env)

    for K in (1, 2, 3):
        r = _lib.SweepRows(K)
        assert (r.bins, r.rows) == (ev("GCI_SWEEP_BINS", K), ev("GCI_SWEEP_ROWS", K)) == (10 ** K, 256 + 2 * 10 ** K + 6)
        assert (r.mapq0, r.clip0, r.clip_undef) == (ev("GCI_SWEEP_MAPQ", 0), ev("GCI_SWEEP_CLIP", K, 0), ev("GCI_SWEEP_CLIP_UNDEF", K))
        assert (r.iden_below, r.iden0, r.iden_above, r.iden_undef) == (ev("GCI_SWEEP_IDEN_BELOW", K), ev("GCI_SWEEP_IDEN", K, 0), ev("GCI_SWEEP_IDEN_ABOVE", K),
                                                                       ev("GCI_SWEEP_IDEN_UNDEF", K))
        assert ev("GCI_SWEEP_CLIP", K, r.bins) + 1 == r.clip_undef and ev("GCI_SWEEP_IDEN", K, r.bins) + 1 == r.iden_above and r.iden_undef + 1 == r.rows
    with pytest.raises(ValueError):
        _lib.SweepRows(4)


@pytest.mark.parametrize("digits", SC.DIGITS)
def test_the_command_lines_text_is_the_statements(digits):
    for name, run in (("random_3000", SC.OTHER), ("special_rows", FC.DEFAULT), ("edges", FC.DEFAULT)):
        table, _ = SC.want(name, run, digits)
        got = filtersweep_cli.file_text(2, "some/path.bam", table, digits)
        assert got == SR.file_text(2, "some/path.bam", table, digits)
        lines = got.split("\n")
        assert lines[0].startswith("#file\t2\tsome/path.bam\tprimary=") and lines[1] == "#mapq" and lines[2].split("\t") == list(pipeline.SWEEP_COLUMNS)
        assert len(lines) == 1 + 3 * 2 + SR.Rows(digits).rows + 1          # every row is written
    rows = SR.Rows(digits)
    assert [pipeline.sweep_value(rows, r) for r in (0, 255, rows.clip0, rows.clip0 + 1, rows.clip0 + rows.bins, rows.clip_undef, rows.iden_below, rows.iden0,
                                                    rows.iden0 + rows.bins - 1, rows.iden0 + rows.bins, rows.iden_above, rows.iden_undef)] == [
        "0", "255", "0." + "0" * digits, "0." + "0" * (digits - 1) + "1", "1." + "0" * digits, "undefined", "<0", "0." + "0" * digits, "0." + "9" * digits,
        "1." + "0" * digits, ">1", "undefined"]


def test_kept_at_is_the_sum_of_the_rows_that_pass():
    """Of the rendering, by hand: three records, thresholds (30, 0.1, 0.9)."""
    rows = SR.Rows(1)
    table = np.zeros((rows.rows, 4), dtype=np.uint64)
    for mapq, clip, iden, bases, others in ((60, 0, 10, 100, (1, 1, 1)), (20, 1, 9, 50, (1, 0, 0)), (60, 3, rows.iden_above - rows.iden0, 7, (0, 1, 0))):
        for k, r in enumerate((mapq, rows.clip0 + clip, rows.iden0 + iden)):
            table[r] += np.array([1, bases, others[k], bases * others[k]], dtype=np.uint64)
    body = {}
    for ln in pipeline.sweep_text(table, 1).split("\n"):
        cols = ln.split("\t")
        if ln.startswith("#"):
            sect = ln[1:]
        elif len(cols) == 7 and cols[0] != "value":
            body[(sect, cols[0])] = cols[5:]
    assert body[("mapq", "0")] == ["2", "150"] and body[("mapq", "20")] == ["2", "150"] and body[("mapq", "21")] == ["1", "100"] and body[("mapq", "61")] == ["0", "0"]
    assert body[("clip", "0.0")] == ["1", "100"] and body[("clip", "0.2")] == ["1", "100"] and body[("clip", "0.3")] == ["2", "107"] and body[("clip", "1.0")] == ["2", "107"]
    assert body[("identity", "1.0")] == ["1", "100"] and body[("identity", "0.9")] == ["1", "100"] and body[("identity", "0.0")] == ["1", "100"]
    assert body[("clip", "undefined")] == ["-", "-"] and body[("identity", "<0")] == ["-", "-"] and body[("identity", ">1")] == ["-", "-"]


# ---- the command line's error messages (none of them reaches the device) -------------------------------------------------------------

def filter_sweep(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "filter_sweep.py")] + list(argv), capture_output=True, text=True,
                          env=dict(os.environ, GCI_EARLY_HIP="0"), timeout=120)


def test_cli_error_messages(tmp_path):
    ok = str(tmp_path / "a.bam")
    bamfmt.write_bam(ok, ["c1", "c2"], [100, 50], [C.rec(0, 3, [(C.M, 5)], aux=FC.nm(0))])
    r = filter_sweep()
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! No BAM file given"
    r = filter_sweep(str(tmp_path / "missing.bam"))
    assert r.returncode != 0 and r.stderr.startswith('ERROR!!! The file "%s" cannot be read as a BAM file' % (tmp_path / "missing.bam"))
    r = filter_sweep("--chrs", "c1,nope", ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The chromosome "nope" of --chrs is not in the header of "%s"' % ok
    for bad in (["--digits", "0"], ["--digits", "4"], ["--classes", "kept"], ["--join"]):
        r = filter_sweep(*bad, ok)
        assert r.returncode == 2 and "Traceback" not in r.stderr, bad
    (tmp_path / "GCI_sweep.sweep.txt").write_bytes(b"")
    r = filter_sweep("-d", str(tmp_path), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s/GCI_sweep.sweep.txt" exists\nPlease use "-f" or "--force" to rewrite' % tmp_path
    (tmp_path / "GCI_sweep.sweep.txt").unlink()
    r = filter_sweep("-d", str(tmp_path), "-R", str(tmp_path / "missing.bed"), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s" does not exist' % (tmp_path / "missing.bed")
    other = str(tmp_path / "b.bam")
    bamfmt.write_bam(other, ["c1", "c2"], [100, 51], [])
    r = filter_sweep("-d", str(tmp_path), ok, other)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The @SQ table of "%s" differs from that of "%s"' % (other, ok)
    assert "Traceback" not in r.stderr and not (tmp_path / "GCI_sweep.sweep.txt").exists()
    h = " ".join(filter_sweep("-h").stdout.split()).replace("- ", "-")      # (argparse breaks lines at hyphens)
    assert "before the -op join" in h and "as bam_depth.py counts them" in h and "flank-trimmed" in h and "below 2^40" in h and "multiples of 10^-K" in h
