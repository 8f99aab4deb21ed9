"""filter_reads.py off the GPU: the CPU twins of gci_bam_reads_size / _write (gci_amd/csrc/cpu/gci_cpu.cpp) against the statement of
tests/reads_ref.py on every case of tests/reads_cases.py, in both stream forms, byte for byte; the argument checks; and the command
line's error messages that need no device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import cover_cases as C
import fate_cases as FC
import reads_cases as RC
import reads_ref as RR
from gci_amd import _lib, cpu
from gci_amd.formats import bam as bamfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    return cpu.CpuEngine(threads=4)


def form_of(name, form):
    c = RC.case(name)
    return (c["stream"], c["offs"]) if form == "stream" else RC.heads(name)


def want_status(name):
    return ((RC.STATUS[name][0] << 8) | -RC.STATUS[name][1]) if name in RC.STATUS else RR.NO_STATUS


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_cases_hold_what_they_are_for(name):
    """Every windowed case (but the two that are about having no row) lists a record and leaves one out; the status words are the ones
    the cases are named for."""
    c, (rows, status) = RC.case(name), RC.want(name)
    assert status == want_status(name)
    if c["win0"] is not None and name not in RC.WINDOWED_WITHOUT_BOTH:
        assert 0 < len(rows) < len(c["offs"])
    if name in RC.WINDOWED_WITHOUT_BOTH:
        assert not rows
    for a, b in zip(c["win0"][:-1] if c["win0"] is not None else [], c["win0"][1:] if c["win0"] is not None else []):
        w = c["win"][int(a):int(b)]
        assert (w[:, 0] < w[:, 1]).all() and (w[:-1, 1] < w[1:, 0]).all()


def test_the_cases_reach_the_shapes_they_are_for():
    by = {n: dict(RC.want(n)[0]) for n in ("groups_257", "groups_513", "stage_overflow", "long_contig_name", "window_edges", "no_reference")}
    assert sorted(by["groups_257"]) == [RC.GROUP - 1, RC.GROUP] and sorted(by["groups_513"]) == [RC.GROUP - 1, 2 * RC.GROUP]
    assert sum(len(r) for i, r in by["stage_overflow"].items() if i < RC.GROUP) > RC.STAGE and len(by["stage_overflow"]) == 300
    assert [len(r) > 300 for r in by["long_contig_name"].values()] == [True, False]
    listed = lambda n: [r.split(b"\t")[1].decode() for r in by[n].values()]                # noqa: E731
    assert listed("window_edges") == ["one_base_left", "inside", "around", "over_both", "one_base_right", "last_base"]
    assert listed("no_reference") == ["at100", "at150", "at199"]
    c = RC.case("chunks")
    assert {C.CH - 1, C.CH, C.CH + 1} <= {len(bamfmt.decode_record(c["stream"], o).cigar) for o in c["offs"].tolist()}
    c = RC.case("names")
    assert {1, 2, 3, 4, 254} <= {len(bamfmt.decode_record(c["stream"], o).name) for o in c["offs"].tolist()}


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name", RC.NAMES)
def test_the_twin_gives_the_rows_of_the_statement(twin, name, form):
    c = RC.case(name)
    stream, offs = form_of(name, form)
    rows, status = RC.want(name)
    twin.set_layout(c["lengths"])
    text, n_rows = twin.bam_reads(stream, offs, c["ref_sel"], RC.classes(name), c["mask"], c["names"], c["win"], c["win0"], has_seq=form == "stream",
                                  check=False, guard=64)
    assert int(twin.last_status[0]) == status
    assert n_rows == len(rows)
    assert text == RR.text(rows)


def test_the_twin_takes_the_file_number_and_the_join_classes(twin):
    c = RC.case("one_per_class")
    twin.set_layout(c["lengths"])
    cls = RC.classes("one_per_class").copy()
    cls[cls == 6] = np.arange(8, 8 + int((cls == 6).sum()), dtype=np.uint8)              # kept -> shadowed, unpaired, ...
    want = RR.stream_rows(c["stream"], c["offs"], c["ref_sel"], c["names"], cls, _lib.READS_CLASS_MASK, file_no=4000000000)[0]
    assert [r.split(b"\t")[-1] for _, r in want][-2:] == [b"shadowed\n", b"unpaired\n"]
    text, n = twin.bam_reads(c["stream"], c["offs"], c["ref_sel"], cls, _lib.READS_CLASS_MASK, c["names"], file_no=4000000000)
    assert text == RR.text(want) and n == len(want) and text.startswith(b"4000000000\t")


def test_a_status_raises_with_its_record(twin):
    c = RC.case("op9")
    twin.set_layout(c["lengths"])
    with pytest.raises(cpu.CpuError) as e:
        twin.bam_reads(c["stream"], c["offs"], c["ref_sel"], RC.classes("op9"), c["mask"], c["names"])
    assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == 3


def test_class_bytes_of_another_input_are_reported(twin):
    """A class bit set on a record that can have no class (an unselected contig): GCI_E_INVALID names it, no row."""
    c = RC.case("one_per_class")
    twin.set_layout(c["lengths"])
    cls = np.full(len(c["offs"]), 6, dtype=np.uint8)
    want, status = RR.stream_rows(c["stream"], c["offs"], c["ref_sel"], c["names"], cls, 1 << 6)
    assert status == (0 << 8) | 1 and len(want) == len(cls) - 1
    text, _ = twin.bam_reads(c["stream"], c["offs"], c["ref_sel"], cls, 1 << 6, c["names"], check=False)
    assert int(twin.last_status[0]) == status and text == RR.text(want)


def test_argument_errors(twin):
    lib, c = twin.lib, RC.case("window_edges")
    stream, offs, sel = c["stream"], c["offs"], c["ref_sel"]
    cls = RC.classes("window_edges")
    p = lambda a: ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    name_len, name_off, names = np.array([1], np.uint32), np.array([0], np.uint64), np.frombuffer(b"a", dtype=np.uint8)
    rows, size, st = ctypes.c_uint64(0), ctypes.c_uint64(0), np.zeros(1, np.uint64)

    def size_call(ctx, mask=RC.ALL, d_class=p(cls), n_rows=ctypes.byref(rows), n_bytes=ctypes.byref(size), status=p(st), lens=p(name_len), win=p(c["win"]),
                  the_offs=offs):
        return lib.gci_bam_reads_size(ctx, p(stream), stream.shape[0], p(the_offs), the_offs.shape[0], 1, p(sel), sel.shape[0], d_class, mask, win,
                                      p(c["win0"]), lens, 1, n_rows, n_bytes, status)

    def write_call(ctx, out, cap, the_stream=stream, the_offs=offs, lens=p(name_len)):
        return lib.gci_bam_reads_write(ctx, p(the_stream), the_stream.shape[0], p(the_offs), the_offs.shape[0], p(names), p(name_off), lens, p(out), cap)

    fresh = cpu.CpuEngine(threads=1)
    assert size_call(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and size_call(None) == _lib.GCI_E_INVALID
    fresh.set_layout(c["lengths"])
    out = np.full(4096, 0xA5, dtype=np.uint8)
    assert write_call(fresh.ctx, out, 4096) == _lib.GCI_E_INVALID                      # no size call yet
    for mask in (1 << 0, 1 << 7, 1 << 13, 1 << 31, RC.ALL | 1):
        assert size_call(fresh.ctx, mask=mask) == _lib.GCI_E_INVALID, mask             # none, error, classes that do not exist
    for kw in (dict(d_class=None), dict(n_rows=None), dict(n_bytes=None), dict(status=None), dict(lens=None), dict(win=None)):
        assert size_call(fresh.ctx, **kw) == _lib.GCI_E_INVALID, kw
    assert size_call(fresh.ctx) == 0
    want = RR.text(RC.want("window_edges")[0])
    assert size.value == len(want) and rows.value == 6 and int(st[0]) == RR.NO_STATUS
    assert write_call(fresh.ctx, out, len(want) - 1) == _lib.GCI_E_CAPACITY and (out == 0xA5).all()      # too small: nothing is written
    assert write_call(fresh.ctx, out, len(want)) == 0 and out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()
    # another input than the size call's: a copy of the stream, of the offsets, another name length
    out[:] = 0xA5
    assert write_call(fresh.ctx, out, 4096, the_stream=stream.copy()) == _lib.GCI_E_INVALID
    assert write_call(fresh.ctx, out, 4096, the_offs=offs.copy()) == _lib.GCI_E_INVALID
    assert write_call(fresh.ctx, out, 4096, lens=p(np.array([2], np.uint32))) == _lib.GCI_E_INVALID
    # ... and after a size call over another input, the first one's buffers are refused
    other = offs[:3].copy()
    assert size_call(fresh.ctx, the_offs=other) == 0
    assert write_call(fresh.ctx, out, 4096) == _lib.GCI_E_INVALID and (out == 0xA5).all()
    assert write_call(fresh.ctx, out, 4096, the_offs=other) == 0


# ---- the command line's error messages (none of them reaches the device) -------------------------------------------------------------

def filter_reads(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "filter_reads.py")] + list(argv), capture_output=True, text=True,
                          env=dict(os.environ, GCI_EARLY_HIP="0"), timeout=120)


def test_cli_error_messages(tmp_path):
    ok = str(tmp_path / "a.bam")
    bamfmt.write_bam(ok, ["c1", "c2"], [100, 50], [C.rec(0, 3, [(C.M, 5)], aux=FC.nm(0))])
    r = filter_reads()
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! No BAM file given"
    r = filter_reads(str(tmp_path / "missing.bam"))
    assert r.returncode != 0 and r.stderr.startswith('ERROR!!! The file "%s" cannot be read as a BAM file' % (tmp_path / "missing.bam"))
    r = filter_reads("--chrs", "c1,nope", ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The chromosome "nope" of --chrs is not in the header of "%s"' % ok
    for asked in ("kept,clipped", "none", "error"):
        r = filter_reads("--classes", asked, ok)
        assert r.returncode != 0 and r.stderr.strip() == ('ERROR!!! The class "%s" of --classes is not one of secondary, supplementary, mapq, clip, '
                                                          "identity, kept" % asked.split(",")[-1])
    r = filter_reads("--classes", "joined", ok)
    assert r.returncode != 0 and r.stderr.strip().endswith("(shadowed, unpaired, contig, overlap, joined need --join)")
    r = filter_reads("--cover", "1", ok)
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! The option --cover needs --join"
    (tmp_path / "GCI_reads.reads.tsv").write_bytes(b"")
    r = filter_reads("-d", str(tmp_path), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s/GCI_reads.reads.tsv" exists\nPlease use "-f" or "--force" to rewrite' % tmp_path
    (tmp_path / "GCI_reads.reads.tsv").unlink()
    r = filter_reads("-d", str(tmp_path), "-R", str(tmp_path / "missing.bed"), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s" does not exist' % (tmp_path / "missing.bed")
    bed = tmp_path / "r.bed"
    bed.write_text("c1\t5\n")
    r = filter_reads("-d", str(tmp_path), "-R", str(bed), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! Line 1 of the bed file "%s" has fewer than three columns' % bed
    other = str(tmp_path / "b.bam")
    bamfmt.write_bam(other, ["c1", "c2"], [100, 51], [])
    r = filter_reads("-d", str(tmp_path), ok, other)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The @SQ table of "%s" differs from that of "%s"' % (other, ok)
    assert "Traceback" not in r.stderr and not (tmp_path / "GCI_reads.reads.tsv").exists()
    h = filter_reads("-h").stdout
    assert "authoritative" in h and "truncated" in h and "GCI.py" in h
