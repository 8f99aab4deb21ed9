"""indel_sites.py off the GPU: the CPU twin of gci_bam_indel_size / _write and gci_indel_sites_size / _write (gci_amd/csrc/cpu/gci_cpu.cpp)
against the statement of tests/indels_ref.py on every case of tests/indels_cases.py in both stream forms; the argument checks; the
command line's error messages; the BED text, read back by bedgraph_cli.parse_regions; and the summary text."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import indels_cases as C
import indels_ref as R
from gci_amd import _lib, bedgraph_cli, cpu, pipeline
from gci_amd.formats import bam as bamfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("contig", "start", "end", "del", "ins", "depth")


@pytest.fixture(scope="module")
def twin():
    return cpu.CpuEngine(threads=4)


def dels_of(ivl):
    assert (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist(), ivl["end"].tolist()))


def inss_of(ivl):
    assert (ivl["start"] == ivl["end"]).all() and (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist()))


# ---- the twin against the statement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name", C.NAMES)
def test_the_twin_gives_the_events_of_the_statement(twin, name, form):
    c = C.case(name)
    stream, offs = (c["stream"], c["offs"]) if form == "stream" else C.heads(name)
    twin.set_layout(c["lengths"])
    for run in c["runs"]:
        want_dels, want_inss, want_counts, want_status = C.want(name, run)
        dels, inss, counts = twin.bam_indel(stream, offs, c["ref_sel"], form == "stream", *run, check=False, guard=16)
        assert int(twin.last_status[0]) == want_status, run
        assert counts == want_counts and dels_of(dels) == want_dels and inss_of(inss) == want_inss, run
        # the built tracks: per base the events over it
        for ivl, want in ((dels, want_dels), (inss, want_inss)):
            track = twin.depth_build(np.ascontiguousarray(ivl), 0)
            assert np.array_equal(track, R.track_of(want, c["lengths"]))


def test_the_twin_gives_the_hand_written_events(twin):
    for (name, run), (dels, inss, counted) in C.EXPECTED.items():
        c = C.case(name)
        twin.set_layout(c["lengths"])
        got_dels, got_inss, counts = twin.bam_indel(c["stream"], c["offs"], c["ref_sel"], True, *run)
        assert (dels_of(got_dels), inss_of(got_inss), counts[0]) == (dels, inss, counted), (name, run)


@pytest.mark.parametrize("name", C.SITE_NAMES)
def test_the_twin_gives_the_sites_of_the_statement(twin, name):
    c = C.site_case(name)
    twin.set_layout(c["lengths"])
    assert twin.total == c["dele"].shape[0]
    for k, (min_reads, windows) in enumerate(c["runs"]):
        for with_depth in (True, False):
            got = twin.indel_sites(c["dele"], c["ins"], c["depth"] if with_depth else None, min_reads, windows)
            assert list(zip(*(got[f].tolist() for f in FIELDS))) == C.want_sites(name, k, with_depth), (k, with_depth)


def test_a_malformed_record_raises_with_its_index(twin):
    for name, rec in C.MALFORMED.items():
        c = C.case(name)
        twin.set_layout(c["lengths"])
        with pytest.raises(cpu.CpuError) as e:
            twin.bam_indel(c["stream"], c["offs"], c["ref_sel"], min_len=5)
        assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == rec, name


# ---- argument errors -------------------------------------------------------------------------------------------------------------------

def test_argument_errors_of_the_record_calls(twin):
    lib, c = twin.lib, C.case("thresholds")
    stream, offs, sel = c["stream"], c["offs"], c["ref_sel"]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    counts, st = np.zeros(3, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    out = np.zeros(64, dtype=cpu.IVL_DTYPE)
    size = lambda ctx, min_len=5, h_counts=p(counts), status=p(st): lib.gci_bam_indel_size(ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1,   # noqa: E731
                                                                                           p(sel), sel.shape[0], 0x704, 0, min_len, h_counts, status)
    write = lambda ctx, cap, n_rec=offs.shape[0]: lib.gci_bam_indel_write(ctx, p(stream), stream.shape[0], p(offs), n_rec, 1, p(out), cap, p(st))   # noqa: E731
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 64) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 64) == _lib.GCI_E_INVALID                           # no size call in front of it
    assert size(None) == _lib.GCI_E_INVALID and size(fresh.ctx, min_len=0) == _lib.GCI_E_INVALID and size(fresh.ctx, min_len=-3) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, h_counts=None) == _lib.GCI_E_INVALID and size(fresh.ctx, status=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and counts.tolist() == [4, 4, 2]
    assert write(fresh.ctx, 64, n_rec=offs.shape[0] - 1) == _lib.GCI_E_INVALID   # not the input the size call measured
    out[:] = (7, 7, 7, 7)
    assert write(fresh.ctx, 5) == _lib.GCI_E_CAPACITY
    assert (out["contig"] == 7).all()                                            # ... and nothing was written
    assert write(fresh.ctx, 6) == 0 and (out["contig"][:6] == 0).all() and (out["contig"][6:] == 7).all()


def test_argument_errors_of_the_site_calls(twin):
    lib, c = twin.lib, C.site_case("random")
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    n = ctypes.c_uint64(0)
    out = np.full((8192, 6), 7, dtype=np.int32)
    win = (_lib.Window * 2)()
    win[0].begin, win[0].end, win[1].begin, win[1].end = 0, 5000, 4999, 6000
    dele, ins, depth = c["dele"], c["ins"], c["depth"]
    size = lambda ctx, l=dele, r=ins, d=depth, m=3, w=None, nw=0, h_n=ctypes.byref(n): lib.gci_indel_sites_size(ctx, p(l), p(r), p(d), m, w, nw, h_n)   # noqa: E731
    write = lambda ctx, cap, m=3, d=depth: lib.gci_indel_sites_write(ctx, p(dele), p(ins), p(d), m, None, 0, p(out), cap)      # noqa: E731
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 8192) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 8192) == _lib.GCI_E_INVALID                          # no size call in front of it
    assert size(None) == _lib.GCI_E_INVALID and size(fresh.ctx, m=0) == _lib.GCI_E_INVALID and size(fresh.ctx, h_n=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, l=None) == _lib.GCI_E_INVALID and size(fresh.ctx, nw=2) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, w=win, nw=2) == _lib.GCI_E_INVALID                    # windows that overlap
    raw = np.zeros(dele.shape[0] + 8, dtype=np.int32)                            # a track that begins one element in: not 16-byte aligned
    k = next(i for i in range(1, 5) if (raw.ctypes.data + 4 * i) % 16)
    for which in "lrd":
        assert size(fresh.ctx, **{which: raw[k:k + dele.shape[0]]}) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and n.value == len(C.want_sites("random", 1)) > 4
    assert write(fresh.ctx, 8192, m=4) == _lib.GCI_E_INVALID and write(fresh.ctx, 8192, d=None) == _lib.GCI_E_INVALID      # not what was measured
    assert write(fresh.ctx, n.value - 1) == _lib.GCI_E_CAPACITY
    assert (out == 7).all()                                                      # ... and nothing was written
    assert write(fresh.ctx, n.value) == 0 and (out[:n.value, 0] >= 0).all() and (out[n.value:] == 7).all()


# ---- the texts -------------------------------------------------------------------------------------------------------------------------

def test_the_bed_text_and_that_parse_regions_reads_it_back(tmp_path):
    sites = np.array([(0, 0, 1, 3, 0, 41), (0, 4090, 4160, 0, 12, 7), (2, 123456789, 123456849, 5, 6, 0)], dtype=cpu.INDEL_SITE_DTYPE)
    text = pipeline.indel_sites_bed(sites, ["chr1", "chr2", "scaffold_3"])
    assert text == "chr1\t0\t1\t3\t0\t41\nchr1\t4090\t4160\t0\t12\t7\nscaffold_3\t123456789\t123456849\t5\t6\t0\n"
    path = tmp_path / "s.bed"
    path.write_text(text)
    assert bedgraph_cli.parse_regions(str(path)) == [("chr1", 0, 1), ("chr1", 4090, 4160), ("scaffold_3", 123456789, 123456849)]
    assert pipeline.indel_sites_bed(sites[:0], ["chr1"]) == ""


def test_the_summary_text():
    text = pipeline.indel_summary_text(["a.bam", "dir/b.bam"], [[10, 2, 3], [5, 0, 1]], 4, [("min_len", 50), ("min_reads", 3), ("regions", ".")])
    assert text == ("#file\trecords\tdeletions\tinsertions\tpath\n1\t10\t2\t3\ta.bam\n2\t5\t0\t1\tdir/b.bam\ntotal\t15\t2\t4\t.\nsites\t4\n"
                    "min_len\t50\nmin_reads\t3\nregions\t.\n")
    assert (pipeline.INDEL_MIN_LEN, pipeline.INDEL_MIN_READS) == (50, 3)


# ---- the command line's error messages (none of them reaches the device) -------------------------------------------------------------

def indel_sites(*argv, cwd=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "indel_sites.py")] + list(argv), capture_output=True, text=True, cwd=cwd,
                          env=dict(os.environ, GCI_EARLY_HIP="0"), timeout=120)


def write_bam(path, refs, records=()):
    bamfmt.write_bam(str(path), [n for n, _ in refs], [l for _, l in refs], list(records))
    return str(path)


def test_cli_error_messages(tmp_path):
    ok = write_bam(tmp_path / "a.bam", [("c1", 100), ("c2", 50)], [C.rec(0, 3, [(C.M, 5)])])
    r = indel_sites()
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! No BAM file given"
    r = indel_sites("-l", "0", ok)
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! -l/--min-len 0 is not at least 1"
    r = indel_sites("-n", "0", ok)
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! -n/--min-reads 0 is not at least 1"
    r = indel_sites(str(tmp_path / "missing.bam"))
    assert r.returncode != 0 and r.stderr.startswith('ERROR!!! The file "%s" cannot be read as a BAM file' % (tmp_path / "missing.bam"))
    r = indel_sites("--chrs", "c1,nope", ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The chromosome "nope" of --chrs is not in the header of "%s"' % ok
    r = indel_sites("-R", str(tmp_path / "missing.bed"), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s" does not exist' % (tmp_path / "missing.bed")
    bed = tmp_path / "r.bed"
    bed.write_text("c1\t10\n")
    r = indel_sites("-R", str(bed), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! Line 1 of the bed file "%s" has fewer than three columns' % bed
    bed.write_text("c1\t10\t20\nc3\t1\t2\n")
    r = indel_sites("-R", str(bed), ok)
    assert r.returncode != 0 and r.stderr.strip().startswith('ERROR!!! The chromosome "c3" of the bed file is not in')
    bed.write_text("c2\t10\t51\n")
    r = indel_sites("-R", str(bed), ok)
    assert r.returncode != 0 and r.stderr.strip().startswith("ERROR!!! The region c2:10-51 of the bed file ends beyond the contig (50 bases)")
    for name in ("GCI_indel.indel.del.depth.gz", "GCI_indel.indel.ins.depth.gz", "GCI_indel.indel.sites.bed", "GCI_indel.indel.txt"):
        (tmp_path / name).write_bytes(b"")
        r = indel_sites("-d", str(tmp_path), ok)
        assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s/%s" exists\nPlease use "-f" or "--force" to rewrite' % (tmp_path, name)
        (tmp_path / name).unlink()
    bad = write_bam(tmp_path / "b.bam", [("c1", 100), ("c2", 51)])
    r = indel_sites("-o", "x", "-d", str(tmp_path), ok, bad)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The @SQ table of "%s" differs from that of "%s"' % (bad, ok)
    r = indel_sites("-h")
    help_text = " ".join(r.stdout.split())
    assert r.returncode == 0 and "a choice, not a measurement" in help_text and "depth + del" in help_text
    assert "Traceback" not in r.stderr
