"""clip_sites.py off the GPU: the CPU twin of gci_bam_clip_size / _write and gci_clip_sites_size / _write (gci_amd/csrc/cpu/gci_cpu.cpp)
against the statement of tests/clips_ref.py on every case of tests/clips_cases.py in both stream forms; the argument checks; the command
line's error messages; the BED text, read back by bedgraph_cli.parse_regions; and the summary text."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import clips_cases as C
import clips_ref as R
from gci_amd import _lib, bedgraph_cli, cpu, pipeline
from gci_amd.formats import bam as bamfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    return cpu.CpuEngine(threads=4)


def pairs_of(ivl):
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
        want_left, want_right, want_counts, want_status = C.want(name, run)
        left, right, counts = twin.bam_clip(stream, offs, c["ref_sel"], form == "stream", *run, check=False, guard=16)
        assert int(twin.last_status[0]) == want_status, run
        assert counts == want_counts and pairs_of(left) == want_left and pairs_of(right) == want_right, run
        # the built tracks: per base the events there
        for ivl, want in ((left, want_left), (right, want_right)):
            track = twin.depth_build(np.ascontiguousarray(ivl), 0)
            assert np.array_equal(track, R.track_of(want, c["lengths"])) and int(track.sum()) == len(want)


def test_the_twin_gives_the_hand_written_events(twin):
    for (name, run), (left, right, counted) in C.EXPECTED.items():
        c = C.case(name)
        twin.set_layout(c["lengths"])
        got_left, got_right, counts = twin.bam_clip(c["stream"], c["offs"], c["ref_sel"], True, *run)
        assert (pairs_of(got_left), pairs_of(got_right), counts[0]) == (left, right, counted), (name, run)


@pytest.mark.parametrize("name", C.SITE_NAMES)
def test_the_twin_gives_the_sites_of_the_statement(twin, name):
    c = C.site_case(name)
    twin.set_layout(c["lengths"])
    assert twin.total == c["left"].shape[0]
    for k, (min_reads, windows) in enumerate(c["runs"]):
        for with_depth in (True, False):
            got = twin.clip_sites(c["left"], c["right"], c["depth"] if with_depth else None, min_reads, windows)
            assert (got["pad"] == 0).all()
            assert list(zip(*(got[f].tolist() for f in ("contig", "pos", "left", "right", "depth")))) == C.want_sites(name, k, with_depth), (k, with_depth)


def test_a_malformed_record_raises_with_its_index(twin):
    c = C.case("op9")
    twin.set_layout(c["lengths"])
    with pytest.raises(cpu.CpuError) as e:
        twin.bam_clip(c["stream"], c["offs"], c["ref_sel"], min_clip=5)
    assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == C.MALFORMED["op9"]


# ---- argument errors -------------------------------------------------------------------------------------------------------------------

def test_argument_errors_of_the_record_calls(twin):
    lib, c = twin.lib, C.case("end_operations")
    stream, offs, sel = c["stream"], c["offs"], c["ref_sel"]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    counts, st = np.zeros(3, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    out = np.zeros(64, dtype=cpu.IVL_DTYPE)
    size = lambda ctx, min_clip=5, h_counts=p(counts), status=p(st): lib.gci_bam_clip_size(ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1,   # noqa: E731
                                                                                           p(sel), sel.shape[0], 0x704, 0, min_clip, h_counts, status)
    write = lambda ctx, cap, n_rec=offs.shape[0]: lib.gci_bam_clip_write(ctx, p(stream), stream.shape[0], p(offs), n_rec, 1, p(out), cap, p(st))   # noqa: E731
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 64) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 64) == _lib.GCI_E_INVALID                           # no size call in front of it
    assert size(None) == _lib.GCI_E_INVALID and size(fresh.ctx, min_clip=0) == _lib.GCI_E_INVALID and size(fresh.ctx, min_clip=-3) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, h_counts=None) == _lib.GCI_E_INVALID and size(fresh.ctx, status=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and counts.tolist() == [9, 5, 4]
    assert write(fresh.ctx, 64, n_rec=offs.shape[0] - 1) == _lib.GCI_E_INVALID   # not the input the size call measured
    out[:] = (7, 7, 7, 7)
    assert write(fresh.ctx, 8) == _lib.GCI_E_CAPACITY
    assert (out["contig"] == 7).all()                                            # ... and nothing was written
    assert write(fresh.ctx, 9) == 0 and (out["contig"][:9] == 0).all() and (out["contig"][9:] == 7).all()


def test_argument_errors_of_the_site_calls(twin):
    lib, c = twin.lib, C.site_case("tiles")
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    n = ctypes.c_uint64(0)
    out = np.full((8192, 6), 7, dtype=np.int32)
    win = (_lib.Window * 2)()
    win[0].begin, win[0].end, win[1].begin, win[1].end = 0, 5000, 4999, 6000
    left, right, depth = c["left"], c["right"], c["depth"]
    size = lambda ctx, l=left, r=right, d=depth, m=3, w=None, nw=0, h_n=ctypes.byref(n): lib.gci_clip_sites_size(ctx, p(l), p(r), p(d), m, w, nw, h_n)   # noqa: E731
    write = lambda ctx, cap, m=3, d=depth: lib.gci_clip_sites_write(ctx, p(left), p(right), p(d), m, None, 0, p(out), cap)      # noqa: E731
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 8192) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 8192) == _lib.GCI_E_INVALID                          # no size call in front of it
    assert size(None) == _lib.GCI_E_INVALID and size(fresh.ctx, m=0) == _lib.GCI_E_INVALID and size(fresh.ctx, h_n=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, l=None) == _lib.GCI_E_INVALID and size(fresh.ctx, nw=2) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, w=win, nw=2) == _lib.GCI_E_INVALID                    # windows that overlap
    raw = np.zeros(left.shape[0] + 8, dtype=np.int32)                            # a track that begins one element in: not 16-byte aligned
    k = next(i for i in range(1, 5) if (raw.ctypes.data + 4 * i) % 16)
    for which in "lrd":
        assert size(fresh.ctx, **{which: raw[k:k + left.shape[0]]}) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and n.value == len(C.want_sites("tiles", 0)) > 4096
    assert write(fresh.ctx, 8192, m=4) == _lib.GCI_E_INVALID and write(fresh.ctx, 8192, d=None) == _lib.GCI_E_INVALID      # not what was measured
    assert write(fresh.ctx, n.value - 1) == _lib.GCI_E_CAPACITY
    assert (out == 7).all()                                                      # ... and nothing was written
    assert write(fresh.ctx, n.value) == 0 and (out[:n.value, 5] == 0).all() and (out[n.value:] == 7).all()


# ---- the texts -------------------------------------------------------------------------------------------------------------------------

def test_the_bed_text_and_that_parse_regions_reads_it_back(tmp_path):
    sites = np.array([(0, 0, 3, 0, 41, 0), (0, 4095, 0, 12, 7, 0), (2, 123456789, 5, 6, 0, 0)], dtype=cpu.SITE_DTYPE)
    text = pipeline.clip_sites_bed(sites, ["chr1", "chr2", "scaffold_3"])
    assert text == "chr1\t0\t1\t3\t0\t41\nchr1\t4095\t4096\t0\t12\t7\nscaffold_3\t123456789\t123456790\t5\t6\t0\n"
    path = tmp_path / "s.bed"
    path.write_text(text)
    assert bedgraph_cli.parse_regions(str(path)) == [("chr1", 0, 1), ("chr1", 4095, 4096), ("scaffold_3", 123456789, 123456790)]
    assert pipeline.clip_sites_bed(sites[:0], ["chr1"]) == ""


def test_the_summary_text():
    text = pipeline.clip_summary_text(["a.bam", "dir/b.bam"], [[10, 2, 3], [5, 0, 1]], 4, [("min_clip", 100), ("min_reads", 3), ("regions", ".")])
    assert text == ("#file\trecords\tleft_events\tright_events\tpath\n1\t10\t2\t3\ta.bam\n2\t5\t0\t1\tdir/b.bam\ntotal\t15\t2\t4\t.\nsites\t4\n"
                    "min_clip\t100\nmin_reads\t3\nregions\t.\n")


# ---- the command line's error messages (none of them reaches the device) -------------------------------------------------------------

def clip_sites(*argv, cwd=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "clip_sites.py")] + list(argv), capture_output=True, text=True, cwd=cwd,
                          env=dict(os.environ, GCI_EARLY_HIP="0"), timeout=120)


def write_bam(path, refs, records=()):
    bamfmt.write_bam(str(path), [n for n, _ in refs], [l for _, l in refs], list(records))
    return str(path)


def test_cli_error_messages(tmp_path):
    ok = write_bam(tmp_path / "a.bam", [("c1", 100), ("c2", 50)], [C.rec(0, 3, [(C.M, 5)])])
    r = clip_sites()
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! No BAM file given"
    r = clip_sites("-c", "0", ok)
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! -c/--min-clip 0 is not at least 1"
    r = clip_sites("-n", "0", ok)
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! -n/--min-reads 0 is not at least 1"
    r = clip_sites(str(tmp_path / "missing.bam"))
    assert r.returncode != 0 and r.stderr.startswith('ERROR!!! The file "%s" cannot be read as a BAM file' % (tmp_path / "missing.bam"))
    r = clip_sites("--chrs", "c1,nope", ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The chromosome "nope" of --chrs is not in the header of "%s"' % ok
    r = clip_sites("-R", str(tmp_path / "missing.bed"), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s" does not exist' % (tmp_path / "missing.bed")
    bed = tmp_path / "r.bed"
    bed.write_text("c1\t10\n")
    r = clip_sites("-R", str(bed), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! Line 1 of the bed file "%s" has fewer than three columns' % bed
    bed.write_text("c1\t10\t20\nc3\t1\t2\n")
    r = clip_sites("-R", str(bed), ok)
    assert r.returncode != 0 and r.stderr.strip().startswith('ERROR!!! The chromosome "c3" of the bed file is not in')
    bed.write_text("c2\t10\t51\n")
    r = clip_sites("-R", str(bed), ok)
    assert r.returncode != 0 and r.stderr.strip().startswith("ERROR!!! The region c2:10-51 of the bed file ends beyond the contig (50 bases)")
    for name in ("GCI_clip.clip.left.depth.gz", "GCI_clip.clip.right.depth.gz", "GCI_clip.clip.sites.bed", "GCI_clip.clip.txt"):
        (tmp_path / name).write_bytes(b"")
        r = clip_sites("-d", str(tmp_path), ok)
        assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s/%s" exists\nPlease use "-f" or "--force" to rewrite' % (tmp_path, name)
        (tmp_path / name).unlink()
    bad = write_bam(tmp_path / "b.bam", [("c1", 100), ("c2", 51)])
    r = clip_sites("-o", "x", "-d", str(tmp_path), ok, bad)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The @SQ table of "%s" differs from that of "%s"' % (bad, ok)
    r = clip_sites("-h")
    assert r.returncode == 0 and "a choice for long reads, not a measurement" in " ".join(r.stdout.split())
    assert "Traceback" not in r.stderr
