"""bam_depth.py off the GPU: the statement of its semantics (tests/cover_ref.py) against a per-base loop and against the depths of the
SAM specification's example alignment written out by hand; the CPU twin of gci_bam_cover_size / _write / gci_track_add
(gci_amd/csrc/cpu/gci_cpu.cpp) against the statement on every case of tests/cover_cases.py; the argument checks; and the command
line's error messages."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import cover_cases as C
import cover_ref as R
from gci_amd import _lib, cpu
from gci_amd.formats import bam as bamfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    return cpu.CpuEngine(threads=4)


# ---- the statement itself -----------------------------------------------------------------------------------------------------------

def test_the_statement_gives_the_hand_written_depths_of_the_sam_specification_example():
    assert C.SAM_SPEC_DEPTH.shape[0] == 45 and C.SAM_SPEC_DEPTH_J.shape[0] == 45
    (plain,), st = C.want("sam_spec", C.PLAIN)
    (with_del,), _ = C.want("sam_spec", C.WITH_DEL)
    assert st == R.NO_STATUS
    assert np.array_equal(plain, C.SAM_SPEC_DEPTH)
    assert np.array_equal(with_del, C.SAM_SPEC_DEPTH_J)


@pytest.mark.parametrize("name", C.NAMES)
def test_the_statement_equals_a_per_base_loop(name):
    c = C.case(name)
    for run in c["runs"]:
        slow = R.stream_depth_per_base(c["stream"], c["offs"], c["lengths"], c["ref_sel"], *run)
        for a, b in zip(C.want(name, run)[0], slow):
            assert np.array_equal(a, b)


def test_the_statement_names_the_first_malformed_record():
    for name in C.NAMES:
        for run in C.case(name)["runs"]:
            st = C.want(name, run)[1]
            assert st == (((C.MALFORMED[name] << 8) | 7) if name in C.MALFORMED else R.NO_STATUS), name


def test_the_cases_hold_what_they_are_named_for():
    ops = [len(bamfmt.decode_record(C.case("chunks")["stream"], o).cigar) for o in C.case("chunks")["offs"][:4]]
    assert ops == [C.CH - 1, C.CH, C.CH + 1, 2 * C.CH + 1] and C.CH == _lib.COVER_CHUNK_OPS
    c = C.case("phases")
    assert {(int(o) + 36 + int(c["stream"][int(o) + 12])) % 4 for o in c["offs"]} == {0, 1, 2, 3}
    assert {int(c["stream"][int(o) + 12]) % 4 for o in c["offs"]} == {0, 1, 2, 3}
    c = C.case("long_cigar")
    first = bamfmt.decode_record(c["stream"], c["offs"][0])
    assert first.n_cigar_field == 2 and len(first.cigar) == 65537
    assert len(bamfmt.decode_record(c["stream"], c["offs"][1]).cigar) == 5 and len(bamfmt.decode_record(c["stream"], c["offs"][2]).cigar) == 2
    assert sum(l for o, l in bamfmt.decode_record(C.case("contig_ends")["stream"], C.case("contig_ends")["offs"][-1]).cigar if o in (0, 2, 3)) > 1 << 31
    # every device scan crosses its 4096-entry blocks in every run: records, chunks, and one record's chunks across the block's edge
    for run in C.case("scan_blocks")["runs"]:
        n = C.chunks_per_record("scan_blocks", run)
        first = np.cumsum(n) - n
        assert n.shape[0] > C.SCAN_BLOCK and int(n.sum()) > C.SCAN_BLOCK
        assert int(first[C.SCAN_BLOCK - 1]) == C.SCAN_BLOCK - 1 and int(n[C.SCAN_BLOCK - 1]) == 3
    # the heads form holds the same records without SEQ / QUAL
    for name in ("sam_spec", "long_cigar"):
        hs, ho = C.heads(name)
        assert len(ho) == len(C.case(name)["offs"]) and hs.shape[0] < C.case(name)["stream"].shape[0]
        assert all(R.bounds_ok(hs, o, has_seq=False) for o in ho)


@pytest.mark.parametrize("name", ["sam_spec", "long_cigar", "random_3000"])
def test_the_heads_form_of_the_cases_is_what_gci_bam_heads_makes(name, tmp_path):
    """cover_cases.to_heads against the host pipeline that feeds the `heads` ingest mode, over the case written as a BAM file."""
    from gci_amd import hostio
    c = C.case(name)
    path = str(tmp_path / "case.bam")
    bamfmt.write_bam_stream(path, c["stream"], level=1, threads=2)
    want_stream, want_offs = C.heads(name)
    with hostio.bam_heads(np.fromfile(path, dtype=np.uint8), threads=2) as h:
        assert np.array_equal(np.asarray(h.offsets), want_offs)
        assert np.asarray(h.stream).tobytes() == want_stream.tobytes()


# ---- the CPU twin against the statement ------------------------------------------------------------------------------------------------

def twin_depths(twin, c, stream, offs, has_seq, run, check=True):
    """-> (depths per contig, status word, intervals) of the twin's size / write pair, built with its depth_build at flank 0."""
    twin.set_layout(c["lengths"])
    ivl = twin.bam_cover(stream, offs, c["ref_sel"], has_seq, run[0], run[1], run[2], check=check)
    track = twin.depth_build(ivl, 0)
    return [twin.contig(track, k).astype(np.int64) for k in range(len(c["lengths"]))], int(twin.last_status[0]), ivl


def covered_total(ivl, lengths):
    """The bases the intervals cover inside their contigs, interval by interval."""
    L = np.asarray(lengths, dtype=np.int64)[ivl["contig"]]
    a, b = ivl["start"].astype(np.int64), np.minimum(ivl["end"].astype(np.int64) + 1, L)
    return int(np.maximum(b - a, 0).sum())


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name, run", C.pairs())
def test_the_twin_equals_the_statement(twin, name, run, form):
    c = C.case(name)
    stream, offs = (c["stream"], c["offs"]) if form == "stream" else C.heads(name)
    want, want_status = C.want(name, run)
    got, status, ivl = twin_depths(twin, c, stream, offs, form == "stream", run, check=False)
    assert status == want_status
    if name in C.MALFORMED:
        return
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert covered_total(ivl, c["lengths"]) == sum(int(w.sum()) for w in want)
    assert (ivl["contig"] >= 0).all() and (ivl["start"] >= 0).all() and (ivl["end"] >= ivl["start"]).all() and (ivl["pad"] == 0).all()


def test_the_twin_gives_the_hand_written_depths(twin):
    c = C.case("sam_spec")
    assert np.array_equal(twin_depths(twin, c, c["stream"], c["offs"], True, C.PLAIN)[0][0], C.SAM_SPEC_DEPTH)
    assert np.array_equal(twin_depths(twin, c, c["stream"], c["offs"], True, C.WITH_DEL)[0][0], C.SAM_SPEC_DEPTH_J)


def test_a_malformed_record_raises_with_its_index(twin):
    c = C.case("op9")
    twin.set_layout(c["lengths"])
    with pytest.raises(cpu.CpuError) as e:
        twin.bam_cover(c["stream"], c["offs"], c["ref_sel"])
    assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == 3


def test_track_add(twin):
    twin.set_layout([1, 4095, 4096, 4097])
    rng = np.random.default_rng(5)
    a, b = (rng.integers(-1000, 1000, twin.total).astype(np.int32) for _ in range(2))
    want = a + b
    assert twin.track_add(a, b) is a and np.array_equal(a, want)
    # whole, 16-byte aligned tracks only (libgci_hip.so adds 16-byte vectors): a slice that begins one element in is refused, untouched
    raw = np.zeros(twin.total + 8, dtype=np.int32)
    k = next(i for i in range(1, 5) if (raw.ctypes.data + 4 * i) % 16)
    ones = np.ones(twin.total, dtype=np.int32)
    with pytest.raises(cpu.CpuError) as e:
        twin.track_add(raw[k:k + twin.total], ones)
    assert e.value.status == _lib.GCI_E_INVALID and not raw.any()


def test_argument_errors(twin):
    lib, c = twin.lib, C.case("sam_spec")
    stream, offs, sel = c["stream"], c["offs"], c["ref_sel"]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    n, st = ctypes.c_uint64(0), np.zeros(1, dtype=np.uint64)
    out = np.zeros(64, dtype=cpu.IVL_DTYPE)
    size = lambda ctx, n_out=ctypes.byref(n), status=p(st): lib.gci_bam_cover_size(ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1, p(sel),   # noqa: E731
                                                                                  sel.shape[0], 0x704, 0, 0, n_out, status)
    write = lambda ctx, cap, n_rec=offs.shape[0]: lib.gci_bam_cover_write(ctx, p(stream), stream.shape[0], p(offs), n_rec, 1, p(out), cap, p(st))   # noqa: E731
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 64) == _lib.GCI_E_NO_LAYOUT
    assert lib.gci_track_add(fresh.ctx, p(out), p(out)) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 64) == _lib.GCI_E_INVALID                           # no size call in front of it
    assert size(fresh.ctx, n_out=None) == _lib.GCI_E_INVALID and size(fresh.ctx, status=None) == _lib.GCI_E_INVALID
    assert size(None) == _lib.GCI_E_INVALID
    assert lib.gci_track_add(fresh.ctx, None, p(out)) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and n.value > 1
    assert write(fresh.ctx, 64, n_rec=offs.shape[0] - 1) == _lib.GCI_E_INVALID   # not the input the size call measured
    out[:] = (7, 7, 7, 7)
    assert write(fresh.ctx, n.value - 1) == _lib.GCI_E_CAPACITY
    assert (out["contig"] == 7).all()                                            # ... and nothing was written
    assert write(fresh.ctx, n.value) == 0 and (out["contig"][:n.value] == 0).all() and (out["contig"][n.value:] == 7).all()


# ---- the command line's error messages (none of them reaches the device) -------------------------------------------------------------

def bam_depth(*argv, cwd=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bam_depth.py")] + list(argv), capture_output=True, text=True, cwd=cwd,
                          env=dict(os.environ, GCI_EARLY_HIP="0"), timeout=120)


def write_bam(path, refs, records=()):
    bamfmt.write_bam(str(path), [n for n, _ in refs], [l for _, l in refs], list(records))
    return str(path)


def test_cli_error_messages(tmp_path):
    ok = write_bam(tmp_path / "a.bam", [("c1", 100), ("c2", 50)], [C.rec(0, 3, [(C.M, 5)])])
    r = bam_depth()
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! No BAM file given"
    r = bam_depth(str(tmp_path / "missing.bam"))
    assert r.returncode != 0 and r.stderr.startswith('ERROR!!! The file "%s" cannot be read as a BAM file' % (tmp_path / "missing.bam"))
    (tmp_path / "junk.bam").write_bytes(b"this is not a BGZF file, however long it is")
    r = bam_depth(ok, str(tmp_path / "junk.bam"))
    assert r.returncode != 0 and r.stderr.startswith('ERROR!!! The file "%s" cannot be read as a BAM file' % (tmp_path / "junk.bam"))
    r = bam_depth("--chrs", "c1,nope", ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The chromosome "nope" of --chrs is not in the header of "%s"' % ok
    (tmp_path / "GCI_raw.depth.gz").write_bytes(b"")
    r = bam_depth("-d", str(tmp_path), ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s/GCI_raw.depth.gz" exists\nPlease use "-f" or "--force" to rewrite' % tmp_path
    for other in ([("c1", 100), ("c2", 51)], [("c2", 50), ("c1", 100)], [("c1", 100)]):
        bad = write_bam(tmp_path / "b.bam", other)
        r = bam_depth("-o", "x", "-d", str(tmp_path), ok, bad)
        assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The @SQ table of "%s" differs from that of "%s"' % (bad, ok)
    r = bam_depth("-G", "0xZZ", ok)
    assert r.returncode == 2 and "is not an integer" in r.stderr
    assert "Traceback" not in r.stderr
