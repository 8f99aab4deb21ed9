"""filter_depth.py off the GPU: the CPU twins of gci_bam_fate and gci_bam_cover_size_sel (gci_amd/csrc/cpu/gci_cpu.cpp) against the
statement of tests/fate_ref.py on every case of tests/fate_cases.py, in both stream forms; the argument checks; and the command
line's error messages that need no device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import cover_cases as C
import fate_cases as FC
import fate_ref as F
from gci_amd import _lib, cpu
from gci_amd.formats import bam as bamfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    return cpu.CpuEngine(threads=4)


def form_of(name, form):
    c = FC.case(name)
    return (c["stream"], c["offs"]) if form == "stream" else FC.heads(name)


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name, run", FC.pairs())
def test_the_twin_gives_the_classes_of_the_statement(twin, name, run, form):
    c = FC.case(name)
    stream, offs = form_of(name, form)
    want_cls, want_counts, want_status = FC.want(name, run)
    cls, counts = twin.bam_fate(stream, offs, c["ref_sel"], *run, has_seq=form == "stream", check=False)
    assert int(twin.last_status[0]) == want_status
    assert np.array_equal(cls, want_cls) and np.array_equal(counts, want_counts)


@pytest.mark.parametrize("form", ["stream", "heads"])
def test_the_twin_on_and_around_every_quotient(twin, form):
    c = FC.case("threshold_band")
    stream, offs = form_of("threshold_band", form)
    seen = set()
    for run in c["runs"]:
        want_cls, want_counts, want_status = FC.want("threshold_band", run)
        cls, counts = twin.bam_fate(stream, offs, c["ref_sel"], *run, has_seq=form == "stream", check=False)
        assert int(twin.last_status[0]) == want_status == F.NO_STATUS
        assert np.array_equal(cls, want_cls) and np.array_equal(counts, want_counts), run
        seen |= set(cls.tolist())
    assert seen == {F.CLIP, F.IDENTITY, F.KEPT}


def test_a_status_raises_with_its_record(twin):
    c = FC.case("clip_no_nm")
    with pytest.raises(cpu.CpuError) as e:
        twin.bam_fate(c["stream"], c["offs"], c["ref_sel"], *FC.DEFAULT)
    assert e.value.status == _lib.GCI_E_NO_NM and e.value.rec == 1


@pytest.mark.parametrize("form", ["stream", "heads"])
@pytest.mark.parametrize("name, run", FC.depth_pairs())
def test_the_selected_cover_gives_the_depth_of_every_class(twin, name, run, form):
    c = FC.case(name)
    stream, offs = form_of(name, form)
    twin.set_layout(c["lengths"])
    cls = FC.want(name, run)[0]
    n_ivl = 0
    for k in range(1, _lib.FATE_CLASSES):              # (`none` is never counted: the callers keep 0x4 among the excluded flags)
        for count_del in (False, True):
            ivl = twin.bam_cover(stream, offs, c["ref_sel"], form == "stream", 0, 0, count_del, check=False, classes=cls, mask=1 << k)
            track = twin.depth_build(ivl, 0)
            for j, w in enumerate(FC.want_depth(name, run, k, count_del)):
                assert np.array_equal(twin.contig(track, j).astype(np.int64), w), (k, count_del, j)
        n_ivl += ivl.shape[0]
    # all classes at once: the same intervals as one class after another, and as the call without classes
    every = twin.bam_cover(stream, offs, c["ref_sel"], form == "stream", 0x4, 0, True, check=False, classes=cls, mask=0xFE)
    plain = twin.bam_cover(stream, offs, c["ref_sel"], form == "stream", 0x4, 0, True, check=False)
    assert every.shape[0] == plain.shape[0] == n_ivl and np.array_equal(np.sort(every, order=list(every.dtype.names)), np.sort(plain, order=list(plain.dtype.names)))
    none = twin.bam_cover(stream, offs, c["ref_sel"], form == "stream", 0, 0, True, check=False, classes=cls, mask=0)
    assert none.shape[0] == 0


def test_cover_size_sel_without_classes_is_cover_size(twin):
    lib = twin.lib
    p = lambda a: ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    for name, run in C.pairs():
        c = C.case(name)
        twin.set_layout(c["lengths"])
        stream, offs, sel = c["stream"], c["offs"], c["ref_sel"]
        want = twin.bam_cover(stream, offs, sel, True, *run, check=False)
        want_status = int(twin.last_status[0])
        n, st = ctypes.c_uint64(0), np.zeros(1, dtype=np.uint64)
        junk = np.full(max(offs.shape[0], 1), 9, dtype=np.uint8)
        for d_class, mask in ((None, 0), (None, 0xFFFFFFFF)):
            assert lib.gci_bam_cover_size_sel(twin.ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1, p(sel), sel.shape[0], run[0], run[1],
                                              int(run[2]), d_class, mask, ctypes.byref(n), p(st)) == 0
            assert n.value == want.shape[0] and int(st[0]) == want_status
            out = np.zeros(max(int(n.value), 1), dtype=cpu.IVL_DTYPE)
            assert lib.gci_bam_cover_write(twin.ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1, p(out), n.value, p(st)) == 0
            assert np.array_equal(np.sort(out[:n.value], order=list(out.dtype.names)), np.sort(want, order=list(want.dtype.names)))
        # a class beyond the mask's 32 bits selects nothing
        assert lib.gci_bam_cover_size_sel(twin.ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1, p(sel), sel.shape[0], run[0], run[1],
                                          int(run[2]), p(junk.astype(np.uint8) + 31), 0xFFFFFFFF, ctypes.byref(n), p(st)) == 0
        assert n.value == 0


def test_argument_errors(twin):
    lib, c = twin.lib, FC.case("one_per_class")
    stream, offs, sel = c["stream"], c["offs"], c["ref_sel"]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    cls, counts, st, n = np.zeros(offs.shape[0], np.uint8), np.zeros(8, np.uint64), np.zeros(1, np.uint64), ctypes.c_uint64(0)
    fate = lambda ctx, d_class=p(cls), h_counts=p(counts), status=p(st), off=p(offs): lib.gci_bam_fate(   # noqa: E731
        ctx, p(stream), stream.shape[0], off, offs.shape[0], 1, p(sel), sel.shape[0], 30, 0.1, 0.9, d_class, h_counts, status)
    size = lambda ctx, n_out=ctypes.byref(n), status=p(st): lib.gci_bam_cover_size_sel(                    # noqa: E731
        ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1, p(sel), sel.shape[0], 0, 0, 0, p(cls), 1 << F.KEPT, n_out, status)
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT
    assert fate(fresh.ctx) == 0 and counts.tolist() == FC.want("one_per_class", FC.DEFAULT)[1].tolist()        # the classes need no layout
    assert fate(None) == _lib.GCI_E_INVALID and size(None) == _lib.GCI_E_INVALID
    for kw in (dict(d_class=None), dict(h_counts=None), dict(status=None), dict(off=None)):
        assert fate(fresh.ctx, **kw) == _lib.GCI_E_INVALID, kw
    fresh.set_layout(c["lengths"])
    assert size(fresh.ctx, n_out=None) == _lib.GCI_E_INVALID and size(fresh.ctx, status=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and n.value == 2


# ---- the command line's error messages (none of them reaches the device) -------------------------------------------------------------

def filter_depth(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "filter_depth.py")] + list(argv), capture_output=True, text=True,
                          env=dict(os.environ, GCI_EARLY_HIP="0"), timeout=120)


def test_cli_error_messages(tmp_path):
    ok = str(tmp_path / "a.bam")
    bamfmt.write_bam(ok, ["c1", "c2"], [100, 50], [C.rec(0, 3, [(C.M, 5)], aux=FC.nm(0))])
    r = filter_depth()
    assert r.returncode != 0 and r.stderr.strip() == "ERROR!!! No BAM file given"
    r = filter_depth(str(tmp_path / "missing.bam"))
    assert r.returncode != 0 and r.stderr.startswith('ERROR!!! The file "%s" cannot be read as a BAM file' % (tmp_path / "missing.bam"))
    r = filter_depth("--chrs", "c1,nope", ok)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The chromosome "nope" of --chrs is not in the header of "%s"' % ok
    r = filter_depth("--classes", "kept,clipped", ok)
    assert r.returncode != 0 and r.stderr.strip() == ('ERROR!!! The class "clipped" of --classes is not one of '
                                                      "secondary, supplementary, mapq, clip, identity, kept")
    for leftover in ("GCI_fate.mapq.depth.gz", "GCI_fate.filter.txt"):
        (tmp_path / leftover).write_bytes(b"")
        r = filter_depth("-d", str(tmp_path), ok)
        assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The file "%s/%s" exists\nPlease use "-f" or "--force" to rewrite' % (tmp_path, leftover)
        (tmp_path / leftover).unlink()
    other = str(tmp_path / "b.bam")
    bamfmt.write_bam(other, ["c1", "c2"], [100, 51], [])
    r = filter_depth("-d", str(tmp_path), ok, other)
    assert r.returncode != 0 and r.stderr.strip() == 'ERROR!!! The @SQ table of "%s" differs from that of "%s"' % (other, ok)
    assert "Traceback" not in r.stderr
    h = filter_depth("-h").stdout
    assert "0x700" in h and "GCI.py" in h
