"""allele_sites.py off the GPU: the CPU twins of gci_bam_allele_size / _write and gci_allele_sites_size / _write
(gci_amd/csrc/cpu/gci_cpu.cpp) against the statement of tests/allele_ref.py on every case of tests/allele_cases.py, into pre-filled
buffers with guard entries; the argument checks; the VCF, BED and summary texts; the command line's refusals; the twins chained over a
synthetic file."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import allele_cases as C
import allele_ref as R
import mismatch_cases as MC
from gci_amd import _lib, allelesites_cli, bedgraph_cli, cpu, pipeline, synth
from gci_amd.formats import bam as bamfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    return cpu.CpuEngine(threads=4)


def events_of(ivl):
    assert (ivl["start"] == ivl["end"]).all() and (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist()))


@pytest.mark.parametrize("name", C.NAMES)
def test_the_twin_gives_the_lists_of_the_statement(twin, name):
    c = C.case(name)
    twin.set_layout(c["lengths"])
    for run in c["runs"]:
        want_lists, want_counts, want_status = C.want(name, run)
        *lists, counts = twin.bam_allele(c["stream"], c["offs"], c["ref_sel"], c["codes"], True, *run, check=False, guard=16)
        assert int(twin.last_status[0]) == want_status, run
        assert counts == want_counts and [events_of(x) for x in lists] == want_lists, run
        for ivl, want in zip(lists, want_lists):                                    # flank 0 over list X gives track X
            assert np.array_equal(twin.depth_build(np.ascontiguousarray(ivl), 0), R.track_of(want, c["lengths"]))


def test_the_twin_gives_the_hand_written_lists(twin):
    for (name, run), want in C.EXPECTED.items():
        c = C.case(name)
        twin.set_layout(c["lengths"])
        *lists, counts = twin.bam_allele(c["stream"], c["offs"], c["ref_sel"], c["codes"], True, *run, check=False)
        assert tuple(events_of(x) for x in lists) == want, (name, run)
        assert counts[1:5] == [len(x) for x in want]


def test_a_malformed_record_raises_with_its_index(twin):
    for name, rec in C.MALFORMED.items():
        c = C.case(name)
        twin.set_layout(c["lengths"])
        with pytest.raises(cpu.CpuError) as e:
            twin.bam_allele(c["stream"], c["offs"], c["ref_sel"], c["codes"])
        assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == rec, name


@pytest.mark.parametrize("name", C.SITE_NAMES)
def test_the_twin_gives_the_sites_of_the_statement(twin, name):
    c = C.site_case(name)
    twin.set_layout(c["lengths"])
    assert twin.total == c["depth"].shape[0]
    for k, (min_reads, frac, windows) in enumerate(c["runs"]):
        got = twin.allele_sites(*(c[key] for key in C.SITE_KEYS), min_reads, frac, windows)
        assert C.site_rows(got) == C.want_sites(name, k), k
        if (name, k) in C.SITES_EXPECTED:
            assert C.site_rows(got) == C.SITES_EXPECTED[(name, k)], k


def test_argument_errors_of_the_record_calls(twin):
    lib, c = twin.lib, C.case("phases")
    stream, offs, sel, codes = c["stream"], c["offs"], c["ref_sel"], c["codes"]
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    counts, st = np.zeros(6, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    out = np.zeros(64, dtype=cpu.IVL_DTYPE)
    size = lambda ctx, has_seq=1, cd=codes, h_counts=counts, status=st: lib.gci_bam_allele_size(      # noqa: E731
        ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], has_seq, p(sel), sel.shape[0], 0x704, 0, p(cd), p(h_counts), p(status))
    write = lambda ctx, cap, n_rec=offs.shape[0], cd=codes: lib.gci_bam_allele_write(ctx, p(stream), stream.shape[0], p(offs), n_rec, 1,     # noqa: E731
                                                                                     p(cd), p(out), cap, p(st))
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 64) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 64) == _lib.GCI_E_INVALID                           # no size call in front of it
    assert size(None) == _lib.GCI_E_INVALID and size(fresh.ctx, has_seq=0) == _lib.GCI_E_INVALID and size(fresh.ctx, cd=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, h_counts=None) == _lib.GCI_E_INVALID and size(fresh.ctx, status=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and counts.tolist() == [5, 0, 3, 0, 2, 24]
    assert write(fresh.ctx, 64, n_rec=offs.shape[0] - 1) == _lib.GCI_E_INVALID   # not the input the size call measured
    assert write(fresh.ctx, 64, cd=codes.copy()) == _lib.GCI_E_INVALID
    out[:] = (7, 7, 7, 7)
    assert write(fresh.ctx, 4) == _lib.GCI_E_CAPACITY
    assert (out["contig"] == 7).all()                                            # ... and nothing was written
    assert write(fresh.ctx, 5) == 0 and (out["contig"][:5] == 0).all() and (out["contig"][5:] == 7).all()
    assert out["start"][:5].tolist() == [4, 6, 0, 4, 14]                         # the C list, then the T list
    # the mismatch pair keeps its own memo: a mismatch size call between the two ends nothing
    mm = np.zeros(3, dtype=np.uint64)
    assert size(fresh.ctx) == 0
    assert lib.gci_bam_mismatch_size(fresh.ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], 1, p(sel), sel.shape[0], 0x704, 0, p(codes), p(mm),
                                     p(st)) == 0
    assert write(fresh.ctx, 5) == 0 and int(mm[1]) == int(counts[1:5].sum())


def test_argument_errors_of_the_site_calls(twin):
    lib, c = twin.lib, C.site_case("random")
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    n = ctypes.c_uint64(0)
    out = np.full((8192, 9), 7, dtype=np.int32)
    win = (_lib.Window * 2)()
    win[0].begin, win[0].end, win[1].begin, win[1].end = 0, 5000, 4999, 6000
    arrays = {k: c[k] for k in C.SITE_KEYS}

    def size(ctx, m=3, f=500000, w=None, nw=0, h_n=ctypes.byref(n), **other):
        t = dict(arrays, **other)
        return lib.gci_allele_sites_size(ctx, *(p(t[k]) for k in C.SITE_KEYS), m, f, w, nw, h_n)

    def write(ctx, cap, m=3, f=500000, **other):
        t = dict(arrays, **other)
        return lib.gci_allele_sites_write(ctx, *(p(t[k]) for k in C.SITE_KEYS), m, f, None, 0, p(out), cap)
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 8192) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 8192) == _lib.GCI_E_INVALID                          # no size call in front of it
    assert size(None) == _lib.GCI_E_INVALID and size(fresh.ctx, m=0) == _lib.GCI_E_INVALID and size(fresh.ctx, h_n=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, f=-1) == _lib.GCI_E_INVALID and size(fresh.ctx, f=1000001) == _lib.GCI_E_INVALID and size(fresh.ctx, nw=2) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, w=win, nw=2) == _lib.GCI_E_INVALID                    # windows that overlap
    raw = np.zeros(c["depth"].shape[0] + 8, dtype=np.int32)                      # a track that begins one element in: not 16-byte aligned
    k = next(i for i in range(1, 5) if (raw.ctypes.data + 4 * i) % 16)
    for which in C.SITE_KEYS:
        assert size(fresh.ctx, **{which: None}) == _lib.GCI_E_INVALID, which
        if which != "codes":
            assert size(fresh.ctx, **{which: raw[k:k + c["depth"].shape[0]]}) == _lib.GCI_E_INVALID, which
    assert size(fresh.ctx) == 0 and n.value == len(C.want_sites("random", 1)) > 4
    assert write(fresh.ctx, 8192, m=4) == _lib.GCI_E_INVALID and write(fresh.ctx, 8192, f=500001) == _lib.GCI_E_INVALID      # not what was measured
    assert write(fresh.ctx, 8192, t=c["t"].copy()) == _lib.GCI_E_INVALID and write(fresh.ctx, 8192, codes=c["codes"].copy()) == _lib.GCI_E_INVALID
    assert write(fresh.ctx, n.value - 1) == _lib.GCI_E_CAPACITY
    assert (out == 7).all()                                                      # ... and nothing was written
    assert write(fresh.ctx, n.value) == 0 and (out[:n.value, 0] >= 0).all() and (out[n.value:] == 7).all()


# ---- the host side ---------------------------------------------------------------------------------------------------------------------

SITES = np.array([(0, 5, 2, 8, (0, 1, 0, 7), 9), (2, 0, 15, 1, (3, 3, 0, 0), 3)], dtype=cpu.ALLELE_SITE_DTYPE)
TARGETS = {"chr1": 100, "chr2": 50, "scaffold_3": 7}


def test_the_defaults_and_the_dtype():
    assert pipeline.ALLELE_MIN_READS == 3 and pipeline.parse_fraction_ppm(pipeline.ALLELE_MIN_FRAC) == 500000
    assert cpu.ALLELE_SITE_DTYPE.itemsize == 36 and cpu.ALLELE_SITE_DTYPE == pipeline.ALLELE_SITE_DTYPE
    assert pipeline._AlleleVisitor.TRACKS == ("A", "C", "G", "T", "depth") and pipeline._AlleleVisitor.NEED_SEQ
    assert issubclass(pipeline._AlleleVisitor, pipeline._ClipVisitor)


def test_the_vcf_text():
    text = pipeline.allele_sites_vcf(SITES, TARGETS, "dir/ref.fa")
    assert text == ("##fileformat=VCFv4.2\n##source=allele_sites.py\n##reference=dir/ref.fa\n"
                    "##contig=<ID=chr1,length=100>\n##contig=<ID=chr2,length=50>\n##contig=<ID=scaffold_3,length=7>\n"
                    '##INFO=<ID=DP,Number=1,Type=Integer,Description="Read-mapping depth at the base, as bam_depth.py counts it">\n'
                    '##INFO=<ID=AO,Number=1,Type=Integer,Description="Counted records that carry ALT at the base">\n'
                    '##INFO=<ID=BC,Number=4,Type=Integer,Description="Counted records that carry A, C, G, T at the base where the assembly holds another">\n'
                    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                    "chr1\t6\t.\tC\tT\t.\t.\tDP=9;AO=7;BC=0,1,0,7\n"
                    "scaffold_3\t1\t.\tN\tA\t.\t.\tDP=3;AO=3;BC=3,3,0,0\n")
    head = pipeline.allele_sites_vcf(SITES[:0], TARGETS, "r.fa")
    assert head.endswith("\tINFO\n") and head.count("\n") == 10


def test_the_bed_text_reads_back_as_regions(tmp_path):
    text = pipeline.allele_sites_bed(SITES, list(TARGETS))
    assert text == "chr1\t5\t6\tC\tT\t7\t9\nscaffold_3\t0\t1\tN\tA\t3\t3\n"
    (tmp_path / "s.bed").write_text(text)
    assert [tuple(r[:3]) for r in bedgraph_cli.parse_regions(str(tmp_path / "s.bed"))] == [("chr1", 5, 6), ("scaffold_3", 0, 1)]
    assert pipeline.allele_sites_bed(SITES[:0], ["chr1"]) == ""


def test_the_summary_text():
    text = pipeline.allele_summary_text(["a.bam", "dir/b.bam"], [[10, 1, 2, 3, 4, 100], [5, 0, 0, 0, 0, 0]], 4, [("min_reads", 3), ("min_frac_ppm", 500000)])
    assert text == ("#file\trecords\tcompared\tA\tC\tG\tT\tpath\n1\t10\t100\t1\t2\t3\t4\ta.bam\n2\t5\t0\t0\t0\t0\t0\tdir/b.bam\n"
                    "total\t15\t100\t1\t2\t3\t4\t.\nsites\t4\nmin_reads\t3\nmin_frac_ppm\t500000\n")


@pytest.mark.parametrize("kind,sub_rate", [("hifi", 0.0), ("hifi", 0.02), ("ont", 0.04)])
def test_the_twins_chained_over_a_synthetic_file(twin, tmp_path, kind, sub_rate):
    """What pipeline.bam_allele_sites does behind the ingestion, on the twins: a seeded random assembly as FASTA, seeded synthetic reads
    that carry its bases with a seeded share of substituted ones, then codes (pipeline.reference_codes), the four lists, the five
    tracks and the sites, each against the statement; the four tracks add up to the mismatch twin's track; a substituted base is one
    of the four at random, so the four classes share the events about evenly."""
    contigs = (("ctgA", 90_000), ("ctgB", 50_000))
    lengths = [l for _, l in contigs]
    ref = synth.random_reference(contigs + (("extra", 3000),), seed=3)
    fa = str(tmp_path / "ref.fa")
    synth.write_fasta(fa, {k: ref[k] for k in ("ctgB", "extra", "ctgA")}, width=61)
    rs = synth.simulate_reads(contigs, 4, kind, seed=42).sorted()
    stream, offs = synth.to_bam_stream(rs, seq_qual="reference", reference=ref, sub_rate=sub_rate, seed=9)
    twin.set_layout(lengths)
    codes = pipeline.reference_codes(twin, fa, dict(contigs))
    sel = np.arange(len(contigs), dtype=np.int32)
    want_lists, want_counts, status = R.stream_events(stream, offs, lengths, sel, codes)
    assert status == R.NO_STATUS
    *lists, counts = twin.bam_allele(stream, offs, sel, codes, guard=16)
    assert counts == want_counts and [events_of(x) for x in lists] == want_lists
    mm_ivl, mm_counts = twin.bam_mismatch(stream, offs, sel, codes)
    assert [counts[0], sum(counts[1:5]), counts[5]] == mm_counts and counts[5] > 200_000
    if sub_rate == 0.0:
        assert counts[1:5] == [0, 0, 0, 0]
    else:
        # each class gets a quarter of the events (3 of 4 substitutions differ, each read base equally often): six standard deviations
        n = sum(counts[1:5])
        assert all(abs(x - n / 4) < 6 * (n * 0.25 * 0.75) ** 0.5 for x in counts[1:5]), counts
    tracks = [twin.depth_build(np.ascontiguousarray(x), 0) for x in lists]
    depth = twin.depth_build(twin.bam_cover(stream, offs, sel), 0)
    for got, want in zip(tracks, want_lists):
        assert np.array_equal(got, R.track_of(want, lengths))
    assert np.array_equal(sum(tracks), twin.depth_build(np.ascontiguousarray(mm_ivl), 0)) and (sum(tracks) <= depth).all()
    for min_reads, frac in ((1, 0), (2, 500000), (3, 1000000)):
        got = twin.allele_sites(*tracks, depth, codes, min_reads, frac)
        assert C.site_rows(got) == R.sites_of(*tracks, depth, codes, lengths, min_reads, frac), (min_reads, frac)
        assert all(r[2] != r[3] for r in C.site_rows(got))                       # the listed allele is never the assembly's base


def test_need_seq_refuses_the_heads_ingest(monkeypatch):
    monkeypatch.setenv("GCI_BAM_INGEST", "heads")
    with pytest.raises(pipeline.SeqNeeded):
        pipeline.bam_allele_sites(None, "ref.fa", ["a.bam"])
    with pytest.raises(ValueError):
        pipeline.bam_allele_sites(None, "ref.fa", ["a.bam"], min_reads=0)
    with pytest.raises(ValueError):
        pipeline.bam_allele_sites(None, "ref.fa", ["a.bam"], min_frac="1.5")


def _cli(tmp_path, *argv, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "allele_sites.py"), *argv], capture_output=True, text=True, cwd=str(tmp_path), env=e)


def test_the_command_line_refuses_before_it_touches_the_device(tmp_path):
    c = MC.case("phases")
    bam = str(tmp_path / "a.bam")
    bamfmt.write_bam_stream(bam, c["stream"])
    ref = str(tmp_path / "ref.fa")
    (tmp_path / "ref.fa").write_bytes(c["fasta"])
    r = _cli(tmp_path, bam)
    assert r.returncode == 2 and "-r/--reference" in r.stderr                    # a usage error
    for frac in ("1.5", "0.1234567", "half"):
        r = _cli(tmp_path, "-r", ref, "-F", frac, bam)
        assert r.returncode == 2 and "-F/--min-frac" in r.stderr, frac
    r = _cli(tmp_path, "-r", ref, "-n", "0", bam)
    assert r.returncode == 1 and "ERROR!!! -n/--min-reads 0 is not at least 1" in r.stderr
    r = _cli(tmp_path, "-r", ref)
    assert r.returncode == 1 and "ERROR!!! No BAM file given" in r.stderr
    r = _cli(tmp_path, "-r", ref, bam, env={"GCI_BAM_INGEST": "heads"})
    assert r.returncode == 1 and "GCI_BAM_INGEST=heads" in r.stderr
    r = _cli(tmp_path, "-r", str(tmp_path / "none.fa"), bam)
    assert r.returncode == 1 and "none.fa\" does not exist" in r.stderr
    (tmp_path / "GCI_allele.allele.sites.vcf").write_text("x")
    r = _cli(tmp_path, "-r", ref, bam)
    assert r.returncode == 1 and "GCI_allele.allele.sites.vcf" in r.stderr and (tmp_path / "GCI_allele.allele.sites.vcf").read_text() == "x"


def test_the_parser_takes_the_sibling_tools_options():
    args = allelesites_cli.build_parser("allele_sites.py").parse_args(["-r", "ref.fa", "-Q", "5", "-G", "0x800", "-J", "-n", "4", "-F", "0.25", "a.bam", "b.bam"])
    assert (args.reference, args.min_mapq, args.excl_add, args.count_del, args.min_reads, args.min_frac, args.bams) == \
        ("ref.fa", 5, 0x800, True, 4, "0.25", ["a.bam", "b.bam"])
    assert allelesites_cli.outputs(allelesites_cli.build_parser("x").parse_args(["-r", "r.fa", "-d", "o", "-o", "p"])) == \
        ["o/p.allele.A.depth.gz", "o/p.allele.C.depth.gz", "o/p.allele.G.depth.gz", "o/p.allele.T.depth.gz", "o/p.allele.sites.vcf",
         "o/p.allele.sites.bed", "o/p.allele.txt"]
