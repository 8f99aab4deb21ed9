"""mismatch_sites.py off the GPU: the CPU twins of gci_fasta_codes, gci_bam_mismatch_size / _write and gci_mismatch_sites_size / _write
(gci_amd/csrc/cpu/gci_cpu.cpp) against the statement of tests/mismatch_ref.py on every case of tests/mismatch_cases.py, into pre-filled
buffers with guard entries; the argument checks; -F's parse; the BED and summary texts; the FASTA / @SQ checks; need_seq."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mismatch_cases as C
import mismatch_ref as R
from gci_amd import _lib, bedgraph_cli, cpu, mismatchsites_cli, pipeline, synth
from gci_amd.formats import bam as bamfmt, fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("contig", "start", "end", "mismatch", "depth")


@pytest.fixture(scope="module")
def twin():
    return cpu.CpuEngine(threads=4)


def events_of(ivl):
    assert (ivl["start"] == ivl["end"]).all() and (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist()))


@pytest.mark.parametrize("name", C.NAMES)
def test_the_twin_gives_the_events_of_the_statement(twin, name):
    c = C.case(name)
    twin.set_layout(c["lengths"])
    for run in c["runs"]:
        want_events, want_counts, want_status = C.want(name, run)
        ivl, counts = twin.bam_mismatch(c["stream"], c["offs"], c["ref_sel"], c["codes"], True, *run, check=False, guard=16)
        assert int(twin.last_status[0]) == want_status, run
        assert counts == want_counts and events_of(ivl) == want_events, run
        assert np.array_equal(twin.depth_build(np.ascontiguousarray(ivl), 0), R.track_of(want_events, c["lengths"]))


def test_the_twin_gives_the_hand_written_events(twin):
    for (name, run), (events, counts) in C.EXPECTED.items():
        c = C.case(name)
        twin.set_layout(c["lengths"])
        ivl, got = twin.bam_mismatch(c["stream"], c["offs"], c["ref_sel"], c["codes"], True, *run, check=False)
        assert (events_of(ivl), got) == (events, counts), (name, run)


def test_a_malformed_record_raises_with_its_index(twin):
    for name, rec in C.MALFORMED.items():
        c = C.case(name)
        twin.set_layout(c["lengths"])
        with pytest.raises(cpu.CpuError) as e:
            twin.bam_mismatch(c["stream"], c["offs"], c["ref_sel"], c["codes"])
        assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == rec, name


@pytest.mark.parametrize("name", C.FASTA_NAMES)
def test_the_twin_gives_the_codes_of_the_statement(twin, name):
    c = C.fasta_case(name)
    twin.set_layout(c["lengths"])
    assert twin.total == c["total"]
    codes = np.full(c["total"], C.FILL, dtype=np.uint8)
    twin.fasta_codes(c["text"], c["bodies"], c["dst"], codes)
    assert np.array_equal(codes, C.want_codes(name))


def test_the_cases_code_arrays_are_the_twins(twin):
    c = C.case("letters")
    twin.set_layout(c["lengths"])
    text = np.frombuffer(c["fasta"], dtype=np.uint8)
    spans = fasta.record_spans(text)
    assert [s[1:] for s in spans] == [s[1:] for s in R.fasta_records(c["fasta"])]       # the product's title lines are the statement's
    codes = np.full(twin.total, 15, dtype=np.uint8)
    twin.fasta_codes(text, np.array([s[1:] for s in spans], dtype=np.int64), twin.offsets, codes)
    assert np.array_equal(codes, c["codes"])


@pytest.mark.parametrize("name", C.SITE_NAMES)
def test_the_twin_gives_the_sites_of_the_statement(twin, name):
    c = C.site_case(name)
    twin.set_layout(c["lengths"])
    assert twin.total == c["mism"].shape[0]
    for k, (min_reads, frac, windows) in enumerate(c["runs"]):
        got = twin.mismatch_sites(c["mism"], c["depth"], min_reads, frac, windows)
        assert list(zip(*(got[f].tolist() for f in FIELDS))) == C.want_sites(name, k), k


def test_argument_errors_of_the_record_calls(twin):
    lib, c = twin.lib, C.case("phases")
    stream, offs, sel, codes = c["stream"], c["offs"], c["ref_sel"], c["codes"]
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    counts, st = np.zeros(3, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    out = np.zeros(64, dtype=cpu.IVL_DTYPE)
    size = lambda ctx, has_seq=1, cd=codes, h_counts=counts, status=st: lib.gci_bam_mismatch_size(      # noqa: E731
        ctx, p(stream), stream.shape[0], p(offs), offs.shape[0], has_seq, p(sel), sel.shape[0], 0x704, 0, p(cd), p(h_counts), p(status))
    write = lambda ctx, cap, n_rec=offs.shape[0], cd=codes: lib.gci_bam_mismatch_write(ctx, p(stream), stream.shape[0], p(offs), n_rec, 1,     # noqa: E731
                                                                                       p(cd), p(out), cap, p(st))
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 64) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 64) == _lib.GCI_E_INVALID                           # no size call in front of it
    assert size(None) == _lib.GCI_E_INVALID and size(fresh.ctx, has_seq=0) == _lib.GCI_E_INVALID and size(fresh.ctx, cd=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, h_counts=None) == _lib.GCI_E_INVALID and size(fresh.ctx, status=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and counts.tolist() == [5, 5, 24]
    assert write(fresh.ctx, 64, n_rec=offs.shape[0] - 1) == _lib.GCI_E_INVALID   # not the input the size call measured
    assert write(fresh.ctx, 64, cd=codes.copy()) == _lib.GCI_E_INVALID
    out[:] = (7, 7, 7, 7)
    assert write(fresh.ctx, 4) == _lib.GCI_E_CAPACITY
    assert (out["contig"] == 7).all()                                            # ... and nothing was written
    assert write(fresh.ctx, 5) == 0 and (out["contig"][:5] == 0).all() and (out["contig"][5:] == 7).all()


def test_argument_errors_of_the_site_calls(twin):
    lib, c = twin.lib, C.site_case("random")
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)             # noqa: E731
    n = ctypes.c_uint64(0)
    out = np.full((8192, 5), 7, dtype=np.int32)
    win = (_lib.Window * 2)()
    win[0].begin, win[0].end, win[1].begin, win[1].end = 0, 5000, 4999, 6000
    mism, depth = c["mism"], c["depth"]
    size = lambda ctx, t=mism, d=depth, m=3, f=500000, w=None, nw=0, h_n=ctypes.byref(n): lib.gci_mismatch_sites_size(ctx, p(t), p(d), m, f, w, nw, h_n)   # noqa: E731
    write = lambda ctx, cap, m=3, f=500000: lib.gci_mismatch_sites_write(ctx, p(mism), p(depth), m, f, None, 0, p(out), cap)      # noqa: E731
    fresh = cpu.CpuEngine(threads=1)
    assert size(fresh.ctx) == _lib.GCI_E_NO_LAYOUT and write(fresh.ctx, 8192) == _lib.GCI_E_NO_LAYOUT
    fresh.set_layout(c["lengths"])
    assert write(fresh.ctx, 8192) == _lib.GCI_E_INVALID                          # no size call in front of it
    assert size(None) == _lib.GCI_E_INVALID and size(fresh.ctx, m=0) == _lib.GCI_E_INVALID and size(fresh.ctx, h_n=None) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, f=-1) == _lib.GCI_E_INVALID and size(fresh.ctx, f=1000001) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, t=None) == _lib.GCI_E_INVALID and size(fresh.ctx, d=None) == _lib.GCI_E_INVALID and size(fresh.ctx, nw=2) == _lib.GCI_E_INVALID
    assert size(fresh.ctx, w=win, nw=2) == _lib.GCI_E_INVALID                    # windows that overlap
    raw = np.zeros(mism.shape[0] + 8, dtype=np.int32)                            # a track that begins one element in: not 16-byte aligned
    k = next(i for i in range(1, 5) if (raw.ctypes.data + 4 * i) % 16)
    for which in "td":
        assert size(fresh.ctx, **{which: raw[k:k + mism.shape[0]]}) == _lib.GCI_E_INVALID
    assert size(fresh.ctx) == 0 and n.value == len(C.want_sites("random", 1)) > 4
    assert write(fresh.ctx, 8192, m=4) == _lib.GCI_E_INVALID and write(fresh.ctx, 8192, f=500001) == _lib.GCI_E_INVALID      # not what was measured
    assert write(fresh.ctx, n.value - 1) == _lib.GCI_E_CAPACITY
    assert (out == 7).all()                                                      # ... and nothing was written
    assert write(fresh.ctx, n.value) == 0 and (out[:n.value, 0] >= 0).all() and (out[n.value:] == 7).all()


# ---- the host side ---------------------------------------------------------------------------------------------------------------------

def test_the_fraction_is_read_from_its_text():
    ok = {"0.5": 500000, "0": 0, "1": 1000000, "1.0": 1000000, "1.000000": 1000000, "0.000001": 1, ".25": 250000, "0.123456": 123456, "0.": 0,
          "0.30": 300000, " 0.7 ": 700000}
    for text, ppm in ok.items():
        assert pipeline.parse_fraction_ppm(text) == ppm, text
    for text in ("", ".", "1.000001", "2", "-0.1", "0.1234567", "1e-3", "0,5", "abc", "0.5x", "+0.5"):
        with pytest.raises(ValueError):
            pipeline.parse_fraction_ppm(text)
    assert pipeline.parse_fraction_ppm(pipeline.MISMATCH_MIN_FRAC) == 500000 and pipeline.MISMATCH_MIN_READS == 3


def test_the_bed_text_reads_back_as_regions(tmp_path):
    sites = np.array([(0, 5, 9, 7, 20), (2, 0, 1, 3, 3)], dtype=cpu.MISMATCH_SITE_DTYPE)
    text = pipeline.mismatch_sites_bed(sites, ["chr1", "chr2", "scaffold_3"])
    assert text == "chr1\t5\t9\t7\t20\nscaffold_3\t0\t1\t3\t3\n"
    (tmp_path / "s.bed").write_text(text)
    assert [tuple(r[:3]) for r in bedgraph_cli.parse_regions(str(tmp_path / "s.bed"))] == [("chr1", 5, 9), ("scaffold_3", 0, 1)]
    assert pipeline.mismatch_sites_bed(sites[:0], ["chr1"]) == ""


def test_the_summary_text():
    text = pipeline.mismatch_summary_text(["a.bam", "dir/b.bam"], [[10, 2, 100], [5, 0, 0]], 4, [("min_reads", 3), ("min_frac_ppm", 500000)])
    assert text == ("#file\trecords\tcompared\tmismatches\trate\tpath\n1\t10\t100\t2\t0.020000\ta.bam\n2\t5\t0\t0\tnan\tdir/b.bam\n"
                    "total\t15\t100\t2\t0.020000\t.\nsites\t4\nmin_reads\t3\nmin_frac_ppm\t500000\n")


def _fa(tmp_path, name, records):
    path = str(tmp_path / name)
    fasta.write(path, records, width=7)
    return path


def test_the_assembly_is_checked_against_the_sq_table(twin, tmp_path):
    """reference_codes over the twin: the ids are matched by name; an id twice, a missing contig and another length are refused."""
    targets = {"b": 10, "a": 5}
    twin.set_layout(list(targets.values()))
    good = _fa(tmp_path, "good.fa", [("a", b"ACGTA"), ("extra", b"GGGGGGGGGGGG"), ("b", b"ACGTACGTNN")])
    codes = pipeline.reference_codes(twin, good, targets)
    assert codes[:10].tolist() == [1, 2, 4, 8, 1, 2, 4, 8, 15, 15] and codes[4096:4101].tolist() == [1, 2, 4, 8, 1] and (codes[10:4096] == 15).all()
    for name, records, word in (("twice.fa", [("a", b"ACGTA"), ("b", b"ACGTACGTNN"), ("a", b"ACGTA")], "twice"),
                                ("missing.fa", [("a", b"ACGTA"), ("c", b"ACGTACGTNN")], "`b` is not in"),
                                ("short.fa", [("a", b"ACGTA"), ("b", b"ACGTACGTN")], "`b` has 9 bases"),
                                ("long.fa", [("a", b"ACGTAC"), ("b", b"ACGTACGTNN")], "`a` has 6 bases")):
        with pytest.raises(pipeline.ReferenceMismatch, match=word):
            pipeline.reference_codes(twin, _fa(tmp_path, name, records), targets)
    assert issubclass(pipeline.ReferenceMismatch, ValueError)
    # the lengths are checked between the tile counts and the codes: a refusal there leaves the array as it was
    buf, spans = fasta.indexed(_fa(tmp_path, "long2.fa", [("a", b"ACGTAC"), ("b", b"ACGTACGTNN")]))
    bodies = np.array([s[1:] for s in spans], dtype=np.int64)
    codes, seen = np.full(twin.total, C.FILL, dtype=np.uint8), []

    def refuse(kept):
        seen.append(fasta.body_lengths(buf, bodies, kept))
        raise pipeline.ReferenceMismatch("too long")
    with pytest.raises(pipeline.ReferenceMismatch):
        twin.fasta_codes(buf, bodies, np.array([4096, 0], dtype=np.int64), codes, before_codes=refuse)
    assert seen == [[6, 10]] and (codes == C.FILL).all()


@pytest.mark.parametrize("kind,sub_rate", [("hifi", 0.0), ("hifi", 0.02), ("ont", 0.04)])
def test_the_twins_chained_over_a_synthetic_file(twin, tmp_path, kind, sub_rate):
    """What pipeline.bam_mismatch_sites does behind the ingestion, on the twins: a seeded random assembly as FASTA (its records in another
    order than @SQ, one extra), seeded synthetic reads that carry its bases with a seeded share of substituted ones, then codes
    (pipeline.reference_codes), events, the two tracks and the sites, each against the statement; mismatch <= depth; the share of
    mismatches is the substituted share that lands on another base (3 of 4)."""
    contigs = (("ctgA", 90_000), ("ctgB", 50_000))
    lengths = [l for _, l in contigs]
    ref = synth.random_reference(contigs + (("extra", 3000),), seed=3)
    fa = str(tmp_path / "ref.fa")
    synth.write_fasta(fa, {k: ref[k] for k in ("ctgB", "extra", "ctgA")}, width=61)
    rs = synth.simulate_reads(contigs, 4, kind, seed=42).sorted()
    stream, offs = synth.to_bam_stream(rs, seq_qual="reference", reference=ref, sub_rate=sub_rate, seed=9)
    plain, plain_offs = synth.to_bam_stream(rs)                                  # the default output: the same bytes but SEQ
    assert plain.shape == stream.shape and np.array_equal(plain_offs, offs) and np.array_equal(plain[:int(offs[0])], stream[:int(offs[0])])
    again, _ = synth.to_bam_stream(rs, seq_qual="reference", reference=ref, sub_rate=sub_rate, seed=9)
    assert np.array_equal(again, stream)                                         # seeded
    twin.set_layout(lengths)
    layout_offs, total = R.layout(lengths)
    want_codes = np.full(total, 15, dtype=np.uint8)
    for (name, L), o in zip(contigs, layout_offs):
        want_codes[o:o + L] = [R.fasta_code(b) for b in ref[name].tolist()]
    codes = pipeline.reference_codes(twin, fa, dict(contigs))
    assert np.array_equal(codes, want_codes)
    sel = np.arange(len(contigs), dtype=np.int32)
    want_events, want_counts, status = R.stream_events(stream, offs, lengths, sel, want_codes)
    assert status == R.NO_STATUS                                                 # every l_seq is its record's S + M + I
    ivl, counts = twin.bam_mismatch(stream, offs, sel, codes, guard=16)
    assert counts == want_counts and events_of(ivl) == want_events
    assert counts[0] > 10 and counts[2] > 200_000
    if sub_rate == 0.0:
        assert counts[1] == 0                                                    # the reads ARE the assembly under M, = and X
    else:
        # a substituted base is one of four at random: 3 of 4 differ.  Binomial over counts[2] pairs: six standard deviations
        p = 0.75 * sub_rate
        assert abs(counts[1] - p * counts[2]) < 6 * (p * (1 - p) * counts[2]) ** 0.5, counts
    mism = twin.depth_build(np.ascontiguousarray(ivl), 0)
    depth = twin.depth_build(twin.bam_cover(stream, offs, sel), 0)
    assert np.array_equal(mism, R.track_of(want_events, lengths)) and int(mism.sum()) == counts[1]
    assert (mism <= depth).all() and int(depth.max()) >= 4
    for min_reads, frac in ((1, 0), (2, 500000), (3, 1000000)):
        got = twin.mismatch_sites(mism, depth, min_reads, frac)
        assert list(zip(*(got[f].tolist() for f in FIELDS))) == R.sites_of(mism, depth, lengths, min_reads, frac), (min_reads, frac)


def test_need_seq_refuses_the_heads_ingest(tmp_path, monkeypatch):
    import inspect
    sig = inspect.signature(pipeline.bam_join_input)
    assert sig.parameters["need_seq"].default is False and list(sig.parameters)[-1] == "need_seq"
    with pytest.raises(pipeline.SeqNeeded):
        pipeline.bam_join_input(None, str(tmp_path / "none.bam"), [], None, ingest="heads", need_seq=True)
    monkeypatch.setenv("GCI_BAM_INGEST", "heads")
    with pytest.raises(pipeline.SeqNeeded):
        pipeline.bam_mismatch_sites(None, "ref.fa", ["a.bam"])
    assert issubclass(pipeline.SeqNeeded, ValueError)
    assert pipeline._MismatchVisitor.NEED_SEQ and not pipeline._IndelVisitor.NEED_SEQ and not pipeline._ClipVisitor.NEED_SEQ


def test_encode_record_takes_bases():
    plain = bamfmt.encode_record(0, 5, "r", 60, 0, [(0, 5)], 5)
    with_seq = bamfmt.encode_record(0, 5, "r", 60, 0, [(0, 5)], 5, seq=b"ACgTN")
    assert len(plain) == len(with_seq)
    at = 4 + 32 + 2 + 4
    assert plain[at:at + 3] == b"\x11\x11\x11" and with_seq[at:at + 3] == b"\x12\x48\xF0" and plain[:at] == with_seq[:at]
    with pytest.raises(bamfmt.BAMError):
        bamfmt.encode_record(0, 5, "r", 60, 0, [(0, 5)], 5, seq=b"ACG")


def _cli(tmp_path, *argv, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "mismatch_sites.py"), *argv], capture_output=True, text=True, cwd=str(tmp_path), env=e)


def test_the_command_line_refuses_before_it_touches_the_device(tmp_path):
    c = C.case("phases")
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
    (tmp_path / "GCI_mismatch.mismatch.txt").write_text("x")
    r = _cli(tmp_path, "-r", ref, bam)
    assert r.returncode == 1 and "GCI_mismatch.mismatch.txt" in r.stderr and (tmp_path / "GCI_mismatch.mismatch.txt").read_text() == "x"


def test_the_parser_takes_the_sibling_tools_options():
    args = mismatchsites_cli.build_parser("mismatch_sites.py").parse_args(["-r", "ref.fa", "-Q", "5", "-G", "0x800", "-J", "-n", "4", "-F", "0.25", "a.bam", "b.bam"])
    assert (args.reference, args.min_mapq, args.excl_add, args.count_del, args.min_reads, args.min_frac, args.bams) == \
        ("ref.fa", 5, 0x800, True, 4, "0.25", ["a.bam", "b.bam"])
    assert mismatchsites_cli.outputs(mismatchsites_cli.build_parser("x").parse_args(["-r", "r.fa", "-d", "o", "-o", "p"])) == \
        ["o/p.mismatch.depth.gz", "o/p.mismatch.sites.bed", "o/p.mismatch.txt"]
