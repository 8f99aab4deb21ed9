"""allele_sites.py on the GPU: gci_bam_allele_size / _write and gci_allele_sites_size / _write (k_mismatch.hip) against the statement of
tests/allele_ref.py on every case of tests/allele_cases.py, into pre-filled buffers with guard entries behind them; against
Engine.bam_mismatch on the same buffers; pipeline.bam_allele_sites over a small file made from a truth sequence and an assembly with
planted substitutions, in one piece, in several and with forced flushes -- the VCF, applied to the assembly, gives the truth; two
files; and the command line once."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import allele_cases as C
import allele_ref as R
from cover_cases import M
from gci_amd import _lib, pipeline, synth
from gci_amd.device import ALLELE_SITE_DTYPE, IVL_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16                                             # entries behind the output that must stay
PATTERN = -0x5A5A5A5B
U64 = 2 ** 64 - 1
STREAM_GUARD = 64                                      # bytes behind the stream: 0x88, the base T in both nibbles


def upload(engine, name):
    c = C.case(name)
    stream, offs = c["stream"], c["offs"]
    padded = np.concatenate([stream, np.full(STREAM_GUARD, 0x88, dtype=np.uint8)])
    up = lambda a: engine.to_device(a if a.shape[0] else np.zeros(1, dtype=a.dtype))      # noqa: E731
    return dict(stream=engine.to_device(padded), offs=up(offs), sel=engine.to_device(c["ref_sel"]), n_bytes=int(stream.shape[0]),
                n_rec=int(offs.shape[0]), codes=engine.to_device(c["codes"]))


@pytest.fixture(scope="module")
def on_device(engine):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = upload(engine, name)
        return cache[name]
    return get


def device_allele(engine, b, run, cap=None, has_seq=1):
    """-> (the four lists, counts, status word, the size call's return, the write call's return, the whole buffer) of the exports as
    they are: the output pre-filled with a pattern, GUARD entries behind it."""
    p, lib = engine._p, engine.lib
    counts = (ctypes.c_uint64 * 6)()
    status = engine.T.zeros(1, engine.T.int64, engine.device)
    offs = p(b["offs"]) if b["n_rec"] else None
    st = lib.gci_bam_allele_size(engine.ctx, p(b["stream"]), b["n_bytes"], offs, b["n_rec"], has_seq, p(b["sel"]), int(b["sel"].shape[0]), run[0],
                                 run[1], p(b["codes"]), counts, p(status))
    if st:
        return None, None, None, st, None, None
    counts = [int(x) for x in counts]
    ends = np.cumsum([0] + counts[1:5]).tolist()
    out = engine.to_device(np.full((ends[4] + GUARD, 4), PATTERN, dtype=np.int32))
    wr = lib.gci_bam_allele_write(engine.ctx, p(b["stream"]), b["n_bytes"], offs, b["n_rec"], has_seq, p(b["codes"]), p(out),
                                  ends[4] if cap is None else cap, p(status))
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 4)
    ivl = host.view(IVL_DTYPE).reshape(-1)
    return [ivl[ends[k]:ends[k + 1]] for k in range(4)], counts, int(status.item()) & U64, st, wr, host


def events_of(ivl):
    assert (ivl["start"] == ivl["end"]).all() and (ivl["pad"] == 0).all()
    return list(zip(ivl["contig"].tolist(), ivl["start"].tolist()))


@pytest.mark.parametrize("name", C.NAMES)
def test_the_device_gives_the_lists_of_the_statement(engine, on_device, name):
    """The four lists, each in (record, reference position) order, status and counts as the statement's, the guard entries untouched;
    the track built from list X holds, per base, the events of X over it."""
    c, b = C.case(name), on_device(name)
    engine.set_layout(c["lengths"])
    for run in c["runs"]:
        want_lists, want_counts, want_status = C.want(name, run)
        lists, counts, status, st, wr, host = device_allele(engine, b, run)
        assert st == 0 and wr == 0 and status == want_status and counts == want_counts, run
        assert (host[sum(counts[1:5]):] == PATTERN).all(), "entries behind the events were written"
        assert [events_of(x) for x in lists] == want_lists, run
        for ivl, want in zip(lists, want_lists):
            if want:
                track = engine.depth_build(engine.to_device(np.ascontiguousarray(ivl).view(np.int32).reshape(-1, 4)), None, 0, engine.new_track())
                assert np.array_equal(track.cpu().numpy(), R.track_of(want, c["lengths"])), run


def test_the_device_gives_the_hand_written_lists(engine, on_device):
    for (name, run), want in C.EXPECTED.items():
        engine.set_layout(C.case(name)["lengths"])
        lists, counts, _, st, wr, _ = device_allele(engine, on_device(name), run)
        assert (st, wr, tuple(events_of(x) for x in lists)) == (0, 0, want), (name, run)
        assert counts[1:5] == [len(x) for x in want]


def test_two_runs_give_the_same_bytes(engine, on_device):
    for name in ("records_4097", "every_base"):
        c, b = C.case(name), on_device(name)
        engine.set_layout(c["lengths"])
        first = device_allele(engine, b, c["runs"][0])[5]
        assert first.shape[0] > 1500 + GUARD and np.array_equal(first, device_allele(engine, b, c["runs"][0])[5]), name


def test_the_merged_lists_are_engine_bam_mismatchs_events(engine, on_device):
    """On the same device buffers: the four lists together are the mismatch walk's events as a multiset, and the outer counts agree."""
    for name in ("lanes", "ops_2049", "records_257", "ont_hifi", "every_base"):
        c, b = C.case(name), on_device(name)
        engine.set_layout(c["lengths"])
        run = c["runs"][0]
        stream = b["stream"][:b["n_bytes"]]
        *lists, counts = engine.bam_allele(stream, b["offs"], True, b["sel"], b["codes"], *run)
        mm, mm_counts = engine.bam_mismatch(stream, b["offs"], True, b["sel"], b["codes"], *run)
        assert [counts[0], sum(counts[1:5]), counts[5]] == mm_counts and [int(x.shape[0]) for x in lists] == counts[1:5], name
        merged = np.concatenate([x.cpu().numpy().reshape(-1, 4) for x in lists])
        key = lambda a: sorted(map(tuple, a.tolist()))      # noqa: E731
        assert key(merged) == key(mm.cpu().numpy().reshape(-1, 4)), name
        assert [events_of(x.cpu().numpy().view(IVL_DTYPE).reshape(-1)) for x in lists] == C.want(name, run)[0], name


def test_engine_bam_allele_raises_on_a_malformed_record(engine, on_device):
    for name, bad in C.MALFORMED.items():
        b = on_device(name)
        engine.set_layout(C.case(name)["lengths"])
        with pytest.raises(_lib.GciError) as e:
            engine.bam_allele(b["stream"][:b["n_bytes"]], b["offs"], True, b["sel"], b["codes"])
        assert e.value.status == _lib.GCI_E_MALFORMED and e.value.rec == bad, name


def test_argument_errors_of_the_record_calls(engine, on_device):
    c, b = C.case("phases"), on_device("phases")
    engine.set_layout(c["lengths"])
    p, lib = engine._p, engine.lib
    assert device_allele(engine, b, (C.EXCL, 0), has_seq=0)[3] == _lib.GCI_E_INVALID            # a heads stream holds no SEQ
    _, counts, _, st, wr, host = device_allele(engine, b, (C.EXCL, 0), cap=4)                  # five events: one entry too few
    assert st == 0 and counts == [5, 0, 3, 0, 2, 24] and wr == _lib.GCI_E_CAPACITY and (host == PATTERN).all()
    out = engine.T.empty((16, 4), engine.T.int32, engine.device)
    write = lambda e, n_rec=b["n_rec"], codes=b["codes"]: lib.gci_bam_allele_write(e.ctx, p(b["stream"]), b["n_bytes"], p(b["offs"]), n_rec, 1,      # noqa: E731
                                                                                   p(codes), p(out), 16, p(engine._status))
    assert write(engine, n_rec=b["n_rec"] - 1) == _lib.GCI_E_INVALID                           # not what the size call measured
    assert write(engine, codes=engine.to_device(c["codes"])) == _lib.GCI_E_INVALID
    assert write(engine) == 0
    # after ANOTHER input's size call the write of this one is refused
    other = on_device("letters")
    engine.set_layout(C.case("letters")["lengths"])
    assert device_allele(engine, other, (C.EXCL, 0))[3] == 0
    assert write(engine) == _lib.GCI_E_INVALID
    from gci_amd.device import Engine
    fresh = Engine(0)
    try:
        assert device_allele(fresh, b, (C.EXCL, 0))[3] == _lib.GCI_E_NO_LAYOUT
        fresh.set_layout(c["lengths"])
        assert write(fresh) == _lib.GCI_E_INVALID                                               # no size call in front of it
    finally:
        fresh.close()


# ---- sites -----------------------------------------------------------------------------------------------------------------------------

def device_sites(engine, t, min_reads, frac, windows, cap=None):
    p, lib = engine._p, engine.lib
    arr, nw = engine._window_array(windows), len(windows)
    n = ctypes.c_uint64(0)
    head = (engine.ctx, *(p(t[k]) for k in C.SITE_KEYS), min_reads, frac, arr, nw)
    assert lib.gci_allele_sites_size(*head, ctypes.byref(n)) == 0
    total = int(n.value)
    out = engine.to_device(np.full((total + GUARD, 9), PATTERN, dtype=np.int32))
    wr = lib.gci_allele_sites_write(*head, p(out), total if cap is None else cap)
    engine.sync()
    host = np.ascontiguousarray(out.cpu().numpy()).reshape(-1, 9)
    return host[:total].view(ALLELE_SITE_DTYPE).reshape(-1), wr, host


@pytest.mark.parametrize("name", C.SITE_NAMES)
def test_the_device_gives_the_sites_of_the_statement(engine, name):
    c = C.site_case(name)
    engine.set_layout(c["lengths"])
    assert int(engine.total) == c["depth"].shape[0]
    t = {k: engine.to_device(c[k]) for k in C.SITE_KEYS}
    for k, (min_reads, frac, windows) in enumerate(c["runs"]):
        got, wr, host = device_sites(engine, t, min_reads, frac, windows)
        assert wr == 0 and (host[got.shape[0]:] == PATTERN).all()
        assert C.site_rows(got) == C.want_sites(name, k), k
        if (name, k) in C.SITES_EXPECTED:
            assert C.site_rows(got) == C.SITES_EXPECTED[(name, k)], k
    sites = engine.allele_sites(*(t[k] for k in C.SITE_KEYS), *c["runs"][0])
    assert C.site_rows(sites) == C.want_sites(name, 0)


def test_argument_errors_of_the_site_calls(engine):
    c = C.site_case("random")
    engine.set_layout(c["lengths"])
    t = {k: engine.to_device(c[k]) for k in C.SITE_KEYS}
    p, lib = engine._p, engine.lib
    n = ctypes.c_uint64(0)

    def size(r=3, f=500000, w=None, nw=0, **other):
        a = dict(t, **other)
        return lib.gci_allele_sites_size(engine.ctx, *(p(a[k]) for k in C.SITE_KEYS), r, f, w, nw, ctypes.byref(n))

    def write(out, cap, r=3, f=500000, **other):
        a = dict(t, **other)
        return lib.gci_allele_sites_write(engine.ctx, *(p(a[k]) for k in C.SITE_KEYS), r, f, None, 0, p(out), cap)
    assert size(r=0) == _lib.GCI_E_INVALID and size(f=-1) == _lib.GCI_E_INVALID and size(f=1000001) == _lib.GCI_E_INVALID
    for which in C.SITE_KEYS:
        assert size(**{which: None}) == _lib.GCI_E_INVALID, which
        if which != "codes":
            assert size(**{which: t[which][1:]}) == _lib.GCI_E_INVALID, which              # not 16-byte aligned
    assert size(w=engine._window_array([(0, 5000), (4999, 6000)]), nw=2) == _lib.GCI_E_INVALID              # windows that overlap
    got, wr, host = device_sites(engine, t, 3, 500000, (), cap=len(C.want_sites("random", 1)) - 1)
    assert wr == _lib.GCI_E_CAPACITY and (host == PATTERN).all()
    out = engine.T.empty((8192, 9), engine.T.int32, engine.device)
    assert write(out, 8192, f=500001) == _lib.GCI_E_INVALID and write(out, 8192, r=4) == _lib.GCI_E_INVALID      # not what was measured
    assert write(out, 8192, g=engine.to_device(c["g"])) == _lib.GCI_E_INVALID                  # another array, the fourth of six
    assert write(out, 8192) == 0
    assert size() == 0
    engine.depth_hist(t["depth"], [(0, 100)], 0)                                                            # ... something else set windows in between
    assert write(out, 8192) == _lib.GCI_E_INVALID
    from gci_amd.device import Engine
    fresh = Engine(0)
    try:
        assert lib.gci_allele_sites_size(fresh.ctx, *(p(t[k]) for k in C.SITE_KEYS), 3, 500000, None, 0, ctypes.byref(n)) == _lib.GCI_E_NO_LAYOUT
    finally:
        fresh.close()


# ---- whole files -----------------------------------------------------------------------------------------------------------------------

CONTIGS = (("ctg1", 9000), ("ctg2", 5000))
PLANTED = [(0, 0), (0, 2000), (0, 2001), (0, 4095), (0, 4096), (0, 8999), (1, 0)]      # (contig, position): where the assembly is wrong
READ, COVER = 1000, 5
_FILES = {}


def _run(script, argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


def _reads(truth, seed, hdr):
    """COVER tilings of every contig with error-free reads of the truth, each tiling shifted by a fifth of a read: every base lies
    under exactly COVER reads.  -> the inflated BAM stream, sorted by position."""
    rng = np.random.default_rng(seed)
    recs = []
    for ref_id, (name, L) in enumerate(CONTIGS):
        seq = truth[name].tobytes()
        for k in range(COVER):
            cuts = [0] + list(range(k * READ // COVER + int(rng.integers(1, 50)), L, READ)) + [L]
            recs += [(ref_id, a, bamfmt.encode_record(ref_id, a, "r%d_%d_%d" % (ref_id, k, a), 60, 0, [(M, b - a)], b - a, seq=seq[a:b]))
                     for a, b in zip(cuts, cuts[1:]) if b > a]
    recs.sort(key=lambda r: r[:2])
    return np.frombuffer(hdr + b"".join(r[2] for r in recs), dtype=np.uint8).copy()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A seeded truth over two contigs, an assembly that is the truth with a substitution at every PLANTED base, and two BAM files
    (BGZF) of COVER x error-free reads of the truth each.  Made once."""
    if not _FILES:
        d = tmp_path_factory.mktemp("alleles")
        truth = synth.random_reference(CONTIGS, seed=5)
        assembly = {k: v.copy() for k, v in truth.items()}
        for c, p in PLANTED:
            a = assembly[CONTIGS[c][0]]
            a[p] = b"ACGT"[(b"ACGT".index(int(a[p])) + 1 + (p % 3)) % 4]
        fa = str(d / "assembly.fa")
        synth.write_fasta(fa, {k: assembly[k] for k in ("ctg2", "ctg1")}, width=61)
        hdr = bamfmt.encode_header([n for n, _ in CONTIGS], [l for _, l in CONTIGS])
        paths = []
        for seed in (1, 2):
            stream = _reads(truth, seed, hdr)
            assert stream.shape[0] > 0xFF00 + 4096                               # more than one BGZF member: several pieces can be made
            paths.append(str(d / ("reads%d.bam" % seed)))
            bamfmt.write_bam_stream(paths[-1], stream, level=1, threads=4)
        _FILES.update(fasta=fa, truth=truth, assembly=assembly, paths=paths, dir=d)
    return _FILES


def host_tracks(res):
    return {k: v.track.cpu().numpy().copy() for k, v in res.tracks.items()}


def apply_vcf(text, assembly):
    """The edit list applied: every line's REF must be the assembly's base there."""
    out = {k: bytearray(v.tobytes()) for k, v in assembly.items()}
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        chrom, pos, _, ref, alt = line.split("\t")[:5]
        assert chr(out[chrom][int(pos) - 1]) == ref and len(alt) == 1 and alt != ref
        out[chrom][int(pos) - 1] = ord(alt)
    return {k: bytes(v) for k, v in out.items()}


def test_the_pipeline_in_one_piece_in_several_and_with_forced_flushes(engine, files, monkeypatch):
    """All three give identical tracks and sites: exactly the planted bases, REF the assembly's base, ALT the truth's, AO = DP = COVER;
    the VCF applied to the assembly is the truth; A + C + G + T is bam_mismatch_sites' mismatch track and depth its depth."""
    path, opts = files["paths"][0], pipeline.CoverOpts()
    truth, assembly = files["truth"], files["assembly"]
    names = [n for n, _ in CONTIGS]
    mm = pipeline.bam_mismatch_sites(engine, files["fasta"], [path], [], opts, 4, 3, "0.5")
    mm_tracks = {k: getattr(mm, k).track.cpu().numpy().copy() for k in ("mismatch", "depth")}
    assert int(mm_tracks["mismatch"].sum()) == COVER * len(PLANTED)
    pieces, visit = [], pipeline._ClipVisitor.visit
    monkeypatch.setattr(pipeline._ClipVisitor, "visit", lambda self, *a: (pieces.append(a[-1]), visit(self, *a))[1])      # (a[-1]: rec_idx_base)
    whole = (pipeline.GPU_INFLATE_MAX, pipeline.BAM_CHUNK_BYTES)
    first = None
    for several, budget in ((False, None), (True, None), (True, 1)):
        monkeypatch.setattr(pipeline, "GPU_INFLATE_MAX", 0 if several else whole[0])
        monkeypatch.setattr(pipeline, "BAM_CHUNK_BYTES", (1 << 16) if several else whole[1])      # (a run per BGZF member of 0xFF00 bytes)
        del pieces[:]
        res = pipeline.bam_allele_sites(engine, files["fasta"], [path], [], opts, 4, 3, "0.5", None, budget)
        assert (len(pieces) > 1) == several and pieces[0] == 0 and sorted(pieces) == pieces, pieces
        assert (res.flushes > 0) == (budget == 1)
        got = host_tracks(res)
        assert np.array_equal(got["A"] + got["C"] + got["G"] + got["T"], mm_tracks["mismatch"]) and np.array_equal(got["depth"], mm_tracks["depth"])
        assert res.counts == [[mm.counts[0][0], *res.counts[0][1:5], mm.counts[0][2]]] and sum(res.counts[0][1:5]) == mm.counts[0][1]
        rows = C.site_rows(res.sites)
        assert [r[:2] for r in rows] == PLANTED, (several, budget)
        for c, p, ref, alt, *n, depth in rows:
            assert "=ACMGRSVTWYHKDBN"[ref] == chr(assembly[names[c]][p]) and "=ACMGRSVTWYHKDBN"[alt] == chr(truth[names[c]][p])
            assert depth == COVER and sorted(n) == [0, 0, 0, COVER]
        if first is None:
            first = (got, rows)
        else:
            assert rows == first[1] and all(np.array_equal(got[k], first[0][k]) for k in got), (several, budget)
        vcf = pipeline.allele_sites_vcf(res.sites, res.depth.targets_length, files["fasta"])
        assert [ln.split("\t")[:2] for ln in vcf.splitlines() if not ln.startswith("#")] == [[names[c], str(p + 1)] for c, p in PLANTED]
        assert apply_vcf(vcf, assembly) == {k: v.tobytes() for k, v in truth.items()}
    monkeypatch.undo()
    # regions select sites, not tracks
    res = pipeline.bam_allele_sites(engine, files["fasta"], [path], [], opts, 4, 3, "0.5", [("ctg1", 2001, 4096), ("nowhere", 0, 9)])
    assert [r[:2] for r in C.site_rows(res.sites)] == [(0, 2001), (0, 4095)] and np.array_equal(host_tracks(res)["depth"], first[0]["depth"])
    res = pipeline.bam_allele_sites(engine, files["fasta"], [path], ["ctg2"], opts, 4, COVER + 1, "0.5")
    assert res.sites.shape[0] == 0 and list(res.depth.keys()) == ["ctg2"]


def test_two_files_add(engine, files):
    both = pipeline.bam_allele_sites(engine, files["fasta"], files["paths"], [], None, 4, 1, "0")
    got = host_tracks(both)
    alone = [pipeline.bam_allele_sites(engine, files["fasta"], [p], [], None, 4, 1, "0") for p in files["paths"]]
    parts = [host_tracks(r) for r in alone]
    assert both.counts == [alone[0].counts[0], alone[1].counts[0]] and sum(both.counts[1][1:5]) == COVER * len(PLANTED)
    for k in got:
        assert np.array_equal(got[k], parts[0][k] + parts[1][k]), k
    rows = C.site_rows(both.sites)
    assert [r[:2] for r in rows] == PLANTED and all(r[8] == 2 * COVER and max(r[4:8]) == 2 * COVER for r in rows)


def test_command_line(engine, files, tmp_path):
    out = str(tmp_path)
    path = files["paths"][0]
    r = _run("allele_sites.py", ["-r", files["fasta"], "-d", out, "-o", "s", "-t", "4", path], dict(GCI_ASSERT_NO_TORCH="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["s.allele.A.depth.gz", "s.allele.C.depth.gz", "s.allele.G.depth.gz", "s.allele.T.depth.gz", "s.allele.sites.bed",
                                       "s.allele.sites.vcf", "s.allele.txt"]
    res = pipeline.bam_allele_sites(engine, files["fasta"], [path], [], None, 4)
    want = host_tracks(res)
    for base in "ACGT":                                                          # ordinary depth files: the project's reader takes them
        tracks, got_lengths = pipeline.read_depth_tracks(engine, os.path.join(out, "s.allele.%s.depth.gz" % base))
        assert dict(got_lengths) == dict(CONTIGS) and np.array_equal(tracks.track.cpu().numpy(), want[base]), base
    vcf = open(os.path.join(out, "s.allele.sites.vcf")).read()
    assert vcf == pipeline.allele_sites_vcf(res.sites, dict(CONTIGS), files["fasta"])
    assert apply_vcf(vcf, files["assembly"]) == {k: v.tobytes() for k, v in files["truth"].items()}
    assert open(os.path.join(out, "s.allele.sites.bed")).read() == pipeline.allele_sites_bed(res.sites, [n for n, _ in CONTIGS])
    text = open(os.path.join(out, "s.allele.txt")).read()
    assert text == pipeline.allele_summary_text([path], res.counts, int(res.sites.shape[0]),
                                                [("reference", files["fasta"]), ("min_reads", 3), ("min_frac_ppm", 500000), ("excl_flags", "0x704"),
                                                 ("min_mapq", 0), ("count_del", 0), ("chrs", "."), ("regions", ".")])
    r = _run("allele_sites.py", ["-r", files["fasta"], "-d", out, "-o", "s", path])          # a second run without -f refuses
    assert r.returncode != 0 and r.stderr.strip().split("\n")[-1] == 'Please use "-f" or "--force" to rewrite'
    r = _run("allele_sites.py", ["-r", files["fasta"], "-d", out, "-o", "h", path], dict(GCI_BAM_INGEST="heads"))
    assert r.returncode != 0 and "Traceback" not in r.stderr and "GCI_BAM_INGEST=heads" in r.stderr
    assert not [x for x in os.listdir(out) if x.startswith("h.")]
