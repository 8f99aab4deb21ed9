"""libgci_cpu.so's twins of gci_name_join_fate and gci_fate_refine against the statement (tests/joinfate_ref.py) on every case of
tests/joinfate_cases.py -- bytes, counts, status word, the bytes behind every output left alone -- and the argument errors of
filter_depth.py --join that need no device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import joinfate_cases as JC
import joinfate_ref as J
from gci_amd import cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    return cpu.CpuEngine(threads=2)


@pytest.mark.parametrize("name, op", JC.pairs())
def test_the_twin_gives_the_bytes_of_the_statement(eng, name, op):
    want_fate, want_counts, want_status, _ = JC.want(name, op)
    fate, counts, status = eng.name_join_fate(JC.inputs(name), op, guard=GUARD)
    assert status == want_status
    for f, (got, want) in enumerate(zip(fate, want_fate)):
        assert (got[want.shape[0]:] == 0xA5).all() and got.shape[0] == want.shape[0] + GUARD, "bytes behind the verdicts were written"
        assert np.array_equal(got[:want.shape[0]], want), (f, np.flatnonzero(got[:want.shape[0]] != want)[:10])
    assert np.array_equal(counts, want_counts)


HAND = np.array([0, 1, 6, 6, 3, 6, 6, 6, 5, 7, 6], dtype=np.uint8)
HAND_JOIN = np.array([0, 0, 12, 8, 0, 9, 10, 11, 0, 0, 12], dtype=np.uint8)


def test_refine_puts_the_join_byte_where_kept_stands(eng):
    want, want_status = J.refine(HAND, HAND_JOIN)
    assert want.tolist() == [0, 1, 12, 8, 3, 9, 10, 11, 5, 7, 12] and want_status == J.NO_STATUS
    cls = np.concatenate([HAND, np.full(GUARD, 0xA5, np.uint8)])
    assert eng.fate_refine(cls, HAND_JOIN) == want_status
    assert np.array_equal(cls[:HAND.shape[0]], want) and (cls[HAND.shape[0]:] == 0xA5).all()


@pytest.mark.parametrize("at, cls_byte, join_byte", [(3, 6, 0), (3, 6, 7), (3, 6, 13), (4, 3, 12), (0, 0, 9)])
def test_refine_reports_a_record_the_two_passes_disagree_about(eng, at, cls_byte, join_byte):
    cls, join = HAND.copy(), HAND_JOIN.copy()
    cls[at], join[at] = cls_byte, join_byte
    cls[9], join[9] = 6, 0                                      # a second one further on: the smaller word is reported
    want, want_status = J.refine(cls, join)
    assert want_status == J.word(at, J.E_INVALID)
    assert eng.fate_refine(cls, join) == want_status and np.array_equal(cls, want) and cls[at] == cls_byte


# ---- the command line's argument errors (nothing here reaches a device) ----------------------------------------------------------------

def _run(argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "filter_depth.py")] + argv, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def _last(r):
    assert r.returncode != 0 and "Traceback" not in r.stderr, r.stderr[-2000:]
    return r.stderr.strip().split("\n")[-1]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from gci_amd import synth
    from gci_amd.formats import bam as bamfmt
    d = tmp_path_factory.mktemp("joinfate_cli")
    rs = synth.simulate_reads((("ctgA", 20_000),), 1.0, "hifi", seed=5)
    stream, _ = synth.to_bam_stream(rs)
    bam = str(d / "a.bam")
    bamfmt.write_bam_stream(bam, stream, level=1, threads=1)
    paf = str(d / "a.paf")
    open(paf, "w").write("".join(synth.to_paf_lines(rs, 3)))
    return dict(dir=str(d), bam=bam, paf=paf)


def test_without_join_the_new_options_and_names_are_errors(tiny):
    d = ["-d", tiny["dir"]]
    assert _last(_run(d + ["--classes", "kept,joined", tiny["bam"]])) == (
        'ERROR!!! The class "joined" of --classes is not one of secondary, supplementary, mapq, clip, identity, kept (shadowed, unpaired, contig, '
        'overlap, joined need --join)')
    for opt, named in ((["-op", "0.8"], "-op"), (["--ovlp-percent", "0.8"], "-op"), (["--mq-cutoff", "40"], "--mq-cutoff"), (["--cover", "1"], "--cover")):
        assert _last(_run(d + opt + [tiny["bam"]])) == "ERROR!!! The option %s needs --join" % named
    assert _last(_run(d + [tiny["bam"], tiny["paf"]])).startswith('ERROR!!! The file "%s" cannot be read as a BAM file (' % tiny["paf"])     # as before


def test_with_join_cover_and_the_files_are_checked(tiny):
    d = ["-d", tiny["dir"], "--join"]
    assert _last(_run(d + [tiny["paf"]])) == "ERROR!!! No BAM file among the files: --join takes its depth from a BAM file"
    for n in ("0", "2"):
        assert _last(_run(d + ["--cover", n, tiny["paf"], tiny["bam"]])) == "ERROR!!! --cover %s: the files hold 1 BAM file(s)" % n
    assert _last(_run(d + ["--classes", "joined,nonsense", tiny["bam"]])).startswith('ERROR!!! The class "nonsense" of --classes is not one of ')
