"""The statement of filter_depth.py's classes (tests/fate_ref.py) against the oracle's restatement of read_sam: `kept` is the oracle's
`passed`, the statement's status word names the record the oracle raises on, the classes partition the records the raw depth counts,
and the cases of tests/fate_cases.py hold what they are named for."""
import numpy as np
import pytest

import cover_ref as R
import fate_cases as FC
import fate_ref as F
from gci_amd import _lib
from gci_amd.formats import bam as bamfmt


def runs_of(name):
    runs = FC.case(name)["runs"]
    return runs if name != "threshold_band" else runs[::7]          # (the GPU test walks all of them)


def pos_ok(c):
    """Every record has pos >= 0: the oracle, like pysam, does not skip pos = -1 (a record no file the reference reads can hold)."""
    return all(bamfmt.decode_record(c["stream"], o).pos >= 0 for o in c["offs"].tolist() if R.bounds_ok(c["stream"], o))


@pytest.mark.parametrize("name", FC.NAMES)
def test_kept_is_the_oracles_passed_and_the_status_names_the_oracles_record(oracle, name):
    c = FC.case(name)
    if not pos_ok(c):
        assert name == "none_op9"
        return
    for run in runs_of(name):
        cls, counts, status = FC.want(name, run)
        assert int(counts.sum()) == len(c["offs"]) and np.array_equal(counts, np.bincount(cls, minlength=8))
        try:
            passed = oracle.bam_filter_arrays(c["stream"], c["offs"], c["ref_sel"], run[0], 50, run[1], run[2])["passed"].astype(bool)
        except oracle.OracleRecordError as e:
            assert status == (e.rec << 8) | -e.status, (name, run)
            assert cls[e.rec] == F.ERROR
            continue
        assert status == F.NO_STATUS and counts[F.ERROR] == 0, (name, run)
        assert np.array_equal(cls == F.KEPT, passed), (name, run)


def test_the_status_words_of_the_error_cases():
    for name in FC.NAMES:
        for run in runs_of(name):
            cls, counts, status = FC.want(name, run)
            if name in FC.ERRORS:
                rec, code = FC.ERRORS[name]
                assert status == (rec << 8) | -code and cls[rec] == F.ERROR, name
            elif name not in ("random_3000", "scan_blocks"):
                assert status == F.NO_STATUS and counts[F.ERROR] == 0, name


@pytest.mark.parametrize("name, run", FC.depth_pairs())
@pytest.mark.parametrize("count_del", [False, True])
def test_the_depths_of_the_classes_add_up_to_the_raw_depth(name, run, count_del):
    """Classes 1 - 7 partition what `bam_depth.py -g 0x700` counts (excl = 0x4); class 0 and class 7 cover nothing the raw depth has
    that the others lack: an `error` record that is not malformed is counted by the raw depth, and shows in class 7's track."""
    c = FC.case(name)
    raw, _ = R.stream_depth(c["stream"], c["offs"], c["lengths"], c["ref_sel"], 0x4, 0, count_del)
    total = [np.zeros_like(r) for r in raw]
    for k in range(1, 8):
        for t, d in zip(total, FC.want_depth(name, run, k, count_del)):
            t += d
    for t, r in zip(total, raw):
        assert np.array_equal(t, r)
    # `none` is never counted: the skip rule of the raw depth (excl = 0x4) drops every record of it
    none = F.class_depth(c["stream"], c["offs"], c["lengths"], c["ref_sel"], FC.want(name, run)[0], F.NONE, count_del, excl=0x4)
    assert all(not d.any() for d in none)


def test_the_cases_hold_what_they_are_named_for():
    assert F.NAMES == _lib.FATE_NAMES and FC.CH == _lib.COVER_CHUNK_OPS
    cls = FC.want("one_per_class", FC.DEFAULT)[0]
    assert sorted(cls.tolist()) == [0, 1, 2, 3, 4, 5, 6, 6]
    assert FC.want("several_tests", FC.DEFAULT)[0].tolist() == [F.SECONDARY, F.MAPQ, F.CLIP, F.NONE, F.SUPPLEMENTARY, F.NONE]
    assert FC.want("on_the_thresholds", FC.DEFAULT)[0].tolist() == [F.KEPT, F.CLIP, F.KEPT, F.KEPT, F.IDENTITY, F.KEPT, F.CLIP]
    assert FC.want("placeholder", FC.DEFAULT)[0].tolist() == [F.KEPT, F.IDENTITY, F.KEPT, F.KEPT, F.CLIP, F.CLIP, F.KEPT]
    assert FC.want("none_op9", FC.DEFAULT)[0].tolist() == [F.NONE] * 5 + [F.KEPT] + [F.NONE] * 3
    c = FC.case("nm_forms")
    assert {bamfmt.decode_record(c["stream"], o).aux["NM"][0] for o in c["offs"]} == set("cCsSiI")
    assert set(FC.want("nm_forms", FC.DEFAULT)[0].tolist()) == {F.IDENTITY, F.KEPT}
    # the chunk sizes; the clipped record and its twin
    c = FC.case("chunks")
    n_ops = [len(bamfmt.decode_record(c["stream"], o).cigar) for o in c["offs"]]
    assert n_ops[0:20:5] == [FC.CH - 1, FC.CH, FC.CH + 1, 2 * FC.CH + 1] and n_ops[1:20:5] == n_ops[0:20:5]
    cls = FC.want("chunks", FC.DEFAULT)[0]
    assert cls[0:20:5].tolist() == [F.CLIP] * 4 and cls[1:20:5].tolist() == [F.KEPT] * 4
    last = bamfmt.decode_record(c["stream"], c["offs"][15]).cigar
    assert [o for o, _ in last].count(FC.S) == 1 and last[-1][0] == FC.S and (len(last) - 1) // FC.CH == 2 and (len(last) - 1) % FC.CH == 0
    # every byte phase
    c = FC.case("phases")
    assert {(int(o) + 36 + int(c["stream"][int(o) + 12])) % 4 for o in c["offs"]} == {0, 1, 2, 3}
    assert sorted(int(c["stream"][int(o) + 12]) for o in c["offs"][::2]) == list(range(1, 9))          # l_read_name: the name and its NUL
    c = FC.case("placeholder")
    first = bamfmt.decode_record(c["stream"], c["offs"][0])
    assert first.n_cigar_field == 2 and len(first.cigar) == 65537
    # every class at least 20 times in the random case; the scan case crosses the device's 4096-entry blocks
    for run in FC.case("random_3000")["runs"]:
        assert (FC.want("random_3000", run)[1][:7] >= 20).all()
    c = FC.case("scan_blocks")
    cls = FC.want("scan_blocks", FC.DEFAULT)[0]
    n = np.array([(len(bamfmt.decode_record(c["stream"], o).cigar) + FC.CH - 1) // FC.CH if k >= F.CLIP else 0 for o, k in zip(c["offs"].tolist(), cls.tolist())])
    first = np.cumsum(n) - n
    assert n.shape[0] > FC.C.SCAN_BLOCK and int(n.sum()) > FC.C.SCAN_BLOCK
    assert int(first[FC.C.SCAN_BLOCK - 1]) == FC.C.SCAN_BLOCK - 1 and int(n[FC.C.SCAN_BLOCK - 1]) == 3
    assert len(set(cls[:FC.C.SCAN_BLOCK].tolist())) >= 3 and len(set(cls[FC.C.SCAN_BLOCK:].tolist())) == 8
    # the heads form holds the same records without SEQ / QUAL
    hs, ho = FC.heads("placeholder")
    assert len(ho) == len(FC.case("placeholder")["offs"]) and all(R.bounds_ok(hs, o, has_seq=False) for o in ho)
