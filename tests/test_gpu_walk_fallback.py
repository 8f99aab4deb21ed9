"""What the ingestion does with what the parallel record walk (gci_bam_record_offsets_device) tells it: a stream whose chain the
walk loses -- a record the strict test rejects and the serial walk accepts -- takes the host path and ends as the `full` ingest
ends, kept records or error alike; a file cut inside its last record is refused by every ingest mode."""
import struct

import numpy as np
import pytest

from gci_amd import _lib, pipeline, synth
from gci_amd._lib import GciError
from gci_amd.device import Engine, REC_DTYPE
from gci_amd.formats import bam as bamfmt

pytestmark = pytest.mark.gpu

CONTIGS = (("a", 120_000), ("b", 60_000))
TARGETS, FILT = ["a", "b"], (30, 50, 0.1, 0.9)
# (name, module knobs, bam_join_input keywords): the device whole and run by run, the host's stream, the host's heads
MODES = [("gpu whole", {}, {"ingest": "gpu"}), ("gpu run by run", {"GPU_INFLATE_MAX": 0, "BAM_CHUNK_BYTES": 400_000}, {"ingest": "gpu"}),
         ("full", {}, {"ingest": "full"}), ("heads", {}, {"ingest": "heads"})]


@pytest.fixture(scope="module")
def reads():
    rs = synth.simulate_reads(CONTIGS, 20, "hifi", seed=31).sorted()
    stream, offs = synth.to_bam_stream(rs)
    assert 150 < len(offs) < 1000 and stream.shape[0] > 3 * 400_000
    return stream, offs.astype(np.int64)


def outcome(engine, path, monkeypatch, knobs, kw):
    """What an ingest of the file comes to: the records without their index in the run, or the error's type, status and record."""
    with monkeypatch.context() as m:
        for k, v in knobs.items():
            m.setattr(pipeline, k, v)
        try:
            ji = pipeline.bam_join_input(engine, path, TARGETS, FILT, threads=4, **kw)
        except (GciError, bamfmt.BAMError) as e:
            return "error", type(e).__name__, getattr(e, "status", None), getattr(e, "rec", None)
    recs = ji.recs.cpu().numpy().reshape(-1).view(REC_DTYPE)
    return ("records",) + tuple(recs[f].tolist() for f in REC_DTYPE.names if f != "rec_idx")


@pytest.mark.parametrize("ending", ["kept", "error"])
def test_a_chain_the_walk_loses_ends_as_the_full_ingest_ends(engine, reads, tmp_path, monkeypatch, ending):
    stream, offs = reads
    stream = stream.copy()
    j = len(offs) * 2 // 3
    stream[int(offs[j]) + 24:int(offs[j]) + 28] = np.frombuffer(struct.pack("<i", len(CONTIGS) + 5), dtype=np.uint8)      # next_refID
    if ending == "error":                                     # further on, a record the reference dies on: mapped, MAPQ 60, no NM tag
        k = j + (len(offs) - j) // 2
        bad = bamfmt.encode_record(0, 1000, "no_nm", 60, 0, [(0, 100)], 100, bamfmt.encode_aux([("AS", "i", 0)]))
        stream = np.concatenate([stream[:int(offs[k])], np.frombuffer(bad, dtype=np.uint8), stream[int(offs[k + 1]):]])
    assert np.array_equal(bamfmt.record_offsets(stream, int(offs[0]))[:j + 1].astype(np.int64), offs[:j + 1])      # the serial walk goes on
    path = str(tmp_path / "lost.bam")
    bamfmt.write_bam_stream(path, stream, level=1, threads=4)
    walks = []
    real = Engine.bam_record_offsets

    def spy(self, d_stream, first_record, n_ref):
        got = real(self, d_stream, first_record, n_ref)
        walks.append((got[1], got[2]))
        return got

    monkeypatch.setattr(Engine, "bam_record_offsets", spy)
    monkeypatch.delenv("GCI_BAM_INGEST", raising=False)
    engine.set_layout([l for _, l in CONTIGS])
    got, lost = {}, {}
    for mode, knobs, kw in MODES:
        del walks[:]
        got[mode] = outcome(engine, path, monkeypatch, knobs, kw)
        lost[mode] = [used for used, ok in walks if not ok]
    # the device walk really lost the chain, once, behind record j - 1 (run by run: inside the run that holds it) -- and only there
    assert len(lost["gpu whole"]) == 1 and lost["gpu whole"][0] == int(offs[j - 1])
    assert len(lost["gpu run by run"]) == 1 and lost["full"] == [] and lost["heads"] == []
    want = got["full"]
    assert want[0] == ("records" if ending == "kept" else "error")
    if ending == "kept":
        assert len(want[1]) == len(offs)
    else:
        assert want[1:] == ("GciError", _lib.GCI_E_NO_NM, k)
    for mode, _, _ in MODES:
        assert got[mode] == want, mode


@pytest.mark.parametrize("into", [1, 20, 40])
def test_a_file_cut_inside_its_last_record_is_refused(engine, reads, tmp_path, monkeypatch, into):
    stream, offs = reads
    path = str(tmp_path / "cut.bam")
    bamfmt.write_bam_stream(path, stream[:int(offs[-1]) + into], level=1, threads=4)
    monkeypatch.delenv("GCI_BAM_INGEST", raising=False)
    engine.set_layout([l for _, l in CONTIGS])
    for mode, knobs, kw in MODES + [("full in chunks", {}, {"ingest": "full", "chunk_bytes": 300_000})]:
        with monkeypatch.context() as m:
            for k, v in knobs.items():
                m.setattr(pipeline, k, v)
            with pytest.raises((bamfmt.BAMError, GciError)) as e:
                pipeline.bam_join_input(engine, path, TARGETS, FILT, threads=4, **kw)
        assert isinstance(e.value, bamfmt.BAMError) or e.value.status == _lib.GCI_E_MALFORMED, (mode, e.value)
