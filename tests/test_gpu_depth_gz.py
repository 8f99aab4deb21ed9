"""k_depth_gz.hip on the MI355X: the three kernels against their CPU twin field for field (the writer's members, forged members, false
candidates in the middle of other members' bits), and pipeline.read_depth_tracks over files of this project's writer -- the same
tracks as the text path, the path it took in the phase log, the fall-back of a damaged file and of a reference-written golden."""
import gzip
import json
import os
import zlib

import numpy as np
import pytest

import depth_gz_cases as cases
from golden_util import GOLDEN
from gci_amd import phases, pipeline
from gci_amd.cpu import CpuEngine
from gci_amd.formats import depthfile

pytestmark = pytest.mark.gpu


def _notes(fn):
    """-> (fn's result or the exception it raised, the "depth_read:" notes of the phase log, in order)"""
    phases.start()
    try:
        try:
            got = fn()
        except (Exception, SystemExit) as e:                                # noqa: BLE001
            got = e
        notes = [v for k, v in phases.report()["notes"].items() if k.startswith("depth_read:")]
        return got, notes
    finally:
        phases.stop()


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_device_equals_the_twin_field_for_field(engine):
    lengths, track, offsets, own = cases.member_set()
    forged = [d for d, _ in list(cases.outside_grammar().values()) + list(cases.inside_grammar().values()) +
              list(cases.off_by_one().values()) + [cases.over_the_line_cap()]]
    rng = np.random.default_rng(31)
    zone = cases.layout_200()[4] * 3
    stamps = np.sort(rng.choice(len(zone) - 10, 2200, replace=False))       # false candidates in the middle of members' bits
    zone = cases.stamped(zone, stamps.tolist())
    starts, data = [], bytearray(own)
    for d in forged:
        starts.append(len(data))
        data += d
    zone_at = len(data)
    data += zone
    data = bytes(data)
    cand = np.unique(np.concatenate([depthfile.member_candidates(data).astype(np.int64), np.asarray(starts), stamps + zone_at,
                                     rng.integers(0, len(data), 500), [len(data) - 1, len(data), len(data) + 7]])).astype(np.uint64)
    assert int((cand >= zone_at).sum()) >= 2200
    raw = np.frombuffer(data, dtype=np.uint8)
    twin = CpuEngine()
    want = twin.depth_gz_scan(raw, cand)
    d_raw = engine.to_device(raw)
    got = engine.depth_gz_scan(d_raw, cand)
    for f in depthfile.DGZ_INFO_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (f, cand[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert int((want["status"] == depthfile.DGZ_OK).sum()) >= 20 and int((want["status"] != depthfile.DGZ_OK).sum()) >= 2000

    # the runs and the track of every member the scan took whole (the chain's and the forged ones, false candidates included)
    ok = np.flatnonzero((want["status"] == depthfile.DGZ_OK) & (want["crc_ok"] == 1) & (want["isize_ok"] == 1))
    table = np.zeros(ok.shape[0], dtype=depthfile.DGZ_MEMBER_DTYPE)
    table["pos"], table["runs"], table["lines"] = cand[ok], want["runs"][ok], want["lines"][ok]
    table["run0"] = np.cumsum(want["runs"][ok].astype(np.uint64)) - want["runs"][ok]
    lines = want["lines"][ok].astype(np.uint64)
    for aligned in (True, False):                                           # elem0 a multiple of 4 (16-byte stores), then any
        step = (lines + 3) // 4 * 4 if aligned else lines + 1
        table["elem0"] = np.cumsum(step) - step + (0 if aligned else 1)
        n_track = int(table["elem0"][-1] + lines[-1]) + 5
        want_runs = twin.depth_gz_runs(raw, table)
        want_track = twin.depth_gz_expand(want_runs, table, np.full(n_track, -1, dtype=np.int32))
        d_runs, d_members = engine.depth_gz_runs(d_raw, table)
        d_track = engine.to_device(np.full(n_track, -1, dtype=np.int32))
        engine.depth_gz_expand(d_runs, d_members, table.shape[0], d_track)
        got_runs = d_runs.cpu().numpy().view(depthfile.DGZ_RUN_DTYPE)[:want_runs.shape[0]]
        assert _same(got_runs[:int(want["runs"][ok].sum())], want_runs[:int(want["runs"][ok].sum())])
        assert np.array_equal(d_track.cpu().numpy(), want_track), aligned
    # ... and the writer's members give back the track they were written from
    chain = depthfile.member_chain(data[:len(own)], cand[cand < len(own)], got[cand < len(own)])
    assert chain is not None and chain[1] == lengths
    members = depthfile.place_members(chain[2], offsets)
    d_track = engine.to_device(np.zeros(track.shape[0], dtype=np.int32))
    engine.depth_gz_track(d_raw, members, d_track)
    assert np.array_equal(d_track.cpu().numpy(), track)
    twin.close()


def _tracks(engine, lengths, host, names):
    engine.set_layout(lengths)
    full = np.zeros(max(engine.total, 1), dtype=np.int32)
    for o, L, src in zip(engine.offsets, lengths, host):
        full[o:o + L] = src
    return pipeline.DepthTracks(engine, dict(zip(names, lengths)), engine.to_device(full)), full


def _layouts():
    names, lengths, track, offsets, _ = cases.layout_200()
    yield "200 contigs", names, lengths, [track[o:o + L] for o, L in zip(offsets, lengths)]
    rng = np.random.default_rng(32)
    L = 64 * 4096 * 3 + 17
    runs = rng.integers(1, 3000, L // 1000 + 2)
    one = np.repeat(rng.choice(cases.VALUES, runs.shape[0]), runs)[:L].astype(np.int32)
    one[64 * 4096 - 3:64 * 4096 + 3] = 7
    yield "one contig of three members and 17 bases", ["chrT"], [L], [one]


@pytest.mark.parametrize("layout", list(_layouts()), ids=lambda x: x[0])
def test_through_the_pipeline_members_then_text(engine, layout, tmp_path, monkeypatch):
    _, names, lengths, host = layout
    orig, full = _tracks(engine, lengths, host, names)
    d = str(tmp_path)
    pipeline.write_depth(d, "OWN", orig)
    path = os.path.join(d, "OWN.depth.gz")
    with open(path, "rb") as f:
        n_cand = depthfile.member_candidates(f.read()).shape[0]
    assert n_cand >= (130 if len(lengths) > 1 else 4)                       # more than one wave of candidates
    monkeypatch.delenv("GCI_DEPTH_READ", raising=False)
    (a, tl_a), notes_a = _notes(lambda: pipeline.read_depth_tracks(engine, path, dict(zip(names, lengths))))
    track_a, lengths_a = a.track.cpu().numpy().copy(), list(a.lengths)
    monkeypatch.setenv("GCI_DEPTH_READ", "text")
    (b, tl_b), notes_b = _notes(lambda: pipeline.read_depth_tracks(engine, path, dict(zip(names, lengths))))
    assert notes_a == ["members"] and notes_b == ["text"]
    assert tl_a == tl_b == dict(zip(names, lengths)) and lengths_a == list(b.lengths) == lengths
    assert np.array_equal(track_a, b.track.cpu().numpy()) and np.array_equal(track_a[:full.shape[0]], full)
    # a contig the reference does not know: nothing uploaded, tracks None, on either path
    monkeypatch.delenv("GCI_DEPTH_READ", raising=False)
    (none, tl), notes = _notes(lambda: pipeline.read_depth_tracks(engine, path, {"elsewhere": 5}))
    assert none is None and tl == tl_a and notes == ["members"]


def test_a_damaged_member_sends_the_file_to_the_text_path(engine, tmp_path, monkeypatch):
    monkeypatch.delenv("GCI_DEPTH_READ", raising=False)
    names, lengths, track, offsets, data = cases.layout_200()
    cand = depthfile.member_candidates(data)
    at = int(cand[len(cand) // 2]) + 14                                     # inside a member the device decodes
    bad = data[:at] + bytes([data[at] ^ 0x10]) + data[at + 1:]
    path = str(tmp_path / "damaged.depth.gz")
    with open(path, "wb") as f:
        f.write(bad)
    got, notes = _notes(lambda: pipeline.read_depth_tracks(engine, path))
    assert notes == ["text"] and isinstance(got, (gzip.BadGzipFile, zlib.error)), got
    with open(path, "wb") as f:
        f.write(data)
    (ok, tl), notes = _notes(lambda: pipeline.read_depth_tracks(engine, path))
    assert notes == ["members"] and tl == dict(zip(names, lengths))


def test_a_golden_case_keeps_the_text_path(engine, tmp_path, capsys, monkeypatch):
    from gci_amd import score_cli
    monkeypatch.delenv("GCI_DEPTH_READ", raising=False)
    case = "score_c1"                                                       # (one that reads a .depth.gz: score_bed reads BED files)
    with open(os.path.join(GOLDEN, case, "manifest.json")) as f:
        m = json.load(f)
    out = str(tmp_path / "out")
    argv = [a.replace("{GOLDEN}", GOLDEN).replace("{IN}", os.path.join(GOLDEN, "score_inputs")).replace("{OUT}", out) for a in m["argv"]]
    pipeline._ENGINE = engine
    _, notes = _notes(lambda: score_cli.main(["GCI_score.py"] + argv))
    capsys.readouterr()
    assert notes and all(v == "text" for v in notes)
    want_dir = os.path.join(GOLDEN, case, "expected")
    assert sorted(os.listdir(out)) == sorted(os.listdir(want_dir)) == m["files"]
    for fn in m["files"]:
        assert open(os.path.join(out, fn), "rb").read() == open(os.path.join(want_dir, fn), "rb").read(), fn
