#!/usr/bin/env python3
"""bam_depth.py's kernels (k_cover.hip), on one MI355X, in one process with the profiler off:

    python tools/measure_cover.py run OUT [RUNS] [SCALE]

Two seeded synth read sets as HEADS streams (what a host holds of a genome-scale file): HiFi, 200 Mb x 30, and ONT, 40 Mb x 15 (both x
SCALE).  Reported per stream, after one untimed call each, RUNS (5) times, alternating run by run, each between two events on the
engine's stream:

  * gci_bam_cover_size, gci_bam_cover_write and the pair,
  * against the bytes the pair must read (36-byte cores + CIGAR words) and write (16 B per interval),
  * record pages + gci_bam_filter_pages over the same stream: the yardstick -- unchanged code that reads the same CIGAR bytes;
  * then the whole command's wall time and phases on the ONT set written as a BAM file (the largest this tool makes).

-> OUT/cover_runs.json."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_bedgraph import _timed  # noqa: E402

SETS = {"hifi": dict(contigs=(("h1", 120_000_000), ("h2", 80_000_000)), coverage=30, seed=21),
        "ont": dict(contigs=(("o1", 25_000_000), ("o2", 15_000_000)), coverage=15, seed=22)}


def _read_set(kind: str, scale: float):
    from gci_amd import synth
    s = SETS[kind]
    contigs = tuple((n, max(300_000, int(L * scale))) for n, L in s["contigs"])
    return contigs, synth.simulate_reads(contigs, s["coverage"], kind, seed=s["seed"]).sorted()


def _one_stream(engine, kind: str, contigs, rs, runs: int) -> dict:
    import ctypes
    from gci_amd import synth
    stream, offs = synth.to_bam_stream(rs, heads=True)
    n_ops = int(np.diff(rs.cigar_off).sum())
    engine.set_layout([L for _, L in contigs])
    d_stream, d_off = engine.to_device(stream), engine.to_device(offs)
    d_sel = engine.to_device(np.arange(len(contigs), dtype=np.int32))
    n_rec, n_bytes = int(offs.shape[0]), int(stream.shape[0])
    lib, p = engine.lib, engine._p
    n_ivl = ctypes.c_uint64(0)

    def chk(st):
        if st != 0:
            raise SystemExit("a call failed: %d" % st)

    def size():
        chk(lib.gci_bam_cover_size(engine.ctx, p(d_stream), n_bytes, p(d_off), n_rec, 0, p(d_sel), len(contigs), 0x704, 0, 0,
                                   ctypes.byref(n_ivl), p(engine._status)))

    size()
    engine.check_status("gci_bam_cover_size")
    out = engine.T.empty((max(int(n_ivl.value), 1), 4), engine.T.int32, engine.device)

    def write():
        chk(lib.gci_bam_cover_write(engine.ctx, p(d_stream), n_bytes, p(d_off), n_rec, 0, p(out), int(n_ivl.value), p(engine._status)))

    def pair():
        size()
        write()

    def yardstick():
        pages = engine.bam_pages(d_stream, d_off, False)
        engine.bam_filter_pages(pages, d_sel, 30, 50, 0.1, 0.9, check=False)

    calls = {"gci_bam_cover_size": size, "gci_bam_cover_write": write, "cover_pair": pair, "record_pages+gci_bam_filter_pages": yardstick}
    for c in calls.values():
        c()
    engine.T.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(runs):
        for k, c in calls.items():
            ms[k].append(round(_timed(engine, c), 4))
    track = engine.new_track()
    engine.depth_build(out[:int(n_ivl.value)], None, 0, track)
    covered = int(engine.depth_sum(track).sum())
    totals = rs.op_totals()                            # (the reads lie inside their contigs: every M, = and X base of a kept record counts)
    expected = int((totals[:, 0] + totals[:, 7] + totals[:, 8])[(rs.flag & 0x704) == 0].sum())
    med = {k: statistics.median(v) for k, v in ms.items()}
    read_bytes, write_bytes = 36 * n_rec + 4 * n_ops, 16 * int(n_ivl.value)
    return {"records": n_rec, "stream_bytes": n_bytes, "cigar_operations": n_ops, "intervals": int(n_ivl.value),
            "chunks": int(sum((int(x) + 2047) // 2048 for x in np.diff(rs.cigar_off))),
            "covered_bases": covered, "covered_bases_expected": expected,
            "bytes_read": read_bytes, "bytes_written": write_bytes, "ms": ms,
            "ms_min_median": {k: [min(v), round(med[k], 4)] for k, v in ms.items()},
            "pair_GB_per_s": round((read_bytes + write_bytes) / med["cover_pair"] / 1e6, 2),
            "pair_over_yardstick": round(med["cover_pair"] / med["record_pages+gci_bam_filter_pages"], 3),
            "yardstick_spread_ms": round(max(ms["record_pages+gci_bam_filter_pages"]) - min(ms["record_pages+gci_bam_filter_pages"]), 4)}


def run(out: str, runs: int = 5, scale: float = 1.0) -> None:
    from gci_amd import pipeline, synth
    os.makedirs(out, exist_ok=True)
    sets = {kind: _read_set(kind, scale) for kind in SETS}
    engine = pipeline.default_engine()
    res = {"scale": scale, "repeats": runs, "streams": {}}
    for kind, (contigs, rs) in sets.items():
        res["streams"][kind] = _one_stream(engine, kind, contigs, rs, runs)
    # the whole command on the ONT set as a BAM file
    contigs, rs = sets["ont"]
    bam, log = os.path.join(out, "ont.bam"), os.path.join(out, "phases.json")
    synth.write_bam_file(bam, rs, threads=8)
    res["command_file_bytes"] = os.path.getsize(bam)
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bam_depth.py"), "-f", "-d", out, "-o", "ont_raw", bam], cwd=ROOT,
                       env=dict(os.environ, GCI_PHASES=log), capture_output=True, text=True)
    res["command_wall_s"] = round(time.perf_counter() - t, 3)
    if r.returncode != 0:
        raise SystemExit("the command failed: " + r.stderr[-2000:])
    res["command_phases_s"] = {k: round(v, 4) for k, v in json.load(open(log))["wall_s"].items()}
    for f in (bam, bam + ".bai", os.path.join(out, "ont_raw.depth.gz")):
        if os.path.exists(f):
            os.remove(f)
    with open(os.path.join(out, "cover_runs.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "run":
        raise SystemExit(__doc__)
    run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5, float(sys.argv[4]) if len(sys.argv) > 4 else 1.0)
