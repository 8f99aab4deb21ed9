#!/usr/bin/env python3
"""What mismatch_sites.py costs on the device next to bam_depth.py (k_mismatch.hip), on one MI355X, in one process,
profiler off:

    python tools/hwtests/mismatch_pass.py [OUT_DIR] [RUNS] [KIND] [SCALE] [SCAN_MB]

A seeded random assembly (6 Mb + 4 Mb, both x SCALE) as FASTA, and a seeded synthetic 20x read set over it (synth.simulate_reads, KIND =
hifi or ont: 200 Mb of read bases at SCALE 1) whose reads carry the assembly's bases with a share of substituted ones (0.2 % for hifi,
4 % for ont), written as one BGZF BAM file.  After one untimed call each, RUNS (5) times, alternating run by run, wall time with a
device synchronise inside the window:

  * pipeline.bam_raw_depth on the file (the yardstick: the cover pass and one depth build),
  * pipeline.bam_mismatch_sites on the file (the FASTA upload and gci_fasta_codes, the cover pass, the mismatch pass, two depth builds,
    the site scan).

The depth tracks of both must be equal.  One more run of bam_mismatch_sites with the phase log on gives the device time of the
"record mismatches" stage (gci_bam_mismatch_size + _write: the walk twice) and of "fasta codes" alone, next to the bytes they must
move: the SEQ bytes and one code byte per compared pair, twice, plus 16 B per event; one byte of FASTA text and one code byte per base.

Then the site scan alone over a mismatch and a depth track of SCAN_MB (3000) million bases with a handful of planted runs
(tools/hwtests/site_scan.py): gci_mismatch_sites_size (reads both tracks) and gci_mismatch_sites_write.

-> one JSON line, and OUT_DIR/mismatch_pass_KIND.json."""
from __future__ import annotations

import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from site_scan import scan_alone  # noqa: E402

CONTIGS = (("h1", 6_000_000), ("h2", 4_000_000))
SUB_RATE = {"hifi": 0.002, "ont": 0.04}
RUN_LENGTHS = (1, 63, 64, 65, 9000)                    # the planted runs of the site scan


def _wall(engine, call) -> float:
    engine.sync()
    t0 = time.perf_counter()
    call()
    engine.sync()
    return (time.perf_counter() - t0) * 1e3


def main(out: str = "", runs: int = 5, kind: str = "hifi", scale: float = 1.0, scan_mb: int = 3000) -> None:
    from gci_amd import phases, pipeline, synth
    from gci_amd.formats import bam as bamfmt
    contigs = tuple((n, max(300_000, int(L * scale))) for n, L in CONTIGS)
    rs = synth.simulate_reads(contigs, 20, kind, seed=23).sorted()
    ref = synth.random_reference(contigs, seed=24)
    n_ops = np.diff(rs.cigar_off)
    res = {"kind": kind, "scale": scale, "repeats": runs, "records": len(rs), "contigs": [L for _, L in contigs], "sub_rate": SUB_RATE[kind],
           "read_bases": int(rs.l_seq.sum()), "operations": int(n_ops.sum()),
           "bases_per_match_operation": round(float((rs.cigar >> 4)[np.isin(rs.cigar & 0xF, (0, 7, 8))].mean()), 1)}
    engine = pipeline.default_engine()
    with tempfile.TemporaryDirectory() as d:
        path, fa = os.path.join(d, "reads.bam"), os.path.join(d, "ref.fa")
        synth.write_fasta(fa, ref)
        stream, _ = synth.to_bam_stream(rs, seq_qual="reference", reference=ref, sub_rate=SUB_RATE[kind], seed=25)
        bamfmt.write_bam_stream(path, stream, level=1, threads=16)
        res["file_bytes"], res["inflated_bytes"], res["fasta_bytes"] = os.path.getsize(path), int(stream.shape[0]), os.path.getsize(fa)
        del stream
        kept = {}

        def raw():
            kept["raw"] = pipeline.bam_raw_depth(engine, [path], [], None, 16)

        def mismatch():
            kept["mismatch"] = pipeline.bam_mismatch_sites(engine, fa, [path], [], None, 16)

        calls = {"bam_raw_depth": raw, "bam_mismatch_sites": mismatch}
        for c in calls.values():
            c()
        if not np.array_equal(kept["raw"].track.cpu().numpy(), kept["mismatch"].depth.track.cpu().numpy()):
            raise SystemExit("the depth track of bam_mismatch_sites is not bam_raw_depth's")
        counts = kept["mismatch"].counts[0]
        res["counts"], res["sites"] = counts, int(kept["mismatch"].sites.shape[0])
        ms = {k: [] for k in calls}
        for _ in range(runs):
            for k, c in calls.items():
                ms[k].append(round(_wall(engine, c), 2))
        phases.start()
        mismatch()
        log = phases.report()
        phases.stop()
        kept.clear()
    res["wall_ms"] = ms
    res["wall_ms_min_median"] = {k: [min(v), round(statistics.median(v), 2)] for k, v in ms.items()}
    res["gpu_ms"] = {k: round(v * 1e3, 3) for k, v in log["gpu_s"].items()}
    # what the two walks (count, write) must move: the SEQ nibbles and the code bytes of the compared pairs, each twice; 16 B per event
    walk_bytes = 2 * (counts[2] // 2 + counts[2]) + 16 * counts[1]
    walk_ms = res["gpu_ms"].get("record mismatches", 0.0)
    res["walk"] = {"bytes": int(walk_bytes), "ms": walk_ms, "GB_per_s": round(walk_bytes / (walk_ms * 1e-3) / 1e9, 1) if walk_ms else None,
                   "ns_per_compared_base": round(walk_ms * 1e6 / max(counts[2], 1), 4)}
    codes_bytes = res["fasta_bytes"] + sum(L for _, L in contigs)
    codes_ms = res["gpu_ms"].get("fasta codes", 0.0)
    res["codes"] = {"bytes": int(codes_bytes), "ms_with_upload": codes_ms}
    # the site scan alone, at the size of a genome
    half = scan_mb * 1_000_000 // 2
    engine.set_layout([half, half])
    mm, depth = engine.new_track(), engine.new_track()
    mm.zero_()
    depth.zero_()                                      # (depth 0: every base with 3 mismatches is hot)
    step = int(engine.total) // (len(RUN_LENGTHS) + 1) // 4096 * 4096
    for k, n in enumerate(RUN_LENGTHS):
        at = (k + 1) * step - n // 2                   # (the longer runs lie across a tile's edge)
        mm[at:at + n].copy_(engine.to_device(np.full(n, 5 + k, dtype=np.int32)))
    lib, p = engine.lib, engine._p
    n_sites = ctypes.c_uint64(0)
    out_buf = engine.T.empty((64, 5), engine.T.int32, engine.device)
    head = (engine.ctx, p(mm), p(depth), 3, 500000, None, 0)

    def size():
        if lib.gci_mismatch_sites_size(*head, ctypes.byref(n_sites)) != 0:
            raise SystemExit("gci_mismatch_sites_size failed")

    def write():
        if lib.gci_mismatch_sites_write(*head, p(out_buf), 64) != 0:
            raise SystemExit("gci_mismatch_sites_write failed")

    size()
    write()
    engine.sync()
    got = out_buf.cpu().numpy()[:int(n_sites.value)]
    if sorted((got[:, 2] - got[:, 1]).tolist()) != sorted(RUN_LENGTHS):
        raise SystemExit("the planted runs were not found: %r" % got.tolist())
    res["scan"] = scan_alone(engine, runs, size, write, lambda: n_sites.value, 2)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "mismatch_pass_%s.json" % kind), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "", int(sys.argv[2]) if len(sys.argv) > 2 else 5, sys.argv[3] if len(sys.argv) > 3 else "hifi",
         float(sys.argv[4]) if len(sys.argv) > 4 else 1.0, int(sys.argv[5]) if len(sys.argv) > 5 else 3000)
