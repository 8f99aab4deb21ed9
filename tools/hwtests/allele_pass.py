#!/usr/bin/env python3
"""What allele_sites.py costs on the device next to mismatch_sites.py (k_mismatch.hip), on one MI355X, in one
process, profiler off:

    python tools/hwtests/allele_pass.py [OUT_DIR] [RUNS] [KIND] [SCALE]

The files of tools/hwtests/mismatch_pass.py: a seeded random assembly (6 Mb + 4 Mb, both x SCALE) as FASTA, and a seeded synthetic 20x
read set over it (KIND = hifi or ont) whose reads carry the assembly's bases with a share of substituted ones (0.2 % for hifi, 4 % for
ont), written as one BGZF BAM file.  After one untimed call each, RUNS (5) times, alternating run by run, wall time with a device
synchronise inside the window:

  * pipeline.bam_mismatch_sites on the file (the yardstick: one event track and the depth),
  * pipeline.bam_allele_sites on the file (the same walk with four counts a chunk and a wave scan a step; four event tracks and the
    depth: five depth builds for two; the single-base lister over five tracks for the run lister over two).

The two must agree: A + C + G + T is the mismatch track, the depth tracks are equal, the outer counts are equal.  Three more runs of
each with the phase log on, the two alternating, give the device time of "record alleles" beside "record mismatches", of "depth build"
and of "allele sites" beside "mismatch sites".  Both walks read the same bytes and store the same number of events.

-> one JSON line, and OUT_DIR/allele_pass_KIND.json."""
from __future__ import annotations

import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONTIGS = (("h1", 6_000_000), ("h2", 4_000_000))
SUB_RATE = {"hifi": 0.002, "ont": 0.04}
STAGES = ("record mismatches", "record alleles", "record cover", "depth build", "mismatch sites", "allele sites", "fasta codes")


def _wall(engine, call) -> float:
    engine.sync()
    t0 = time.perf_counter()
    call()
    engine.sync()
    return (time.perf_counter() - t0) * 1e3


def main(out: str = "", runs: int = 5, kind: str = "hifi", scale: float = 1.0) -> None:
    from gci_amd import phases, pipeline, synth
    from gci_amd.formats import bam as bamfmt
    contigs = tuple((n, max(300_000, int(L * scale))) for n, L in CONTIGS)
    rs = synth.simulate_reads(contigs, 20, kind, seed=23).sorted()
    ref = synth.random_reference(contigs, seed=24)
    res = {"kind": kind, "scale": scale, "repeats": runs, "records": len(rs), "contigs": [L for _, L in contigs], "sub_rate": SUB_RATE[kind],
           "read_bases": int(rs.l_seq.sum())}
    engine = pipeline.default_engine()
    with tempfile.TemporaryDirectory() as d:
        path, fa = os.path.join(d, "reads.bam"), os.path.join(d, "ref.fa")
        synth.write_fasta(fa, ref)
        stream, _ = synth.to_bam_stream(rs, seq_qual="reference", reference=ref, sub_rate=SUB_RATE[kind], seed=25)
        bamfmt.write_bam_stream(path, stream, level=1, threads=16)
        res["file_bytes"], res["inflated_bytes"] = os.path.getsize(path), int(stream.shape[0])
        del stream
        kept = {}

        def mismatch():
            kept["mismatch"] = pipeline.bam_mismatch_sites(engine, fa, [path], [], None, 16)

        def allele():
            kept["allele"] = pipeline.bam_allele_sites(engine, fa, [path], [], None, 16)

        calls = {"bam_mismatch_sites": mismatch, "bam_allele_sites": allele}
        for c in calls.values():
            c()
        mm, al = kept["mismatch"], kept["allele"]
        host = lambda t: t.track.cpu().numpy()      # noqa: E731
        if not np.array_equal(sum(host(al.tracks[b]) for b in "ACGT"), host(mm.mismatch)) or not np.array_equal(host(al.depth), host(mm.depth)):
            raise SystemExit("the tracks of bam_allele_sites are not bam_mismatch_sites'")
        a, m = al.counts[0], mm.counts[0]
        if [a[0], sum(a[1:5]), a[5]] != m:
            raise SystemExit("the counts of bam_allele_sites are not bam_mismatch_sites': %r %r" % (a, m))
        res["counts"], res["sites"] = {"mismatch": m, "allele": a}, {"mismatch": int(mm.sites.shape[0]), "allele": int(al.sites.shape[0])}
        ms = {k: [] for k in calls}
        for _ in range(runs):
            for k, c in calls.items():
                ms[k].append(round(_wall(engine, c), 2))
        gpu = {k: {} for k in calls}                   # stage -> its device ms in three logged calls, the two alternating
        for _ in range(3):
            for k, c in calls.items():
                phases.start()
                c()
                log = phases.report()
                phases.stop()
                for s in STAGES:
                    if s in log["gpu_s"]:
                        gpu[k].setdefault(s, []).append(round(log["gpu_s"][s] * 1e3, 3))
        kept.clear()
    res["wall_ms"] = ms
    res["wall_ms_median_min_spread"] = {k: [round(statistics.median(v), 2), min(v), round(max(v) - min(v), 2)] for k, v in ms.items()}
    res["gpu_ms"] = gpu
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "allele_pass_%s.json" % kind), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "", int(sys.argv[2]) if len(sys.argv) > 2 else 5, sys.argv[3] if len(sys.argv) > 3 else "hifi",
         float(sys.argv[4]) if len(sys.argv) > 4 else 1.0)
