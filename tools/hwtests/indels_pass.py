#!/usr/bin/env python3
"""What indel_sites.py costs on the device next to bam_depth.py and clip_sites.py (k_indels.hip), on one MI355X,
in one process, profiler off:

    python tools/hwtests/indels_pass.py [OUT_DIR] [RUNS] [SCALE] [SCAN_MB]

The seeded synthetic 20x HiFi read set of clips_pass.py (synth.simulate_reads over 30 Mb + 20 Mb, both x SCALE) written as one BGZF
BAM file.  After one untimed call each, RUNS (5) times, alternating run by run, wall time with a device synchronise inside the window:

  * pipeline.bam_raw_depth on the file (the yardstick: the cover pass and one depth build),
  * pipeline.bam_clip_sites on the file (the cover pass, the clip pass, three depth builds, the site scan),
  * pipeline.bam_indel_sites on the file (the cover pass, the indel pass, three depth builds, the site scan) at the default -l 50, at
    which a synthetic HiFi read set holds no event, and at -l 1, at which every D and I operation is one.

The depth tracks of all three must be equal.  Then the site scan alone over three zeroed tracks of SCAN_MB (3000) million bases with
a dozen planted runs, between two events on the engine's stream: gci_indel_sites_size (reads the del and ins tracks) and
gci_indel_sites_write (the run starts, then a wave per site), with the bytes over time of the size pass.

-> one JSON line, and OUT_DIR/indels_pass.json."""
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

CONTIGS = (("h1", 30_000_000), ("h2", 20_000_000))
RUN_LENGTHS = (1, 63, 64, 65, 200, 9000)               # planted twice: in the del track, in the ins track


def _wall(engine, call) -> float:
    engine.sync()
    t0 = time.perf_counter()
    call()
    engine.sync()
    return (time.perf_counter() - t0) * 1e3


def main(out: str = "", runs: int = 5, scale: float = 1.0, scan_mb: int = 3000) -> None:
    from gci_amd import pipeline, synth
    contigs = tuple((n, max(300_000, int(L * scale))) for n, L in CONTIGS)
    rs = synth.simulate_reads(contigs, 20, "hifi", seed=23).sorted()
    engine = pipeline.default_engine()
    res = {"scale": scale, "repeats": runs, "records": len(rs), "contigs": [L for _, L in contigs]}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.bam")
        synth.write_bam_file(path, rs, level=1, threads=16)
        res["file_bytes"] = os.path.getsize(path)
        kept = {}

        def raw():
            kept["raw"] = pipeline.bam_raw_depth(engine, [path], [], None, 16)

        def clips():
            kept["clips"] = pipeline.bam_clip_sites(engine, [path], [], None, 16)

        def indels():
            kept["indels"] = pipeline.bam_indel_sites(engine, [path], [], None, 16)

        def indels_l1():
            kept["indels_l1"] = pipeline.bam_indel_sites(engine, [path], [], None, 16, 1, pipeline.INDEL_MIN_READS)

        calls = {"bam_raw_depth": raw, "bam_clip_sites": clips, "bam_indel_sites": indels, "bam_indel_sites_l1": indels_l1}
        for c in calls.values():
            c()
        depth = kept["raw"].track.cpu().numpy()
        if not (np.array_equal(depth, kept["clips"].depth.track.cpu().numpy()) and np.array_equal(depth, kept["indels"].depth.track.cpu().numpy())):
            raise SystemExit("the depth tracks of bam_clip_sites and bam_indel_sites are not bam_raw_depth's")
        res["counts"], res["sites"] = kept["indels"].counts, int(kept["indels"].sites.shape[0])
        res["counts_min_len_1"], res["sites_min_len_1"] = kept["indels_l1"].counts, int(kept["indels_l1"].sites.shape[0])
        del depth
        ms = {k: [] for k in calls}
        for _ in range(runs):
            for k, c in calls.items():
                ms[k].append(round(_wall(engine, c), 2))
        kept.clear()
    res["wall_ms"] = ms
    res["wall_ms_min_median"] = {k: [min(v), round(statistics.median(v), 2)] for k, v in ms.items()}
    # the site scan alone, at the size of a genome
    half = scan_mb * 1_000_000 // 2
    engine.set_layout([half, half])
    tracks = [engine.new_track() for _ in range(3)]
    for t in tracks:
        t.zero_()
    step = int(engine.total) // (len(RUN_LENGTHS) + 1) // 4096 * 4096
    for k, n in enumerate(RUN_LENGTHS):
        plant = engine.to_device(np.full(n, 3 + k, dtype=np.int32))
        at = (k + 1) * step - n // 2                   # (the longer runs lie across a tile's edge)
        tracks[0][at:at + n].copy_(plant)
        tracks[1][at + 20000:at + 20000 + n].copy_(plant)
    lib, p = engine.lib, engine._p
    n = ctypes.c_uint64(0)
    out_buf = engine.T.empty((64, 6), engine.T.int32, engine.device)
    head = (engine.ctx, p(tracks[0]), p(tracks[1]), p(tracks[2]), 3, None, 0)

    def size():
        if lib.gci_indel_sites_size(*head, ctypes.byref(n)) != 0:
            raise SystemExit("gci_indel_sites_size failed")

    def write():
        if lib.gci_indel_sites_write(*head, p(out_buf), 64) != 0:
            raise SystemExit("gci_indel_sites_write failed")

    size()
    write()
    engine.sync()
    got = out_buf.cpu().numpy()[:int(n.value)]
    if int(n.value) != 2 * len(RUN_LENGTHS) or sorted((got[:, 2] - got[:, 1]).tolist()) != sorted(2 * list(RUN_LENGTHS)):
        raise SystemExit("the planted runs were not found: %r" % got.tolist())
    res["scan"] = scan_alone(engine, runs, size, write, lambda: n.value, 2)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "indels_pass.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "", int(sys.argv[2]) if len(sys.argv) > 2 else 5, float(sys.argv[3]) if len(sys.argv) > 3 else 1.0,
         int(sys.argv[4]) if len(sys.argv) > 4 else 3000)
