#!/usr/bin/env python3
"""depth_dist.py at CHM13 size, on one MI355X, in one process with the profiler off:

    python tools/measure_hist.py run OUT [RUNS] [SCALE]

The track of tools/measure_bedgraph.py: seeded, over the CHM13 contig lengths (every contig x SCALE), run lengths geometric with mean
205 bases (about 20 run starts per 4096 bases), the 25 contigs whole as windows.  Reported, after one untimed call each, RUNS (5)
times, alternating run by run in ONE process, each between two events on the engine's stream:

  * gci_depth_hist with n_bins = 0 (the statistics-only round of pipeline.depth_distribution),
  * gci_depth_hist at the n_bins the data asks for (largest depth + 1),
  * gci_depth_classes over the same windows: the yardstick, one int4 read of the same bytes with per-base integer work;
  * then, on a track of 2^30 alternating 0 / 1 depths in one window -- no runs, one LDS add per base: the worst case, reported as
    such --, the same three calls;
  * the whole command's wall time and phases on the file this project's writer makes of the genome-size track.

-> OUT/hist_runs.json."""
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

from measure_bedgraph import _contig, _timed  # noqa: E402


def _three_calls(engine, track, wins, n, runs):
    """-> (n_bins, ms per call, the histogram and statistics of the last call)."""
    from gci_amd import _lib
    T, lib, p = engine.T, engine.lib, engine._p

    def chk(st):
        if st != 0:
            raise SystemExit("a call failed: %d" % st)

    d_stats = T.empty(4 * n, T.int64, engine.device)
    d_over = T.empty(2 * n, T.int64, engine.device)
    chk(lib.gci_depth_hist(engine.ctx, p(track), wins, n, 0, p(d_over), p(d_stats)))
    top = int(d_stats.cpu().numpy().reshape(n, 4)[:, 2].max())
    n_bins = max(1, min(top + 1, _lib.HIST_MAX_BINS))
    d_hist = T.empty(n * (n_bins + 2), T.int64, engine.device)
    cap = 1 << 22
    keys = T.empty(2 * cap, T.int64, engine.device)
    counts = T.zeros(2, T.int32, engine.device)
    d_cstats = T.zeros(2 * n, T.int64, engine.device)
    calls = {
        "gci_depth_hist_stats_only": lambda: chk(lib.gci_depth_hist(engine.ctx, p(track), wins, n, 0, p(d_over), p(d_stats))),
        "gci_depth_hist": lambda: chk(lib.gci_depth_hist(engine.ctx, p(track), wins, n, n_bins, p(d_hist), p(d_stats))),
        "gci_depth_classes": lambda: chk(lib.gci_depth_classes(engine.ctx, p(track), wins, n, 5, p(keys), cap, p(counts), p(d_cstats))),
    }
    order = ["gci_depth_hist_stats_only", "gci_depth_hist", "gci_depth_classes"]
    for k in order:
        calls[k]()
    T.synchronize()
    ms = {k: [] for k in order}
    for _ in range(runs):
        for k in order:
            ms[k].append(round(_timed(engine, calls[k]), 4))
    calls["gci_depth_hist"]()
    hist = d_hist.cpu().numpy().view(np.uint64).reshape(n, n_bins + 2)
    return n_bins, ms, hist, d_stats.cpu().numpy().reshape(n, 4)


def _summary(ms):
    out = {"ms": ms, "ms_min_median": {k: [min(v), round(statistics.median(v), 4)] for k, v in ms.items()}}
    ref = statistics.median(ms["gci_depth_classes"])
    out["median_over_depth_classes"] = {k: round(statistics.median(v) / ref, 3) for k, v in ms.items()}
    out["depth_classes_spread_ms"] = round(max(ms["gci_depth_classes"]) - min(ms["gci_depth_classes"]), 4)
    return out


def run(out: str, runs: int = 5, scale: float = 1.0) -> None:
    from gci_amd import pipeline, synth
    from gci_amd._lib import Window
    os.makedirs(out, exist_ok=True)
    engine = pipeline.default_engine()
    contigs = [(n, max(10_000, int(L * scale))) for n, L in synth.CHM13]
    lengths = [L for _, L in contigs]
    engine.set_layout(lengths)
    rng = np.random.default_rng(12)
    host = np.zeros(engine.total, dtype=np.int32)
    for o, L in zip(engine.offsets, lengths):
        host[o:o + L] = _contig(L, rng)
    track = engine.upload_staged(host).view(engine.T.int32)
    n = len(lengths)
    wins = (Window * n)()
    for c, (o, L) in enumerate(zip(engine.offsets, lengths)):
        wins[c].begin, wins[c].end = int(o), int(o) + int(L)
    n_bins, ms, hist, stats = _three_calls(engine, track, wins, n, runs)
    small = min(range(n), key=lambda c: (lengths[c] < 10_000_000 * scale, lengths[c]))      # (chr21; not the 16 kb chrM)
    seg = host[engine.offsets[small]:engine.offsets[small] + lengths[small]]
    tile_bytes = sum((L + 4095) // 4096 for L in lengths) * 16384
    res = {"contigs": n, "bases": int(sum(lengths)), "scale": scale, "repeats": runs, "n_bins": n_bins, "bytes_read": tile_bytes,
           "workgroups": int(sum(((L + 4095) // 4096 + 63) // 64 for L in lengths)),
           "every_base_counted_once": bool((hist.sum(axis=1) == np.asarray(lengths, dtype=np.uint64)).all()),
           "one_contig_equals_numpy": bool(np.array_equal(hist[small, :n_bins], np.bincount(seg, minlength=n_bins).astype(np.uint64))
                                           and stats[small].tolist() == [int(seg.sum(dtype=np.int64)), int(seg.min()), int(seg.max()), int(seg.shape[0])])}
    res.update(_summary(ms))

    # the whole command on the file this project's writer makes of the track
    tracks = pipeline.DepthTracks(engine, dict(contigs), track)
    pipeline.write_depth(out, "genome", tracks)
    del tracks, track, host, seg
    genome, log = os.path.join(out, "genome.depth.gz"), os.path.join(out, "phases.json")
    res["file_bytes"] = os.path.getsize(genome)
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_dist.py"), "-f", genome, os.path.join(out, "genome")], cwd=ROOT,
                       env=dict(os.environ, GCI_PHASES=log), capture_output=True, text=True)
    res["command_wall_s"] = round(time.perf_counter() - t, 3)
    if r.returncode != 0:
        raise SystemExit("the command failed: " + r.stderr[-2000:])
    res["command_phases_s"] = {k: round(v, 4) for k, v in json.load(open(log))["wall_s"].items()}
    res["command_total_row"] = open(os.path.join(out, "genome.depth.summary.txt")).read().split("\n")[-2]
    os.remove(genome)

    # the worst case: no runs at all, one LDS add per base (2^30 bases x scale, one window)
    L = max(10_000, int((1 << 30) * scale))
    engine.set_layout([L])
    alt = np.zeros(engine.total, dtype=np.int32)
    alt[:L] = np.arange(L, dtype=np.int32) & 1
    d_alt = engine.upload_staged(alt).view(engine.T.int32)
    one = (Window * 1)()
    one[0].begin, one[0].end = 0, L
    nb, ms, hist, stats = _three_calls(engine, d_alt, one, 1, runs)
    worst = {"bases": L, "n_bins": nb, "exact": hist[0].tolist() == [(L + 1) // 2, L // 2, 0, 0] and stats[0].tolist() == [L // 2, 0, 1, L]}
    worst.update(_summary(ms))
    res["alternating_worst_case"] = worst
    with open(os.path.join(out, "hist_runs.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "run":
        raise SystemExit(__doc__)
    run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5, float(sys.argv[4]) if len(sys.argv) > 4 else 1.0)
