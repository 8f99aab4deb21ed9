#!/usr/bin/env python3
"""depth_plotter_v2.py at CHM13 size ("depth_plotter_v2.py"), on one MI355X, in one process with the profiler off, over
the files `python tools/measure_score.py make DIR [SCALE]` wrote:

    python tools/measure_plotter_v2.py run DIR OUT [RUNS]

  * the device time of gci_depth_classes over all contigs (one window per contig), between two events on the engine's stream;
  * for comparison the calls that give the same numbers without it: gci_issue_scan_windows twice (depth == 0, 0 < depth < 5) plus
    gci_range_sums over the same windows (one wave per window: what that export is built for is millions of short ranges), and --
    the kinder comparison -- gci_depth_sum in its place;
  * the phases of the whole command for `--region <first contig, whole> -w 50000 -f png` with both files.

min / median of RUNS (5) timed calls after one untimed call each -> OUT/plotter_v2_runs.json."""
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


def _timed(engine, call, runs: int):
    """-> (min, median) device milliseconds of call() between two events on the engine's stream."""
    T = engine.T
    call()
    T.synchronize()
    ms = []
    for _ in range(runs):
        a, b = T.Event(enable_timing=True), T.Event(enable_timing=True)
        a.record(engine.stream)
        call()
        b.record(engine.stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(min(ms), 4), round(statistics.median(ms), 4)


def run(d: str, out: str, runs: int = 5) -> None:
    from gci_amd import pipeline
    from gci_amd._lib import Window
    os.makedirs(out, exist_ok=True)
    engine = pipeline.default_engine()
    tracks, lengths = pipeline.read_depth_tracks(engine, os.path.join(d, "hifi.depth.gz"), None, plotter_v2=True)
    tracks._bind()
    n = len(lengths)
    res = {"contigs": n, "bases": int(sum(lengths.values())), "runs": runs}
    wins = (Window * n)()
    for c, (o, L) in enumerate(zip(engine.offsets, tracks.lengths)):
        wins[c].begin, wins[c].end = int(o), int(o) + int(L)
    zero, low, stats = engine.depth_classes(tracks.track, [(w.begin, w.end) for w in wins], 5)
    cap = 2 * max(sum(z.shape[0] for z in zero), sum(z.shape[0] for z in low), 1)          # every key fits: one launch per call
    res["zero_runs"], res["low_runs"] = int(sum(z.shape[0] for z in zero)), int(sum(z.shape[0] for z in low))
    T, lib, p = engine.T, engine.lib, engine._p
    keys = T.empty(2 * cap, T.int64, engine.device)
    counts = T.zeros(2, T.int32, engine.device)
    d_stats = T.zeros(2 * n, T.int64, engine.device)
    d_sums = T.zeros(n, T.int64, engine.device)
    ranges = engine.to_device(np.array([(w.begin, w.end) for w in wins], dtype=np.int64))

    def chk(st):
        if st != 0:
            raise SystemExit("a call failed: %d" % st)

    res["gci_depth_classes_ms_min_median"] = _timed(engine, lambda: chk(lib.gci_depth_classes(
        engine.ctx, p(tracks.track), wins, n, 5, p(keys), cap, p(counts), p(d_stats))), runs)
    got = d_stats.cpu().numpy()[:2 * n].reshape(n, 2)
    res["scan_zero_ms_min_median"] = _timed(engine, lambda: chk(lib.gci_issue_scan_windows(
        engine.ctx, p(tracks.track), wins, n, -1.0, 0.0, p(keys), cap, p(counts))), runs)
    res["scan_low_ms_min_median"] = _timed(engine, lambda: chk(lib.gci_issue_scan_windows(
        engine.ctx, p(tracks.track), wins, n, 0.0, 4.0, p(keys), cap, p(counts))), runs)
    res["range_sums_same_windows_ms_min_median"] = _timed(engine, lambda: chk(lib.gci_range_sums(
        engine.ctx, p(tracks.track), p(ranges), n, p(d_sums))), runs)
    assert np.array_equal(d_sums.cpu().numpy()[:n], got[:, 0]), "the window sums differ"   # (no depth is negative)
    res["depth_sum_ms_min_median"] = _timed(engine, lambda: chk(lib.gci_depth_sum(engine.ctx, p(tracks.track), p(d_sums))), runs)
    assert np.array_equal(d_sums.cpu().numpy()[:n], got[:, 0]), "the contig sums differ"
    for k in (0, 1):
        three = res["scan_zero_ms_min_median"][k] + res["scan_low_ms_min_median"][k]
        res["three_calls_with_range_sums_ms_" + ("min", "median")[k]] = round(three + res["range_sums_same_windows_ms_min_median"][k], 4)
        res["three_calls_with_depth_sum_ms_" + ("min", "median")[k]] = round(three + res["depth_sum_ms_min_median"][k], 4)
    del tracks, keys, d_stats, d_sums, ranges

    # the whole command, one region: the first contig, whole
    name, L = next(iter(lengths.items()))
    fai = os.path.join(out, "ref.fai")
    with open(fai, "w") as f:
        for nm, ln in lengths.items():
            f.write("%s\t%d\n" % (nm, ln))
    ph = os.path.join(out, "plotter_v2_phases.json")
    cmd = [sys.executable, os.path.join(ROOT, "depth_plotter_v2.py"), "-r", fai, "--hifi", os.path.join(d, "hifi.depth.gz"),
           "--nano", os.path.join(d, "nano.depth.gz"), "--region", "%s:0-%d" % (name, L - 1), "-w", "50000", "-f", "png",
           "-o", os.path.join(out, "images")]
    t = time.perf_counter()
    with open(os.path.join(out, "plotter_v2_command.log"), "w") as f:
        r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, GCI_PHASES=ph), stdout=f, stderr=subprocess.STDOUT)
    res["command_wall_s"] = round(time.perf_counter() - t, 3)
    res["command_exit"] = r.returncode
    if r.returncode == 0:
        log = json.load(open(ph))
        res["command_phases_s"] = {k: round(v, 4) for k, v in log["wall_s"].items()}
        res["command_path"] = log["notes"].get("plotter_v2")
        res["command_depth_read"] = {os.path.basename(k): v for k, v in log["notes"].items() if k.startswith("depth_read:")}
    with open(os.path.join(out, "plotter_v2_runs.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) < 4 or sys.argv[1] != "run":
        raise SystemExit(__doc__)
    run(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 5)
