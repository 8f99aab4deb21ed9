#!/usr/bin/env python3
"""depth_to_bedgraph.py at CHM13 size, on one MI355X, in one process with the profiler off:

    python tools/measure_bedgraph.py run OUT [RUNS] [SCALE]

A seeded synthetic track over the CHM13 contig lengths (every contig x SCALE) whose run lengths are those of a 40x long-read track:
geometric with mean 205 bases, about 20 run starts per 4096 bases.  Reported, after one untimed call each, RUNS (5) times:

  * the four calls of the conversion -- gci_depth_runs_count, gci_depth_runs_write, gci_bedgraph_size, gci_bedgraph_write -- between
    two events on the engine's stream (the count and the size call end with an 8-byte read of their total, which is inside), with
    the bytes each must read and write, computed from the shapes;
  * in the same process, alternating with them run by run, gci_issue_scan_windows (depth == 0) and gci_depth_classes over the same
    whole-contig windows, and the run-to-run spread (max - min) of gci_depth_classes;
  * the whole command's wall time and phases on the file this project's writer makes of the track, and -- on a file of the smallest
    chromosome alone (chr21), which a line-by-line conversion finishes -- the command next to a plain Python/numpy conversion of the same file
    (gzip, numpy's text parser, runs by flatnonzero, lines by %-formatting): what a user would otherwise write.

-> OUT/bedgraph_runs.json."""
from __future__ import annotations

import ctypes
import gzip
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN_RUN = 205


def _contig(L: int, rng) -> np.ndarray:
    lens = rng.geometric(1.0 / MEAN_RUN, int(L / MEAN_RUN * 1.1) + 64)
    while int(lens.sum()) < L:
        lens = np.concatenate([lens, rng.geometric(1.0 / MEAN_RUN, 4096)])
    vals = np.clip(rng.normal(40, 8, lens.shape[0]), 0, 200).astype(np.int32)
    vals[1:][vals[1:] == vals[:-1]] += 1
    return np.repeat(vals, lens)[:L]


def _timed(engine, call):
    T = engine.T
    a, b = T.Event(enable_timing=True), T.Event(enable_timing=True)
    a.record(engine.stream)
    call()
    b.record(engine.stream)
    b.synchronize()
    return a.elapsed_time(b)


def _plain(path: str, out: str) -> None:
    """The conversion as a user would write it with gzip and numpy."""
    with gzip.open(path, "rb") as f, open(out, "wb") as o:
        text = f.read()
        for block in text.split(b">")[1:]:
            name, _, body = block.partition(b"\n")
            d = np.fromstring(body, dtype=np.int64, sep="\n")
            s = np.concatenate([[0], np.flatnonzero(d[1:] != d[:-1]) + 1])
            e = np.concatenate([s[1:], [d.shape[0]]])
            o.write(b"".join(b"%s\t%d\t%d\t%d\n" % (name, a, b, v) for a, b, v in zip(s.tolist(), e.tolist(), d[s].tolist())))


def _command(path: str, prefix: str, log: str):
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_to_bedgraph.py"), "-f", path, prefix], cwd=ROOT,
                       env=dict(os.environ, GCI_PHASES=log), capture_output=True, text=True)
    wall = round(time.perf_counter() - t, 3)
    if r.returncode != 0:
        raise SystemExit("the command failed: " + r.stderr[-2000:])
    return wall, {k: round(v, 4) for k, v in json.load(open(log))["wall_s"].items()}


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
    T, lib, p = engine.T, engine.lib, engine._p
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731

    def chk(st):
        if st != 0:
            raise SystemExit("a call failed: %d" % st)

    names = [nm.encode() for nm, _ in contigs]
    name_len = np.array([len(x) for x in names], dtype=np.uint32)
    name_off = np.concatenate([[0], np.cumsum(name_len[:-1])]).astype(np.uint64)
    d_names = engine.to_device(np.frombuffer(b"".join(names), dtype=np.uint8))
    coord = np.zeros(n, dtype=np.int64)
    d_run0, d_byte0 = T.empty(n + 1, T.int64, engine.device), T.empty(n + 1, T.int64, engine.device)
    chk(lib.gci_depth_runs_count(engine.ctx, p(track), wins, n, p(d_run0)))
    n_runs = int(d_run0.cpu().numpy().view(np.uint64)[n])
    d_runs = T.empty(max(n_runs, 1), T.int64, engine.device)
    chk(lib.gci_depth_runs_write(engine.ctx, p(track), p(d_runs), n_runs))
    chk(lib.gci_bedgraph_size(engine.ctx, p(d_runs), p(d_run0), wins, n, vp(coord), vp(name_len), p(d_byte0)))
    n_bytes = int(d_byte0.cpu().numpy().view(np.uint64)[n])
    d_out = T.empty(max(n_bytes, 1), T.uint8, engine.device)
    cap = 1 << 22
    keys = T.empty(2 * cap, T.int64, engine.device)
    counts = T.zeros(2, T.int32, engine.device)
    d_stats = T.zeros(2 * n, T.int64, engine.device)
    tile_bytes = sum((L + 4095) // 4096 for L in lengths) * 16384
    calls = {
        "gci_depth_runs_count": lambda: chk(lib.gci_depth_runs_count(engine.ctx, p(track), wins, n, p(d_run0))),
        "gci_depth_runs_write": lambda: chk(lib.gci_depth_runs_write(engine.ctx, p(track), p(d_runs), n_runs)),
        "gci_bedgraph_size": lambda: chk(lib.gci_bedgraph_size(engine.ctx, p(d_runs), p(d_run0), wins, n, vp(coord), vp(name_len), p(d_byte0))),
        "gci_bedgraph_write": lambda: chk(lib.gci_bedgraph_write(engine.ctx, p(d_runs), p(d_run0), wins, n, vp(coord), p(d_names), vp(name_off),
                                                                 vp(name_len), p(d_out), n_bytes)),
        "gci_issue_scan_windows": lambda: chk(lib.gci_issue_scan_windows(engine.ctx, p(track), wins, n, -1.0, 0.0, p(keys), cap, p(counts))),
        "gci_depth_classes": lambda: chk(lib.gci_depth_classes(engine.ctx, p(track), wins, n, 5, p(keys), cap, p(counts), p(d_stats))),
    }
    order = ["gci_depth_runs_count", "gci_depth_runs_write", "gci_issue_scan_windows", "gci_bedgraph_size", "gci_bedgraph_write",
             "gci_depth_classes"]                   # (a write call directly behind its count / size call: the scans set other windows)
    for k in order:
        calls[k]()
    T.synchronize()
    ms = {k: [] for k in order}
    for _ in range(runs):
        for k in order:
            ms[k].append(round(_timed(engine, calls[k]), 4))
    res = {"contigs": n, "bases": int(sum(lengths)), "scale": scale, "repeats": runs, "runs": n_runs, "text_bytes": n_bytes,
           "run_starts_per_4096_bases": round(n_runs * 4096.0 / sum(lengths), 2),
           "bytes_read_written": {"gci_depth_runs_count": [tile_bytes, tile_bytes // 16384 * 4], "gci_depth_runs_write": [tile_bytes, n_runs * 8],
                                  "gci_bedgraph_size": [n_runs * 8, (n_runs + 255) // 256 * 4], "gci_bedgraph_write": [n_runs * 8, n_bytes],
                                  "gci_issue_scan_windows": [tile_bytes, 0], "gci_depth_classes": [tile_bytes, tile_bytes // 16384 * 16]},
           "ms": ms, "ms_min_median": {k: [min(v), round(statistics.median(v), 4)] for k, v in ms.items()},
           "depth_classes_spread_ms": round(max(ms["gci_depth_classes"]) - min(ms["gci_depth_classes"]), 4)}
    del d_runs, d_out, keys, d_stats

    # the whole command on the file this project's writer makes of the track; then the smallest contig alone, next to the plain conversion
    tracks = pipeline.DepthTracks(engine, dict(contigs), track)
    pipeline.write_depth(out, "genome", tracks)
    small = min(range(n), key=lambda c: (lengths[c] < 10_000_000 * scale, lengths[c]))      # (chr21; not the 16 kb chrM)
    o, L = engine.offsets[small], lengths[small]
    one = host[o:o + L].copy()
    del tracks, track, host
    engine.set_layout([L])
    pipeline.write_depth(out, "small", pipeline.DepthTracks(engine, {contigs[small][0]: L}, engine.to_device(np.concatenate([one, np.zeros(engine.total - L, np.int32)]))))
    genome, small_gz = os.path.join(out, "genome.depth.gz"), os.path.join(out, "small.depth.gz")
    res["file_bytes"] = os.path.getsize(genome)
    res["command_wall_s"], res["command_phases_s"] = _command(genome, os.path.join(out, "genome"), os.path.join(out, "phases.json"))
    res["bedgraph_file_bytes"] = os.path.getsize(os.path.join(out, "genome.bedgraph"))
    os.remove(os.path.join(out, "genome.bedgraph"))
    os.remove(genome)
    res["small_bases"] = L
    res["small_command_wall_s"], res["small_command_phases_s"] = _command(small_gz, os.path.join(out, "small"), os.path.join(out, "phases_small.json"))
    t = time.perf_counter()
    _plain(small_gz, os.path.join(out, "small_plain.bedgraph"))
    res["small_plain_numpy_wall_s"] = round(time.perf_counter() - t, 3)
    res["small_outputs_equal"] = open(os.path.join(out, "small.bedgraph"), "rb").read() == open(os.path.join(out, "small_plain.bedgraph"), "rb").read()
    for fn in ("small.bedgraph", "small_plain.bedgraph", "small.depth.gz"):
        os.remove(os.path.join(out, fn))
    with open(os.path.join(out, "bedgraph_runs.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "run":
        raise SystemExit(__doc__)
    run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5, float(sys.argv[4]) if len(sys.argv) > 4 else 1.0)
