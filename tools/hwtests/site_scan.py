"""The site scan alone, at the size of a genome: what clips_pass.py, indels_pass.py and mismatch_pass.py share.  A *_sites_size call
and its *_sites_write call between two events on the engine's stream, after one untimed call each."""
from __future__ import annotations

import statistics


def timed(engine, call) -> float:
    T = engine.T
    a, b = T.Event(enable_timing=True), T.Event(enable_timing=True)
    a.record(engine.stream)
    call()
    b.record(engine.stream)
    b.synchronize()
    return a.elapsed_time(b)


def scan_alone(engine, runs: int, size, write, n_sites, tracks_read: int) -> dict:
    """size / write: the two calls, already made once; n_sites(): what the size call found; tracks_read: the tracks the size pass reads."""
    ms = {"size": [], "write": []}
    for _ in range(max(runs, 5)):
        ms["size"].append(round(timed(engine, size), 4))
        ms["write"].append(round(timed(engine, write), 4))
    read_bytes = tracks_read * 4 * int(engine.total)
    return {"elements": int(engine.total), "sites": int(n_sites()), "ms": ms,
            "ms_min_median": {k: [min(v), round(statistics.median(v), 4)] for k, v in ms.items()},
            "size_pass_bytes": read_bytes, "size_pass_GB_per_s": round(read_bytes / (statistics.median(ms["size"]) * 1e-3) / 1e9, 1)}
