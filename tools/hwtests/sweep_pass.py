#!/usr/bin/env python3
"""What filter_sweep.py's pass costs on the device (k_sweep.hip), on one MI355X, in one process, profiler off:

    python tools/hwtests/sweep_pass.py [OUT_DIR] [RUNS] [SCALE]

The seeded synthetic 40x HiFi read set of tools/hwtests/reads_pass.py (synth.simulate_reads over 120 Mb + 80 Mb, both x SCALE) as a
heads stream, resident on the device, at -mq 30 -cp 0.1 -ip 0.9.  After one untimed call each, RUNS (5) times, alternating run by run,
each between two events on the engine's stream:

  * gci_bam_sweep at K = 3 without windows: every primary record is counted,
  * the same with the ~1000 windows of 1 kb of reads_pass.py,
  * the yardstick: gci_bam_fate alone.

-> one JSON line, and OUT_DIR/sweep_pass.json."""
from __future__ import annotations

import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FILT = (30, 0.1, 0.9)
DIGITS = 3
CONTIGS = (("h1", 120_000_000), ("h2", 80_000_000))


def _timed(engine, call) -> float:
    T = engine.T
    a, b = T.Event(enable_timing=True), T.Event(enable_timing=True)
    a.record(engine.stream)
    call()
    b.record(engine.stream)
    b.synchronize()
    return a.elapsed_time(b)


def main(out: str = "", runs: int = 5, scale: float = 1.0) -> None:
    from gci_amd import _lib, pipeline, synth
    contigs = tuple((n, max(300_000, int(L * scale))) for n, L in CONTIGS)
    rs = synth.simulate_reads(contigs, 40, "hifi", seed=21).sorted()
    stream, offs = synth.to_bam_stream(rs, heads=True)
    engine = pipeline.default_engine()
    engine.set_layout([L for _, L in contigs])
    d_stream, d_off = engine.to_device(stream), engine.to_device(offs)
    d_sel = engine.to_device(np.arange(len(contigs), dtype=np.int32))
    n_rec, n_bytes = int(offs.shape[0]), int(stream.shape[0])
    lib, p = engine.lib, engine._p
    head = (engine.ctx, p(d_stream), n_bytes, p(d_off), n_rec)
    d_cls = engine.T.empty(n_rec, engine.T.uint8, engine.device)
    counts = (ctypes.c_uint64 * _lib.FATE_CLASSES)()
    per = 1000 // len(contigs)
    regions = [(n, k * (L // per), k * (L // per) + 1000) for n, L in contigs for k in range(per)]
    win, win0 = pipeline.merge_windows(regions, dict(contigs))
    d_win, d_win0 = engine.to_device(win), engine.to_device(win0)
    rows = _lib.SweepRows(DIGITS)
    tables = {w: np.zeros((rows.rows, _lib.SWEEP_COLS), dtype=np.uint64) for w in (False, True)}

    def chk(st):
        if st != 0:
            raise SystemExit("a call failed: %d" % st)

    def fate():
        chk(lib.gci_bam_fate(*head, 0, p(d_sel), len(contigs), *FILT, p(d_cls), counts, p(engine._status)))

    def sweep(windows: bool):
        chk(lib.gci_bam_sweep(*head, 0, p(d_sel), len(contigs), p(d_win) if windows else None, p(d_win0) if windows else None, *FILT, DIGITS,
                              tables[windows].ctypes.data_as(ctypes.c_void_p), p(engine._status)))

    calls = {"gci_bam_fate": fate, "gci_bam_sweep": lambda: sweep(False), "gci_bam_sweep_1000_windows": lambda: sweep(True)}
    for c in calls.values():
        c()
        engine.check_status("sweep_pass")
    engine.T.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(runs):
        for k, c in calls.items():
            ms[k].append(round(_timed(engine, c), 4))
    kept = [int(tables[False][rows.mapq0 + FILT[0]:rows.clip0, 2].sum()), int(tables[False][rows.clip0:rows.clip0 + round(FILT[1] * rows.bins) + 1, 2].sum()),
            int(tables[False][rows.iden0 + round(FILT[2] * rows.bins):rows.iden_above + 1, 2].sum())]
    if kept != [int(counts[6])] * 3:
        raise SystemExit("kept_at of the three tables %r is not gci_bam_fate's kept count %d" % (kept, int(counts[6])))
    res = {"scale": scale, "repeats": runs, "digits": DIGITS, "records": n_rec, "stream_bytes": n_bytes, "cigar_operations": int(np.diff(rs.cigar_off).sum()),
           "records_per_class": dict(zip(_lib.FATE_NAMES, [int(x) for x in counts])), "windows": int(win.shape[0]),
           "primary_records": {"no_windows": int(tables[False][:256, 0].sum()), "windows": int(tables[True][:256, 0].sum())},
           "rows_hit": {t: int((tables[False][a:b, 0] > 0).sum()) for t, a, b in (("mapq", 0, rows.clip0), ("clip", rows.clip0, rows.iden_below),
                                                                                ("identity", rows.iden_below, rows.rows))},
           "ms": ms, "ms_min_median": {k: [min(v), round(statistics.median(v), 4)] for k, v in ms.items()}}
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "sweep_pass.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "", int(sys.argv[2]) if len(sys.argv) > 2 else 5, float(sys.argv[3]) if len(sys.argv) > 3 else 1.0)
