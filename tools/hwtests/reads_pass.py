#!/usr/bin/env python3
"""What filter_reads.py's pass costs on the device (k_reads.hip), on one MI355X, in one process, profiler off:

    python tools/hwtests/reads_pass.py [OUT_DIR] [RUNS] [SCALE]

A seeded synthetic 40x HiFi read set (synth.simulate_reads over 120 Mb + 80 Mb, both x SCALE) as a heads stream, resident on the
device.  After one untimed call each, RUNS (5) times, alternating run by run, each between two events on the engine's stream:

  * gci_bam_fate alone (-mq 30, -cp 0.1, -ip 0.9): the class bytes the other calls take,
  * gci_bam_reads_size + _write of every class, no windows: every record that belongs to a class is a row,
  * the same with ~1000 windows of 1 kb spread evenly over the contigs,
  * the yardstick: gci_bam_cover_size_sel + gci_bam_cover_write of the class `kept` -- the walk filter_depth.py makes over the same
    class bytes.

-> one JSON line, and OUT_DIR/reads_pass.json."""
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
    names = [n.encode() for n, _ in contigs]
    name_len = np.array([len(x) for x in names], dtype=np.uint32)
    name_off = np.concatenate(([0], np.cumsum(name_len[:-1]))).astype(np.uint64)
    d_names = engine.to_device(np.frombuffer(b"".join(names), dtype=np.uint8))
    per = 1000 // len(contigs)
    regions = [(n, k * (L // per), k * (L // per) + 1000) for n, L in contigs for k in range(per)]
    win, win0 = pipeline.merge_windows(regions, dict(contigs))
    d_win, d_win0 = engine.to_device(win), engine.to_device(win0)
    rows, size, n_ivl = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                   # noqa: E731

    def chk(st):
        if st != 0:
            raise SystemExit("a call failed: %d" % st)

    def fate():
        chk(lib.gci_bam_fate(*head, 0, p(d_sel), len(contigs), *FILT, p(d_cls), counts, p(engine._status)))

    fate()
    engine.check_status("gci_bam_fate")
    seen = {}

    def reads(windows: bool):
        chk(lib.gci_bam_reads_size(*head, 0, p(d_sel), len(contigs), p(d_cls), 0x7E, p(d_win) if windows else None, p(d_win0) if windows else None,
                                   vp(name_len), 1, ctypes.byref(rows), ctypes.byref(size), p(engine._status)))
        seen[windows] = (int(rows.value), int(size.value))
        chk(lib.gci_bam_reads_write(*head, p(d_names), vp(name_off), vp(name_len), p(text), len_text))

    chk(lib.gci_bam_reads_size(*head, 0, p(d_sel), len(contigs), p(d_cls), 0x7E, None, None, vp(name_len), 1, ctypes.byref(rows), ctypes.byref(size),
                               p(engine._status)))
    len_text = int(size.value)
    text = engine.T.empty(max(len_text, 1), engine.T.uint8, engine.device)
    chk(lib.gci_bam_cover_size_sel(*head, 0, p(d_sel), len(contigs), 0x4, 0, 0, p(d_cls), 1 << 6, ctypes.byref(n_ivl), p(engine._status)))
    ivl = engine.T.empty((max(int(n_ivl.value), 1), 4), engine.T.int32, engine.device)

    def kept_cover():
        chk(lib.gci_bam_cover_size_sel(*head, 0, p(d_sel), len(contigs), 0x4, 0, 0, p(d_cls), 1 << 6, ctypes.byref(n_ivl), p(engine._status)))
        chk(lib.gci_bam_cover_write(*head, 0, p(ivl), int(n_ivl.value), p(engine._status)))

    calls = {"gci_bam_fate": fate, "reads_size+write": lambda: reads(False), "reads_size+write_1000_windows": lambda: reads(True),
             "kept_cover_size_sel+write": kept_cover}
    for c in calls.values():
        c()
    engine.T.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(runs):
        for k, c in calls.items():
            ms[k].append(round(_timed(engine, c), 4))
    res = {"scale": scale, "repeats": runs, "records": n_rec, "stream_bytes": n_bytes, "cigar_operations": int(np.diff(rs.cigar_off).sum()),
           "records_per_class": dict(zip(_lib.FATE_NAMES, [int(x) for x in counts])), "windows": int(win.shape[0]),
           "rows_and_bytes": {"no_windows": seen[False], "windows": seen[True]}, "ms": ms,
           "ms_min_median": {k: [min(v), round(statistics.median(v), 4)] for k, v in ms.items()}}
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "reads_pass.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "", int(sys.argv[2]) if len(sys.argv) > 2 else 5, float(sys.argv[3]) if len(sys.argv) > 3 else 1.0)
