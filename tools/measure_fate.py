#!/usr/bin/env python3
"""filter_depth.py's kernels (k_fate.hip, gci_bam_cover_size_sel), on one MI355X, in one process with the
profiler off:

    python tools/measure_fate.py run OUT [RUNS] [SCALE]

The two seeded synth read sets of tools/measure_cover.py as HEADS streams (HiFi, 200 Mb x 30, and ONT, 40 Mb x 15, both x SCALE).
Reported per stream, after one untimed call each, RUNS (5) times, alternating run by run, each between two events on the engine's
stream:

  * gci_bam_fate (-mq 30, -cp 0.1, -ip 0.9),
  * gci_bam_cover_size_sel + gci_bam_cover_write once per class secondary .. kept with that class's mask, the six pairs summed,
  * gci_bam_cover_size_sel + gci_bam_cover_write without classes (excl = 0x4): every record the six classes hold in one walk,
  * measure_cover.py's yardsticks in the same process: gci_bam_cover_size + _write (excl = 0x704) and record pages +
    gci_bam_filter_pages.

-> OUT/fate_runs.json.

    python tools/measure_fate.py join OUT [RUNS] [SCALE]

filter_depth.py --join's export: the HiFi read set and synth.perturb of it as two files of one read set (heads streams, record pages,
gci_bam_filter_pages), then, as above, gci_name_join_fate against gci_name_join on the classic table over the same inputs, and
gci_fate_refine over the first file's classes.  -> OUT/joinfate_runs.json."""
from __future__ import annotations

import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_bedgraph import _timed  # noqa: E402
from measure_cover import SETS, _read_set  # noqa: E402

FILT = (30, 0.1, 0.9)


def _one_stream(engine, contigs, rs, runs: int) -> dict:
    from gci_amd import _lib, synth
    stream, offs = synth.to_bam_stream(rs, heads=True)
    engine.set_layout([L for _, L in contigs])
    d_stream, d_off = engine.to_device(stream), engine.to_device(offs)
    d_sel = engine.to_device(np.arange(len(contigs), dtype=np.int32))
    n_rec, n_bytes = int(offs.shape[0]), int(stream.shape[0])
    lib, p = engine.lib, engine._p
    head = (engine.ctx, p(d_stream), n_bytes, p(d_off), n_rec, 0)
    d_cls = engine.T.empty(n_rec, engine.T.uint8, engine.device)
    counts = (ctypes.c_uint64 * _lib.FATE_CLASSES)()
    n_ivl = ctypes.c_uint64(0)
    wanted = list(range(1, 7))

    def chk(st):
        if st != 0:
            raise SystemExit("a call failed: %d" % st)

    def fate():
        chk(lib.gci_bam_fate(*head, p(d_sel), len(contigs), *FILT, p(d_cls), counts, p(engine._status)))

    def size(excl, cls, mask):
        chk(lib.gci_bam_cover_size_sel(*head, p(d_sel), len(contigs), excl, 0, 0, cls, mask, ctypes.byref(n_ivl), p(engine._status)))
        return int(n_ivl.value)

    fate()
    engine.check_status("gci_bam_fate")
    per_class = {c: size(0x4, p(d_cls), 1 << c) for c in wanted}
    n_all = size(0x4, None, 0)
    out = engine.T.empty((max(n_all, 1), 4), engine.T.int32, engine.device)

    def write():
        chk(lib.gci_bam_cover_write(*head, p(out), int(n_ivl.value), p(engine._status)))

    def six_selected():
        for c in wanted:
            size(0x4, p(d_cls), 1 << c)
            write()

    def unselected():
        size(0x4, None, 0)
        write()

    def cover_pair():
        chk(lib.gci_bam_cover_size(*head, p(d_sel), len(contigs), 0x704, 0, 0, ctypes.byref(n_ivl), p(engine._status)))
        write()

    def yardstick():
        pages = engine.bam_pages(d_stream, d_off, False)
        engine.bam_filter_pages(pages, d_sel, 30, 50, FILT[1], FILT[2], check=False)

    calls = {"gci_bam_fate": fate, "six_selected_cover_pairs": six_selected, "unselected_cover_pair": unselected,
             "gci_bam_cover_size+write": cover_pair, "record_pages+gci_bam_filter_pages": yardstick}
    for c in calls.values():
        c()
    engine.T.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(runs):
        for k, c in calls.items():
            ms[k].append(round(_timed(engine, c), 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_ops = int(np.diff(rs.cigar_off).sum())
    return {"records": n_rec, "stream_bytes": n_bytes, "cigar_operations": n_ops, "records_per_class": dict(zip(_lib.FATE_NAMES, [int(x) for x in counts])),
            "intervals_per_class": {_lib.FATE_NAMES[c]: n for c, n in per_class.items()}, "intervals_unselected": n_all,
            "intervals_agree": sum(per_class.values()) == n_all, "ms": ms,
            "ms_min_median": {k: [min(v), round(med[k], 4)] for k, v in ms.items()},
            "fate_over_cover_size_pair": round(med["gci_bam_fate"] / med["gci_bam_cover_size+write"], 3),
            "fate_over_filter_yardstick": round(med["gci_bam_fate"] / med["record_pages+gci_bam_filter_pages"], 3),
            "six_selected_over_unselected": round(med["six_selected_cover_pairs"] / med["unselected_cover_pair"], 3)}


def run(out: str, runs: int = 5, scale: float = 1.0) -> None:
    from gci_amd import pipeline
    os.makedirs(out, exist_ok=True)
    engine = pipeline.default_engine()
    res = {"scale": scale, "repeats": runs, "streams": {}}
    for kind in SETS:
        contigs, rs = _read_set(kind, scale)
        res["streams"][kind] = _one_stream(engine, contigs, rs, runs)
        with open(os.path.join(out, "fate_runs.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


def join(out: str, runs: int = 5, scale: float = 1.0) -> None:
    from gci_amd import _lib, pipeline, synth
    from gci_amd.device import JoinInput
    os.makedirs(out, exist_ok=True)
    engine = pipeline.default_engine()
    contigs, rs = _read_set("hifi", scale)
    d_sel = engine.to_device(np.arange(len(contigs), dtype=np.int32))
    files, first = [], None
    for k, one in enumerate((rs, synth.perturb(rs, 12))):
        stream, offs = synth.to_bam_stream(one, heads=True)
        d_stream, d_off = engine.to_device(stream), engine.to_device(offs)
        pages = engine.bam_pages(d_stream, d_off, False)
        recs, noff = engine.bam_filter_pages(pages, d_sel, 30, 50, FILT[1], FILT[2])
        files.append(JoinInput(recs, pages.buf, noff, 0))
        if k == 0:
            first = (d_stream, d_off)
    cls, _ = engine.bam_fate(first[0], first[1], False, d_sel, *FILT)
    engine.set_join_mode("classic")
    kept = {}

    def fate():
        kept["fate"], kept["counts"] = engine.name_join_fate(files, 0.9)

    def plain():
        kept["n"] = int(engine.name_join(files, 0.9)[1].item())

    fate()
    work = engine.T.empty(int(cls.shape[0]), engine.T.uint8, engine.device)

    def refine():
        work.copy_(cls)
        engine.fate_refine(work, kept["fate"][0])

    calls = {"gci_name_join_fate": fate, "gci_name_join(classic)": plain, "copy+gci_fate_refine": refine}
    for c in calls.values():
        c()
    engine.T.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(runs):
        for k, c in calls.items():
            ms[k].append(round(_timed(engine, c), 4))
    names = _lib.ALL_FATE_NAMES
    res = {"scale": scale, "repeats": runs, "records": [int(f.recs.shape[0]) for f in files], "intervals_of_gci_name_join": kept["n"],
           "records_per_join_class": [{names[c]: row[c] for c in range(8, 13)} for row in kept["counts"]], "ms": ms,
           "ms_min_median": {k: [min(v), round(statistics.median(v), 4)] for k, v in ms.items()}}
    res["fate_over_join"] = round(res["ms_min_median"]["gci_name_join_fate"][1] / res["ms_min_median"]["gci_name_join(classic)"][1], 3)
    with open(os.path.join(out, "joinfate_runs.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] not in ("run", "join"):
        raise SystemExit(__doc__)
    (run if sys.argv[1] == "run" else join)(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5, float(sys.argv[4]) if len(sys.argv) > 4 else 1.0)
