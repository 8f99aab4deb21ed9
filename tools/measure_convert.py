#!/usr/bin/env python3
"""convert_samtools_depth.py at chromosome size ("convert_samtools_depth.py"): the new parse kernels against the pair
they are modelled on, on the same track.  Run on one MI355X:

    python tools/measure_convert.py all OUT [BASES]   everything below, each GPU step a process of its own under a time limit; the
                                                      first failure ends it.  -> OUT/convert_depth.txt
    python tools/measure_convert.py make DIR [BASES]  one contig of BASES (default 50 M) + 100 small ones: big.depth (`samtools
                                                      depth -a` text), RT.depth.gz (what the converter makes of it) and track.depth
                                                      (its payload: the `.depth` text of the same track)
    python tools/measure_convert.py kernels DIR       both kernel pairs in ONE process, alternating, a warm-up round and five timed
                                                      ones: k_sdepth_index + k_sdepth_parse over big.depth, k_depth_text_index +
                                                      k_depth_text_parse over track.depth (the process rocprofv3 --kernel-trace wraps)
    python tools/measure_convert.py summarize DIR OUT the kernel times of that trace over the bytes of text, both pairs and their
                                                      ratio; the phases of the whole command; PMC counters when a run left them
    python tools/measure_convert.py reference FILE N  the reference utility (CPU, where the reference tree is) over the first N lines
                                                      of FILE: lines per second, for context only
"""
from __future__ import annotations

import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
NONE = (1 << 64) - 1


def make(d: str, bases: int = 50_000_000) -> None:
    from gci_amd import hostio, pipeline, synth
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(23)
    lengths = [bases] + [int(x) for x in rng.integers(1_000, 200_000, 100)]
    names = ["chr1"] + ["ctg%03d_hap%d" % (k, k % 2 + 1) for k in range(1, 101)]
    items = []
    for nm, L in zip(names, lengths):
        runs = rng.integers(10_000, 60_000, L // 20_000 + 2)
        vals = rng.choice([0, 1, 2, 17, 38, 41, 250, 123_456], runs.shape[0]).astype(np.int32)
        items.append((nm, np.repeat(vals, runs)[:L]))
    text = synth.samtools_depth_text(items)
    text.tofile(os.path.join(d, "big.depth"))
    taken = pipeline.convert_samtools_depth(pipeline.default_engine(), os.path.join(d, "big.depth"), os.path.join(d, "RT"))
    assert taken == "device", taken
    with hostio.GzipText(np.fromfile(os.path.join(d, "RT.depth.gz"), dtype=np.uint8), hostio.pick_threads(1)) as gz:
        payload = gz.export()
    payload.tofile(os.path.join(d, "track.depth"))
    info = {"lines": int(sum(lengths)), "contigs": len(lengths), "samtools_text_bytes": int(text.shape[0]),
            "depth_text_bytes": int(payload.shape[0]), "depth_gz_bytes": os.path.getsize(os.path.join(d, "RT.depth.gz"))}
    with open(os.path.join(d, "inputs.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))


def kernels(d: str) -> None:
    from gci_amd import pipeline
    from gci_amd.formats import depthfile
    eng = pipeline.default_engine()
    sam = np.memmap(os.path.join(d, "big.depth"), dtype=np.uint8, mode="r")
    dep = np.fromfile(os.path.join(d, "track.depth"), dtype=np.uint8)
    d_sam, d_dep = eng.upload_staged(sam), eng.upload_staged(dep)
    for k in range(1 + ROUNDS):                                         # (round 0: the warm-up; the trace holds all six)
        d_line0, line0, keys, bad = eng.sdepth_index(d_sam)
        assert bad == NONE
        found = depthfile.sdepth_segments(sam, keys, line0)
        first = np.array([g for _, g in found] + [int(line0[-1])], dtype=np.int64)
        lengths = np.diff(first)
        eng.set_layout(lengths.tolist())
        track_a = eng.T.zeros(max(eng.total, 1), eng.T.int32, eng.device)
        eng.sdepth_parse(d_sam, d_line0, np.stack([first[:-1], lengths, np.asarray(eng.offsets, dtype=np.int64)], axis=1), track_a)
        d_line0, line0, keys, bad = eng.depth_text_index(d_dep)
        assert bad == NONE
        names, lens, segs = depthfile.header_segments(dep, keys, line0)
        assert lens == lengths.tolist()
        track_b = eng.T.zeros(max(eng.total, 1), eng.T.int32, eng.device)
        eng.depth_text_parse(d_dep, d_line0, segs(eng.offsets), track_b)
        if k == 0:
            assert np.array_equal(track_a.cpu().numpy(), track_b.cpu().numpy()), "the two parses disagree"
    print("kernels ok: %d rounds" % (1 + ROUNDS))


def summarize(d: str, out: str) -> None:
    info = json.load(open(os.path.join(d, "inputs.json")))
    kt = {}
    for path in glob.glob(os.path.join(out, "trace", "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            for k in ("k_sdepth_index", "k_sdepth_parse", "k_depth_text_index", "k_depth_text_parse"):
                if k in r["Name"]:
                    kt[k] = (int(r["Calls"]), float(r["TotalDurationNs"]) * 1e-9, float(r["MinNs"]) * 1e-9, float(r["MaxNs"]) * 1e-9)
    lines = ["inputs: %s" % json.dumps(info)]
    for k, (n, s, lo, hi) in sorted(kt.items()):
        lines.append("%-20s %d calls, mean %.3f ms (min %.3f, max %.3f; the first call is the warm-up)" % (k, n, s / n * 1e3, lo * 1e3, hi * 1e3))
    rate = {}
    for pair, size in ((("k_sdepth_index", "k_sdepth_parse"), info["samtools_text_bytes"]),
                       (("k_depth_text_index", "k_depth_text_parse"), info["depth_text_bytes"])):
        if all(k in kt for k in pair):
            s = sum(kt[k][1] / kt[k][0] for k in pair)
            rate[pair[0]] = size / s
            lines.append("%s + %s: %.3f ms over %d bytes of text = %.1f GB of text per second, %.2f G lines per second" % (
                pair[0], pair[1], s * 1e3, size, size / s / 1e9, info["lines"] / s / 1e9))
    if len(rate) == 2:
        lines.append("ratio, text bytes per second, new pair over the yardstick: %.3f" % (rate["k_sdepth_index"] / rate["k_depth_text_index"]))
    for path in sorted(glob.glob(os.path.join(out, "phases_run*.json"))):
        ph = json.load(open(path))
        lines.append("%s: total %.3f s; %s; path %s" % (os.path.basename(path), ph["total_s"],
                                                        ", ".join("%s %.3f" % kv for kv in ph["wall_s"].items()),
                                                        ph["notes"].get("convert_samtools_depth_path")))
    runs = os.path.join(out, "runs.json")
    if os.path.exists(runs):
        lines.append("whole command, wall seconds of the process: %s" % json.dumps(json.load(open(runs))))
    pmc = {}
    for path in glob.glob(os.path.join(out, "pmc", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            for k in ("k_sdepth_index", "k_sdepth_parse", "k_depth_text_index", "k_depth_text_parse"):
                if k in r.get("Kernel_Name", ""):
                    pmc.setdefault((k, r["Counter_Name"]), []).append(float(r["Counter_Value"]))
    for (k, c), v in sorted(pmc.items()):
        lines.append("pmc: %s %s = %.4g per dispatch (mean of %d)" % (k, c, sum(v) / len(v), len(v)))
    txt = "\n".join(lines) + "\n"
    with open(os.path.join(out, "convert_depth.txt"), "w") as f:
        f.write(txt)
    print(txt)


def _step(cmd, limit: int, log: str, env=None) -> float:
    t = time.perf_counter()
    with open(log, "w") as f:
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, stdout=f, stderr=subprocess.STDOUT).returncode
    if rc != 0:
        sys.stderr.write(open(log).read()[-3000:])
        raise SystemExit("failed (%d), nothing more is started: %s" % (rc, " ".join(cmd)))
    return round(time.perf_counter() - t, 3)


def run_all(out: str, bases: int, pmc: bool) -> None:
    os.makedirs(out, exist_ok=True)
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), "gci_convert_measure")
    me = [sys.executable, os.path.abspath(__file__)]
    _step(me + ["make", d, str(bases)], 600, os.path.join(out, "make.log"))
    walls = {}
    for k in range(2):                                                   # the whole command, profiler off
        env = dict(os.environ, GCI_PHASES=os.path.join(out, "phases_run%d.json" % k))
        walls["run%d" % k] = _step([sys.executable, os.path.join(ROOT, "convert_samtools_depth.py"), os.path.join(d, "big.depth"),
                                    os.path.join(d, "W")], 300, os.path.join(out, "run%d.log" % k), env)
    with open(os.path.join(out, "runs.json"), "w") as f:
        json.dump(walls, f)
    _step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(out, "trace"), "-o", "convert", "--"]
          + me + ["kernels", d], 400, os.path.join(out, "trace.log"))
    summarize(d, out)
    if pmc:                                                              # counters in runs of their own, no tracing beside them
        groups = {"sq": ["SQ_WAVE_CYCLES", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAIT_INST_ANY"],
                  "sq2": ["SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_LDS_BANK_CONFLICT", "GRBM_GUI_ACTIVE"],
                  "fetch": ["FETCH_SIZE"], "write": ["WRITE_SIZE"]}
        for name, counters in groups.items():
            _step(["rocprofv3", "--pmc"] + counters + ["--output-format", "csv", "-d", os.path.join(out, "pmc", name), "-o", "convert", "--"]
                  + me + ["kernels", d], 400, os.path.join(out, "pmc_%s.log" % name))
        summarize(d, out)


def reference(path: str, n_lines: int) -> None:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tempfile
    import load_reference
    utility = os.path.join(os.path.dirname(load_reference.REF), "utility", "convert_samtools_depth.py")
    with tempfile.TemporaryDirectory() as td:
        piece = os.path.join(td, "slice.depth")
        with open(path, "rb") as f, open(piece, "wb") as g:
            for k, line in enumerate(f):
                if k >= n_lines:
                    break
                g.write(line)
        t = time.perf_counter()
        subprocess.run([sys.executable, utility, piece, os.path.join(td, "ref")], check=True)
        s = time.perf_counter() - t
    print("reference utility (CPU, one thread, gzip level 9): %d lines in %.1f s = %.3f M lines per second" % (n_lines, s, n_lines / s / 1e6))


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "make":
        make(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 50_000_000)
    elif cmd == "kernels":
        kernels(sys.argv[2])
    elif cmd == "summarize":
        summarize(sys.argv[2], sys.argv[3])
    elif cmd == "all":
        rest = [a for a in sys.argv[2:] if a != "--pmc"]
        run_all(rest[0], int(rest[1]) if len(rest) > 1 else 50_000_000, "--pmc" in sys.argv)
    elif cmd == "reference":
        reference(sys.argv[2], int(sys.argv[3]))
    else:
        raise SystemExit(__doc__)
