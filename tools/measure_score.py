#!/usr/bin/env python3
"""GCI_score.py at CHM13 size ("GCI_score.py"): inputs, timed runs and the summary of the profiles.
Run on one MI355X by tools/measure_score.sh, which adds the rocprofv3 runs.

    python tools/measure_score.py make DIR [SCALE]   CHM13 geometry (every contig x SCALE): ref.fa, three ~40x .depth.gz files of
                                                    this project's writer (hifi, nano, two), one reference-style file (Python's
                                                    gzip, level 9, FNAME, one member per contig) of the hifi track
    python tools/measure_score.py run DIR OUT        wall time and peak host RSS of `GCI_score.py --hifi --nano --two-type -f` under
                                                    GCI_PHASES, with GCI_DEPTH_READ=members and =text in turn, and of
                                                    `GCI_score.py --hifi <reference-style file> -f` -> OUT/score_runs.json
    python tools/measure_score.py summarize DIR OUT  kernel times (rocprofv3 --kernel-trace --stats) and FETCH_SIZE / WRITE_SIZE
                                                    (rocprofv3 --pmc, a run of its own) of the two parse kernels against the bytes
                                                    they must move -> OUT/score_summary.txt
"""
from __future__ import annotations

import csv
import glob
import gzip
import io
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
KINDS = (("hifi", 40, 1), ("nano", 38, 2), ("two", 44, 3))


def _track_of(L: int, mean: int, rng) -> np.ndarray:
    """Piecewise-constant depth around `mean`: runs of 1 - 300 bases, a few stretches of 0 and of low depth."""
    runs = rng.integers(1, 300, L // 150 + 16)
    vals = np.clip(rng.normal(mean, 8, runs.shape[0]), 0, 200).astype(np.int32)
    vals[rng.random(runs.shape[0]) < 0.0005] = 0
    d = np.repeat(vals, runs)
    while d.shape[0] < L:
        d = np.concatenate([d, d])
    return d[:L]


def make(d: str, scale: float = 1.0) -> None:
    from gci_amd import pipeline, synth
    from gci_amd.device import Engine
    os.makedirs(d, exist_ok=True)
    contigs = [(n, max(10_000, int(L * scale))) for n, L in synth.CHM13]
    gaps = {n: [(L // 3, L // 3 + 5000)] for n, L in contigs[:5]}
    synth.write_reference_fasta(os.path.join(d, "ref.fa"), contigs, gaps)
    eng = Engine(0)
    tl = dict(contigs)
    info = {"contigs": len(contigs), "bases": int(sum(tl.values())), "files": {}}
    for kind, mean, seed in KINDS:
        rng = np.random.default_rng(seed)
        eng.set_layout([L for _, L in contigs])
        host = np.zeros(eng.total, dtype=np.int32)
        for o, (_, L) in zip(eng.offsets, contigs):
            host[o:o + L] = _track_of(L, mean, rng)
        depths = pipeline.DepthTracks(eng, tl, eng.to_device(host))
        pipeline.write_depth(d, kind, depths)
        info["files"][kind + ".depth.gz"] = os.path.getsize(os.path.join(d, kind + ".depth.gz"))
        if kind == "hifi":                                   # the same track as the reference's writer lays it out
            text, offs = eng.depth_text(depths.track)
            host_text = text.cpu().numpy()
            info["text_bytes"] = int(host_text.shape[0] + sum(len(n) + 2 for n, _ in contigs))

            def member(c):
                buf = io.BytesIO()
                with gzip.GzipFile(filename="hifi.depth.gz", mode="wb", compresslevel=9, fileobj=buf, mtime=0) as g:
                    g.write(b">" + contigs[c][0].encode() + b"\n")
                    g.write(memoryview(host_text)[int(offs[c]):int(offs[c + 1])])
                return buf.getvalue()
            with ThreadPoolExecutor(16) as ex, open(os.path.join(d, "refstyle.depth.gz"), "wb") as f:
                for blob in ex.map(member, range(len(contigs))):
                    f.write(blob)
            info["files"]["refstyle.depth.gz"] = os.path.getsize(os.path.join(d, "refstyle.depth.gz"))
            del text, host_text
        del depths, host
    with open(os.path.join(d, "inputs.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))


def _timed(cmd, env=None, log=None):
    """-> (wall seconds, peak resident set of the child in MB)"""
    t = time.perf_counter()
    with open(log or os.devnull, "w") as f:
        p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=f, stderr=subprocess.STDOUT)
        _, status, usage = os.wait4(p.pid, 0)
        p.returncode = os.waitstatus_to_exitcode(status)
    if p.returncode != 0:
        raise SystemExit("failed (%d): %s" % (p.returncode, " ".join(cmd)))
    return round(time.perf_counter() - t, 3), round(usage.ru_maxrss / 1024.0, 1)


def run(d: str, out: str) -> None:
    os.makedirs(out, exist_ok=True)
    entry = [sys.executable, os.path.join(ROOT, "GCI_score.py"), "-r", os.path.join(d, "ref.fa")]
    three = ["--hifi", os.path.join(d, "hifi.depth.gz"), "--nano", os.path.join(d, "nano.depth.gz"), "--two-type", os.path.join(d, "two.depth.gz")]
    res = {"inputs": json.load(open(os.path.join(d, "inputs.json")))}
    for k in range(2):                                       # the two paths of the read in turn, twice
        for mode in ("members", "text"):
            ph = os.path.join(out, "score_phases_three_files_%s_run%d.json" % (mode, k))
            wall, rss = _timed(entry + three + ["-d", os.path.join(d, "out_" + mode), "-o", "M", "-f"],
                               env=dict(os.environ, GCI_PHASES=ph, GCI_DEPTH_READ=mode), log=os.path.join(out, "score_%s_run%d.log" % (mode, k)))
            res["three_files_%s_wall_s_run%d" % (mode, k)], res["three_files_%s_peak_rss_mb_run%d" % (mode, k)] = wall, rss
            wall_s = json.load(open(ph))["wall_s"]
            res["three_files_%s_phases_s_run%d" % (mode, k)] = {n: round(v, 4) for n, v in wall_s.items() if n.startswith("depth_")}
    same = all(open(os.path.join(d, "out_members", fn), "rb").read() == open(os.path.join(d, "out_text", fn), "rb").read()
               for fn in sorted(os.listdir(os.path.join(d, "out_text"))))
    res["outputs_of_the_two_paths_identical"] = bool(same and sorted(os.listdir(os.path.join(d, "out_members"))) ==
                                                     sorted(os.listdir(os.path.join(d, "out_text"))))
    ph = os.path.join(out, "score_phases_reference_style.json")
    res["reference_style_hifi_wall_s"], res["reference_style_hifi_peak_rss_mb"] = _timed(
        entry + ["--hifi", os.path.join(d, "refstyle.depth.gz"), "-d", os.path.join(d, "out_ref"), "-o", "R", "-f"],
        env=dict(os.environ, GCI_PHASES=ph))
    with open(os.path.join(out, "score_runs.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def summarize(d: str, out: str) -> None:
    info = json.load(open(os.path.join(out, "inputs.json")))
    lines = []
    stats = glob.glob(os.path.join(out, "trace", "**", "*kernel_stats.csv"), recursive=True)
    kt = {}
    for path in stats:
        for r in csv.DictReader(open(path)):
            if "k_depth_text" in r["Name"]:
                key = "index" if "index" in r["Name"] else "parse"
                kt[key] = (int(r["Calls"]), float(r["TotalDurationNs"]) * 1e-9)
    text, bases = info["text_bytes"], info["bases"]
    calls = 3                                                # three files in the traced run
    need = {"index": calls * text * (1 + 32 / 4096), "parse": calls * (text * (1 + 32 / 4096) + 4 * bases)}
    lines.append("inputs: %d contigs, %d bases per file, %d text bytes per file (hifi)" % (info["contigs"], bases, text))
    lines.append("compressed: %s" % json.dumps(info["files"]))
    tot_s = tot_b = 0.0
    for k in ("index", "parse"):
        if k in kt:
            n, s = kt[k]
            tot_s += s
            tot_b += need[k]
            lines.append("k_depth_text_%s: %d calls, %.3f ms in all, %.3f ms per file; bytes it must move %.2f GB per file -> "
                         "%.2f TB/s = %.3f of the 8 TB/s peak" % (k, n, s * 1e3, s * 1e3 / n, need[k] / calls / 1e9,
                                                                need[k] / s / 1e12, need[k] / s / HBM_PEAK))
    if tot_s:
        lines.append("both passes: %.3f of the 8 TB/s peak (bytes they must move over their kernel time)" % (tot_b / tot_s / HBM_PEAK))
    # the compressed-domain read (k_depth_gz.hip): raw bytes in, 8 B per run, 4 B per base out
    for path in stats:
        for r in csv.DictReader(open(path)):
            if "k_dgz_" in r["Name"]:
                name = r["Name"][r["Name"].index("k_dgz_"):].split("(")[0]
                lines.append("%s: %d calls, %.3f ms in all, %.3f ms per call" % (name, int(r["Calls"]), float(r["TotalDurationNs"]) * 1e-6,
                                                                              float(r["TotalDurationNs"]) * 1e-6 / max(int(r["Calls"]), 1)))
    own = [v for k, v in info["files"].items() if not k.startswith("refstyle")]
    if own:
        lines.append("k_dgz_*: bytes they must move per file: %.3f GB raw in (scan and runs each), 8 B per run (not counted here), "
                     "%.2f GB of track out" % (sum(own) / len(own) / 1e9, 4 * bases / 1e9))
    pmc = {}
    for path in glob.glob(os.path.join(out, "pmc", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "k_depth_text" in r.get("Kernel_Name", ""):
                key = ("index" if "index" in r["Kernel_Name"] else "parse", r["Counter_Name"])
                pmc[key] = pmc.get(key, 0.0) + float(r["Counter_Value"])
    for (k, c), v in sorted(pmc.items()):
        lines.append("pmc (one file, %s): k_depth_text_%s %s = %.3f GB as counted%s" % (
            "hifi", k, c, v / 1e9, ", x2 = %.3f GB (gfx950 counts wide streaming reads at half)" % (2 * v / 1e9) if c == "FETCH_SIZE" else ""))
    txt = "\n".join(lines) + "\n"
    with open(os.path.join(out, "score_summary.txt"), "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "make":
        make(sys.argv[2], float(sys.argv[3]) if len(sys.argv) > 3 else 1.0)
    elif cmd == "run":
        run(sys.argv[2], sys.argv[3])
    elif cmd == "summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
