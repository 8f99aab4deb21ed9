#!/usr/bin/env python3
"""Generate the depth_plotter_v2.py fixtures under tests/golden/dpv2_*/ by running the UNMODIFIED reference utility
(utility/depth_plotter_v2.py of the reference tree tools/load_reference.py finds) through its own `__main__` block with matplotlib's
Agg backend.  Only data is written: inputs of this tool's own making, the files the utility wrote, its transcript and its exit.
Nothing at test time needs the reference.

    python tools/make_golden_plotter_v2.py

  tests/golden/dpv2_inputs/                 depth files, a .fai and a BED file of this tool's own
  tests/golden/dpv2_<case>/manifest.json    argv, stdout, stderr of a run that completes, the names of the files it wrote;
                                            expected/ the PNG figures, when there are any (PDF and SVG figures are not kept: a test checks that they exist)
  tests/golden/dpv2_errors.json             the runs that end early or by an exception (and one -f svg run): argv, exit or exception,
                                            stdout, stderr, the files left behind

In argv, {GOLDEN} stands for tests/golden, {DIN} for tests/golden/dpv2_inputs and {OUT} for the output directory.

The inputs are three sequences of 13 000, 4 096 and 700 bases whose runs sit where a kernel that works in tiles of 4096 elements
can go wrong: zero and low runs of one base at elements 4095, 4096, 8191 and 8192, a zero run beside a low run beside a 5, runs at
both ends of a sequence, a zero run longer than a window and a stretch between two zero runs that is shorter than one."""
from __future__ import annotations

import contextlib
import gzip
import io
import json
import os
import shutil
import sys
import tempfile
import types

os.environ["MPLBACKEND"] = "Agg"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import load_reference  # noqa: E402

UTILITY = os.path.join(os.path.dirname(load_reference.REF), "utility", "depth_plotter_v2.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")
DIN = os.path.join(GOLDEN, "dpv2_inputs")
LENGTHS = (("s1", 13000), ("s2", 4096), ("s3", 700))


def make_depths(seed: int, base: int):
    """{name: int array}; `base` is the ordinary depth, the two read types differ in it and in which of a pair of runs is zero."""
    rng = np.random.default_rng(seed)
    out = {name: base + rng.integers(-4, 5, size=n) + (np.arange(n) // 900) % 3 for name, n in LENGTHS}
    flip = seed & 1
    s1, s2, s3 = out["s1"], out["s2"], out["s3"]
    for at, kind in ((4095, 0), (4096, 1), (8191, 1), (8192, 0)):      # one base each, either side of a tile boundary
        s1[at] = 0 if kind ^ flip == 0 else 2
    s1[0:3] = 0                                                        # a zero run at the first base
    s1[1000:1010] = 0                                                  # zero | low | 5
    s1[1010:1020] = [1, 2, 3, 4, 4, 3, 2, 1, 1, 4]
    s1[1020] = 5
    s1[6000:6350] = 0                                                  # longer than a window of 100 (and of 64)
    s1[6380:6400] = 0                                                  # ... and 30 bases between two zero runs: shorter than one
    s1[8500:8700] = 3                                                  # a low run longer than a window
    s1[12990:13000] = [4, 3, 2, 1, 1, 2, 3, 4, 4, 4]                   # a low run at the last base
    s2[0:5] = 1 + flip                                                 # a low run at the first base
    s2[2000:2100] = 0
    s2[4090:4096] = 0                                                  # a zero run at the last base (the last element of a tile)
    s3[100:130] = 0
    s3[300:320] = 4
    if flip:
        s3[:] = np.where(np.arange(700) < 350, s3, 0)                  # the second half of the shortest sequence: nothing
    return out


def depth_text(depths, short=None) -> bytes:
    parts = []
    for name, arr in depths.items():
        a = arr[:-1] if name == short else arr
        parts.append(">%s\n" % name + "".join("%d\n" % v for v in a.tolist()))
    return "".join(parts).encode()


def make_inputs() -> None:
    shutil.rmtree(DIN, ignore_errors=True)
    os.makedirs(DIN)
    hifi, ont = make_depths(20, 24), make_depths(31, 14)
    for fn, text in (("hifi.depth.gz", depth_text(hifi)), ("ont.depth.gz", depth_text(ont)), ("ont_s2_short.depth.gz", depth_text(ont, "s2"))):
        with open(os.path.join(DIN, fn), "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(text)
    with open(os.path.join(DIN, "hifi.depth"), "wb") as f:              # the same text, not compressed
        f.write(depth_text(hifi))
    with open(os.path.join(DIN, "text_named.depth.gz"), "wb") as f:     # plain text behind a .gz name
        f.write(b">s3\n7\n7\n")
    with open(os.path.join(DIN, "ref.fa.fai"), "w") as f:               # (s4 is in none of the depth files)
        at = 0
        for name, n in LENGTHS + (("s4", 500),):
            at += len(name) + 2
            f.write("%s\t%d\t%d\t60\t61\n" % (name, n, at))
            at += n + (n + 59) // 60
    with open(os.path.join(DIN, "regions.bed"), "w") as f:
        f.write("# two overlapping regions, two bases across elements 4095 | 4096, a region that reaches beyond the shortest sequence\n"
                "s1\t4000\t7000\n"
                "s1\t2000\t5000\tname\n"
                "s1\t4095\t4096\n"
                "s1\t12\n"
                "s3\t600\t9999\n")


def run_utility(argv_t, out: str):
    """The utility's __main__ as `python depth_plotter_v2.py ...` would run it: (exit, exception, stdout, stderr), normalised."""
    sub = lambda a: a.replace("{GOLDEN}", GOLDEN).replace("{DIN}", DIN).replace("{OUT}", out)      # noqa: E731
    norm = lambda t: t.replace(out, "{OUT}").replace(DIN, "{DIN}").replace(GOLDEN, "{GOLDEN}")     # noqa: E731
    so, se = io.StringIO(), io.StringIO()
    old = sys.argv
    sys.argv = ["depth_plotter_v2.py"] + [sub(a) for a in argv_t]
    code, exc = "completed", None
    try:
        with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
            mod = types.ModuleType("__main__")
            mod.__file__ = UTILITY
            saved = sys.modules["__main__"]
            sys.modules["__main__"] = mod
            try:
                exec(compile(open(UTILITY).read(), UTILITY, "exec"), mod.__dict__)
            finally:
                sys.modules["__main__"] = saved
    except SystemExit as e:
        code = e.code
    except Exception as e:                                      # noqa: BLE001  (the reference's uncaught exceptions are results too)
        code, exc = "exception", {"type": type(e).__name__, "message": norm(str(e))}
    finally:
        sys.argv = old
    return (norm(code) if isinstance(code, str) else code), exc, norm(so.getvalue()), norm(se.getvalue())


D, C6 = "{DIN}/", "{GOLDEN}/c6_plot/expected/"
FAI = ["-r", D + "ref.fa.fai"]
CASES = {
    "dpv2_both_whole": FAI + ["--hifi", D + "hifi.depth.gz", "--nano", D + "ont.depth.gz", "-w", "100", "-f", "png"],
    "dpv2_text_regions": FAI + ["--hifi", D + "hifi.depth", "--regions", D + "regions.bed", "-f", "png"],
    "dpv2_ont_region_ignored_flags": FAI + ["--nano", D + "ont.depth.gz", "--region", "s1:8000-9500", "-w", "64", "--min-safe-depth", "10",
                                            "--max-depth-ratio", "2", "-f", "png"],
    "dpv2_default_pdf": FAI + ["--hifi", D + "hifi.depth.gz", "--region", "s2:0-4095"],
    "dpv2_one_base_short": FAI + ["--hifi", D + "hifi.depth.gz", "--nano", D + "ont_s2_short.depth.gz", "-w", "500", "-f", "png"],
    "dpv2_c6_pair": ["-r", "{DIN}/c6.fai", "--hifi", C6 + "GCI_hifi.depth.gz", "--nano", C6 + "GCI_nano.depth.gz", "-w", "2000", "-f", "png"],
}
# (name, argv, whether the run gets as far as device work in this implementation); each in an output directory of its own
ERRORS = [
    ("no_depth_file", FAI, False),
    ("bad_region", FAI + ["--hifi", D + "hifi.depth.gz", "--region", "s1:100", "-o", "{OUT}"], False),
    ("fai_missing", ["-r", D + "nope.fai", "--hifi", D + "hifi.depth.gz", "-o", "{OUT}"], False),
    ("depth_file_missing", FAI + ["--hifi", D + "hifi.depth.gz", "--nano", D + "nope.depth.gz", "-o", "{OUT}"], False),
    ("text_named_gz", FAI + ["--hifi", D + "text_named.depth.gz", "-o", "{OUT}"], True),
    ("svg", FAI + ["--nano", D + "ont.depth.gz", "--region", "s3:0-699", "-f", "svg", "-o", "{OUT}"], True),
]


def make_c6_fai() -> None:
    """A .fai for the depth files of the c6 golden (files of the reference's own writer): names and lengths from the file."""
    with gzip.open(os.path.join(GOLDEN, "c6_plot", "expected", "GCI_hifi.depth.gz"), "rt") as f, \
            open(os.path.join(DIN, "c6.fai"), "w") as out:
        name, n = None, 0
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    out.write("%s\t%d\n" % (name, n))
                name, n = line.strip()[1:], 0
            else:
                n += 1
        out.write("%s\t%d\n" % (name, n))


def make_cases() -> None:
    for case, argv in CASES.items():
        case_dir = os.path.join(GOLDEN, case)
        shutil.rmtree(case_dir, ignore_errors=True)
        os.makedirs(case_dir)
        tmp = tempfile.mkdtemp(prefix="gci_dpv2_")
        out = os.path.join(tmp, "out")
        code, exc, so, se = run_utility(argv + ["-o", "{OUT}"], out)
        assert code == "completed" and exc is None, (case, code, exc, so[-500:], se[-500:])
        files = sorted(os.listdir(out))
        assert 0 < len(files) <= 4, (case, files)
        for fn in files:
            if fn.endswith(".png"):
                os.makedirs(os.path.join(case_dir, "expected"), exist_ok=True)
                shutil.copy(os.path.join(out, fn), os.path.join(case_dir, "expected", fn))
        with open(os.path.join(case_dir, "manifest.json"), "w") as f:
            json.dump({"argv": argv + ["-o", "{OUT}"], "stdout": so, "stderr": se, "files": files}, f, indent=1)
        shutil.rmtree(tmp)
        print(case, "->", ", ".join(files))


def _tree(root: str):
    return sorted(os.path.relpath(os.path.join(d, fn), root) for d, _, fns in os.walk(root) for fn in fns) if os.path.isdir(root) else []


def make_errors() -> None:
    os.environ["COLUMNS"] = "100"
    results = []
    for name, argv, gpu in ERRORS:
        tmp = tempfile.mkdtemp(prefix="gci_dpv2_err_")
        out = os.path.join(tmp, "out")
        cwd = os.getcwd()
        os.chdir(tmp)                                            # (no -o: the utility makes ./images)
        try:
            code, exc, so, se = run_utility(argv, out)
        finally:
            os.chdir(cwd)
        results.append({"name": name, "argv": argv, "gpu": gpu, "exit": code, "exception": exc, "stdout": so, "stderr": se,
                        "files": _tree(out), "made_out": os.path.isdir(out)})
        print("dpv2_errors:", name, "->", repr(code)[:90], exc)
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(GOLDEN, "dpv2_errors.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    if not (load_reference.available() and os.path.exists(UTILITY)):
        sys.exit("needs the reference utility (build container only)")
    make_inputs()
    make_c6_fai()
    make_cases()
    make_errors()
