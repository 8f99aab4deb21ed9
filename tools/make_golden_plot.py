#!/usr/bin/env python3
"""Generate the plot_depth.py fixtures under tests/golden/plot_*/ by running the UNMODIFIED reference utility (utility/plot_depth.py
of the reference tree tools/load_reference.py finds) through its own `__main__` block, with tools/ref_shim standing in for Bio and
matplotlib's Agg backend.  Only data is written: two hand-made region files, the files the utility wrote, its transcript and its
exit.  Nothing at test time needs the reference.

    python tools/make_golden_plot.py

  tests/golden/plot_inputs/                 region files of this tool's own
  tests/golden/plot_<case>/manifest.json    argv, stdout, stderr of a run that completes, the names of the files it wrote;
                                            expected/ those files (PDF figures are not kept: a test checks that they exist)
  tests/golden/plot_errors.json             the runs that end early: argv, exit or exception, stdout, stderr, the files left behind

In argv, {GOLDEN} stands for tests/golden, {IN} for tests/golden/score_inputs, {PIN} for tests/golden/plot_inputs and {OUT} for the
output directory.  The depth files are those of the GCI.py goldens (c5, c6, c7) and of tools/make_golden_score.py."""
from __future__ import annotations

import contextlib
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

import load_reference  # noqa: E402

UTILITY = os.path.join(os.path.dirname(load_reference.REF), "utility", "plot_depth.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")
IN = os.path.join(GOLDEN, "score_inputs")
PIN = os.path.join(GOLDEN, "plot_inputs")


def make_inputs() -> None:
    shutil.rmtree(PIN, ignore_errors=True)
    os.makedirs(PIN)
    with open(os.path.join(PIN, "c7_regions.bed"), "w") as f:            # (chrM is shorter than the window: the utility warns)
        f.write("chr21\t1000\t30000\nchrM\t0\t9000\n")
    with open(os.path.join(PIN, "unknown_contig.bed"), "w") as f:
        f.write("ctgA\t10\t2000\nzz\t0\t5\n")


def run_utility(argv_t, out: str):
    """The utility's __main__ as `python plot_depth.py ...` would run it: (exit, exception, stdout, stderr), normalised."""
    shim = os.path.join(ROOT, "tools", "ref_shim")
    if shim not in sys.path:
        sys.path.insert(0, shim)
    sub = lambda a: a.replace("{GOLDEN}", GOLDEN).replace("{IN}", IN).replace("{PIN}", PIN).replace("{OUT}", out)      # noqa: E731
    norm = lambda t: t.replace(out, "{OUT}").replace(PIN, "{PIN}").replace(IN, "{IN}").replace(GOLDEN, "{GOLDEN}")     # noqa: E731
    so, se = io.StringIO(), io.StringIO()
    old = sys.argv
    sys.argv = ["plot_depth.py"] + [sub(a) for a in argv_t]
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


G, I, P = "{GOLDEN}/", "{IN}/", "{PIN}/"
C5, C6, C7 = G + "c5_two_type/", G + "c6_plot/", G + "c7_t2t_geometry/"
CASES = {
    "plot_c6_two_types": ["-r", C6 + "inputs/ref.fa", "--hifi", C6 + "expected/GCI_hifi.depth.gz", "--nano", C6 + "expected/GCI_nano.depth.gz",
                          "-dmean", "20,15", "-ws", "2000"],
    "plot_c6_regions_hifi": ["-r", C6 + "inputs/ref.fa", "--hifi", C6 + "expected/GCI_hifi.depth.gz", "-R", C6 + "inputs/regions.bed",
                             "-dmean", "18.5", "-ws", "500", "-ts", "1", "-dmin", "0.3", "-dmax", "2", "-f"],
    "plot_c7_regions_two_types": ["-r", C7 + "inputs/ref.fa", "--hifi", C7 + "expected/GCI_hifi.depth.gz",
                                  "--nano", C7 + "expected/GCI_nano.depth.gz", "-R", P + "c7_regions.bed", "-dmean", "30,22", "-ws", "10000"],
    "plot_c5_nano_pdf": ["-r", C5 + "inputs/ref.fa", "--nano", C5 + "expected/GCI_nano.depth.gz", "-dmean", "25", "-it", "PDF"],
}
# (name, argv, whether the run gets as far as device work in this implementation); they share one output directory, in order
ERRORS = [
    ("help", ["-h"], False),
    ("no_arguments", [], False),
    ("no_input", ["-r", I + "ref.fa"], False),
    ("hifi_missing", ["-r", I + "ref.fa", "--hifi", I + "nope.depth.gz"], False),
    ("nano_missing", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "--nano", I + "nope.depth.gz"], False),
    ("no_reference", ["--hifi", I + "nonl.depth.gz"], False),
    ("reference_missing", ["-r", I + "nope.fa", "--hifi", I + "nonl.depth.gz"], False),
    ("prefix_with_slash", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-o", "x/", "-d", "{OUT}"], False),
    ("no_dmean", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-d", "{OUT}/a"], True),
    ("gaps_exist", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-dmean", "30", "-d", "{OUT}/a"], True),       # (after the one above)
    ("dmean_count", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-dmean", "30,20", "-d", "{OUT}/b"], True),
    ("dmean_not_a_number", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-dmean", "thirty", "-d", "{OUT}/b", "-f"], True),
    ("contig_not_in_fasta", ["-r", I + "ref.fa", "--hifi", I + "extra.depth.gz", "-dmean", "30", "-d", "{OUT}/c"], True),
    ("ont_contig_not_in_fasta", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "--nano", I + "extra.depth.gz", "-dmean", "30,30",
                                 "-d", "{OUT}/c", "-f"], True),
    ("contig_sets_differ", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "--nano", I + "partial.depth.gz", "-dmean", "30,30",
                            "-d", "{OUT}/c", "-f"], True),
    ("lengths_differ", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "--nano", I + "short.depth.gz", "-dmean", "30,30",
                        "-d", "{OUT}/c", "-f"], True),
    ("regions_missing", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-dmean", "30", "-R", P + "nope.bed", "-d", "{OUT}/c", "-f"], True),
    ("region_on_unknown_contig", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-dmean", "30", "-R", P + "unknown_contig.bed",
                                  "-d", "{OUT}/c", "-f"], True),
    ("image_type", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-dmean", "30", "-it", "svg", "-d", "{OUT}/c", "-f"], True),
]


def make_cases() -> None:
    for case, argv in CASES.items():
        case_dir = os.path.join(GOLDEN, case)
        shutil.rmtree(case_dir, ignore_errors=True)
        os.makedirs(os.path.join(case_dir, "expected"))
        tmp = tempfile.mkdtemp(prefix="gci_plot_")
        out = os.path.join(tmp, "out")
        code, exc, so, se = run_utility(argv + ["-d", "{OUT}", "-o", "GCI"], out)
        assert code == "completed" and exc is None, (case, code, exc, so[-500:], se[-500:])
        for fn in sorted(os.listdir(out)):
            if not fn.endswith(".pdf"):
                shutil.copy(os.path.join(out, fn), os.path.join(case_dir, "expected", fn))
        with open(os.path.join(case_dir, "manifest.json"), "w") as f:
            json.dump({"argv": argv + ["-d", "{OUT}", "-o", "GCI"], "stdout": so, "stderr": se, "files": sorted(os.listdir(out))},
                      f, indent=1)
        shutil.rmtree(tmp)
        print(case, "->", ", ".join(sorted(os.listdir(os.path.join(case_dir, "expected")))))


def _tree(root: str):
    return sorted(os.path.relpath(os.path.join(d, fn), root) for d, _, fns in os.walk(root) for fn in fns) if os.path.isdir(root) else []


def make_errors() -> None:
    tmp = tempfile.mkdtemp(prefix="gci_plot_err_")
    out = os.path.join(tmp, "out")
    os.environ["COLUMNS"] = "100"
    results = []
    for name, argv, gpu in ERRORS:
        code, exc, so, se = run_utility(argv, out)
        results.append({"name": name, "argv": argv, "gpu": gpu, "exit": code, "exception": exc, "stdout": so, "stderr": se,
                        "files": _tree(out)})
        print("plot_errors:", name, "->", repr(code)[:90], exc)
    shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(GOLDEN, "plot_errors.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    if not (load_reference.available() and os.path.exists(UTILITY)):
        sys.exit("needs the reference utility (build container only)")
    make_inputs()
    make_cases()
    make_errors()
