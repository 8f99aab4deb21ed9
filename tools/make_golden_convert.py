#!/usr/bin/env python3
"""Generate the convert_samtools_depth.py fixtures under tests/golden/convert_*/ by running the UNMODIFIED reference utility
(utility/convert_samtools_depth.py of the reference tree tools/load_reference.py finds) through its own `__main__` block.  Only
data is written: small hand-made inputs, the DECOMPRESSED payload of the file the utility wrote, its transcript and its exit.
Nothing at test time needs the reference.

    python tools/make_golden_convert.py

  tests/golden/convert_inputs/                 the hand-made `samtools depth` texts
  tests/golden/convert_<case>/manifest.json    argv, stdout, stderr of a run that completes, and whether the text is inside the
                                               device's strict grammar; expected.depth = the payload of the .depth.gz it wrote
  tests/golden/convert_errors.json             the runs that end early: argv, exit or exception, stdout, stderr, whether the
                                               output file exists afterwards

In argv, {IN} stands for tests/golden/convert_inputs and {OUT} for the output directory."""
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import load_reference  # noqa: E402

UTILITY = os.path.join(os.path.dirname(load_reference.REF), "utility", "convert_samtools_depth.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")
IN = os.path.join(GOLDEN, "convert_inputs")


def samtools_text(items) -> bytes:
    """`samtools depth -a`: name, 1-based position, depth."""
    return b"".join(b"%s\t%d\t%d\n" % (name.encode(), k + 1, int(v)) for name, d in items for k, v in enumerate(d))


def depths(n: int, rng) -> np.ndarray:
    d = np.repeat(rng.integers(0, 60, n // 7 + 1), 7)[:n]
    d[rng.integers(0, n, 3)] = [0, 2147483647, 1000000000]
    return d


def make_inputs() -> None:
    shutil.rmtree(IN, ignore_errors=True)
    os.makedirs(IN)
    rng = np.random.default_rng(77)
    three = [("chr1", depths(2600, rng)), ("chr2_hap1", depths(1200, rng)), ("chrM", depths(90, rng))]
    files = {
        "three.depth": samtools_text(three),
        # a name that returns gets a second header and a segment of its own
        "returns.depth": samtools_text([("ctgA", depths(700, rng)), ("ctgB", depths(300, rng)), ("ctgA", depths(450, rng))]),
        "nonl.depth": samtools_text(three[1:])[:-1],
        # outside what samtools writes, inside what the utility takes: leading zeros, a sign, blank-padded depth, CRLF, a lone CR as
        # a line end, a blank inside a name, an empty position column, blanks around the line
        "quirks.depth": (b"ctg 1\t1\t007\nctg 1\t2\t+3\nctg 1\t\t12\r\nctg 1\t4\t 4 \r\nctg2\t1\t5\rctg2\t2\t6\n  ctg2\t3\t7\n"
                         b"ctg3\tx\t-1\nctg3\t2\t1e3\n"),
        "empty_line.depth": b"a\t1\t5\n\na\t2\t6\n",
        "two_fields.depth": b"a\t1\t5\na\t6\n",
        "four_fields.depth": b"a\t1\t5\na\t2\t6\t7\n",
        "empty_depth.depth": b"a\t1\t5\na\t2\t\n",
    }
    for fn, data in files.items():
        with open(os.path.join(IN, fn), "wb") as f:
            f.write(data)


def run_utility(argv_t, out: str):
    """The utility as `python convert_samtools_depth.py ...` would run it: (exit, exception, stdout, stderr), normalised."""
    sub = lambda a: a.replace("{IN}", IN).replace("{OUT}", out)        # noqa: E731
    norm = lambda t: t.replace(out, "{OUT}").replace(IN, "{IN}")       # noqa: E731
    so, se = io.StringIO(), io.StringIO()
    old = sys.argv
    sys.argv = ["convert_samtools_depth.py"] + [sub(a) for a in argv_t]
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


# case -> (input, inside the device's strict grammar)
CASES = {"convert_three": ("three.depth", True), "convert_returns": ("returns.depth", True), "convert_nonl": ("nonl.depth", True),
         "convert_quirks": ("quirks.depth", False)}
# (name, argv, whether the run gets as far as device work in this implementation)
ERRORS = [
    ("no_arguments", [], False),
    ("one_argument", ["{IN}/three.depth"], False),
    ("input_missing", ["{IN}/nope.depth", "{OUT}/missing"], False),
    ("empty_line", ["{IN}/empty_line.depth", "{OUT}/empty_line"], True),
    ("two_fields", ["{IN}/two_fields.depth", "{OUT}/two_fields"], True),
    ("four_fields", ["{IN}/four_fields.depth", "{OUT}/four_fields"], True),
    ("empty_depth", ["{IN}/empty_depth.depth", "{OUT}/empty_depth"], True),
]


def make_cases() -> None:
    for case, (fn, strict) in CASES.items():
        case_dir = os.path.join(GOLDEN, case)
        shutil.rmtree(case_dir, ignore_errors=True)
        os.makedirs(case_dir)
        out = tempfile.mkdtemp(prefix="gci_convert_")
        argv = ["{IN}/" + fn, "{OUT}/GCI"]
        code, exc, so, se = run_utility(argv, out)
        assert code == "completed" and exc is None, (case, code, exc)
        with gzip.open(os.path.join(out, "GCI.depth.gz"), "rb") as g, open(os.path.join(case_dir, "expected.depth"), "wb") as f:
            f.write(g.read())
        with open(os.path.join(case_dir, "manifest.json"), "w") as f:
            json.dump({"argv": argv, "stdout": so, "stderr": se, "strict": strict, "files": sorted(os.listdir(out))}, f, indent=1)
        shutil.rmtree(out)
        print(case, "->", os.path.getsize(os.path.join(case_dir, "expected.depth")), "bytes of payload")


def make_errors() -> None:
    out = tempfile.mkdtemp(prefix="gci_convert_err_")
    results = []
    for name, argv, gpu in ERRORS:
        code, exc, so, se = run_utility(argv, out)
        made = os.path.exists(argv[-1].replace("{OUT}", out) + ".depth.gz") if len(argv) == 2 else None
        results.append({"name": name, "argv": argv, "gpu": gpu, "exit": code, "exception": exc, "stdout": so, "stderr": se,
                        "output_exists": made})
        print("convert_errors:", name, "->", repr(code)[:80], exc)
    shutil.rmtree(out, ignore_errors=True)
    with open(os.path.join(GOLDEN, "convert_errors.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    if not (load_reference.available() and os.path.exists(UTILITY)):
        sys.exit("needs the reference utility (build container only)")
    make_inputs()
    make_cases()
    make_errors()
