#!/usr/bin/env python3
"""Generate the GCI_score.py fixtures under tests/golden/score_*/ by running the UNMODIFIED reference utility
(utility/GCI_score.py of the reference tree tools/load_reference.py finds) through its own `__main__` block, with tools/ref_shim standing in for
Bio (as tools/load_reference.py does for GCI.py).  Only data is written: small hand-made inputs, the files the utility wrote,
its transcript and its exit.  Nothing at test time needs the reference.

    python tools/make_golden_score.py

  tests/golden/score_inputs/                 the hand-made inputs (assembly, depth files of both writers' layouts, BED files)
  tests/golden/score_<case>/manifest.json    argv, stdout, exit of a run that completes; expected/ the files it wrote
  tests/golden/score_errors.json             the runs that end early: argv, exit or exception, stdout, stderr

In argv, {GOLDEN} stands for tests/golden, {IN} for tests/golden/score_inputs and {OUT} for the output directory.  The depth
files of the GCI.py goldens (c1, c3, c5, c7) are used where they lie."""
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

UTILITY = os.path.join(os.path.dirname(load_reference.REF), "utility", "GCI_score.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")
IN = os.path.join(GOLDEN, "score_inputs")

CONTIGS = (("ctgA", 6000), ("ctgB", 2500), ("ctgC", 900))
GAPS = {"ctgA": [(3000, 3100)], "ctgC": [(850, 900)]}


def depth_track(length: int, rng) -> np.ndarray:
    """Piecewise-constant depths around 30 with a few zero and low stretches."""
    d = np.empty(length, dtype=np.int64)
    i = 0
    while i < length:
        n = int(rng.integers(20, 400))
        r = rng.random()
        d[i:i + n] = 0 if r < 0.08 else int(rng.integers(1, 4)) if r < 0.2 else int(rng.integers(20, 45))
        i += n
    return d


def text_of(name: str, d, eol: str = "\n") -> str:
    return f">{name}{eol}" + "".join(f"{int(v)}{eol}" for v in d)


def reference_style(path: str, items, chunk_lines: int = 700) -> None:
    """One member per (contig, chunk of lines), written by Python's gzip at level 9 with the file name in the header -- the
    layout of the reference's own writer."""
    with open(path, "wb") as f:
        for name, d in items:
            lines = [f"{int(v)}\n" for v in d]
            for k in range(0, max(len(lines), 1), chunk_lines):
                body = (f">{name}\n" if k == 0 else "") + "".join(lines[k:k + chunk_lines])
                with gzip.GzipFile(filename=os.path.basename(path), mode="wb", compresslevel=9, fileobj=f, mtime=0) as g:
                    g.write(body.encode())


def single_member(path: str, text: str) -> None:
    with open(path, "wb") as f:
        f.write(gzip.compress(text.encode(), 9, mtime=0))


def write_fasta(path: str, contigs, gaps) -> None:
    rng = np.random.default_rng(5)
    with open(path, "w") as f:
        for name, n in contigs:
            s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
            for a, b in gaps.get(name, []):
                s[a:b] = ord("N")
            seq = s.tobytes().decode()
            f.write(f">{name} synthetic\n" + "".join(seq[i:i + 60] + "\n" for i in range(0, n, 60)))


def make_inputs() -> None:
    shutil.rmtree(IN, ignore_errors=True)
    os.makedirs(IN)
    rng = np.random.default_rng(2024)
    write_fasta(os.path.join(IN, "ref.fa"), CONTIGS, GAPS)
    tr = {name: depth_track(n, rng) for name, n in CONTIGS}
    tr2 = {name: depth_track(n, rng) for name, n in CONTIGS}
    # reference-style members (FNAME, one member per chunk)
    reference_style(os.path.join(IN, "refstyle.depth.gz"), [(n, tr[n]) for n, _ in CONTIGS])
    # one member; CRLF line ends, '+' and blank-padded numbers, a repeated header (its last segment wins, first place kept)
    early_c = depth_track(400, rng)
    quirks = (text_of("ctgC", early_c) + text_of("ctgA", tr2["ctgA"], "\r\n")
              + ">ctgB\n" + "".join((f"+{v}\n" if k % 7 == 0 else f"  {v} \n" if k % 11 == 0 else f"{v}\n")
                                     for k, v in enumerate(tr2["ctgB"].tolist()))
              + text_of("ctgC", tr2["ctgC"]))
    single_member(os.path.join(IN, "quirks.depth.gz"), quirks)
    # one member without a final newline
    single_member(os.path.join(IN, "nonl.depth.gz"), "".join(text_of(n, tr[n] // 2 + 1) for n, _ in CONTIGS)[:-1])
    # for the refusals: a contig the assembly lacks, a contig shorter than in the other file, a contig of the assembly missing
    single_member(os.path.join(IN, "extra.depth.gz"), "".join(text_of(n, tr[n]) for n, _ in CONTIGS) + text_of("zz", tr["ctgC"]))
    single_member(os.path.join(IN, "short.depth.gz"), "".join(text_of(n, tr[n][:-100] if n == "ctgB" else tr[n]) for n, _ in CONTIGS))
    single_member(os.path.join(IN, "partial.depth.gz"), "".join(text_of(n, tr[n]) for n, _ in CONTIGS[:2]))
    with open(os.path.join(IN, "regions.bed"), "w") as f:
        f.write("ctgA\t500\t4500\nctgB\t0\t2500\nctgC\t100\t100\n")
    with open(os.path.join(IN, "hifi.bed"), "w") as f:
        f.write("ctgA\t900\t1300\nctgA\t3000\t3100\nctgB\t40\t700\n")
    with open(os.path.join(IN, "nano.bed"), "w") as f:
        f.write("ctgB\t1200\t1290\nctgC\t300\t340\n")
    with open(os.path.join(IN, "unknown.bed"), "w") as f:
        f.write("ctgA\t10\t20\nzz\t0\t5\n")


def run_utility(argv_t, out: str):
    """The utility's __main__ as `python GCI_score.py ...` would run it: (exit, exception, stdout, stderr), normalised."""
    load_reference.load()                                       # (the stand-ins on sys.path)
    sub = lambda a: a.replace("{GOLDEN}", GOLDEN).replace("{IN}", IN).replace("{OUT}", out)      # noqa: E731
    norm = lambda t: t.replace(out, "{OUT}").replace(IN, "{IN}").replace(GOLDEN, "{GOLDEN}")     # noqa: E731
    so, se = io.StringIO(), io.StringIO()
    old = sys.argv
    sys.argv = ["GCI_score.py"] + [sub(a) for a in argv_t]
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
        code, exc = "exception", {"type": type(e).__name__, "message": str(e)}
    finally:
        sys.argv = old
    return (norm(code) if isinstance(code, str) else code), exc, norm(so.getvalue()), norm(se.getvalue())


G = "{GOLDEN}/"
I = "{IN}/"
CASES = {
    "score_c1": ["-r", G + "c1_single_bam/inputs/ref.fa", "--hifi", G + "c1_single_bam/expected/GCI.depth.gz"],
    "score_c5_chrs": ["-r", G + "c5_two_type/inputs/ref.fa", "--nano", G + "c5_two_type/expected/GCI_nano.depth.gz",
                      "--chrs", "mat_chr1,pat_chr1", "-ts", "1", "-fl", "20"],
    "score_c5_three_types": ["-r", G + "c5_two_type/inputs/ref.fa", "--hifi", G + "c5_two_type/expected/GCI_hifi.depth.gz",
                             "--nano", G + "c5_two_type/expected/GCI_nano.depth.gz",
                             "--two-type", G + "c5_two_type/expected/GCI_two_type.depth.gz", "-ts", "2",
                             "-R", G + "c5_two_type/inputs/regions.bed", "-f"],
    "score_c7_hifi_nano": ["-r", G + "c7_t2t_geometry/inputs/ref.fa", "--hifi", G + "c7_t2t_geometry/expected/GCI_hifi.depth.gz",
                           "--nano", G + "c7_t2t_geometry/expected/GCI_nano.depth.gz", "-dp", "0.01", "-ts", "1", "-f"],
    "score_refstyle_regions": ["-r", I + "ref.fa", "--two-type", I + "refstyle.depth.gz", "-R", I + "regions.bed", "-ts", "3"],
    "score_quirks": ["-r", I + "ref.fa", "--hifi", I + "quirks.depth.gz", "--nano", I + "nonl.depth.gz", "-f", "-fl", "5"],
    "score_bed": ["-r", I + "ref.fa", "--bed", "--hifi", I + "hifi.bed", "--nano", I + "nano.bed", "--chrs", "ctgA,ctgB"],
}
# (name, argv, whether the run gets as far as device work in this implementation)
ERRORS = [
    ("help", ["-h"], False),
    ("no_arguments", [], False),
    ("no_input", ["-r", I + "ref.fa"], False),
    ("hifi_missing", ["-r", I + "ref.fa", "--hifi", I + "nope.depth.gz"], False),
    ("no_reference", ["--hifi", I + "nonl.depth.gz"], False),
    ("reference_missing", ["-r", I + "nope.fa", "--hifi", I + "nonl.depth.gz"], False),
    ("bed_with_regions", ["-r", I + "ref.fa", "--bed", "--hifi", I + "hifi.bed", "-R", I + "regions.bed"], False),
    ("prefix_with_slash", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-o", "x/", "-d", "{OUT}"], False),
    ("chrs_unknown", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "--chrs", "ctgA,zz", "-d", "{OUT}"], False),
    ("contig_not_in_fasta", ["-r", I + "ref.fa", "--hifi", I + "extra.depth.gz", "-d", "{OUT}/a"], True),
    ("lengths_differ", ["-r", I + "ref.fa", "--two-type", I + "nonl.depth.gz", "--nano", I + "short.depth.gz", "-d", "{OUT}/b", "-f"], True),
    ("second_type_exists", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "--nano", I + "refstyle.depth.gz", "-d", "{OUT}/c"], True),
    ("gaps_exist", ["-r", I + "ref.fa", "--hifi", I + "nonl.depth.gz", "-d", "{OUT}/c"], True),           # (after the one above)
    ("fasta_contig_missing", ["-r", I + "ref.fa", "--hifi", I + "partial.depth.gz", "-d", "{OUT}/d"], True),
    # the depth file of a `--chrs` run of GCI.py holds only those contigs: compute_index meets the others and raises
    ("depth_of_a_chrs_run", ["-r", G + "c3_three_bam_chrs/inputs/ref.fa", "--hifi", G + "c3_three_bam_chrs/expected/GCI.depth.gz",
                             "--chrs", "chrA,chrC", "-ts", "1", "-d", "{OUT}/f"], True),
    ("bed_contig_unknown", ["-r", I + "ref.fa", "--bed", "--hifi", I + "unknown.bed", "-d", "{OUT}/e"], True),
]


def make_cases() -> None:
    for case, argv in CASES.items():
        case_dir = os.path.join(GOLDEN, case)
        shutil.rmtree(case_dir, ignore_errors=True)
        os.makedirs(os.path.join(case_dir, "expected"))
        tmp = tempfile.mkdtemp(prefix="gci_score_")
        out = os.path.join(tmp, "out")
        code, exc, so, se = run_utility(argv + ["-d", "{OUT}", "-o", "GCI"], out)
        assert code == "completed" and exc is None, (case, code, exc, so[-500:])
        for fn in sorted(os.listdir(out)):
            shutil.copy(os.path.join(out, fn), os.path.join(case_dir, "expected", fn))
        with open(os.path.join(case_dir, "manifest.json"), "w") as f:
            json.dump({"argv": argv + ["-d", "{OUT}", "-o", "GCI"], "stdout": so, "stderr": se, "files": sorted(os.listdir(out))},
                      f, indent=1)
        shutil.rmtree(tmp)
        print(case, "->", ", ".join(sorted(os.listdir(os.path.join(case_dir, "expected")))))


def make_errors() -> None:
    tmp = tempfile.mkdtemp(prefix="gci_score_err_")
    out = os.path.join(tmp, "out")
    os.environ["COLUMNS"] = "100"
    results = []
    for name, argv, gpu in ERRORS:
        code, exc, so, se = run_utility(argv, out)
        results.append({"name": name, "argv": argv, "gpu": gpu, "exit": code, "exception": exc, "stdout": so, "stderr": se})
        print("score_errors:", name, "->", repr(code)[:80], exc)
    shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(GOLDEN, "score_errors.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    if not (load_reference.available() and os.path.exists(UTILITY)):
        sys.exit("needs the reference utility (build container only)")
    make_inputs()
    make_cases()
    make_errors()
