"""plot_depth.py off the GPU: the refusals of the reference utility that end before any device work, transcript included
(tests/golden/plot_errors.json, tools/make_golden_plot.py), the additions to gci_amd.plot that leave `GCI.py -p` as it was, and the
entry point."""
import contextlib
import inspect
import io
import json
import os

import pytest

from golden_util import GOLDEN

SCENARIOS = json.load(open(os.path.join(GOLDEN, "plot_errors.json")))
SCORE_IN = os.path.join(GOLDEN, "score_inputs")
PLOT_IN = os.path.join(GOLDEN, "plot_inputs")


def sub(t, out_root):
    return t.replace("{GOLDEN}", GOLDEN).replace("{IN}", SCORE_IN).replace("{PIN}", PLOT_IN).replace("{OUT}", out_root)


def norm(t, out_root):
    return t.replace(out_root, "{OUT}").replace(PLOT_IN, "{PIN}").replace(SCORE_IN, "{IN}").replace(GOLDEN, "{GOLDEN}")


def tree(root):
    return sorted(os.path.relpath(os.path.join(d, fn), root) for d, _, fns in os.walk(root) for fn in fns) if os.path.isdir(root) else []


def run_plot_scenario(sc, out_root, monkeypatch):
    from gci_amd import plot_cli
    monkeypatch.setenv("COLUMNS", "100")
    so, se = io.StringIO(), io.StringIO()
    code, exc = "completed", None
    try:
        with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
            plot_cli.main(["plot_depth.py"] + [sub(a, out_root) for a in sc["argv"]])
    except SystemExit as e:
        code = e.code
    except Exception as e:                                 # noqa: BLE001
        code, exc = "exception", {"type": type(e).__name__, "message": norm(str(e), out_root)}
    got = {"exit": norm(code, out_root) if isinstance(code, str) else code, "exception": exc, "stdout": norm(so.getvalue(), out_root),
           "stderr": norm(se.getvalue(), out_root), "files": tree(out_root)}
    assert got == {k: sc[k] for k in got}, sc["name"]


@pytest.mark.parametrize("sc", [s for s in SCENARIOS if not s["gpu"]], ids=lambda s: s["name"])
def test_plot_refused_before_any_gpu_work(sc, tmp_path, monkeypatch):
    run_plot_scenario(sc, str(tmp_path / "out"), monkeypatch)


def test_the_scenarios_cover_what_the_utility_refuses():
    names = {s["name"] for s in SCENARIOS}
    assert {"no_dmean", "dmean_count", "contig_not_in_fasta", "contig_sets_differ", "lengths_differ", "region_on_unknown_contig"} <= names
    no_dmean = next(s for s in SCENARIOS if s["name"] == "no_dmean")
    assert no_dmean["exception"] == {"type": "AttributeError", "message": "'NoneType' object has no attribute 'split'"}
    assert no_dmean["files"] == ["a/GCI.gaps.bed"]                      # (it dies after it has written the gaps file)


def test_plot_additions_leave_the_defaults_of_gci_py_alone():
    from gci_amd import plot
    sig = inspect.signature(plot.figure_spec)
    assert sig.parameters["images_dir"].default is None
    assert "depth_mean" not in inspect.signature(plot.plot_depth).parameters
    assert inspect.signature(plot.plot_depth_utility).parameters["depth_mean"].default is None
    spec = plot.figure_spec([], "t", [], [], 0.0, 0, 0.1, 0.005, 0, 10, "png", "D", "P", 5, False, 0)
    assert spec.path == "D/images/P.t.png"
    assert plot.figure_spec([], "t", [], [], 0.0, 3, 0.1, 0.005, 0, 10, "pdf", "D", "P", 5, True, 0, images_dir="D").path == "D/P.t:3-5.pdf"


def test_entry_point_exists_and_imports_no_torch():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, runpy; sys.argv = ['plot_depth.py', '-r', 'x.fa']\n"
            "try:\n    runpy.run_path(%r, run_name='__main__')\nexcept SystemExit as e:\n    print(repr(e.code))\n"
            "print('torch' in sys.modules)\n") % os.path.join(root, "plot_depth.py")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=120)
    assert r.stdout.strip().splitlines() == [repr('ERROR!!! Please input at least one depth file\n'
                                                  'Please read the help message using "-h" or "--help"'), "False"], r.stderr
