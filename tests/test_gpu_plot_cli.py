"""plot_depth.py on the GPU: the plotting command line against the files and transcripts of the UNMODIFIED reference utility
(tests/golden/plot_*, tools/make_golden_plot.py) -- file names, the gaps file, stdout and stderr, the PNG figures pixel for pixel --,
its refusals that get as far as device work, and the entry point as a user starts it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLDEN
from gci_amd import pipeline
from test_plot_cli_cpu import SCENARIOS, norm, run_plot_scenario, sub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(d for d in os.listdir(GOLDEN) if d.startswith("plot_") and os.path.isdir(os.path.join(GOLDEN, d, "expected")))


def _manifest(case):
    with open(os.path.join(GOLDEN, case, "manifest.json")) as f:
        return json.load(f)


def _pixels(path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.image as mpimg                     # (the reader of golden_util.images)
    return mpimg.imread(path)


def _same_outputs(out, case, m):
    want_dir = os.path.join(GOLDEN, case, "expected")
    assert sorted(os.listdir(out)) == m["files"]
    for fn in sorted(os.listdir(want_dir)):
        got, want = os.path.join(out, fn), os.path.join(want_dir, fn)
        if fn.endswith(".png"):
            a, b = _pixels(got), _pixels(want)
            assert a.shape == b.shape and np.array_equal(a, b), fn
        else:
            assert open(got, "rb").read() == open(want, "rb").read(), fn
    for fn in m["files"]:
        assert os.path.getsize(os.path.join(out, fn)) > 0, fn            # (PDF figures: only that they are there)


def test_the_cases_are_there():
    assert len(CASES) >= 4 and any(fn.endswith(".pdf") for c in CASES for fn in _manifest(c)["files"])


@pytest.mark.parametrize("case", CASES)
def test_plot_cli_reproduces_the_reference_utility(engine, case, tmp_path, capsys):
    from gci_amd import plot_cli
    out = str(tmp_path / "out")
    m = _manifest(case)
    pipeline._ENGINE = engine
    plot_cli.main(["plot_depth.py"] + [sub(a, out) for a in m["argv"]])
    cap = capsys.readouterr()
    assert norm(cap.out, out) == m["stdout"] and norm(cap.err, out) == m["stderr"]
    _same_outputs(out, case, m)
    # refuses to overwrite without -f, like the reference; -f writes the same files again
    plain = [sub(a, out) for a in m["argv"] if a != "-f"]
    with pytest.raises(SystemExit) as e:
        plot_cli.main(["plot_depth.py"] + plain)
    assert "exists" in str(e.value) and "--force" in str(e.value)
    plot_cli.main(["plot_depth.py"] + plain + ["-f"])
    _same_outputs(out, case, m)
    capsys.readouterr()


def test_plot_refusals_after_device_work(engine, tmp_path, monkeypatch):
    """The scenarios of plot_errors.json that get as far as the device, in their order (one of them finds the gaps file the one
    before it wrote): the exit message, or the utility's uncaught exception, the transcript up to it and the files left behind."""
    pipeline._ENGINE = engine
    out = str(tmp_path / "out")
    for sc in [s for s in SCENARIOS if s["gpu"]]:
        run_plot_scenario(sc, out, monkeypatch)


def test_a_figure_that_exists_is_refused_after_the_gaps_file_was_rewritten(engine, tmp_path, capsys):
    from gci_amd import plot_cli
    pipeline._ENGINE = engine
    out = str(tmp_path / "out")
    m = _manifest("plot_c6_regions_hifi")
    os.makedirs(out)
    open(os.path.join(out, "GCI.ctgQ:0-24000.png"), "wb").close()
    with pytest.raises(SystemExit) as e:
        plot_cli.main(["plot_depth.py"] + [sub(a, out) for a in m["argv"] if a != "-f"])
    assert str(e.value) == f'ERROR!!! The file "{out}/GCI.ctgQ:0-24000.png" exists\nPlease use "-f" or "--force" to rewrite'
    # the region in front of it was drawn already: the utility checks, computes and draws region by region
    assert sorted(os.listdir(out)) == ["GCI.ctgP:8000-12000.png", "GCI.ctgQ:0-24000.png", "GCI.gaps.bed"]
    capsys.readouterr()


def test_the_entry_point_on_the_native_provider(tmp_path):
    """`python plot_depth.py ...` as a user starts it: the library's own HBM buffers (no torch in the process), same files."""
    case = "plot_c6_two_types"
    out = str(tmp_path / "out")
    env = dict(os.environ, GCI_ASSERT_NO_TORCH="1")
    env.pop("GCI_HBM", None)
    m = _manifest(case)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "plot_depth.py")] + [sub(a, out) for a in m["argv"]],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert norm(r.stdout, out) == m["stdout"]
    _same_outputs(out, case, m)
