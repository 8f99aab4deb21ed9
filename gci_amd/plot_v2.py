"""The figures of the reference's newer plotter (utility/depth_plotter_v2.py, DepthPlotter.plot_single_sequence): bars of windowed
mean depth, the zero-depth and low-depth stretches shaded behind them, HiFi above and ONT mirrored below y = 0 when both are given.

Split as gci_amd/plot.py is, so that the numbers can be checked without looking at pixels:

  figure_spec()   everything one figure shows, as plain data, from pipeline.depth_profile_v2's per-region numbers (gci_depth_classes
                  + gci_range_sums on the GPU);
  render()        draws one FigureSpecV2 with matplotlib (host only; imported lazily), call for call what the utility draws, so
                  that the PNG comes out pixel for pixel.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

COLOR = {"hifi": "#2ca25f", "ont": "#3C5488"}
LABEL = {"hifi": "HiFi", "ont": "ONT"}
COLOR_ZERO, COLOR_LOW = "#FAD7DD", "#B7DBEA"
FIGURE_INCHES, DPI = (15, 4), 300
MAX_DEPTH_RATIO = 4.0                 # (the utility parses --max-depth-ratio and never hands it on: its plotter keeps 4.0)
LOW_BELOW = 5                         # (... and --min-safe-depth likewise: 5)


@dataclass
class LayerV2:
    """One read type in one figure; positions relative to the region's first base."""
    kind: str                           # "hifi" | "ont"
    zero: np.ndarray                    # int64 [k, 2], inclusive runs of depth == 0
    low: np.ndarray                     # int64 [k, 2], inclusive runs of 0 < depth < 5
    means: np.ndarray                   # float64, one per window
    starts: np.ndarray                  # int64, inclusive
    ends: np.ndarray                    # int64, inclusive
    mean_line: Optional[float]          # np.mean(means): the dashed line; None without windows


@dataclass
class FigureSpecV2:
    seq_id: str
    length: int                         # bases of the region
    layers: List[LayerV2]
    avg_depth: float                    # mean over the bases with depth > 0 of all layers, 1.0 without any
    path: str

    @property
    def mirrored(self) -> bool:
        return len(self.layers) == 2

    @property
    def y_limits(self):
        top = self.avg_depth * MAX_DEPTH_RATIO
        return (-top, top) if self.mirrored else (0, top)


def figure_spec(seq_id: str, length: int, profiles, path: str) -> FigureSpecV2:
    """profiles: [(kind, one entry of pipeline.depth_profile_v2)] -- HiFi first."""
    layers = []
    total, bases = 0, 0
    for kind, p in profiles:
        means = np.asarray(p["means"], dtype=np.float64)
        # (a host np.mean over the device's means: a pairwise float sum, as the utility's)
        layers.append(LayerV2(kind, p["zero"], p["low"], means, p["starts"], p["ends"], float(np.mean(means)) if means.shape[0] else None))
        total += p["sum_pos"]
        bases += p["n_pos"]
    avg = float(total) / float(bases) if bases else 1.0          # integers below 2^53: np.mean of the int64 values
    return FigureSpecV2(seq_id, int(length), layers, avg, path)


def _position_label(x, pos):
    if x >= 1000000:
        return f"{x / 1000000:.1f}M"
    if x >= 1000:
        return f"{x / 1000:.1f}k"
    return f"{int(x)}"


def render(spec: FigureSpecV2) -> None:
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.ticker import FuncFormatter

    fig, ax = plt.subplots(figsize=FIGURE_INCHES, dpi=DPI)
    for i, layer in enumerate(spec.layers):
        up = i == 0
        lo, hi = (0.5, 0.95) if up else (0.05, 0.5)
        ax.get_ylim()                                   # (the utility asks for the limits here; it settles the view before the spans)
        for runs, color in ((layer.zero, COLOR_ZERO), (layer.low, COLOR_LOW)):
            for a, b in runs.tolist():
                ax.axvspan(a, b, ymin=lo, ymax=hi, color=color, alpha=0.8)
        if layer.means.shape[0]:
            sign = 1 if up else -1
            centers = (layer.starts + layer.ends) / 2
            ax.bar(centers, layer.means if up else -layer.means, width=layer.ends - layer.starts + 1, color=COLOR[layer.kind], alpha=0.8,
                   edgecolor="none")
            ax.axhline(y=sign * layer.mean_line, color=COLOR[layer.kind], linestyle="--", alpha=0.8, linewidth=1)
    ax.set_title(f"Depth Coverage for {spec.seq_id}", fontsize=14, fontweight="bold")
    ax.xaxis.set_major_formatter(FuncFormatter(_position_label))
    unit = "Mbp" if spec.length >= 1000000 else "kbp" if spec.length >= 1000 else "bp"
    ax.set_xlabel(f"Position ({unit})", fontsize=12)
    ax.set_xlim(0, spec.length)
    ax.set_ylabel("Depth", fontsize=12)
    ax.set_ylim(*spec.y_limits)
    if spec.mirrored:
        ax.axhline(y=0, color="black", linestyle="-", linewidth=0.5, alpha=0.7)
        ax.yaxis.set_major_formatter(FuncFormatter(lambda y, pos: str(abs(int(y)))))
    ax.grid(True, alpha=0.2)
    handles = [plt.Rectangle((0, 0), 1, 1, facecolor=COLOR[layer.kind], alpha=0.8, label=LABEL[layer.kind]) for layer in spec.layers]
    handles.append(plt.Rectangle((0, 0), 1, 1, facecolor=COLOR_ZERO, alpha=1.0, label="Zero Depth"))
    handles.append(plt.Rectangle((0, 0), 1, 1, facecolor=COLOR_LOW, alpha=0.8, label="Low Depth"))
    ax.legend(handles=handles, loc="upper center", bbox_to_anchor=(0.5, 0.98), ncol=len(handles), frameon=True, fancybox=False,
              shadow=False)
    fig.savefig(spec.path, dpi=DPI, bbox_inches="tight", facecolor="white")
    plt.close(fig)
