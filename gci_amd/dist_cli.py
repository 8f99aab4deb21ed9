"""`python depth_dist.py [--chrs a,b,...] [-R regions.bed] [-q 0.25,0.5,0.75] [--at-least 1] [--max-depth 65535] [-f] input.depth.gz
output_prefix`: how depth is distributed in a saved `.depth.gz` -- `{output_prefix}.depth.summary.txt` (per contig or BED window:
bases, covered bases, mean, min, quantiles, max, bases at or above given depths) and `{output_prefix}.depth.hist.txt` (the
histogram and its cumulative form).  The reference has no such utility; the options are depth_to_bedgraph.py's where it has them.

The file goes into an int32 track in HBM (pipeline.read_depth_tracks) and the counting is done on the device
(pipeline.depth_distribution: k_hist.hip, one statistics pass and one histogram pass); the host turns integers into text.
Without `-R` every contig is one item and a last row `total` covers all written contigs: its mean is the whole-genome mean depth
`plot_depth.py -dmean` asks for."""
from __future__ import annotations

import argparse
import os
import sys
from fractions import Fraction
from typing import List, Sequence, Tuple

import numpy as np

from . import phases, pipeline
from .bedgraph_cli import parse_regions, plan_items


def build_parser(prog: str) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=prog, description="Depth histogram and summary (mean, min, max, quantiles, breadth) of a .depth.gz file; "
                                     "the mean on the `total` row of the summary is the value plot_depth.py takes as -dmean")
    parser.add_argument("depth", metavar="input.depth.gz", help="The depth file (as GCI.py writes it)")
    parser.add_argument("prefix", metavar="output_prefix", help="The outputs are {output_prefix}.depth.summary.txt and {output_prefix}.depth.hist.txt")
    parser.add_argument("--chrs", default="", help="A list of chromosomes separated by comma")
    parser.add_argument("-R", "--regions", metavar="FILE", default=None, help="Bed file containing regions to summarise, one item per line (no `total` row then)")
    parser.add_argument("-q", "--quantiles", default="0.25,0.5,0.75", help="Quantiles separated by comma, decimals or fractions in [0, 1] [0.25,0.5,0.75]")
    parser.add_argument("--at-least", default="1", help="Depths separated by comma: one column `ge{t}` of bases with depth >= t each [1]")
    parser.add_argument("--max-depth", type=int, default=65535, help="Depths above this are counted as one class `>{max-depth}` [65535]")
    parser.add_argument("-f", "--force", action="store_true", help="Force rewriting of existing files [False]")
    return parser


def parse_quantiles(text: str) -> List[Tuple[str, Fraction]]:
    out = []
    for part in [p for p in text.split(",") if p.strip()]:
        try:
            q = Fraction(part.strip())
        except (ValueError, ZeroDivisionError):
            sys.exit(f'ERROR!!! The quantile "{part}" is not a number')
        if not 0 <= q <= 1:
            sys.exit(f'ERROR!!! The quantile "{part}" is not in [0, 1]')
        out.append((part.strip(), q))
    return out


def parse_at_least(text: str, max_depth: int) -> List[int]:
    out = []
    for part in [p for p in text.split(",") if p.strip()]:
        try:
            t = int(part)
        except ValueError:
            sys.exit(f'ERROR!!! The depth "{part}" of --at-least is not an integer')
        if not 0 <= t <= max_depth + 1:
            sys.exit(f'ERROR!!! The depth "{part}" of --at-least is not in [0, {max_depth + 1}] (--max-depth + 1)')
        out.append(t)
    return out


def quantile(counts: np.ndarray, bases: int, q: Fraction, max_depth: int) -> str:
    """The smallest depth d with count(depth <= d) >= max(1, ceil(q * bases)) -- np.sort(x)[k - 1] --, `>{max_depth}` when it lies in
    the over class; `counts` are the bins alone."""
    k = max(1, -((-q.numerator * bases) // q.denominator))
    d = int(np.searchsorted(np.cumsum(counts, dtype=np.uint64), np.uint64(k), side="left"))
    return str(d) if d < counts.shape[0] else f">{max_depth}"


def _rows(items, hist: np.ndarray, stats: np.ndarray, with_total: bool):
    """(name, start, end, counts per bin, over, sum, min, max, bases) per item, then `total`."""
    n_bins = hist.shape[1] - 2
    rows = [(name, int(a), int(b), hist[k, :n_bins], int(hist[k, n_bins]), int(stats[k, 0]), int(stats[k, 1]), int(stats[k, 2]), int(stats[k, 3]))
            for k, (name, a, b) in enumerate(items)]
    if with_total:
        bases = int(stats[:, 3].sum())
        rows.append(("total", 0, sum(int(b) - int(a) for _, a, b in items), hist[:, :n_bins].sum(axis=0, dtype=np.uint64), int(hist[:, n_bins].sum()),
                     int(stats[:, 0].sum()), int(stats[:, 1].min()) if bases else 0, int(stats[:, 2].max()) if bases else 0, bases))
    return rows


def summary_text(items, hist, stats, quantiles: Sequence[Tuple[str, Fraction]], at_least: Sequence[int], max_depth: int, with_total: bool) -> str:
    n_bins = hist.shape[1] - 2
    head = ["#name", "start", "end", "bases", "covered", "mean", "min"] + ["q" + t for t, _ in quantiles] + ["max"] + [f"ge{t}" for t in at_least]
    lines = ["\t".join(head)]
    for name, a, b, counts, over, total, lo, hi, bases in _rows(items, hist, stats, with_total):
        if bases == 0:                                 # an empty item has no depth to speak of
            cols = [name, a, b, 0, 0, "nan", "nan"] + ["nan"] * len(quantiles) + ["nan"] + [0] * len(at_least)
        else:
            cols = [name, a, b, bases, bases - int(counts[0]), f"{total / bases:.4f}", lo]
            cols += [quantile(counts, bases, q, max_depth) for _, q in quantiles] + [hi]
            cols += [bases - int(counts[:min(t, n_bins)].sum(dtype=np.uint64)) for t in at_least]
        lines.append("\t".join(str(c) for c in cols))
    return "\n".join(lines) + "\n"


def hist_text(items, hist, stats, max_depth: int, with_total: bool) -> str:
    lines = ["#name\tstart\tend\tdepth\tbases\tat_least"]
    for name, a, b, counts, over, _, _, _, bases in _rows(items, hist, stats, with_total):
        left = bases
        for d in np.flatnonzero(counts).tolist():
            lines.append(f"{name}\t{a}\t{b}\t{d}\t{int(counts[d])}\t{left}")
            left -= int(counts[d])
        if over:
            lines.append(f"{name}\t{a}\t{b}\t>{max_depth}\t{over}\t{left}")
    return "\n".join(lines) + "\n"


def run(args) -> Tuple[str, str]:
    outs = (f"{args.prefix}.depth.summary.txt", f"{args.prefix}.depth.hist.txt")
    for out in outs:
        if os.path.exists(out) and not args.force:
            sys.exit(f'ERROR!!! The file "{out}" exists\nPlease use "-f" or "--force" to rewrite')
    if not 0 <= args.max_depth <= 65535:
        sys.exit(f"ERROR!!! --max-depth {args.max_depth} is not in [0, 65535]")
    quantiles = parse_quantiles(args.quantiles)
    at_least = parse_at_least(args.at_least, args.max_depth)
    chrs = [c for c in args.chrs.split(",") if c]
    regions = parse_regions(args.regions) if args.regions else None
    engine = pipeline.default_engine()
    with phases.wall("read_depth_tracks[%s]" % args.depth):
        tracks, lengths = pipeline.read_depth_tracks(engine, args.depth)
    items = plan_items(lengths, chrs, regions)
    hist, stats = pipeline.depth_distribution(tracks, items, args.max_depth)
    negative = np.flatnonzero(hist[:, -1])
    if negative.shape[0]:
        sys.exit(f'ERROR!!! The depth file holds a negative depth on "{items[int(negative[0])][0]}"')
    with phases.wall("dist_write_files"):
        text = (summary_text(items, hist, stats, quantiles, at_least, args.max_depth, regions is None),
                hist_text(items, hist, stats, args.max_depth, regions is None))
        for out, body in zip(outs, text):
            with open(out, "w") as f:
                f.write(body)
    return outs


def main(argv=None) -> Tuple[str, str]:
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: depth_dist.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
