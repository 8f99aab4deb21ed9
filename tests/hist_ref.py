"""The depth distribution stated in numpy (depth_dist.py; include/gci_hip.h gci_depth_hist): per window of a flat int32 track the
histogram with its over / under classes and sum / min / max / count, the quantile rule, and the two text files from (hist, stats).
What the CPU twin and the device are held against."""
import math
from fractions import Fraction

import numpy as np

from bedgraph_ref import clip

I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def window_hist(seg, n_bins):
    """-> (uint64 [n_bins + 2], [sum, min, max, count]) of one clamped window."""
    seg = np.asarray(seg, dtype=np.int64)
    h = np.zeros(n_bins + 2, dtype=np.uint64)
    inside = seg[(seg >= 0) & (seg < n_bins)]
    h[:n_bins] = np.bincount(inside, minlength=n_bins)[:n_bins] if n_bins else 0
    h[n_bins] = int((seg >= n_bins).sum())
    h[n_bins + 1] = int((seg < 0).sum())
    if seg.shape[0] == 0:
        return h, [0, I32_MAX, I32_MIN, 0]
    return h, [int(seg.sum()), int(seg.min()), int(seg.max()), int(seg.shape[0])]


def hist(track, windows, n_bins):
    """-> (uint64 [n, n_bins + 2], int64 [n, 4])."""
    H = np.zeros((len(windows), n_bins + 2), dtype=np.uint64)
    S = np.zeros((len(windows), 4), dtype=np.int64)
    for k, w in enumerate(windows):
        a, b = clip(w, track.shape[0])
        H[k], S[k] = window_hist(track[a:b], n_bins)
    return H, S


def quantile(counts, bases, q, max_depth):
    """The smallest depth d with count(depth <= d) >= max(1, ceil(q * bases)), q a Fraction; `>{max_depth}` in the over class."""
    k = max(1, math.ceil(Fraction(q) * bases))
    run = 0
    for d, c in enumerate(counts.tolist()):
        run += c
        if run >= k:
            return str(d)
    return ">%d" % max_depth


def _rows(items, H, S, with_total):
    n_bins = H.shape[1] - 2
    rows = [(name, a, b, H[k, :n_bins], int(H[k, n_bins]), [int(x) for x in S[k]]) for k, (name, a, b) in enumerate(items)]
    if with_total:
        bases = int(S[:, 3].sum())
        st = [int(S[:, 0].sum()), int(S[:, 1].min()) if bases else I32_MAX, int(S[:, 2].max()) if bases else I32_MIN, bases]
        rows.append(("total", 0, sum(b - a for _, a, b in items), H[:, :n_bins].sum(axis=0, dtype=np.uint64), int(H[:, n_bins].sum()), st))
    return rows


def summary(items, H, S, quantiles, at_least, max_depth, with_total):
    """`{prefix}.depth.summary.txt`; quantiles as the option's texts."""
    n_bins = H.shape[1] - 2
    out = ["\t".join(["#name", "start", "end", "bases", "covered", "mean", "min"] + ["q" + q for q in quantiles] + ["max"] + ["ge%d" % t for t in at_least])]
    for name, a, b, counts, over, (total, lo, hi, bases) in _rows(items, H, S, with_total):
        if bases == 0:
            cols = [name, a, b, 0, 0, "nan", "nan"] + ["nan"] * len(quantiles) + ["nan"] + [0] * len(at_least)
        else:
            cols = [name, a, b, bases, bases - int(counts[0]), "%.4f" % (total / bases), lo]
            cols += [quantile(counts, bases, Fraction(q), max_depth) for q in quantiles] + [hi]
            cols += [over + sum(int(c) for c in counts[t:n_bins].tolist()) if t <= n_bins else 0 for t in at_least]
        out.append("\t".join(str(c) for c in cols))
    return "\n".join(out) + "\n"


def histogram(items, H, S, max_depth, with_total):
    """`{prefix}.depth.hist.txt`."""
    out = ["#name\tstart\tend\tdepth\tbases\tat_least"]
    for name, a, b, counts, over, (_, _, _, bases) in _rows(items, H, S, with_total):
        c = counts.tolist()
        for d in range(len(c)):
            if c[d] > 0:
                out.append("%s\t%d\t%d\t%d\t%d\t%d" % (name, a, b, d, c[d], over + sum(c[d:])))
        if over:
            out.append("%s\t%d\t%d\t>%d\t%d\t%d" % (name, a, b, max_depth, over, over))
    return "\n".join(out) + "\n"


def distribution(depths, items, max_depth=65535):
    """pipeline.depth_distribution over {name: per-base array}: (hist, stats) with n_bins = min(largest max + 1, max_depth + 1)."""
    segs = [np.asarray(depths[name][a:b], dtype=np.int64) for name, a, b in items]
    tops = [int(s.max()) for s in segs if s.shape[0]]
    n_bins = max(1, min(max(tops) + 1, max_depth + 1)) if tops else 1
    H = np.zeros((len(items), n_bins + 2), dtype=np.uint64)
    S = np.zeros((len(items), 4), dtype=np.int64)
    for k, s in enumerate(segs):
        H[k], S[k] = window_hist(s, n_bins)
    return H, S
