"""The bedGraph conversion stated in numpy (depth_to_bedgraph.py; include/gci_hip.h gci_depth_runs_* / gci_bedgraph_*): per window
of a flat int32 track the maximal runs of equal depth, and their lines.  What the CPU twin and the device are held against."""
import numpy as np

RUN_DTYPE = np.dtype([("start", "<u4"), ("depth", "<i4")])


def clip(window, total):
    """A window as the library clamps it to a track of `total` elements."""
    a, b = max(int(window[0]), 0), min(int(window[1]), int(total))
    return a, max(a, b)


def window_runs(seg):
    """-> (starts relative to the segment, depths) of the maximal runs of equal values in `seg`."""
    seg = np.asarray(seg)
    if seg.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    starts = np.concatenate([[0], np.flatnonzero(seg[1:] != seg[:-1]) + 1]).astype(np.int64)
    return starts, seg[starts].astype(np.int32)


def runs(track, windows):
    """-> (RUN_DTYPE [total] window after window, uint64 [n + 1] first run of every window, then the total)."""
    parts, run0 = [], [0]
    for w in windows:
        a, b = clip(w, track.shape[0])
        s, d = window_runs(track[a:b])
        r = np.zeros(s.shape[0], dtype=RUN_DTYPE)
        r["start"], r["depth"] = s, d
        parts.append(r)
        run0.append(run0[-1] + s.shape[0])
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=RUN_DTYPE)), np.asarray(run0, dtype=np.uint64)


def window_text(seg, name, coord0):
    s, d = window_runs(seg)
    e = np.concatenate([s[1:], [np.asarray(seg).shape[0]]]).astype(np.int64) if s.shape[0] else s
    return b"".join(b"%s\t%d\t%d\t%d\n" % (name, coord0 + a, coord0 + b, v) for a, b, v in zip(s.tolist(), e.tolist(), d.tolist()))


def text(track, windows, names, coord0):
    """-> (the lines of every window in order, uint64 [n + 1] first byte of every window, then the total)."""
    parts, byte0 = [], [0]
    for w, name, c in zip(windows, names, coord0):
        a, b = clip(w, track.shape[0])
        parts.append(window_text(track[a:b], name, int(c)))
        byte0.append(byte0[-1] + len(parts[-1]))
    return b"".join(parts), np.asarray(byte0, dtype=np.uint64)


def expand(bedgraph: bytes):
    """The lines back to {name: [depth per base]} in order of first appearance -- `end - start` copies of `depth` under each name."""
    out = {}
    for line in bedgraph.split(b"\n")[:-1]:
        name, a, b, d = line.split(b"\t")
        out.setdefault(name, []).extend([int(d)] * (int(b) - int(a)))
    return out
