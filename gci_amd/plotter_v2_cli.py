"""Drop-in for the reference's newer plotter, `python utility/depth_plotter_v2.py ...`: one figure per sequence or region of saved
depth files -- bars of windowed means, zero-depth and low-depth stretches shaded, HiFi above and ONT mirrored below --, with the
utility's options, messages, order of events and output files, driving the HIP path.

The utility parses one Python int() per line of both files in lock-step and then walks every base of every sequence three times
per read type.  Here each file goes into an int32 track in HBM (pipeline.read_depth_tracks; this project's own `.depth.gz` in the
compressed domain, plain text as it is) and every figure's numbers are two device calls per track (pipeline.depth_profile_v2:
gci_depth_classes + gci_range_sums).  That is the DEVICE path, taken when every given file is wholly inside the strict grammar,
begins with a header and names every sequence once, and -- with two files -- both hold the same names with the same lengths in the
same order: then the lock-step read yields exactly the files' sequences.  Any other input takes the HOST path: the lock-step read
itself, line by line (formats/depthfile.lockstep_sequences), each sequence it yields uploaded and measured by the same two calls.
Which one ran is in the phase log as "plotter_v2".

Quirks of the utility that are kept: `--max-depth-ratio` and `--min-safe-depth` are parsed and ignored (4.0 and 5 apply), a missing
depth file or a bad `--region` is a message and exit code 0, a figure is named `{seq}_{start}-{end}.{format}` also for a whole
sequence, existing figures are overwritten, and a failure inside one sequence is counted and reported, not raised.  The stated
deviation is the one of the other depth tools: a depth outside int32 and a sequence beyond 2^31 - 1 bases are refused."""
from __future__ import annotations

import argparse
import os
import sys
from collections import defaultdict
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import phases, pipeline
from .formats import depthfile


def build_parser(prog: str) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=prog, description="Depth data visualization tool - Enhanced version",
                                     formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-r", "--fai", required=True, help="Reference genome fai index file")
    parser.add_argument("--hifi", help="HiFi depth file (supports .gz compression)")
    parser.add_argument("--nano", help="ONT depth file (supports .gz compression)")
    parser.add_argument("--regions", help="BED format region file")
    parser.add_argument("--region", help="Single region, format: chr:start-end")
    parser.add_argument("-o", "--output_dir", default="images", help="Output directory (default: images)")
    parser.add_argument("-f", "--output-format", choices=["png", "pdf", "svg"], default="pdf", help="Output format (default: pdf)")
    parser.add_argument("-w", "--window-size", type=int, default=1000, help="Sliding window size (default: 1000)")
    parser.add_argument("--max-depth-ratio", type=float, default=3.0,
                        help="Maximum depth ratio (relative to average depth, default: 3.0)")
    parser.add_argument("--min-safe-depth", type=int, default=5,
                        help="Minimum safe depth threshold, regions below this value will be marked with blue background (default: 5)")
    return parser


def parse_fai(path: str) -> Dict[str, int]:
    """{name: length} of a `.fai`: the first two tab-separated columns of every line that has them."""
    lengths = {}
    with open(path, "r") as f:
        for line in f:
            cols = line.strip().split("\t")
            if len(cols) >= 2:
                lengths[cols[0]] = int(cols[1])
    return lengths


def parse_bed(path: str) -> Dict[str, List[Tuple[int, int]]]:
    """{name: sorted [(start, end)]} of a BED file; `#` lines, empty lines and rows with fewer than three columns are skipped.  The
    utility reads both ends as INCLUSIVE positions."""
    regions = defaultdict(list)
    with open(path, "r") as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            cols = line.split("\t")
            if len(cols) >= 3:
                regions[cols[0]].append((int(cols[1]), int(cols[2])))
    return {name: sorted(rows) for name, rows in regions.items()}


class _Side:
    """One read type of one sequence: its length and where its depths are (a DepthTracks and the contig's name), or nothing."""

    def __init__(self, tracks: Optional[pipeline.DepthTracks] = None, name: str = "", length: int = 0):
        self.tracks, self.name, self.length = tracks, name, int(length)


def _device_sources(paths) -> Optional[list]:
    """The device path's tracks, one per given file (None for a file not given), or None: the host path takes the input."""
    engine = pipeline.default_engine()
    tracks, shape = [], None
    for path in paths:
        if path is None:
            tracks.append(None)
            continue
        with phases.wall("read_depth_tracks[%s]" % path):
            got, lengths = pipeline.read_depth_tracks(engine, path, None, plotter_v2=True)
        if got is None:
            return None
        if shape is not None and list(lengths.items()) != shape:
            return None
        shape = list(lengths.items())
        tracks.append(got)
    return tracks


def _upload(engine, name: str, depths: list) -> _Side:
    """A sequence of the host path into HBM (a layout of its own)."""
    if len(depths) == 0:
        return _Side()
    if min(depths) < depthfile.INT32_MIN or max(depths) > depthfile.INT32_MAX:
        sys.exit(f'ERROR!!! The depth file holds a depth of "{name}" outside the 32-bit range (-2^31 .. 2^31 - 1), which is not supported')
    if len(depths) > depthfile.INT32_MAX:
        sys.exit("ERROR!!! A contig of the depth file is longer than 2^31 - 1 bases, which is not supported")
    tracks, _ = pipeline._upload_depths(engine, {name: np.asarray(depths, dtype=np.int64)})
    return _Side(tracks, name, len(depths))


def _sequences(hifi: Optional[str], nano: Optional[str], wanted, n_targets: int):
    """(name, HiFi side, ONT side) of every sequence the utility's reader yields, with its transcript."""
    files = []
    try:
        for p in (hifi, nano):                     # (opened first, as there: a missing file raises before anything is read)
            files.append(None if p is None else depthfile.open_depth_lines(p))
        tracks = _device_sources((hifi, nano))
        phases.note("plotter_v2", "device" if tracks is not None else "host")
        if tracks is not None:
            names = next(t for t in tracks if t is not None).targets
            for name in depthfile.conforming_sequences(names, wanted, n_targets):
                yield (name,) + tuple(_Side() if t is None else _Side(t, name, t.targets_length[name]) for t in tracks)
        else:
            engine = pipeline.default_engine()
            for name, h, o in depthfile.lockstep_sequences(files[0], files[1], wanted, n_targets):
                yield name, _upload(engine, name, h), _upload(engine, name, o)
    finally:
        for f in files:
            if f is not None:
                f.close()


def _plot_sequence(seq_id: str, hifi: _Side, ont: _Side, regions: Optional[list], window_size: int, output_dir: str, fmt: str,
                   tally: Dict[str, int]) -> None:
    """Every region of one sequence, as the utility's loop body; tally["successful"] / ["failed"] are counted region by region, so
    that what was drawn before a later region raises stays counted (the caller adds the one failure of the exception).  The
    numbers of all regions come from the device first (one depth_profile_v2 per read type), then the regions are drawn and
    reported in order."""
    from . import plot_v2
    length = hifi.length if hifi.length > 0 else ont.length
    if length == 0:
        print(f"Warning: No depth data for sequence {seq_id}")
        tally["failed"] += 1
        return
    plan, items = [], {"hifi": [], "ont": []}
    for start, end in (regions if regions else [(0, length - 1)]):
        start, end = max(0, start), min(length - 1, end)
        if start > end:
            plan.append(("invalid", start, end, None))
            continue
        # what the slices [start : end + 1] of the two arrays hold
        n = {kind: max(0, min(side.length, end + 1) - start) for kind, side in (("hifi", hifi), ("ont", ont))}
        if n["hifi"] == 0 and n["ont"] == 0:
            plan.append(("empty", start, end, None))
            continue
        if n["hifi"] and n["ont"] and n["hifi"] != n["ont"]:
            plan.append(("mismatch", start, end, n))
            break                                              # (the utility raises here: the sequence's later regions are not looked at)
        slots = {}
        for kind in ("hifi", "ont"):
            if n[kind]:
                slots[kind] = len(items[kind])
                items[kind].append((seq_id, start, start + n[kind] - 1))
        plan.append(("figure", start, end, (slots, max(n.values()))))
    profiles = {kind: pipeline.depth_profile_v2(side.tracks, items[kind], window_size, plot_v2.LOW_BELOW) if items[kind] else []
                for kind, side in (("hifi", hifi), ("ont", ont))}
    for what, start, end, arg in plan:
        if what == "invalid":
            print(f"Warning: Invalid region [{start}, {end}] for sequence {seq_id}")
        elif what == "empty":
            print(f"Error: No depth data for sequence {seq_id}")
            tally["failed"] += 1
        elif what == "mismatch":
            raise ValueError(f"Error: HiFi and ONT data length mismatch for sequence {seq_id}. HiFi length: {arg['hifi']}, "
                             f"ONT length: {arg['ont']}. Both datasets must have the same length.")
        else:
            slots, n = arg
            path = os.path.join(output_dir, f"{seq_id}_{start}-{end}.{fmt}")
            plot_v2.render(plot_v2.figure_spec(seq_id, n, [(kind, profiles[kind][slots[kind]]) for kind in ("hifi", "ont") if kind in slots],
                                               path))
            tally["successful"] += 1
            print(f"  Generated: {path}")


def run(args) -> None:
    if not args.hifi and not args.nano:
        print("Error: Must provide at least one depth file (--hifi or --nano)")
        return
    os.makedirs(args.output_dir, exist_ok=True)
    print("Parsing fai file...")
    fai_lengths = parse_fai(args.fai)
    print(f"Found {len(fai_lengths)} reference sequences")
    regions = None
    if args.regions:
        print(f"Parsing BED region file: {args.regions}")
        regions = parse_bed(args.regions)
        print(f"Found {sum(len(rows) for rows in regions.values())} regions, involving {len(regions)} sequences")
    if args.region:                                            # (wins over --regions)
        try:
            seq_id, span = args.region.split(":")[:2]
            start, end = map(int, span.split("-"))
        except Exception:                                      # noqa: BLE001  (whatever is wrong with it: the utility's one message)
            print(f"Error: Invalid region format {args.region}")
            return
        regions = {seq_id: [(start, end)]}
        print(f"Will plot single specified region: {args.region}")
    if regions:
        targets = set(regions)
        print(f"Will process specified regions of {len(targets)} sequences")
    else:
        regions = None
        targets = set(fai_lengths)
        print(f"Will process all {len(targets)} reference sequences")

    def wanted(name: str) -> bool:
        return not targets or name in targets

    print("Starting sequential processing...")
    tally = {"successful": 0, "failed": 0}
    for seq_id, hifi, ont in _sequences(args.hifi or None, args.nano or None, wanted, len(targets)):
        try:
            print(f"Processing sequence: {seq_id}")
            with phases.wall("plot_sequence"):
                _plot_sequence(seq_id, hifi, ont, regions.get(seq_id) if regions else None, args.window_size, args.output_dir,
                               args.output_format, tally)
        except Exception as e:                                 # noqa: BLE001  (the utility's: one sequence's failure is counted)
            print(f"Error processing sequence {seq_id}: {e}")
            tally["failed"] += 1
    print("\nProcessing completed!")
    print(f"Successful: {tally['successful']}, Failed: {tally['failed']}")


def main(argv=None) -> None:
    """`python depth_plotter_v2.py ...` as the utility's main()."""
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: depth_plotter_v2.py imported torch")
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
