"""`python depth_to_bedgraph.py [--chrs a,b,...] [-R regions.bed] [-f] input.depth.gz output_prefix`: a saved `.depth.gz` as
`{output_prefix}.bedgraph`, the format IGV, the UCSC browser, bedGraphToBigWig, bedtools and tabix read -- one line
`name\\tstart\\tend\\tdepth` per maximal run of equal depth, 0-based half-open, no `track` line.  The reference has no such utility
(its depth files are read by its own scripts alone); the options are GCI.py's where it has them.

The file goes into an int32 track in HBM (pipeline.read_depth_tracks: this project's own files in the compressed domain, any other
as text, odd grammar by the host statements) and the lines are made on the device (pipeline.depth_bedgraph: k_bedgraph.hip).
Without `-R` every contig is one window; with it every BED line is one window, in the file's order, overlaps allowed; `--chrs`
keeps the named contigs (and the windows on them), in the file's order."""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional, Tuple

from . import phases, pipeline


def build_parser(prog: str) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=prog, description="Convert a .depth.gz file into bedGraph (one line per run of equal depth)")
    parser.add_argument("depth", metavar="input.depth.gz", help="The depth file (as GCI.py writes it)")
    parser.add_argument("prefix", metavar="output_prefix", help="The output is {output_prefix}.bedgraph")
    parser.add_argument("--chrs", default="", help="A list of chromosomes separated by comma")
    parser.add_argument("-R", "--regions", metavar="FILE", default=None, help="Bed file containing regions to write, one window per line")
    parser.add_argument("-f", "--force", action="store_true", help="Force rewriting of existing files [False]")
    return parser


def parse_regions(path: str) -> List[Tuple[str, int, int]]:
    """(chrom, start, end) of every line of a BED file, in the file's order; empty lines are skipped, a line with fewer than three
    columns or a coordinate that is no integer is refused."""
    rows = []
    with open(path, "r") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            cols = line.rstrip("\n").split("\t")
            if len(cols) < 3:
                sys.exit(f'ERROR!!! Line {no} of the bed file "{path}" has fewer than three columns')
            try:
                rows.append((cols[0], int(cols[1]), int(cols[2])))
            except ValueError:
                sys.exit(f'ERROR!!! Line {no} of the bed file "{path}" has a coordinate that is not an integer')
    return rows


def plan_items(targets_length, chrs: List[str], regions: Optional[List[Tuple[str, int, int]]]) -> List[Tuple[str, int, int]]:
    """The windows to write: the refusals first (an unknown name, a region outside its contig), then `--chrs` as a filter."""
    for name in chrs:
        if name not in targets_length:
            sys.exit(f'ERROR!!! The chromosome "{name}" is not in the depth file')
    if regions is None:
        items = [(t, 0, int(L)) for t, L in targets_length.items()]
    else:
        for name, start, end in regions:
            if name not in targets_length:
                sys.exit(f'ERROR!!! The chromosome "{name}" of the bed file is not in the depth file')
            if start < 0 or start > end:
                sys.exit(f'ERROR!!! The region {name}:{start}-{end} of the bed file does not have 0 <= start <= end')
            if end > targets_length[name]:
                sys.exit(f'ERROR!!! The region {name}:{start}-{end} of the bed file ends beyond the contig ({targets_length[name]} bases)')
        items = list(regions)
    keep = set(chrs)
    return [it for it in items if not chrs or it[0] in keep]


def run(args) -> str:
    out = f"{args.prefix}.bedgraph"
    if os.path.exists(out) and not args.force:
        sys.exit(f'ERROR!!! The file "{out}" exists\nPlease use "-f" or "--force" to rewrite')
    chrs = [c for c in args.chrs.split(",") if c]
    regions = parse_regions(args.regions) if args.regions else None
    engine = pipeline.default_engine()
    with phases.wall("read_depth_tracks[%s]" % args.depth):
        tracks, lengths = pipeline.read_depth_tracks(engine, args.depth)
    items = plan_items(lengths, chrs, regions)
    with open(out, "wb") as f:
        if items:
            pipeline.depth_bedgraph(tracks, items, f)
    return out


def main(argv=None) -> str:
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: depth_to_bedgraph.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
