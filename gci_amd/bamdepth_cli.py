"""`python bam_depth.py [-d DIR] [-o PREFIX] [--chrs a,b] [-Q INT] [-G INT] [-g INT] [-J] [-t INT] [-f] a.bam [b.bam ...]`: the original
read-mapping depth of BAM files as `{DIR}/{PREFIX}.depth.gz` -- the file `samtools depth -a | convert_samtools_depth.py` would have
produced, which plot_depth.py, depth_plotter_v2.py, depth_dist.py, depth_to_bedgraph.py and GCI_score.py read as they read GCI.py's.
The reference has no such utility: its README sends the user through samtools.

The semantics are `samtools depth -a`'s as its manual states them (include/gci_hip.h: gci_bam_cover_size; tests/cover_ref.py pins the
reading): records with a flag bit of 0x704 (UNMAP, SECONDARY, QCFAIL, DUP; `-G` adds bits, `-g` removes them) or a MAPQ below `-Q` are
skipped, supplementary alignments count, deletions count only with `-J`, reference skips never.  `-q` (base quality), `-l` and `-s`
are not offered.  Several files add; contig names, lengths and order are the first file's.

The BAM bytes are inflated, walked and turned into covered intervals on the device (pipeline.bam_raw_depth: k_cover.hip), built into an
int32 track in HBM and written through the project's own DEFLATE writer (k_deflate.hip)."""
from __future__ import annotations

import argparse
import os
import sys
import zlib

from . import phases, pipeline
from ._lib import GCI_E_MALFORMED, GciError
from .formats import bam as bamfmt


def _flag_int(text: str) -> int:
    try:
        return int(text, 0)                           # decimal or 0x hex, as samtools takes them
    except ValueError:
        raise argparse.ArgumentTypeError(f'"{text}" is not an integer (decimal or 0x hex)')


def build_parser(prog: str) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog=prog, description="Per-base read-mapping depth of BAM file(s), as `samtools depth -a` counts it, "
                                     "written as {DIR}/{PREFIX}.depth.gz")
    parser.add_argument("bams", metavar="in.bam", nargs="*", help="BAM file(s); their depths add, the contigs are those of the first")
    parser.add_argument("-d", dest="directory", metavar="DIR", default=".", help="The directory of the output file [.]")
    parser.add_argument("-o", "--output", dest="prefix", metavar="PREFIX", default="GCI_raw", help="Prefix of the output file [GCI_raw]")
    parser.add_argument("--chrs", default="", help="A list of chromosomes separated by comma")
    parser.add_argument("-Q", "--min-MQ", dest="min_mapq", type=int, default=0, help="Skip records with a mapping quality below INT [0]")
    parser.add_argument("-G", dest="excl_add", type=_flag_int, default=0, metavar="INT", help="Add flag bits to the set that skips a record [UNMAP,SECONDARY,QCFAIL,DUP]")
    parser.add_argument("-g", dest="excl_remove", type=_flag_int, default=0, metavar="INT", help="Remove flag bits from the set that skips a record")
    parser.add_argument("-J", dest="count_del", action="store_true", help="Count deletions as covered [False]")
    parser.add_argument("-t", "--threads", type=int, default=1, help="Host threads for the ingest paths that inflate on the host [1]")
    parser.add_argument("-f", "--force", action="store_true", help="Force rewriting of existing files [False]")
    return parser


def run(args) -> str:
    if not args.bams:
        sys.exit("ERROR!!! No BAM file given")
    out = f"{args.directory}/{args.prefix}.depth.gz"
    pipeline.refuse_overwrite(out, args.force)
    for path in args.bams:
        try:
            bamfmt.read_header(path)
        except (OSError, ValueError, EOFError, zlib.error) as e:
            sys.exit(f'ERROR!!! The file "{path}" cannot be read as a BAM file ({e})')
    try:
        first = pipeline.same_sq_table(args.bams)
    except pipeline.SqMismatch as e:
        sys.exit(f"ERROR!!! {e}")
    chrs = [c for c in args.chrs.split(",") if c]
    for c in chrs:
        if c not in first.references:
            sys.exit(f'ERROR!!! The chromosome "{c}" of --chrs is not in the header of "{args.bams[0]}"')
    if not os.path.isdir(args.directory):
        os.makedirs(args.directory, exist_ok=True)
    opts = pipeline.CoverOpts((pipeline.COVER_EXCL_DEFAULT | args.excl_add) & ~args.excl_remove & 0xFFFF, args.min_mapq, args.count_del)
    engine = pipeline.default_engine()
    try:
        depths = pipeline.bam_raw_depth(engine, args.bams, chrs, opts, args.threads)
    except GciError as e:
        if e.status != GCI_E_MALFORMED or e.rec < 0:
            raise
        sys.exit(f'ERROR!!! The file "{getattr(e, "path", "?")}" holds a malformed BAM record (record {e.rec})')
    with phases.wall("write_depth_gz (deflate on the device, D2H, file)"):
        pipeline._write_depth_members(args.directory, args.prefix, depths)
    return out


def main(argv=None) -> str:
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: bam_depth.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
