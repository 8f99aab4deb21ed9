"""`python filter_reads.py [-d DIR] [-o PREFIX] [--chrs a,b] [-R regions.bed] [-mq INT] [-ip FLOAT] [-cp FLOAT] [--classes a,b]
[--join [-op FLOAT] [--mq-cutoff INT] [--cover N]] [-t INT] [-f] a.bam [b.bam | b.paf ...]`: WHICH READS lie over a region, and what
became of each of them.  GCI.py says where the filtered depth is low, filter_depth.py which test of the record filter took the depth
away, base by base; this utility lists the records themselves -- what the reference's README does with `samtools view -L issues.bed`,
utility/filter_bam.py and a genome browser -- as a table, `{DIR}/{PREFIX}.reads.tsv`:

    #file<TAB>k<TAB>path                 one line per BAM file listed (k from 1)
    #file name contig start end strand flag mapq M I D S NM clip identity class
    one row per selected record, in the file's own record order, file after file

start = pos (0-based), end = pos + the bases under M, D, N, = and X (not clamped to the contig); M = the bases under M, = and X
together, I, D and S the totals of their operations; NM = the first NM tag, `.` without one; clip = S / (M + I + S) and identity =
(M + I + D - NM) / (M + I + D) as decimals of six digits, TRUNCATED, `.` where the quotient does not exist; class = the name
filter_depth.py gives the record's class, with `--join` a `kept` record carries its join class (shadowed, unpaired, contig, overlap,
joined).  THE CLASS COLUMN IS AUTHORITATIVE -- it is the record filter's own decision, made with its arithmetic --; the two decimals
are for the eye.

A record is selected when its class is among `--classes` (default: every class) and, with `-R`, its reference span [start, max(end,
start + 1)) overlaps a region of the BED file; it is listed once however many regions it overlaps.  Records that belong to no class
(unmapped, on no or an unselected contig) are never listed.  Every other option means what it means in filter_depth.py; with `--join`
only the `--cover` BAM is listed.

The BAM bytes are inflated and walked on the device as for GCI.py; gci_bam_fate (k_fate.hip) gives every record its class,
gci_bam_reads_size / _write (k_reads.hip) select, measure and render the rows there, and only the rows cross to the host
(pipeline.bam_filter_reads)."""
from __future__ import annotations

import argparse
import os
import sys

from . import bedgraph_cli, filterdepth_cli, phases, pipeline
from ._lib import GciError


def build_parser(prog: str) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog=prog, description="The records of BAM file(s) that lie over a set of regions, one row each, with what GCI.py's record filter does "
        "with them: {DIR}/{PREFIX}.reads.tsv with the columns " + " ".join(pipeline.READS_COLUMNS) + ".",
        epilog="The class column is authoritative: it is the record filter's own decision (the class names of filter_depth.py; with --join a "
        "`kept` record carries its join class).  clip = S / (M + I + S) and identity = (M + I + D - NM) / (M + I + D) are decimals of six "
        "digits, truncated, for the eye.  start is 0-based, end = start + the reference bases the CIGAR consumes.")
    parser.add_argument("bams", metavar="in.bam", nargs="*", help="BAM file(s), listed one after the other; the contigs are those of the first.  "
                        "With --join: BAM and PAF files of one read set, joined by read name; the --cover BAM is listed")
    filterdepth_cli.add_filter_arguments(parser, "GCI_reads", "list")
    parser.add_argument("-R", dest="regions", metavar="BED", default=None, help="List only the records whose reference span overlaps a region "
                        "of this BED file [every record of the classes]")
    return parser


def run(args) -> str:
    classes, bams, join = filterdepth_cli.checked_options(args)
    table = f"{args.directory}/{args.prefix}.reads.tsv"
    pipeline.refuse_overwrite(table, args.force)
    regions = None
    if args.regions is not None:
        if not os.path.isfile(args.regions):
            sys.exit(f'ERROR!!! The file "{args.regions}" does not exist')
        regions = bedgraph_cli.parse_regions(args.regions)
    chrs = filterdepth_cli.checked_files(args, bams)
    opts = pipeline.FateOpts(args.map_qual, args.clip_percent, args.iden_percent)
    engine = pipeline.default_engine()
    try:
        pipeline.bam_filter_reads(engine, bams, chrs, opts, args.threads, classes, regions, table, join=join)
    except GciError as e:
        filterdepth_cli.exit_for_record(e)
    return table


def main(argv=None) -> str:
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: filter_reads.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
