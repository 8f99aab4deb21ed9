"""`python indel_sites.py [-d DIR] [-o PREFIX] [--chrs a,b] [-R regions.bed] [-Q INT] [-G INT] [-g INT] [-J] [-l INT] [-n INT] [-t INT] [-f]
a.bam [b.bam ...]`: LONG INSERTIONS AND DELETIONS IN READS, base by base.  clip_sites.py finds misjoins and collapsed repeats, where the
aligner gives up and clips.  A collapsed or expanded tandem repeat, a missing or duplicated stretch of a few dozen to a few thousand
bases, a mis-polished block leave another mark: the aligner carries the read through with one long D or I operation, and several reads
do so at the same reference base.  The identity quotient of the record filter dilutes a 200-base deletion in a 20 kb read to 1 %;
filter_reads.py prints a record's total I and D, not where they lie.  The reference has no utility for it.

    {DIR}/{PREFIX}.indel.del.depth.gz    per base, the counted records that delete it with one D operation of at least -l bases
    {DIR}/{PREFIX}.indel.ins.depth.gz    per base, the I operations of at least -l bases anchored there: the base in front of the inserted
                                         bases (VCF's anchor)
                                         ordinary depth files: depth_dist.py, depth_to_bedgraph.py, plot_depth.py and
                                         depth_plotter_v2.py read them as they read any other
    {DIR}/{PREFIX}.indel.sites.bed       contig, start, end, del, ins, depth -- one line per maximal run of bases where del >= -n or
                                         ins >= -n, with the maxima of the three tracks over the run, in contig order and then by
                                         position, no header: `filter_reads.py -R` lists the reads of every site
    {DIR}/{PREFIX}.indel.txt             per file and in total the records counted, the deletions and the insertions; the sites; the options

A record counts as bam_depth.py counts it (`-Q`, `-G`, `-g`: include/gci_hip.h, gci_bam_indel_size); operations are never merged (5D5D is
two deletions of 5), N is no deletion.  `depth` is the read-mapping depth bam_depth.py gives with the same `-Q/-G/-g/-J`: without `-J` it
does not count a read over the bases it deletes, so the reads that span a deleted base are depth + del.  With `-R` only the sites inside
the regions are listed; the two tracks are whole.  Several files add; contig names, lengths and order are the first file's.  Nearby
sites are not merged and there is no support-fraction threshold: the two tracks feed `depth_dist.py -R` and the plotters.

The BAM bytes are inflated and walked on the device, every file once (pipeline.bam_indel_sites: k_cover.hip, k_indels.hip), the three
tracks are built in HBM, the sites are found there, and the tracks leave through the project's own DEFLATE writer (k_deflate.hip); the
host renders the few lines of the BED file and of the summary."""
from __future__ import annotations

import os
import sys
import zlib

from . import bamdepth_cli, bedgraph_cli, phases, pipeline
from ._lib import GCI_E_MALFORMED, GciError
from .formats import bam as bamfmt


def build_parser(prog: str):
    parser = bamdepth_cli.build_parser(prog)
    parser.description = ("The long insertions and deletions the reads of BAM file(s) carry: per base the records that delete it with one long D "
                          "and the long I operations anchored there, as {DIR}/{PREFIX}.indel.del.depth.gz and .indel.ins.depth.gz, and the runs "
                          "of bases where several do as {DIR}/{PREFIX}.indel.sites.bed (contig, start, end, del, ins, depth); without -J the "
                          "depth column does not count a read over the bases it deletes: the reads that span a deleted base are depth + del")
    parser.set_defaults(prefix="GCI_indel")
    for action in parser._actions:
        if action.dest == "prefix":
            action.help = "Prefix of the output files [GCI_indel]"
        elif action.dest == "directory":
            action.help = "The directory of the output files [.]"
        elif action.dest == "count_del":
            action.help = ("Count deletions as covered in the depth column; without it the depth does not count a read over the bases it "
                           "deletes, and the reads that span a deleted base are depth + del [False]")
    parser.add_argument("-R", dest="regions", metavar="BED", default=None, help="List only the sites inside the regions of this BED file (the two "
                        "tracks stay whole) [every site]")
    parser.add_argument("-l", "--min-len", dest="min_len", type=int, default=pipeline.INDEL_MIN_LEN, metavar="INT",
                        help="Length from which one D or I operation counts; the default is the conventional floor of a structural variant, "
                        "a choice, not a measurement [%d]" % pipeline.INDEL_MIN_LEN)
    parser.add_argument("-n", "--min-reads", dest="min_reads", type=int, default=pipeline.INDEL_MIN_READS, metavar="INT",
                        help="List a run of bases as a site when at least INT records delete each of them, or at least INT insertions are "
                        "anchored at each [%d]" % pipeline.INDEL_MIN_READS)
    return parser


def outputs(args):
    stem = f"{args.directory}/{args.prefix}.indel"
    return [stem + ".del.depth.gz", stem + ".ins.depth.gz", stem + ".sites.bed", stem + ".txt"]


def run(args):
    if not args.bams:
        sys.exit("ERROR!!! No BAM file given")
    if args.min_len < 1:
        sys.exit(f"ERROR!!! -l/--min-len {args.min_len} is not at least 1")
    if args.min_reads < 1:
        sys.exit(f"ERROR!!! -n/--min-reads {args.min_reads} is not at least 1")
    outs = outputs(args)
    for out in outs:
        pipeline.refuse_overwrite(out, args.force)
    regions = None
    if args.regions is not None:
        if not os.path.isfile(args.regions):
            sys.exit(f'ERROR!!! The file "{args.regions}" does not exist')
        regions = bedgraph_cli.parse_regions(args.regions)
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
    if regions is not None:                            # the refusals of plan_items: an unknown name, a region outside its contig
        regions = bedgraph_cli.plan_items(dict(zip(first.references, first.lengths)), chrs, regions)
    if not os.path.isdir(args.directory):
        os.makedirs(args.directory, exist_ok=True)
    excl = (pipeline.COVER_EXCL_DEFAULT | args.excl_add) & ~args.excl_remove & 0xFFFF
    opts = pipeline.CoverOpts(excl, args.min_mapq, args.count_del)
    engine = pipeline.default_engine()
    try:
        res = pipeline.bam_indel_sites(engine, args.bams, chrs, opts, args.threads, args.min_len, args.min_reads, regions)
    except pipeline.TracksDoNotFit as e:
        sys.exit(f"ERROR!!! {e}; select fewer contigs with --chrs")
    except GciError as e:
        if e.status != GCI_E_MALFORMED or e.rec < 0:
            raise
        sys.exit(f'ERROR!!! The file "{getattr(e, "path", "?")}" holds a malformed BAM record (record {e.rec})')
    with phases.wall("write_depth_gz (deflate on the device, D2H, file)"):
        pipeline._write_depth_members(args.directory, args.prefix + ".indel.del", res.dele)
        pipeline._write_depth_members(args.directory, args.prefix + ".indel.ins", res.ins)
    options = [("min_len", args.min_len), ("min_reads", args.min_reads), ("excl_flags", "0x%x" % excl), ("min_mapq", args.min_mapq),
               ("count_del", int(args.count_del)), ("chrs", args.chrs or "."), ("regions", args.regions or ".")]
    with open(outs[2], "w") as f:
        f.write(pipeline.indel_sites_bed(res.sites, res.dele.targets))
    with open(outs[3], "w") as f:
        f.write(pipeline.indel_summary_text(args.bams, res.counts, int(res.sites.shape[0]), options))
    return outs


def main(argv=None):
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: indel_sites.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
