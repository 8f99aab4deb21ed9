"""`python clip_sites.py [-d DIR] [-o PREFIX] [--chrs a,b] [-R regions.bed] [-Q INT] [-G INT] [-g INT] [-J] [-c INT] [-n INT] [-t INT] [-f]
a.bam [b.bam ...]`: WHERE ALIGNMENTS BREAK OFF, base by base.  A misjoin or a collapsed repeat shows as a pile of reads whose alignments
all stop at the same reference base and carry a long soft or hard clip from there on.  filter_depth.py's `clip` class says that clipped
reads lie over a region, filter_reads.py lists them with their total S; neither says on which side the clip is or where it starts.  The
reference has no utility for it: its README sends the user to a genome browser.

    {DIR}/{PREFIX}.clip.left.depth.gz    per base, the counted records whose alignment BEGINS there with a clip of at least -c bases
    {DIR}/{PREFIX}.clip.right.depth.gz   ... ENDS there (pos + reference length - 1) with such a clip behind it
                                         ordinary depth files: depth_dist.py, depth_to_bedgraph.py, plot_depth.py and
                                         depth_plotter_v2.py read them as they read any other
    {DIR}/{PREFIX}.clip.sites.bed        contig, pos, pos + 1, left, right, depth -- one line per base where left >= -n or right >= -n, in
                                         contig order and then by position, no header: `filter_reads.py -R` lists the reads of every site
    {DIR}/{PREFIX}.clip.txt              per file and in total the records counted, the left and the right events; the sites; the options

A record counts as bam_depth.py counts it (`-Q`, `-G`, `-g`: include/gci_hip.h, gci_bam_clip_size); a clip is the soft and hard clipped
bases at that end of the CIGAR together (minimap2 writes supplementary alignments with hard clips); `depth` is the read-mapping depth
bam_depth.py gives with the same `-Q/-G/-g/-J`.  With `-R` only the sites inside the regions are listed; the two tracks are whole.
Several files add; contig names, lengths and order are the first file's.  Sites a few bases apart are not merged: alignment wobble on
ONT reads is real, the two tracks feed `depth_dist.py -R` and the plotters do the windowing.

The BAM bytes are inflated and walked on the device, every file once (pipeline.bam_clip_sites: k_cover.hip, k_clips.hip), the three
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
    parser.description = ("Where the alignments of BAM file(s) break off: per base the records that begin (left) or end (right) there with a long "
                          "clip, as {DIR}/{PREFIX}.clip.left.depth.gz and .clip.right.depth.gz, and the bases where several do as "
                          "{DIR}/{PREFIX}.clip.sites.bed (contig, pos, pos + 1, left, right, depth)")
    parser.set_defaults(prefix="GCI_clip")
    for action in parser._actions:
        if action.dest == "prefix":
            action.help = "Prefix of the output files [GCI_clip]"
        elif action.dest == "directory":
            action.help = "The directory of the output files [.]"
        elif action.dest == "count_del":
            action.help = "Count deletions as covered in the depth column [False]"
    parser.add_argument("-R", dest="regions", metavar="BED", default=None, help="List only the sites inside the regions of this BED file (the two "
                        "tracks stay whole) [every site]")
    parser.add_argument("-c", "--min-clip", dest="min_clip", type=int, default=pipeline.CLIP_MIN_CLIP, metavar="INT",
                        help="Soft plus hard clipped bases at an end of the alignment from which it counts as broken off there; the default is a "
                        "choice for long reads, not a measurement [%d]" % pipeline.CLIP_MIN_CLIP)
    parser.add_argument("-n", "--min-reads", dest="min_reads", type=int, default=pipeline.CLIP_MIN_READS, metavar="INT",
                        help="List a base as a site when at least INT records break off there on one side [%d]" % pipeline.CLIP_MIN_READS)
    return parser


def outputs(args):
    stem = f"{args.directory}/{args.prefix}.clip"
    return [stem + ".left.depth.gz", stem + ".right.depth.gz", stem + ".sites.bed", stem + ".txt"]


def run(args):
    if not args.bams:
        sys.exit("ERROR!!! No BAM file given")
    if args.min_clip < 1:
        sys.exit(f"ERROR!!! -c/--min-clip {args.min_clip} is not at least 1")
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
        res = pipeline.bam_clip_sites(engine, args.bams, chrs, opts, args.threads, args.min_clip, args.min_reads, regions)
    except pipeline.TracksDoNotFit as e:
        sys.exit(f"ERROR!!! {e}; select fewer contigs with --chrs")
    except GciError as e:
        if e.status != GCI_E_MALFORMED or e.rec < 0:
            raise
        sys.exit(f'ERROR!!! The file "{getattr(e, "path", "?")}" holds a malformed BAM record (record {e.rec})')
    with phases.wall("write_depth_gz (deflate on the device, D2H, file)"):
        pipeline._write_depth_members(args.directory, args.prefix + ".clip.left", res.left)
        pipeline._write_depth_members(args.directory, args.prefix + ".clip.right", res.right)
    options = [("min_clip", args.min_clip), ("min_reads", args.min_reads), ("excl_flags", "0x%x" % excl), ("min_mapq", args.min_mapq),
               ("count_del", int(args.count_del)), ("chrs", args.chrs or "."), ("regions", args.regions or ".")]
    with open(outs[2], "w") as f:
        f.write(pipeline.clip_sites_bed(res.sites, res.left.targets))
    with open(outs[3], "w") as f:
        f.write(pipeline.clip_summary_text(args.bams, res.counts, int(res.sites.shape[0]), options))
    return outs


def main(argv=None):
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: clip_sites.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
