"""`python mismatch_sites.py -r ref.fa [-d DIR] [-o PREFIX] [--chrs a,b] [-R regions.bed] [-Q INT] [-G INT] [-g INT] [-J] [-n INT] [-F FRAC]
[-t INT] [-f] a.bam [b.bam ...]`: BASES WHERE THE READS DISAGREE WITH THE ASSEMBLY.  clip_sites.py finds where alignments break off,
indel_sites.py the long D and I operations.  A mis-polished or wrong base makes no aligner clip and opens no long gap: every read simply
carries another base than the assembly there.  This tool reads the records' SEQ field and the assembly's bases, which nothing else in
the tree does.

    {DIR}/{PREFIX}.mismatch.depth.gz     per base, the counted records whose base there and the assembly's are both one of A, C, G, T
                                         and differ -- an ordinary depth file: depth_dist.py, depth_to_bedgraph.py, plot_depth.py and
                                         depth_plotter_v2.py read it as they read any other
    {DIR}/{PREFIX}.mismatch.sites.bed    contig, start, end, mismatch, depth -- one line per maximal run of bases where mismatch >= -n
                                         and mismatch >= -F of the depth; mismatch is the largest count of the run, depth the depth at
                                         the first base that reaches it; in contig order and then by position, no header:
                                         `filter_reads.py -R` lists the reads of every site
    {DIR}/{PREFIX}.mismatch.txt          per file and in total the records counted, the pairs compared, the mismatches and their
                                         quotient; the sites; the options

A record counts as bam_depth.py counts it (`-Q`, `-G`, `-g`: include/gci_hip.h, gci_bam_mismatch_size).  Under M, = and X the read's base
faces the assembly's; the letter of the operation does not matter, the bases decide; N, `=` in SEQ and every ambiguity code on either side
are never compared; a record with SEQ `*` is counted and compares nothing.  `depth` is the read-mapping depth bam_depth.py gives with the
same `-Q/-G/-g/-J`.  `-F` is read from its decimal text to parts per million, exactly.  The FASTA ids are matched to the @SQ names by
name and the lengths are checked before a record is read.  The reads' bases are needed: GCI_BAM_INGEST=heads is refused.

The FASTA bytes become one code per base on the device (k_mismatch.hip: gci_fasta_codes), the BAM bytes are inflated and walked there,
every file once (pipeline.bam_mismatch_sites: k_cover.hip, k_mismatch.hip), the two tracks are built in HBM, the sites are found there,
and the mismatch track leaves through the project's own DEFLATE writer; the host renders the few lines of the BED file and of the
summary."""
from __future__ import annotations

import os
import sys
import zlib

from . import bamdepth_cli, bedgraph_cli, phases, pipeline
from ._lib import GCI_E_MALFORMED, GciError
from .formats import bam as bamfmt


def build_parser(prog: str):
    parser = bamdepth_cli.build_parser(prog)
    parser.description = ("The bases where the reads of BAM file(s) carry another base than the assembly: per base the records that do, as "
                          "{DIR}/{PREFIX}.mismatch.depth.gz, and the runs of bases where several do as {DIR}/{PREFIX}.mismatch.sites.bed "
                          "(contig, start, end, mismatch, depth)")
    parser.set_defaults(prefix="GCI_mismatch")
    for action in parser._actions:
        if action.dest == "prefix":
            action.help = "Prefix of the output files [GCI_mismatch]"
        elif action.dest == "directory":
            action.help = "The directory of the output files [.]"
    parser.add_argument("-r", "--reference", dest="reference", metavar="FASTA", required=True, help="The assembly the reads were aligned to")
    parser.add_argument("-R", dest="regions", metavar="BED", default=None, help="List only the sites inside the regions of this BED file (the "
                        "track stays whole) [every site]")
    parser.add_argument("-n", "--min-reads", dest="min_reads", type=int, default=pipeline.MISMATCH_MIN_READS, metavar="INT",
                        help="List a run of bases as a site when at least INT records carry another base at each [%d]" % pipeline.MISMATCH_MIN_READS)
    parser.add_argument("-F", "--min-frac", dest="min_frac", default=pipeline.MISMATCH_MIN_FRAC, metavar="FRAC",
                        help="... and at least this share of the depth does, a decimal between 0 and 1 with at most six digits behind the "
                        "point [%s]" % pipeline.MISMATCH_MIN_FRAC)
    return parser


def outputs(args):
    stem = f"{args.directory}/{args.prefix}.mismatch"
    return [stem + ".depth.gz", stem + ".sites.bed", stem + ".txt"]


def run(args, parser=None):
    if not args.bams:
        sys.exit("ERROR!!! No BAM file given")
    if args.min_reads < 1:
        sys.exit(f"ERROR!!! -n/--min-reads {args.min_reads} is not at least 1")
    try:
        frac_ppm = pipeline.parse_fraction_ppm(args.min_frac)
    except ValueError as e:
        if parser is not None:
            parser.error(f"-F/--min-frac: {e}")       # a usage error
        sys.exit(f"ERROR!!! -F/--min-frac: {e}")
    if os.environ.get("GCI_BAM_INGEST") == "heads":
        sys.exit("ERROR!!! mismatch_sites.py reads the reads' bases, which GCI_BAM_INGEST=heads drops: use gpu or full")
    outs = outputs(args)
    for out in outs:
        pipeline.refuse_overwrite(out, args.force)
    if not os.path.isfile(args.reference):
        sys.exit(f'ERROR!!! The file "{args.reference}" does not exist')
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
        res = pipeline.bam_mismatch_sites(engine, args.reference, args.bams, chrs, opts, args.threads, args.min_reads, frac_ppm, regions)
    except pipeline.TracksDoNotFit as e:
        sys.exit(f"ERROR!!! {e}; select fewer contigs with --chrs")
    except GciError as e:
        if e.status != GCI_E_MALFORMED or e.rec < 0:
            raise
        sys.exit(f'ERROR!!! The file "{getattr(e, "path", "?")}" holds a malformed BAM record (record {e.rec})')
    except pipeline.ReferenceMismatch as e:            # the assembly does not fit the @SQ table
        sys.exit(f"ERROR!!! {e}")
    with phases.wall("write_depth_gz (deflate on the device, D2H, file)"):
        pipeline._write_depth_members(args.directory, args.prefix + ".mismatch", res.mismatch)
    options = [("reference", args.reference), ("min_reads", args.min_reads), ("min_frac_ppm", frac_ppm), ("excl_flags", "0x%x" % excl),
               ("min_mapq", args.min_mapq), ("count_del", int(args.count_del)), ("chrs", args.chrs or "."), ("regions", args.regions or ".")]
    with open(outs[1], "w") as f:
        f.write(pipeline.mismatch_sites_bed(res.sites, res.mismatch.targets))
    with open(outs[2], "w") as f:
        f.write(pipeline.mismatch_summary_text(args.bams, res.counts, int(res.sites.shape[0]), options))
    return outs


def main(argv=None):
    argv = sys.argv if argv is None else list(argv)
    parser = build_parser(os.path.basename(argv[0]))
    args = parser.parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args, parser)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: mismatch_sites.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
