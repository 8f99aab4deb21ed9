"""`python allele_sites.py -r ref.fa [-d DIR] [-o PREFIX] [--chrs a,b] [-R regions.bed] [-Q INT] [-G INT] [-g INT] [-J] [-n INT] [-F FRAC]
[-t INT] [-f] a.bam [b.bam ...]`: WHICH BASE THE READS CARRY WHERE THEY DISAGREE WITH THE ASSEMBLY.  mismatch_sites.py finds the bases
where the reads carry another base than the assembly and throws that base away; for a mis-polished or wrong base the repair is known as
soon as it is kept.  This tool keeps it: the same walk, its events dealt to four tracks by the read's base, and an edit list.

    {DIR}/{PREFIX}.allele.{A,C,G,T}.depth.gz   per base, the counted records that carry that base where the assembly holds another of
                                               A, C, G, T -- four ordinary depth files: depth_dist.py, depth_to_bedgraph.py,
                                               plot_depth.py and depth_plotter_v2.py read them as they read any other
    {DIR}/{PREFIX}.allele.sites.vcf            a sites-only VCF 4.2: one line per base where ONE allele is carried by >= -n records and
                                               by >= -F of the depth; REF the assembly's base, ALT that allele (a tie goes to the earlier
                                               of A, C, G, T), INFO DP (the depth), AO (the records that carry ALT), BC (the A, C, G, T
                                               counts); in contig order and then by position
    {DIR}/{PREFIX}.allele.sites.bed            contig, pos, pos+1, REF, ALT, AO, DP -- the same sites, no header: `filter_reads.py -R`
                                               lists the reads of every site
    {DIR}/{PREFIX}.allele.txt                  per file and in total the records counted, the pairs compared and the events per read
                                               base; the sites; the options

Records, pairs and `depth` are mismatch_sites.py's (`-Q`, `-G`, `-g`, `-J`: include/gci_hip.h, gci_bam_allele_size).  The test is per
allele: two alleles at 30 % of the depth each make mismatch_sites.py's site at `-F 0.5` and none here, for a site names one replacement
base.  Sites are single bases; adjacent hot bases are adjacent lines.  `-F` is read from its decimal text to parts per million, exactly.
The reads' bases are needed: GCI_BAM_INGEST=heads is refused.

Out of scope: inserted and deleted bases as alleles (`indel_sites.py -l 1` finds where they are), genotypes and qualities, more than one
ALT per line, and writing the corrected FASTA -- the VCF is the edit list, and ten lines of Python apply it.

The FASTA bytes become one code per base on the device, the BAM bytes are inflated and walked there, every file once
(pipeline.bam_allele_sites: k_cover.hip, k_mismatch.hip), the five tracks are built in HBM, the sites are found there, and the four
allele tracks leave through the project's own DEFLATE writer; the host renders the few lines of the VCF, the BED file and the summary."""
from __future__ import annotations

import os
import sys
import zlib

from . import bamdepth_cli, bedgraph_cli, phases, pipeline
from ._lib import GCI_E_MALFORMED, GciError
from .formats import bam as bamfmt


def build_parser(prog: str):
    parser = bamdepth_cli.build_parser(prog)
    parser.description = ("Which base the reads of BAM file(s) carry where they disagree with the assembly: per base and read base the records "
                          "that do, as {DIR}/{PREFIX}.allele.{A,C,G,T}.depth.gz, and the bases where one allele prevails as a sites-only VCF, "
                          "{DIR}/{PREFIX}.allele.sites.vcf, and as {DIR}/{PREFIX}.allele.sites.bed (contig, pos, pos+1, REF, ALT, AO, DP)")
    parser.set_defaults(prefix="GCI_allele")
    for action in parser._actions:
        if action.dest == "prefix":
            action.help = "Prefix of the output files [GCI_allele]"
        elif action.dest == "directory":
            action.help = "The directory of the output files [.]"
    parser.add_argument("-r", "--reference", dest="reference", metavar="FASTA", required=True, help="The assembly the reads were aligned to")
    parser.add_argument("-R", dest="regions", metavar="BED", default=None, help="List only the sites inside the regions of this BED file (the "
                        "tracks stay whole) [every site]")
    parser.add_argument("-n", "--min-reads", dest="min_reads", type=int, default=pipeline.ALLELE_MIN_READS, metavar="INT",
                        help="List a base as a site when at least INT records carry one other base there [%d]" % pipeline.ALLELE_MIN_READS)
    parser.add_argument("-F", "--min-frac", dest="min_frac", default=pipeline.ALLELE_MIN_FRAC, metavar="FRAC",
                        help="... and at least this share of the depth carries it, a decimal between 0 and 1 with at most six digits behind "
                        "the point [%s]" % pipeline.ALLELE_MIN_FRAC)
    return parser


def outputs(args):
    stem = f"{args.directory}/{args.prefix}.allele"
    return [stem + f".{b}.depth.gz" for b in "ACGT"] + [stem + ".sites.vcf", stem + ".sites.bed", stem + ".txt"]


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
        sys.exit("ERROR!!! allele_sites.py reads the reads' bases, which GCI_BAM_INGEST=heads drops: use gpu or full")
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
        res = pipeline.bam_allele_sites(engine, args.reference, args.bams, chrs, opts, args.threads, args.min_reads, frac_ppm, regions)
    except pipeline.TracksDoNotFit as e:
        sys.exit(f"ERROR!!! {e}; select fewer contigs with --chrs")
    except GciError as e:
        if e.status != GCI_E_MALFORMED or e.rec < 0:
            raise
        sys.exit(f'ERROR!!! The file "{getattr(e, "path", "?")}" holds a malformed BAM record (record {e.rec})')
    except pipeline.ReferenceMismatch as e:            # the assembly does not fit the @SQ table
        sys.exit(f"ERROR!!! {e}")
    with phases.wall("write_depth_gz (deflate on the device, D2H, file)"):
        for base in "ACGT":
            pipeline._write_depth_members(args.directory, args.prefix + ".allele." + base, res.tracks[base])
    options = [("reference", args.reference), ("min_reads", args.min_reads), ("min_frac_ppm", frac_ppm), ("excl_flags", "0x%x" % excl),
               ("min_mapq", args.min_mapq), ("count_del", int(args.count_del)), ("chrs", args.chrs or "."), ("regions", args.regions or ".")]
    with open(outs[4], "w") as f:
        f.write(pipeline.allele_sites_vcf(res.sites, res.depth.targets_length, args.reference))
    with open(outs[5], "w") as f:
        f.write(pipeline.allele_sites_bed(res.sites, res.depth.targets))
    with open(outs[6], "w") as f:
        f.write(pipeline.allele_summary_text(args.bams, res.counts, int(res.sites.shape[0]), options))
    return outs


def main(argv=None):
    argv = sys.argv if argv is None else list(argv)
    parser = build_parser(os.path.basename(argv[0]))
    args = parser.parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args, parser)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: allele_sites.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
