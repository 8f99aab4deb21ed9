"""`python filter_sweep.py [-d DIR] [-o PREFIX] [--chrs a,b] [-R regions.bed] [-mq INT] [-cp FLOAT] [-ip FLOAT] [--digits K] [-t INT] [-f]
a.bam [b.bam ...]`: WHICH THRESHOLDS fit this data.  GCI.py says where the filtered depth is low, filter_depth.py which test of the
record filter took the depth away, filter_reads.py lists the reads; all of them at one setting of `-mq`, `-cp` and `-ip`.  This
utility writes the distribution of the three quantities those thresholds cut -- MAPQ, the clip quotient S / (M + I + S), the identity
quotient (M + I + D - NM) / (M + I + D) -- over the primary records of every file (those filter_depth.py calls mapq, clip, identity
or kept), and what each threshold TAKEN ALONE would keep at every value of it, as `{DIR}/{PREFIX}.sweep.txt`:

    #filter_sweep<TAB>digits=K<TAB>mq=..<TAB>cp=..<TAB>ip=..<TAB>regions=..          one line
    #file<TAB>k<TAB>path<TAB>primary=<n>                                          per BAM file (k from 1), then its three tables
    #mapq       256 rows: the MAPQ byte
    #clip       rows 0.000 .. 1.000 (the quotient ROUNDED UP to K digits: row v holds (v - 10^-K, v]), then `undefined` (M + I + S = 0)
    #identity   `<0` (NM beyond the alignment), rows 0.000 .. 1.000 (TRUNCATED: row v holds [v, v + 10^-K)), `>1` (a negative NM),
                `undefined` (no NM tag, one that is no integer, M + I + D = 0)
    value records bases records_others bases_others kept_at kept_bases_at          the columns of every row; every row is written

records / bases count the primary records on the row and the reference bases they cover; the `_others` columns those of them that pass
the OTHER TWO tests at the run's thresholds.  kept_at / kept_bases_at say what would be `kept` if this one threshold were set to the
row's value while the other two stay: the `_others` columns summed over the rows >= the value (mapq, identity; `>1` passes every
identity threshold up to 1) or <= it (clip).  The special rows carry `-` there.  With `-R`, only the records whose reference span
overlaps a region of the BED file are counted (filter_reads.py's rule).

The BAM bytes are inflated and walked on the device as for GCI.py; gci_bam_sweep (k_sweep.hip) reads every primary record's CIGAR and
first NM tag, bins the quotients in exact integers and tests them with the record filter's own arithmetic, and only the tables cross to
the host (pipeline.bam_filter_sweep)."""
from __future__ import annotations

import argparse
import os
import sys

from . import _lib, bedgraph_cli, filterdepth_cli, phases, pipeline
from ._lib import GciError


def build_parser(prog: str) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog=prog, description="How the thresholds of GCI.py's record filter cut BAM file(s): the distribution of MAPQ, clip quotient and identity "
        "quotient over the primary records, and what every value of each threshold, taken alone, would keep: {DIR}/{PREFIX}.sweep.txt with "
        "the columns " + " ".join(pipeline.SWEEP_COLUMNS) + ".",
        epilog="The counts are of the records of ONE file, before the -op join across files: reads that join drops count as kept here.  "
        "`bases` are covered reference bases as bam_depth.py counts them (the bases under M, = and X), not GCI.py's flank-trimmed spans.  "
        "A quotient is binned in exact integers, the thresholds of a run are compared as the filter compares them, in IEEE f64: a row's "
        "edge agrees with the filter's comparison for thresholds that are multiples of 10^-K whenever the denominators are below 2^40 -- "
        "two distinct quotients with denominators d and 10^K are at least 1 / (d * 10^K) apart, more than the two roundings involved -- "
        "and every real read is far below that.")
    parser.add_argument("bams", metavar="in.bam", nargs="*", help="BAM file(s), one set of tables each; the contigs are those of the first")
    parser.add_argument("-d", dest="directory", metavar="DIR", default=".", help="The directory of the output file [.]")
    parser.add_argument("-o", "--output", dest="prefix", metavar="PREFIX", default="GCI_sweep", help="Prefix of the output file [GCI_sweep]")
    parser.add_argument("--chrs", default="", help="A list of chromosomes separated by comma")
    parser.add_argument("-R", dest="regions", metavar="BED", default=None, help="Count only the records whose reference span overlaps a region "
                        "of this BED file [every primary record]")
    parser.add_argument("-mq", "--map-qual", dest="map_qual", metavar="INT", type=int, default=30, help="Minium mapping quality for alignments [30]")
    parser.add_argument("-cp", "--clip-percent", dest="clip_percent", metavar="FLOAT", type=float, default=0.1,
                        help="Maximum clipped percentage of the alignment [0.1]")
    parser.add_argument("-ip", "--iden-percent", dest="iden_percent", metavar="FLOAT", type=float, default=0.9,
                        help="Minimum identity (num_match_res/len_aln) of alignments [0.9]")
    parser.add_argument("--digits", metavar="K", type=int, default=3, choices=(1, 2, 3), help="Decimal digits of a quotient's rows [3]")
    parser.add_argument("-t", "--threads", type=int, default=1, help="Host threads for the ingest paths that inflate on the host [1]")
    parser.add_argument("-f", "--force", action="store_true", help="Force rewriting of existing files [False]")
    parser.set_defaults(classes=None, join=False, ovlp_percent=None, mq_cutoff=None, cover=None)      # (what filter_depth.py's option checks look at)
    return parser


def header_line(args) -> str:
    return "#filter_sweep\tdigits=%d\tmq=%d\tcp=%r\tip=%r\tregions=%s\n" % (args.digits, args.map_qual, args.clip_percent, args.iden_percent,
                                                                        args.regions if args.regions is not None else "-")


def file_text(k: int, path: str, table, digits: int) -> str:
    """The `#file` line of the k-th file (from 1) and its three tables."""
    primary = int(table[:_lib.SweepRows(digits).clip0, 0].sum())
    return "#file\t%d\t%s\tprimary=%d\n" % (k, path, primary) + pipeline.sweep_text(table, digits)


def run(args) -> str:
    _, bams, _ = filterdepth_cli.checked_options(args)
    out = f"{args.directory}/{args.prefix}.sweep.txt"
    pipeline.refuse_overwrite(out, args.force)
    regions = None
    if args.regions is not None:
        if not os.path.isfile(args.regions):
            sys.exit(f'ERROR!!! The file "{args.regions}" does not exist')
        regions = bedgraph_cli.parse_regions(args.regions)
    chrs = filterdepth_cli.checked_files(args, bams)
    opts = pipeline.FateOpts(args.map_qual, args.clip_percent, args.iden_percent)
    engine = pipeline.default_engine()
    try:
        result = pipeline.bam_filter_sweep(engine, bams, chrs, opts, args.threads, args.digits, regions)
    except GciError as e:
        filterdepth_cli.exit_for_record(e)
    with open(out, "w") as f:
        f.write(header_line(args))
        for k, (path, table) in enumerate(zip(result.files, result.tables)):
            f.write(file_text(k + 1, path, table, args.digits))
    return out


def main(argv=None) -> str:
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: filter_sweep.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
