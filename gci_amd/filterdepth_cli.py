"""`python filter_depth.py [-d DIR] [-o PREFIX] [--chrs a,b] [-mq INT] [-ip FLOAT] [-cp FLOAT] [-J] [--classes a,b] [-t INT] [-f] a.bam
[b.bam ...]`: WHY the filtered depth of GCI.py is low where it is low.  Every record of the BAM file(s) falls into exactly one class,
named after the first test of the reference's read_sam (GCI.py:152-168) it fails, in the reference's order -- secondary,
supplementary, mapq (`-mq`), clip (`-cp`), identity (`-ip`) -- or `kept`; the per-base depth of every class is written as
`{DIR}/{PREFIX}.{class}.depth.gz`, which plot_depth.py, depth_plotter_v2.py, depth_dist.py (`-R sample.0.depth.bed`),
depth_to_bedgraph.py and GCI_score.py read as they read GCI.py's, and `{DIR}/{PREFIX}.filter.txt` holds the records per file and
class and the covered bases per contig and class.  The reference answers the question with utility/filter_bam.py (write the filtered
BAM, compare it with the raw one in a genome browser); this utility has no counterpart there.

Coverage is counted as bam_depth.py counts it: CIGAR-aware (M, = and X cover; D only with `-J`; N never), no flank.  So the six
tracks add up, base for base, to `bam_depth.py -g 0x700` on the same files (unmapped records, and records on no or an unselected
contig, belong to no class).  `kept` is NOT GCI.py's depth: that one counts the span of every kept alignment with its flank cut off,
and drops reads in the `-op` join across files; reads the join drops show as `kept` here.  QCFAIL and DUP are no tests of read_sam
and no classes.

The BAM bytes are inflated and walked on the device as for GCI.py; gci_bam_fate (k_fate.hip) gives every record its class with the
record filter's own arithmetic, gci_bam_cover_size_sel / _write (k_cover.hip) turn the records of a class into covered intervals,
the depth build adds them and the project's DEFLATE writer (k_deflate.hip) writes the files (pipeline.bam_filter_depth)."""
from __future__ import annotations

import argparse
import os
import sys
import zlib

from . import phases, pipeline
from ._lib import GCI_E_BAD_NM_TYPE, GCI_E_MALFORMED, GCI_E_NO_NM, GCI_E_ZERO_DIV, GciError
from .formats import bam as bamfmt

WHAT_THE_RECORD_IS = {
    GCI_E_MALFORMED: "holds a malformed BAM record (record %d)",
    GCI_E_NO_NM: "holds a record without an NM tag (record %d): GCI.py would have raised KeyError",
    GCI_E_BAD_NM_TYPE: "holds a record whose NM tag is not an integer (record %d)",
    GCI_E_ZERO_DIV: "holds a record whose CIGAR leaves a quotient of the filter without a denominator (record %d): GCI.py would have raised "
                    "ZeroDivisionError",
}


def build_parser(prog: str) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog=prog, description="Per-base depth of the records of BAM file(s) split by what GCI.py's record filter does with them: one "
        "{DIR}/{PREFIX}.{class}.depth.gz per class, named after the first test the class's records fail (secondary, supplementary, mapq, "
        "clip, identity) or `kept`, and {DIR}/{PREFIX}.filter.txt with the record counts and covered bases.",
        epilog="Coverage is counted as bam_depth.py counts it (CIGAR-aware, -J for deletions, no flank): the six tracks add up, base for base, "
        "to `bam_depth.py -g 0x700` on the same files.  `kept` is not GCI.py's depth: that one uses the alignments' spans with their flank "
        "cut off, and the -op join across files is not applied here (reads it drops show as `kept`).")
    parser.add_argument("bams", metavar="in.bam", nargs="*", help="BAM file(s); their depths add per class, the contigs are those of the first")
    parser.add_argument("-d", dest="directory", metavar="DIR", default=".", help="The directory of the output files [.]")
    parser.add_argument("-o", "--output", dest="prefix", metavar="PREFIX", default="GCI_fate", help="Prefix of the output files [GCI_fate]")
    parser.add_argument("--chrs", default="", help="A list of chromosomes separated by comma")
    parser.add_argument("-mq", "--map-qual", dest="map_qual", metavar="INT", type=int, default=30, help="Minium mapping quality for alignments [30]")
    parser.add_argument("-ip", "--iden-percent", dest="iden_percent", metavar="FLOAT", type=float, default=0.9,
                        help="Minimum identity (num_match_res/len_aln) of alignments [0.9]")
    parser.add_argument("-cp", "--clip-percent", dest="clip_percent", metavar="FLOAT", type=float, default=0.1,
                        help="Maximum clipped percentage of the alignment [0.1]")
    parser.add_argument("-J", dest="count_del", action="store_true", help="Count deletions as covered [False]")
    parser.add_argument("--classes", default=",".join(pipeline.FATE_WANTED), help="The classes to write, separated by comma [%(default)s]")
    parser.add_argument("-t", "--threads", type=int, default=1, help="Host threads for the ingest paths that inflate on the host [1]")
    parser.add_argument("-f", "--force", action="store_true", help="Force rewriting of existing files [False]")
    return parser


def write_table(path: str, bams, counts, classes, targets, sums) -> None:
    """{PREFIX}.filter.txt: the records per file and class, then the covered bases (the track sums) per contig and class of the run."""
    names = pipeline.FATE_NAMES[:7]
    with open(path, "w") as f:
        f.write("#records\n" + "\t".join(("file",) + names) + "\n")
        for bam, row in zip(bams, counts):
            f.write("\t".join([bam] + [str(row[k]) for k in range(7)]) + "\n")
        f.write("#covered_bases\n" + "\t".join(["contig"] + list(classes)) + "\n")
        for k, t in enumerate(targets):
            f.write("\t".join([t] + [str(int(sums[c][k])) for c in classes]) + "\n")
        f.write("\t".join(["total"] + [str(int(sums[c].sum())) for c in classes]) + "\n")


def run(args) -> str:
    if not args.bams:
        sys.exit("ERROR!!! No BAM file given")
    classes = []
    for c in (c for c in args.classes.split(",") if c):
        if c not in pipeline.FATE_WANTED:
            sys.exit(f'ERROR!!! The class "{c}" of --classes is not one of {", ".join(pipeline.FATE_WANTED)}')
        if c not in classes:
            classes.append(c)
    if not classes:
        sys.exit("ERROR!!! No class given with --classes")
    table = f"{args.directory}/{args.prefix}.filter.txt"
    for path in [f"{args.directory}/{args.prefix}.{c}.depth.gz" for c in classes] + [table]:
        pipeline.refuse_overwrite(path, args.force)
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
    opts = pipeline.FateOpts(args.map_qual, args.clip_percent, args.iden_percent, args.count_del)
    engine = pipeline.default_engine()
    try:
        result = pipeline.bam_filter_depth(engine, args.bams, chrs, opts, args.threads, classes)
    except pipeline.TracksDoNotFit as e:
        sys.exit(f"ERROR!!! The {e.n_tracks} depth tracks of this run ({e.track_bytes} bytes each) do not fit into the free device memory "
                 f"({e.free_bytes} bytes)\nPlease ask for fewer classes (--classes) or fewer contigs (--chrs)")
    except GciError as e:
        if e.status not in WHAT_THE_RECORD_IS or e.rec < 0:
            raise
        sys.exit(f'ERROR!!! The file "{getattr(e, "path", "?")}" ' + WHAT_THE_RECORD_IS[e.status] % e.rec)
    sums = {}
    for c in classes:
        depths = result.tracks[c]
        sums[c] = engine.depth_sum(depths.track)
        with phases.wall("write_depth_gz[%s] (deflate on the device, D2H, file)" % c):
            pipeline._write_depth_members(args.directory, f"{args.prefix}.{c}", depths)
    write_table(table, args.bams, result.counts, classes, result.tracks[classes[0]].targets, sums)
    return table


def main(argv=None) -> str:
    argv = sys.argv if argv is None else list(argv)
    args = build_parser(os.path.basename(argv[0])).parse_args(argv[1:])
    phase_file = phases.env_start()                   # GCI_PHASES=<file.json>: where the run spends its time (nothing is printed)
    try:
        out = run(args)
        if os.environ.get("GCI_ASSERT_NO_TORCH") == "1" and "torch" in sys.modules:      # (tests: a run holds its buffers itself)
            sys.exit("ERROR!!! internal: filter_depth.py imported torch")
        return out
    finally:
        if phase_file:
            pipeline.note_device_memory()
            phases.report(phase_file)
            phases.stop()


if __name__ == "__main__":
    main()
