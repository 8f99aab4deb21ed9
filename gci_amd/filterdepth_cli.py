"""`python filter_depth.py [-d DIR] [-o PREFIX] [--chrs a,b] [-mq INT] [-ip FLOAT] [-cp FLOAT] [-J] [--classes a,b] [-t INT] [-f]
[--join [-op FLOAT] [--mq-cutoff INT] [--cover N]] a.bam [b.bam | b.paf ...]`: WHY the filtered depth of GCI.py is low where it is low.  Every record of the BAM file(s) falls into exactly one class,
named after the first test of the reference's read_sam (GCI.py:152-168) it fails, in the reference's order -- secondary,
supplementary, mapq (`-mq`), clip (`-cp`), identity (`-ip`) -- or `kept`; the per-base depth of every class is written as
`{DIR}/{PREFIX}.{class}.depth.gz`, which plot_depth.py, depth_plotter_v2.py, depth_dist.py (`-R sample.0.depth.bed`),
depth_to_bedgraph.py and GCI_score.py read as they read GCI.py's, and `{DIR}/{PREFIX}.filter.txt` holds the records per file and
class and the covered bases per contig and class.  The reference answers the question with utility/filter_bam.py (write the filtered
BAM, compare it with the raw one in a genome browser); this utility has no counterpart there.

Coverage is counted as bam_depth.py counts it: CIGAR-aware (M, = and X cover; D only with `-J`; N never), no flank.  So the six
tracks add up, base for base, to `bam_depth.py -g 0x700` on the same files (unmapped records, and records on no or an unselected
contig, belong to no class).  `kept` is NOT GCI.py's depth: that one counts the span of every kept alignment with its flank cut off,
and drops reads in the `-op` join across files; without `--join`, reads the join drops show as `kept` here.  QCFAIL and DUP are no
tests of read_sam and no classes.

`--join`: the files -- BAM and PAF, told apart as GCI.py tells them apart -- are ONE read set aligned several times, as GCI.py's
`--hifi` list: they are joined by read name (GCI.py:272-301), not added, and the depth is that of the N-th BAM of the command line
(`--cover N`).  Every `kept` record of that file then falls into one of five further classes: shadowed (a later record of the same
name in the same file replaces it in the reference's dict), unpaired (below `--mq-cutoff` everywhere, and some file has no passing
record of the read), contig (another file places the read on another contig), overlap (it overlaps too little between two files,
`-op`) or joined.  `joined` is the set of reads GCI.py counts; it is not GCI.py's depth, which counts each read's span narrowed to
the intersection over the files, with the flank cut off -- GCI.py itself writes that one.  The ten tracks still add up to
`bam_depth.py -g 0x700` on the covered file, and the five new ones to the `kept` track of a run without `--join`.  The covered BAM
is read twice: once for the join, once for the depth.

The BAM bytes are inflated and walked on the device as for GCI.py; gci_bam_fate (k_fate.hip) gives every record its class with the
record filter's own arithmetic, gci_bam_cover_size_sel / _write (k_cover.hip) turn the records of a class into covered intervals,
the depth build adds them and the project's DEFLATE writer (k_deflate.hip) writes the files (pipeline.bam_filter_depth).  With
`--join`, gci_name_join_fate (k_join.hip) says what the join does with every record and gci_fate_refine moves the `kept` ones."""
from __future__ import annotations

import argparse
import os
import sys
import zlib

from . import _lib, phases, pipeline
from ._lib import GCI_E_BAD_NM_TYPE, GCI_E_MALFORMED, GCI_E_NO_NM, GCI_E_ZERO_DIV, GciError
from .formats import bam as bamfmt

JOIN_DEFAULT = pipeline.FATE_WANTED[:5] + pipeline.JOIN_FATE_NAMES      # the five record tests, then what becomes of `kept` in the join

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
        "cut off, and without --join the -op join across files is not applied (reads it drops show as `kept`).  With --join the files are "
        "one read set aligned several times: `kept` splits into shadowed, unpaired, contig, overlap and joined -- the reads GCI.py counts, "
        "not its depth -- and the BAM file --cover names is read twice.")
    parser.add_argument("bams", metavar="in.bam", nargs="*", help="BAM file(s); their depths add per class, the contigs are those of the first.  "
                        "With --join: BAM and PAF files of one read set, joined by read name")
    add_filter_arguments(parser, "GCI_fate", "write")
    parser.add_argument("-J", dest="count_del", action="store_true", help="Count deletions as covered [False]")
    return parser


def add_filter_arguments(parser: argparse.ArgumentParser, prefix: str, verb: str) -> None:
    """The options filter_depth.py and filter_reads.py share: where the output goes, the contigs, the record filter's thresholds, the
    classes to `verb`, the join across files, host threads, -f."""
    parser.add_argument("-d", dest="directory", metavar="DIR", default=".", help="The directory of the output files [.]")
    parser.add_argument("-o", "--output", dest="prefix", metavar="PREFIX", default=prefix, help="Prefix of the output files [%s]" % prefix)
    parser.add_argument("--chrs", default="", help="A list of chromosomes separated by comma")
    parser.add_argument("-mq", "--map-qual", dest="map_qual", metavar="INT", type=int, default=30, help="Minium mapping quality for alignments [30]")
    parser.add_argument("-ip", "--iden-percent", dest="iden_percent", metavar="FLOAT", type=float, default=0.9,
                        help="Minimum identity (num_match_res/len_aln) of alignments [0.9]")
    parser.add_argument("-cp", "--clip-percent", dest="clip_percent", metavar="FLOAT", type=float, default=0.1,
                        help="Maximum clipped percentage of the alignment [0.1]")
    parser.add_argument("--classes", default=None, help="The classes to %s, separated by comma [%s; with --join: %s]"
                        % (verb, ",".join(pipeline.FATE_WANTED), ",".join(JOIN_DEFAULT)))
    parser.add_argument("--join", action="store_true", help="Apply the join across files by read name and split `kept` by what it does [False]")
    parser.add_argument("-op", "--ovlp-percent", dest="ovlp_percent", metavar="FLOAT", type=float, default=None,
                        help="With --join: minimum overlapping percentage of the same read alignment between files [0.9]")
    parser.add_argument("--mq-cutoff", dest="mq_cutoff", metavar="INT", type=int, default=None,
                        help="With --join: the cutoff of mapping quality for keeping an alignment that only some files hold [50]")
    parser.add_argument("--cover", metavar="N", type=int, default=None, help="With --join: the N-th BAM file of the command line gives the depth [1]")
    parser.add_argument("-t", "--threads", type=int, default=1, help="Host threads for the ingest paths that inflate on the host [1]")
    parser.add_argument("-f", "--force", action="store_true", help="Force rewriting of existing files [False]")


def write_table(path: str, bams, counts, classes, targets, sums, join=None) -> None:
    """{PREFIX}.filter.txt: the records per file and class, then the covered bases (the track sums) per contig and class of the run.
    join (the result of a --join run): every file of the join gets a row -- the covered BAM all columns, any other file `-` under the
    record tests, its passing records under `kept` and what the join does with them."""
    names = pipeline.FATE_NAMES[:7]
    with open(path, "w") as f:
        if join is None:
            f.write("#records\n" + "\t".join(("file",) + names) + "\n")
            for bam, row in zip(bams, counts):
                f.write("\t".join([bam] + [str(row[k]) for k in range(7)]) + "\n")
        else:
            first, n = _lib.JOIN_FATE_FIRST, len(pipeline.JOIN_FATE_NAMES)
            f.write("#records\n" + "\t".join(("file",) + names + pipeline.JOIN_FATE_NAMES) + "\n")
            for k, (name, row) in enumerate(zip(join.join_files, join.join_counts)):
                if k == join.cover_file:
                    cells = [str(counts[0][c]) for c in range(7)] + [str(counts[0][c]) for c in range(first, first + n)]
                else:
                    cells = ["-"] * 6 + [str(sum(row[first:first + n]))] + [str(row[c]) for c in range(first, first + n)]
                f.write("\t".join([name] + cells) + "\n")
        f.write("#covered_bases\n" + "\t".join(["contig"] + list(classes)) + "\n")
        for k, t in enumerate(targets):
            f.write("\t".join([t] + [str(int(sums[c][k])) for c in classes]) + "\n")
        f.write("\t".join(["total"] + [str(int(sums[c].sum())) for c in classes]) + "\n")


def checked_options(args):
    """The option checks that need no file -> (classes, BAM files, pipeline.JoinFateOpts or None); every refusal exits."""
    if not args.bams:
        sys.exit("ERROR!!! No BAM file given")
    if not args.join:
        for opt, value in (("-op", args.ovlp_percent), ("--mq-cutoff", args.mq_cutoff), ("--cover", args.cover)):
            if value is not None:
                sys.exit(f"ERROR!!! The option {opt} needs --join")
    wanted = pipeline.FATE_WANTED + (pipeline.JOIN_FATE_NAMES if args.join else ())
    given = args.classes if args.classes is not None else ",".join(JOIN_DEFAULT if args.join else pipeline.FATE_WANTED)
    classes = []
    for c in (c for c in given.split(",") if c):
        if c not in wanted:
            hint = f' ({", ".join(pipeline.JOIN_FATE_NAMES)} need --join)' if c in pipeline.JOIN_FATE_NAMES else ""
            sys.exit(f'ERROR!!! The class "{c}" of --classes is not one of {", ".join(wanted)}{hint}')
        if c not in classes:
            classes.append(c)
    if not classes:
        sys.exit("ERROR!!! No class given with --classes")
    bams, pafs, join = list(args.bams), [], None
    if args.join:                                         # BAM and PAF files are told apart as GCI.py tells them apart (gci_amd/cli.py)
        bams, pafs = [p for p in args.bams if p.endswith(".bam")], [p for p in args.bams if not p.endswith(".bam")]
        if not bams:
            sys.exit("ERROR!!! No BAM file among the files: --join takes its depth from a BAM file")
        cover = 1 if args.cover is None else args.cover
        if not 1 <= cover <= len(bams):
            sys.exit(f"ERROR!!! --cover {cover}: the files hold {len(bams)} BAM file(s)")
        for path in pafs:
            if not os.path.isfile(path):
                sys.exit(f'ERROR!!! The file "{path}" does not exist')
        join = pipeline.JoinFateOpts(pafs, 50 if args.mq_cutoff is None else args.mq_cutoff, 0.9 if args.ovlp_percent is None else args.ovlp_percent,
                                     cover - 1)
    return classes, bams, join


def checked_files(args, bams) -> list:
    """Every BAM file readable, one @SQ table, --chrs in it, the output directory there -> the chromosomes asked for; every refusal exits."""
    for path in bams:
        try:
            bamfmt.read_header(path)
        except (OSError, ValueError, EOFError, zlib.error) as e:
            sys.exit(f'ERROR!!! The file "{path}" cannot be read as a BAM file ({e})')
    try:
        first = pipeline.same_sq_table(bams)
    except pipeline.SqMismatch as e:
        sys.exit(f"ERROR!!! {e}")
    chrs = [c for c in args.chrs.split(",") if c]
    for c in chrs:
        if c not in first.references:
            sys.exit(f'ERROR!!! The chromosome "{c}" of --chrs is not in the header of "{bams[0]}"')
    if not os.path.isdir(args.directory):
        os.makedirs(args.directory, exist_ok=True)
    return chrs


def exit_for_record(e: GciError) -> None:
    """A GciError that names a record the reference would have raised on (or a malformed one) as the command line's message; any other
    is raised again."""
    if getattr(e, "in_join", False):
        sys.exit(f'ERROR!!! The file "{getattr(e, "path", "?")}" holds an alignment of query length zero that the join across files divides by '
                 f"(record {e.rec}): GCI.py would have raised ZeroDivisionError")
    if e.status not in WHAT_THE_RECORD_IS or e.rec < 0:
        raise e
    sys.exit(f'ERROR!!! The file "{getattr(e, "path", "?")}" ' + WHAT_THE_RECORD_IS[e.status] % e.rec)


def run(args) -> str:
    classes, bams, join = checked_options(args)
    table = f"{args.directory}/{args.prefix}.filter.txt"
    for path in [f"{args.directory}/{args.prefix}.{c}.depth.gz" for c in classes] + [table]:
        pipeline.refuse_overwrite(path, args.force)
    chrs = checked_files(args, bams)
    opts = pipeline.FateOpts(args.map_qual, args.clip_percent, args.iden_percent, args.count_del)
    engine = pipeline.default_engine()
    try:
        if join is None:
            result = pipeline.bam_filter_depth(engine, bams, chrs, opts, args.threads, classes)
        else:
            result = pipeline.bam_filter_depth(engine, bams, chrs, opts, args.threads, classes, join=join)
    except pipeline.TracksDoNotFit as e:
        sys.exit(f"ERROR!!! The {e.n_tracks} depth tracks of this run ({e.track_bytes} bytes each) do not fit into the free device memory "
                 f"({e.free_bytes} bytes)\nPlease ask for fewer classes (--classes) or fewer contigs (--chrs)")
    except GciError as e:
        exit_for_record(e)
    sums = {}
    for c in classes:
        depths = result.tracks[c]
        sums[c] = engine.depth_sum(depths.track)
        with phases.wall("write_depth_gz[%s] (deflate on the device, D2H, file)" % c):
            pipeline._write_depth_members(args.directory, f"{args.prefix}.{c}", depths)
    write_table(table, bams, result.counts, classes, result.tracks[classes[0]].targets, sums, result if join is not None else None)
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
