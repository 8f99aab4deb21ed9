"""Host-side mirror of the reference's hot-path functions, driving the HIP kernels.

Same names, argument meaning, outputs and error behaviour as /root/reference/GCI.py so that a
maintainer (and the parity tests) can read one against the other:

    get_Ns_ref            GCI.py:18-46      filter                  GCI.py:172-312
    merge_gaps_depths     GCI.py:315-329    merge_two_type_depth    GCI.py:332-353
    collapse_depth_range  GCI.py:356-390    merge_depth             GCI.py:393-419
    compute_index         GCI.py:522-657    GCI                     GCI.py:897-1028

What differs is where the work happens: `depths` is a `DepthTracks` object whose per-base
data lives in HBM as one int32 buffer for all contigs; records are decoded and filtered, names
joined, depth built, masked, merged, scanned and rendered to text by gfx950 kernels
(gci_amd/csrc/gci_hip.hip).  The host parses containers (BGZF, PAF, FASTA), does the tiny
interval algebra (gci_amd/score.py) and writes files.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import queue
import threading
import warnings
import sys
from concurrent.futures import Future, ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from . import hbm, hostio, phases, score
from .device import ALLELE_SITE_DTYPE, Buffer, Engine, INDEL_SITE_DTYPE, JoinInput, MISMATCH_SITE_DTYPE, REC_DTYPE, SITE_DTYPE, name_hash_np
from . import _lib
from ._lib import GciError, REC_HQ, REC_PASS
from .formats import bam as bamfmt
from .formats import bgzf
from .formats import fasta

_ENGINE: Optional[Engine] = None
SHARD = None              # gci_amd.shard.Context of a multi-GPU run (set by cli.main), None for a single process


_ENGINE_LOCK = threading.Lock()


def default_engine() -> Engine:
    global _ENGINE
    with _ENGINE_LOCK:                                    # (the helper thread of prefetch_member_tables may be the first to ask)
        if _ENGINE is None:
            # (a contig-sharded run exchanges tensors through torch.distributed: its buffers are torch's; a single process holds its
            # own -- hbm.py -- unless GCI_HBM or an already imported torch says otherwise)
            _ENGINE = Engine(SHARD.device_index if SHARD is not None else 0, backend="torch" if SHARD is not None else None)
        return _ENGINE


def note_device_memory() -> None:
    """Into the phase log: what the process took from the driver (the arena's slabs: include/gci_hip.h gci_dev_arena_info) and what of it
    is handed out at the end of the run -- a driver allocation costs by the GB on this chip, so this is a number to keep small."""
    if _ENGINE is None or not phases.on():
        return
    try:
        r, u, n = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _ENGINE.lib.gci_dev_arena_info(_ENGINE.device.index or 0, ctypes.byref(r), ctypes.byref(u), ctypes.byref(n))
        phases.note("device_memory", {"provider": _ENGINE.T.name, "arena_slab_bytes": int(r.value), "arena_bytes_handed_out": int(u.value),
                                      "arena_slabs": int(n.value), "pool_bytes_held": int(hbm.memory_held(_ENGINE.device.index or 0)) if _ENGINE.T.name == "native" else None})
    except Exception:                                      # noqa: BLE001  (a note, not a result)
        pass


def _slice_bound(v: int, L: int) -> int:
    if v < 0:
        return max(v + L, 0)
    return min(v, L)


class DepthTracks:
    """The reference's `depths` dict (contig -> per-base array), resident in HBM."""

    def __init__(self, engine: Engine, targets_length: Dict[str, int], track: Buffer):
        self.engine = engine
        self.targets_length = dict(targets_length)
        self.targets = list(targets_length.keys())
        self.lengths = [int(targets_length[t]) for t in self.targets]
        self.track = track
        self.all_targets = list(self.targets)      # contig-sharded run: every selected contig in header order (this rank holds `targets`)
        # by-products of the fused build, valid until the track is modified (gap mask)
        self._fresh_runs = None        # ((lo, hi, flank), per-contig raw runs)
        self._fresh_sums = None
        # N runs whose mask is still to be applied (merge_gaps_depths(lazy=True): a two-read-type run masks both tracks in the one
        # pass that also merges them, merge_two_type_depth) -- applied by whatever looks at the track first
        self._pending_gaps: Optional[np.ndarray] = None
        self._masked_with: Optional[bytes] = None      # the rows of the mask this track already carries

    def invalidate(self) -> None:
        self._fresh_runs = None
        self._fresh_sums = None

    def _bind_layout(self) -> None:
        if self.engine.lengths != self.lengths:
            self.engine.set_layout(self.lengths)

    def _bind(self) -> None:
        self._bind_layout()
        if self._pending_gaps is not None:
            rows, self._pending_gaps = self._pending_gaps, None
            self.engine.gap_mask(self.track, self.engine.to_device(rows))
            self._masked_with = rows.tobytes()
            self.invalidate()

    def keys(self):
        return self.targets_length.keys()

    def __contains__(self, t) -> bool:
        return t in self.targets_length

    def __len__(self) -> int:
        return len(self.targets)

    def __getitem__(self, target: str) -> np.ndarray:
        """Host copy of one contig (int64, as the reference's arrays are)."""
        self._bind()
        c = self.targets.index(target)
        o = self.engine.offsets[c]
        return self.track[o:o + self.lengths[c]].cpu().numpy().astype(np.int64)

    def to_host(self) -> Dict[str, np.ndarray]:
        return {t: self[t] for t in self.targets}

    def sums(self) -> np.ndarray:
        if self._fresh_sums is not None:
            return self._fresh_sums
        self._bind()
        return self.engine.depth_sum(self.track)

    def mean(self) -> float:
        """np.mean over the concatenation of all contigs (GCI.py:862-868): integers, so exact.  In a contig-sharded run
        the numerator and denominator are ONE integer all-reduce over the ranks (RCCL over xGMI)."""
        total, bases = int(self.sums().sum()), sum(self.lengths)
        if _sharded():
            total, bases = SHARD.all_reduce_sum([total, bases])
        return float(total) / float(bases)


# ==============================================================================================
# gaps
# ==============================================================================================

def _is_root() -> bool:
    return SHARD is None or SHARD.root


def _sharded() -> bool:
    """A contig-sharded run: more than one rank -- or ONE rank made to take the sharded path (GCI_FORCE_SHARDED=1 under
    torch.distributed.run --nproc-per-node 1: every collective of the multi-GPU path, RCCL included, on a single GPU)."""
    return SHARD is not None and (SHARD.world > 1 or SHARD.forced)


def refuse_overwrite(path: str, force) -> None:
    """The reference's guard in front of every output file (`-f` / `--force`).  In a contig-sharded run rank 0 looks -- another
    rank could find what rank 0 has written in the meantime -- and all ranks leave together."""
    hit = os.path.exists(path) and force == False  # noqa: E712
    if _sharded():
        hit = SHARD.all_reduce_sum([1 if (hit and _is_root()) else 0])[0] > 0
    if hit:
        sys.exit(f'ERROR!!! The file "{path}" exists\nPlease use "-f" or "--force" to rewrite')


def get_Ns_ref(reference=None, prefix="GCI", directory=".", force=False):
    if _INGEST_AHEAD:                                                     # (a helper thread owns the default context just now)
        side = _side_engine()
        with side.T.stream(side.stream):
            _, ns_bed = fasta.n_runs_device(side, reference)
    else:
        _, ns_bed = fasta.n_runs_device(default_engine(), reference)      # N4: the scan itself runs on the GPU
    if len(ns_bed) > 0:
        path = f"{directory}/{prefix}.gaps.bed"
        refuse_overwrite(path, force)
        if _is_root():
            with open(path, "w") as f:
                for target, segments in ns_bed.items():
                    for a, b in segments:
                        f.write(f"{target}\t{a}\t{b}\n")
        return ns_bed, path
    return None, None


def merge_gaps_depths(depths: DepthTracks = None, Ns_bed=None, lazy: bool = False) -> DepthTracks:
    """lazy: the mask is noted and applied by whatever reads the track first -- in a two-read-type run that is the one pass of
    merge_two_type_depth, which masks both tracks, merges them and finds the issue runs of all three."""
    if Ns_bed is not None:
        rows = [(depths.targets.index(t), a, b, 0) for t, segs in Ns_bed.items() if t in depths for a, b in segs]
        if rows:
            arr = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
            if depths._pending_gaps is None and depths._masked_with == arr.tobytes():
                return depths                         # masked with exactly these runs already (the merged track of two masked ones)
            depths._bind()
            if lazy:
                depths._pending_gaps = arr
                depths.invalidate()
                return depths
            depths.engine.gap_mask(depths.track, depths.engine.to_device(arr))
            depths._masked_with = arr.tobytes()
            depths.invalidate()
    return depths


# ==============================================================================================
# PAF path (host; SURVEY.md R3 -- GPU tokeniser is a "next" row)
# ==============================================================================================

def _merge_span(pairs: List[Tuple[int, int]]) -> Tuple[int, int, int]:
    """Union of closed-touching blocks: (covered length, start, end of the longest merged block,
    the leftmost one on ties).  GCI.py:83-93 holds the first sorted block against itself: one whose end lies before
    its start is counted twice, and the longest piece is the maximum over all pieces, whatever their sign."""
    pairs = sorted(pairs)
    lo, hi = pairs[0]
    covered = hi - lo if hi < lo else 0
    best = (hi - lo, lo, hi)
    for a, b in pairs[1:] + [(None, None)]:
        if a is not None and hi >= a:
            hi = max(hi, b)
            continue
        covered += hi - lo
        if hi - lo > best[0]:
            best = (hi - lo, lo, hi)
        if a is not None:
            lo, hi = a, b
    return covered, best[1], best[2]


def paf_filter(paf_files: Sequence[str], targets: Sequence[str], map_qual: int, mq_cutoff: int, iden_percent: float
               ) -> Tuple[List[Dict[str, Tuple[str, int, int, int]]], Set[str]]:
    """GCI.py:211-254 as dicts, from the native filter (hostio.paf_filter / gci_paf_filter): what the reference's
    paf_lines and high_qual hold.  The product path (filter()) uploads the native records directly."""
    per_file, high_qual = [], set()
    for recs, names, off in hostio.paf_filter(paf_files, targets, map_qual, mq_cutoff, iden_percent):
        r = recs.reshape(-1).view(REC_DTYPE)
        d = {}
        for i in range(r.shape[0]):
            q = bytes(names[int(off[i]):int(off[i + 1])]).decode()
            d[q] = (targets[int(r["contig"][i])], int(r["start"][i]), int(r["end"][i]), int(r["qlen"][i]))
            if int(r["flags"][i]) & REC_HQ:
                high_qual.add(q)
        per_file.append(d)
    return per_file, high_qual


def _paf_join_input(engine: Engine, d: Dict[str, Tuple[str, int, int, int]], high_qual: Set[str],
                    tindex: Dict[str, int]) -> JoinInput:
    names = [q.encode() for q in d.keys()]
    n = len(names)
    recs = np.zeros(n, dtype=REC_DTYPE)
    if n:
        recs["name_hash"] = name_hash_np(names)
        vals = list(d.values())
        recs["contig"] = [tindex[v[0]] for v in vals]
        for fld, k in (("start", 1), ("end", 2), ("qlen", 3)):
            col = np.asarray([v[k] for v in vals], dtype=np.int64)
            if (col > 0x7FFFFFFF).any() or (col < -0x80000000).any():
                raise GciError(-1, "PAF coordinate does not fit int32")
            recs[fld] = col
        recs["rec_idx"] = np.arange(n)
        recs["flags"] = [REC_PASS | (REC_HQ if q in high_qual else 0) for q in d.keys()]
        recs["name_len"] = [len(x) for x in names]
    lens = np.fromiter((len(x) for x in names), dtype=np.int64, count=n)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    blob = np.frombuffer(b"".join(names) or b"\x00", dtype=np.uint8)
    return JoinInput(engine.to_device(recs.view(np.uint8).reshape(n, 32) if n else np.zeros((0, 32), np.uint8)),
                     engine.to_device(blob), engine.to_device(off), 0)


# Where the PAF path of filter() runs: "gpu" (default, k_paf.hip) or "host" (native threads, gci_paf_filter).
PAF_FILTER = os.environ.get("GCI_PAF", "gpu")

# Every BGZF member's CRC-32 is verified while inflating, as htslib does (a corrupted block that still inflates to the
# right size must not pass silently); GCI_BGZF_CRC=0 skips the check.
BGZF_CRC = os.environ.get("GCI_BGZF_CRC", "1") != "0"

# ingest = "gpu" keeps the whole inflated stream of a file on the device: only files up to this size go that way
GPU_INFLATE_MAX = int(os.environ.get("GCI_GPU_INFLATE_MAX", str(32 << 30)))

# A BAM whose inflated stream exceeds this many bytes is streamed through the GPU chunk by chunk (K1 per chunk,
# compact records + packed names kept, SEQ/QUAL bytes dropped): real 40x whole-genome BAMs inflate to hundreds of GB.
BAM_CHUNK_BYTES = int(os.environ.get("GCI_BAM_CHUNK_BYTES", str(4 << 30)))     # (8 GiB until round 6: the same wall time, 10 GB more device memory)


# What the record filter runs over.  "pages" (default): the records are laid out as RECORD PAGES on the device first
# (gci_bam_pages_*: the ~400 bytes of a record read_sam looks at, 16-byte aligned, no offset table) and filtered there
# (gci_bam_filter_pages) -- the kernel bench.py times; the inflated stream (SEQ / QUAL: 98 % of it) is released as soon as its
# pages exist, the names stay addressable inside the pages.  "stream": gci_bam_filter[_heads] over the stream itself.
K1_MODE = os.environ.get("GCI_K1", "pages")


class StreamVisitor:
    """What a BAM file's ingestion hands its streams to INSTEAD of the record filter, given as `filt`: every ingest mode (`gpu` whole
    and run by run, `heads`, `full`) and GCI_BAM_CHUNK_BYTES end in _filter_stream, which calls the visitor with the inflated (or
    heads) stream of a piece of the file and its record offsets -- no pages, no K1 -- and passes on the empty join input it returns.
    `engine` is the context the piece lives on: in the `gpu` mode the walk engine, not the caller's (its work is ordered against the
    caller's stream when the file is through: _gpu_runs).  rec_idx_base counts the records of the file in front of the piece; a pass
    over a file begins with 0, and a file whose device walk gives up part-way is read again from the start by the next ingest path:
    begin_file() / abort_file() discard what was collected for the file."""

    def begin_file(self) -> None:
        pass

    def abort_file(self) -> None:
        pass

    def visit(self, engine: Engine, d_stream: Buffer, d_off: Buffer, has_seq: bool, ref_sel: Buffer, rec_idx_base: int) -> None:
        raise NotImplementedError

    def __call__(self, engine: Engine, d_stream: Buffer, d_off: Buffer, has_seq: bool, ref_sel: Buffer, rec_idx_base: int) -> JoinInput:
        if rec_idx_base == 0:                             # the file from its first record (again): nothing of an earlier pass counts
            self.abort_file()
            self.begin_file()
        self.visit(engine, d_stream, d_off, has_seq, ref_sel, rec_idx_base)
        return _concat_parts(engine, [])


def _filter_stream(engine: Engine, d_stream: Buffer, d_off: Buffer, has_seq: bool, ref_sel: Buffer, filt,
                   rec_idx_base: int = 0) -> JoinInput:
    """K1 over the records of an inflated BAM stream (has_seq) or a heads stream -> join input (records + where their names are).
    `filt`: the record filter's (map_qual, mq_cutoff, clip_percent, iden_percent) -- or a StreamVisitor, which gets the stream instead."""
    if isinstance(filt, StreamVisitor):
        return filt(engine, d_stream, d_off, has_seq, ref_sel, rec_idx_base)
    map_qual, mq_cutoff, clip_percent, iden_percent = filt
    if K1_MODE == "pages" or not has_seq:                 # (a heads stream is only ever read through its pages)
        with phases.gpu("record pages"):
            pages = engine.bam_pages(d_stream, d_off, has_seq)
        with phases.gpu("record filter (K1)"):
            recs, noff = engine.bam_filter_pages(pages, ref_sel, map_qual, mq_cutoff, clip_percent, iden_percent, rec_idx_base=rec_idx_base)
        ji = JoinInput(recs, pages.buf, noff, 0)
        ji.blob_bytes = int(pages.buf.shape[0]) - pages.blob_off - 16      # CIGARs / oversize records behind the pages (ONT: GBs)
        return ji
    recs = engine.bam_filter(d_stream, d_off, ref_sel, map_qual, mq_cutoff, clip_percent, iden_percent, rec_idx_base=rec_idx_base)
    return JoinInput(recs, d_stream, d_off, 36)


def _keep_part(engine: Engine, ji: JoinInput) -> JoinInput:
    """What is kept of one run of a file that goes through the device run by run: the records and their names -- the pages
    as they are (they ARE the compact form), or, of a whole stream, the names packed (gci_pack_names)."""
    if ji.name_delta == 0 and getattr(ji, "blob_bytes", 0) == 0:
        return JoinInput(ji.recs.clone(), ji.name_base, ji.name_off.clone(), 0)
    # pages with a blob behind them (an ONT run: ~12 KB of CIGAR words per record, tens of GB per file) or a whole stream: only
    # the names are needed from here on -- packed, the rest is released with the run
    names, noff = engine.pack_names(ji)
    recs = ji.recs.clone()
    if ji.name_delta == 0:
        engine.T.rec_flags_and(recs, 3)                   # packed names no longer lie at 16 k + 4: not GCI_REC_NAME16
    return JoinInput(recs, names.clone(), noff[:-1].clone(), 0)


def _concat_parts(engine: Engine, parts: List[JoinInput]) -> JoinInput:
    dev, T = engine.device, engine.T
    if not parts:
        return JoinInput(T.zeros((0, 32), T.uint8, dev), T.zeros(1, T.uint8, dev), T.zeros(1, T.int64, dev), 0)
    if len(parts) == 1:
        return parts[0]
    offs, base = [], 0
    for p in parts:
        offs.append(T.add_i64(p.name_off, base))
        base += (int(p.name_base.shape[0]) + 15) // 16 * 16            # (pages keep their 16-byte phase: GCI_REC_NAME16)
    names = T.zeros(max(base, 1), T.uint8, dev)
    at = 0
    for p in parts:
        names[at:at + int(p.name_base.shape[0])] = p.name_base
        at += (int(p.name_base.shape[0]) + 15) // 16 * 16
    return JoinInput(T.cat([p.recs for p in parts]), names, T.cat(offs), 0)


@contextlib.contextmanager
def _rebased(base: int):
    """A GciError raised inside counts its record (or member) from the beginning of a piece of the file: outside, from `base`."""
    try:
        yield
    except GciError as e:
        if e.rec >= 0:
            e.rec += base
        raise


class _Parts:
    """A file that goes through the device piece by piece (runs of members, chunks of the host's stream, a rank's contigs): K1 over
    every piece on `engine`, records counted from the beginning of the file, and what is kept of each (_keep_part) for the join --
    which reads it on the stream of `join`, where that is another engine."""

    def __init__(self, engine: Engine, ref_sel: Buffer, filt, join: Optional[Engine] = None):
        self.engine, self.ref_sel, self.filt, self.join = engine, ref_sel, filt, join
        self.parts: List[JoinInput] = []
        self.n_done = 0

    def add(self, d_buf: Buffer, d_off: Buffer) -> None:
        with _rebased(self.n_done):
            ji = _filter_stream(self.engine, d_buf, d_off, True, self.ref_sel, self.filt, rec_idx_base=self.n_done)
        kept = _keep_part(self.engine, ji)
        if self.join is not None:
            for t in (kept.recs, kept.name_base, kept.name_off):    # (made in this engine's stream order, joined in the other's)
                t.record_stream(self.join.stream)
        self.parts.append(kept)
        self.n_done += int(d_off.shape[0])

    def result(self) -> JoinInput:
        return _concat_parts(self.join or self.engine, self.parts)


def _runs_of_members(engine: Engine, isz: np.ndarray, chunk_bytes: int, whole_rounds: bool = True) -> List[Tuple[int, int]]:
    """Runs of members of at most chunk_bytes inflated -- and a whole number of the device's decode rounds each: every member takes
    about as long as every other, so 65 536 members (4 GiB) on a device that decodes 28 672 at a time cost three rounds for the
    work of 2.3 (bench.py's ingest of 64.5 GB: 4.1 s; with whole rounds per run: see DESIGN.md section 5).  Greedy, cut by cut
    on the running sum (a loop over the 3.4 M members of a whole-genome file is a quarter of a second of interpreter).
    whole_rounds=False: by the bytes alone, the device not asked (the groups the host threads inflate: _ingest_full)."""
    n = int(isz.shape[0])
    cs = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(isz.astype(np.int64))])
    total = int(cs[-1])
    rnd = engine.inflate_round() if whole_rounds else 0
    per_run = 0
    if rnd > 0:
        per_run = max(1, int(chunk_bytes // max(1, total // max(1, n))) // rnd) * rnd
    groups, a = [], 0
    while a < n:
        i = int(np.searchsorted(cs, cs[a] + chunk_bytes, side="right")) - 1      # the most members that stay within chunk_bytes
        if per_run:
            i = min(i, a + per_run)
        i = min(n, max(i, a + 1))
        groups.append((a, i))
        a = i
    return groups or [(0, 0)]


class _Members:
    """The member table of a BGZF file as far as it is known -- the whole of it, or the table of the BEGINNING of the file with more
    still being made (`rest`: a future of (offsets, ISIZEs, the future behind that or None)) -- and the runs of members the
    ingestion goes through (`group(k)`).  Runs are cut from what is known (all but the last, possibly partial, one while more is
    to come), so that the first run can be on the device before the walk through the 3.4 M member headers of a whole-genome file
    (0.7 s of page faults) is over; asking for a run behind the known ones waits for the next piece."""

    def __init__(self, engine: Engine, chunk_bytes: int, pos: np.ndarray, isz: np.ndarray, rest=None):
        self.engine, self.chunk_bytes = engine, int(chunk_bytes)
        self.pos, self.isz, self._rest = pos, isz, None
        self.lock = threading.Lock()
        self.groups: List[Tuple[int, int]] = []
        self._extend(pos, isz, rest)

    def _extend(self, pos, isz, rest) -> None:
        done = self.groups[-1][1] if self.groups else 0
        if done < int(isz.shape[0]):
            more = [(a + done, b + done) for a, b in _runs_of_members(self.engine, isz[done:], self.chunk_bytes)]
            self.groups += more[:-1] if rest is not None else more
        self.pos, self.isz, self._rest = pos, isz, rest

    def group(self, k: int) -> Optional[Tuple[int, int]]:
        """Run k as (first member, one past its last), None behind the last run; self.pos / self.isz cover it afterwards."""
        # (The wait for the next piece IS under the lock, and the main thread, asking for run k while the uploader of run k + 1 waits
        #  here for a piece, stands behind it -- 0.25 s at the head of a whole-genome file.  Waiting outside the lock, with pieces of 1,
        #  2 and 4 run sizes, was built and measured on the round's last day and gained nothing: 5.08 s against 5.10 for the command
        #  line at genome size -- the first inflate, now beside the walk through the next piece and the assembly's upload, took what the
        #  wait had taken.  DESIGN.md section 8 "The head of the ingestion".)
        with self.lock:
            while k >= len(self.groups) and self._rest is not None:
                self._extend(*self._rest.result())
            return self.groups[k] if k < len(self.groups) else None

    def is_last(self, k: int) -> bool:
        """Run k is known to be the last one (False while more of the table is to come)."""
        with self.lock:
            return self._rest is None and k + 1 >= len(self.groups)

    def run_bytes(self) -> List[int]:
        """File bytes of every run known so far."""
        with self.lock:
            return [int(self.pos[hi]) - int(self.pos[lo]) for lo, hi in self.groups]

    def whole(self) -> Tuple[np.ndarray, np.ndarray]:
        with self.lock:
            while self._rest is not None:
                self._extend(*self._rest.result())
            return self.pos, self.isz

    def lazy(self) -> bool:
        return self._rest is not None


class _RunUploads:
    """Uploads of a large BGZF file run by run of members, one run AHEAD of its consumer: two device buffers taken in turns, the
    bytes staged through pinned memory by host threads (`_Staging`) and copied on a stream of their own from a helper thread, so
    that run k + 1 crosses PCIe while the device inflates, walks and filters run k."""

    def __init__(self, engine: Engine, raw, members: _Members):
        self.engine, self.raw, self.m = engine, raw, members
        self.bufs = [None, None]
        self.copy = engine.copy_stream()
        self.freed = [None, None]                            # main-stream event behind the last kernel that read the buffer
        self.staged = isinstance(raw, np.memmap)               # (a mapped file goes through the ring of pinned slots; an array in memory as it is)
        self.staging = engine.staging() if self.staged else None
        self.last_sent = threading.Event()                   # the last run's bytes are all enqueued: the ring is the next file's
        self.pool = ThreadPoolExecutor(1)
        self.pending = {}
        self._start(0)

    def _buffer(self, k: int, need: int):
        """The device buffer of run k (>= need bytes): one of two, made -- or made larger -- when a run asks for more than is there
        (all the runs known by then are looked at, so that a file is served by two allocations, three when its first run was cut
        from the beginning of the table)."""
        i = k & 1
        if self.bufs[i] is None or int(self.bufs[i].shape[0]) < need:
            want = max([need] + [n + 16 for n in self.m.run_bytes()])
            self.bufs[i] = None
            # from the COPY stream's pool: a block recycled there was last used in that stream's order, so the upload need not wait
            # for whatever the main stream is busy with (the file in front is still being inflated when the next file's first
            # run leaves); the main stream's use of it is told to the allocator instead
            T = self.engine.T
            with T.stream(self.copy):
                self.bufs[i] = T.empty(want, T.uint8, self.engine.device)
            self.bufs[i].record_stream(self.engine.stream)
        return self.bufs[i]

    def _start(self, k: int):
        freed = self.freed[k & 1]

        def run():
            g = self.m.group(k)                              # (a run behind the first may wait here for the rest of the table)
            if g is None:
                self.last_sent.set()
                return None
            lo, hi = g
            p0, p1 = int(self.m.pos[lo]), int(self.m.pos[hi])
            n = p1 - p0
            buf = self._buffer(k, n + 16)
            t_send = phases.now()
            T = self.engine.T
            with T.stream(self.copy), warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)     # a read-only memmap is only read
                if freed is not None:
                    self.copy.wait_event(freed)
                if self.staged:
                    self.staging.send(self.raw, p0, p1, buf, self.copy)
                else:
                    buf[:n].copy_(self.engine._host_src(self.raw[p0:p1]))
                buf[n:n + 16].zero_()
                ev = T.Event()
                ev.record(self.copy)
            phases.trace("upload", k, t_send, phases.now(), n)
            if self.m.is_last(k):
                self.last_sent.set()
            return buf[:n + 16], ev

        self.pending[k] = self.pool.submit(run)

    def take(self, k: int):
        """-> run k's bytes on the device (+ 16 zero bytes), ordered before whatever the main stream does next; None: no run k."""
        got = self.pending.pop(k).result()
        if got is None:
            return None
        d_raw, ev = got
        self.engine.stream.wait_event(ev)
        self._start(k + 1)                                   # into the other buffer: its last reader (run k - 1) is enqueued
        return d_raw

    def release(self, k: int):
        """Everything that reads run k's buffer has been enqueued on the main stream: the run after next may overwrite it."""
        ev = self.engine.T.Event()
        ev.record(self.engine.stream)
        self.freed[k & 1] = ev

    def close(self):
        for f in list(self.pending.values()):
            try:
                f.result()
            except Exception:                             # noqa: BLE001
                pass
        self.pending.clear()
        self.pool.shutdown(wait=True)
        self.last_sent.set()


def _bam_join_input_gpu(engine: Engine, path: str, raw, members: _Members, ref_sel_for, filt, upload=None,
                        uploads: Optional[_RunUploads] = None) -> Optional[JoinInput]:
    """ingest = "gpu".  A file whose inflated stream fits GCI_GPU_INFLATE_MAX stays on the device whole (the join reads
    the names inside it); a larger one goes through run by run of members (at most chunk_bytes inflated each): inflate,
    record walk, K1, and only the 32-byte records and the packed names are kept -- the partial record a run ends in is
    put in front of the next one.  None: the parallel record walk lost the chain (the caller takes the host path)."""
    hdr = bamfmt.read_header(path)
    ref_sel = ref_sel_for(hdr)
    if not members.lazy() and int(members.isz.sum()) <= GPU_INFLATE_MAX:
        if uploads is not None:
            uploads.close()
        return _gpu_whole(engine, hdr, raw, members, ref_sel, filt, upload)
    if upload is not None:                                  # larger than it looked: uploaded run by run instead
        upload.future.result()
    return _gpu_runs(engine, hdr, raw, members, ref_sel, filt, uploads)


def _gpu_whole(engine: Engine, hdr, raw, members: _Members, ref_sel: Buffer, filt, upload) -> Optional[JoinInput]:
    """The file inflated into one buffer (from the upload that is under way, if one is), walked and filtered there."""
    pos, isz = members.pos, members.isz
    total = int(isz.sum())
    with phases.gpu("bgzf_inflate + crc"):
        if upload is not None:
            d_bam = engine.bgzf_inflate_uploaded(upload, pos, isz, check_crc=BGZF_CRC)
        else:
            d_bam = engine.bgzf_inflate(raw, pos, isz, check_crc=BGZF_CRC)
    with phases.gpu("record walk"):
        d_off, used, ok = engine.bam_record_offsets(d_bam, hdr.first_record, len(hdr.references))
    if not ok:
        return None
    if used != total:
        raise bamfmt.BAMError("truncated BAM: %d trailing bytes do not form a record" % (total - used))
    return _filter_stream(engine, d_bam, d_off, True, ref_sel, filt)


def _with_carry(engine: Engine, buf: Buffer, carry: Optional[Buffer]) -> Buffer:
    """A run's bytes, inflated INGEST_HEADROOM into `buf`, with the partial record the run before ended in in front of them: in
    the headroom -- or, a record of more than the headroom, put together in a buffer of its own."""
    T = engine.T
    n_carry = int(carry.shape[0]) if carry is not None else 0
    if n_carry > INGEST_HEADROOM:
        whole = T.empty(n_carry + int(buf.shape[0]) - INGEST_HEADROOM, T.uint8, engine.device)
        whole[:n_carry].copy_(carry)
        whole[n_carry:].copy_(buf[INGEST_HEADROOM:])
        return whole
    if n_carry:
        buf[INGEST_HEADROOM - n_carry:INGEST_HEADROOM].copy_(carry)
    return buf[INGEST_HEADROOM - n_carry:]


def _gpu_runs(engine: Engine, hdr, raw, members: _Members, ref_sel: Buffer, filt, uploads: Optional[_RunUploads]) -> Optional[JoinInput]:
    """The file run by run.  The bytes of run k + 1 travel while run k is inflated and filtered (the first run may be on its way
    already: prefetch_member_tables); and (round 6) run k + 1 is INFLATED while run k is walked, paged and filtered: the inflate stays on
    this engine's stream, everything behind it runs on a second context with a stream of its own (Engine.walk_engine), two output buffers
    in turns.  The partial record run k ends in is known only when run k has been walked -- by then run k + 1 is being inflated --, so
    every run is inflated INGEST_HEADROOM bytes into its buffer and the carried bytes are put in front of it afterwards (_with_carry)."""
    ahead = uploads if uploads is not None else _RunUploads(engine, raw, members)
    T = engine.T
    walk = engine.walk_engine()
    parts = _Parts(walk, ref_sel, filt, join=engine)
    n_ref = len(hdr.references)
    carry, start = None, hdr.first_record

    def launch(k: int):
        """Run k's inflate on the engine's stream, as soon as its bytes are on the device; None behind the last run."""
        t_take = phases.now()
        with phases.wall("  wait for the upload of a run (host blocked)"):
            d_raw = ahead.take(k)
        if d_raw is None:
            return None
        t_got = phases.now()
        lo, hi = members.group(k)
        pos, isz = members.pos, members.isz
        p0 = int(pos[lo])
        with phases.gpu("bgzf_inflate + crc"):
            buf, status, _ = engine.bgzf_inflate_ahead(d_raw, pos[lo:hi + 1] - np.uint64(p0), isz[lo:hi], INGEST_HEADROOM, check_crc=BGZF_CRC)
        ahead.release(k)
        ev = T.Event()
        ev.record(engine.stream)
        buf.record_stream(walk.stream)                       # (read over there: not handed out again before that is through)
        status.record_stream(walk.stream)
        phases.trace("run", k, t_take, t_got, phases.now())
        return dict(buf=buf, status=status, lo=lo, ev=ev)

    try:
        k = 0
        cur = launch(0)
        while cur is not None:
            nxt = launch(k + 1)                              # enqueued BEFORE run k is walked: the two overlap on the device
            with T.stream(walk.stream):
                walk.stream.wait_event(cur["ev"])
                with _rebased(cur["lo"]):
                    walk.check_status_word(cur["status"], "gci_bgzf_inflate_device")
                d_buf = _with_carry(engine, cur["buf"], carry)
                cur = None
                if int(d_buf.shape[0]) <= start:              # still inside the header
                    carry, start = None, start - int(d_buf.shape[0])
                else:
                    with phases.gpu("record walk"):
                        d_off, used, ok = walk.bam_record_offsets(d_buf, start, n_ref)
                    if not ok:
                        return None
                    carry, start = (d_buf[used:].clone() if used < int(d_buf.shape[0]) else None), 0
                    if int(d_off.shape[0]):
                        parts.add(d_buf, d_off)
                    del d_off
                del d_buf
            phases.trace("run_done", k, phases.now())
            cur, nxt = nxt, None
            k += 1
    finally:
        ahead.close()
        engine.stream.wait_stream(walk.stream)               # (what the join reads was written over there)
    if carry is not None:
        raise bamfmt.BAMError("truncated BAM: %d trailing bytes do not form a record" % int(carry.shape[0]))
    return parts.result()


# A large file's runs: the bytes kept free in front of every run's inflated bytes for the record the run before it ended in (a longer
# one -- an ONT read of megabases -- is put together in a buffer of its own).
INGEST_HEADROOM = 8 << 20


_DROP_QUEUE = None


def _drop_later(*objs) -> None:
    """Give the last reference of `objs` to a helper thread.  Unmapping a 1.5 GB file mapping whose pages were all touched takes
    14 - 18 ms on the GPU boxes (tools/exp_cli_teardown.py) -- a tenth of the command line's time at chr19, spent by the thread that
    should be launching kernels."""
    global _DROP_QUEUE
    if _DROP_QUEUE is None:
        _DROP_QUEUE = queue.SimpleQueue()

        def run(q):
            while True:
                q.get()                      # (taken and dropped: the last reference dies here)

        threading.Thread(target=run, args=(_DROP_QUEUE,), daemon=True).start()
    _DROP_QUEUE.put(objs)


_TABLES: Dict[str, object] = {}        # path -> (memory map of the file, future of (member offsets, ISIZEs, first-run uploader or
                                       # None)): prefetch_member_tables


def prefetch_member_tables(paths: Sequence[str]) -> None:
    """Start on the BAM files of a run before anything needs them, on a helper thread, file after file: the BGZF member table
    (host threads over the mapping of the file) and, for a file that will go through the device run by run, the upload
    of its FIRST run.  The first file's table is made in pieces (_Members): its first run leaves as soon as the table of the
    file's beginning is there; a later file's as soon as the file in front of it has put its last run on the copy stream.  The
    command line calls this as soon as it knows its inputs, so what used to sit in front of a file's first byte on the device --
    0.7 s of table and a third of a second of upload per file at genome size -- happens beside the assembly's N scan and beside
    the inflate of the file in front.  bam_join_input() picks the results up; an unreadable or damaged file raises there (a
    damaged member behind the table's first piece: where the run that holds it is asked for)."""
    if _ingest_mode() != "gpu" or not paths or _sharded():
        return                                            # (a contig-sharded run reads only its contigs' members, through the index)
    todo = []
    for path in paths:
        if path in _TABLES:
            continue
        try:
            if not os.path.getsize(path):
                continue
            raw = np.memmap(path, dtype=np.uint8, mode="r")
        except OSError:
            continue                                      # (bam_join_input meets the same error itself)
        fut = Future()
        _TABLES[path] = (raw, fut)
        todo.append((path, raw, fut))
    # (the first file's table is wanted as soon as the assembly has been scanned; the later ones have the seconds the file before
    # them takes on the device, and their threads would compete with the ones that stage that file's bytes: a quarter as many)
    many = hostio.default_threads()
    # The tables of the files BEHIND the first are walked beside the first one's (a thread each), not one after the other: with the
    # uploads at 40 - 57 GB/s a 77 GB file is through the device in under two seconds, and the table of the file behind it -- 1.2 s of page
    # faults over 3.4 M member headers, started only when the first file's own 1.2 s were over -- was not there yet (round 6, one run
    # of the command line at genome size: 1.3 s of waiting for it, 5.7 s instead of 4.4).
    later_pool = ThreadPoolExecutor(max(1, min(4, len(todo) - 1))) if len(todo) > 1 else None
    later = {k: later_pool.submit(_table_ahead, path, raw, max(2, many // 4)) for k, (path, raw, _) in enumerate(todo) if k > 0} if later_pool else {}
    first_run = os.environ.get("GCI_FIRST_RUN_AHEAD", "1") != "0"
    th = threading.Thread(target=_chain_ahead, args=(todo, later, later_pool, many, first_run), daemon=True)
    _CHAINS.append(th)
    th.start()


def _table_ahead(path, raw, threads, limit=None, known=None):
    """The member table up to byte `limit` (None: all of the file); known = the table of a beginning of the file: only what lies
    behind it is walked."""
    with phases.wall("bgzf_member_table (ahead, on a helper thread)"):
        begin = int(known[0][-1]) if known is not None else 0
        if begin >= int(raw.shape[0]):
            return known
        pos, isz = hostio.bgzf_blocks(np.asarray(raw[begin:]), threads=threads, limit=None if limit is None else limit - begin)
        if known is None:
            return pos, isz
        return np.concatenate([known[0][:-1], pos + np.uint64(begin)]), np.concatenate([known[1], isz])


def _first_file_in_pieces(path, raw, fut, threads) -> _RunUploads:
    """A first file with more bytes than a whole-file ingestion may inflate to -- run by run for certain: the table of its beginning,
    the first run on its way (`fut` is told), only then the rest of the table, piece by piece (a failure: raised by the run that needs it)."""
    engine = default_engine()
    n_raw = int(raw.shape[0])
    # (5/8 of a run's inflated size in file bytes holds a whole first run at the usual 2.4 - 4 : 1; four times a
    # run's size holds eight more: a second of inflate, which covers the walk through the rest)
    limits = [x for x in (BAM_CHUNK_BYTES * 5 // 8, BAM_CHUNK_BYTES * 4) if x < n_raw]
    rests = [Future() for _ in limits]
    first = _table_ahead(path, raw, threads, limit=limits[0]) if limits else _table_ahead(path, raw, threads)
    members = _Members(engine, BAM_CHUNK_BYTES, first[0], first[1], rests[0] if rests else None)
    uploads = _RunUploads(engine, raw, members)
    fut.set_result((members, uploads))
    nxt = first
    for j, rest in enumerate(rests):
        try:
            nxt = _table_ahead(path, raw, threads, limit=limits[j + 1] if j + 1 < len(limits) else None, known=nxt)
            rest.set_result((nxt[0], nxt[1], rests[j + 1] if j + 1 < len(rests) else None))
        except BaseException as e:        # noqa: BLE001
            for r in rests[j:]:
                r.set_exception(e)
            break
    return uploads


def _chain_ahead(todo, later, later_pool, many, first_run) -> None:
    """The helper thread of prefetch_member_tables: file after file, every outcome handed to the file's future."""
    before = None                                         # the uploader of the file in front
    try:
        for k, (path, raw, fut) in enumerate(todo):
            if _QUIESCE.is_set():                         # (the run is over: nobody will ask for this file's table)
                if not fut.done():
                    fut.set_exception(RuntimeError("the run ended before %s was reached" % path))
                continue
            try:
                threads = max(2, many // 2) if k == 0 else max(2, many // 4)
                n_raw = int(raw.shape[0])
                if k == 0 and first_run and n_raw > GPU_INFLATE_MAX + (GPU_INFLATE_MAX >> 6):
                    before = _first_file_in_pieces(path, raw, fut, threads)
                    continue
                pos, isz = later.pop(k).result() if k in later else _table_ahead(path, raw, threads)
                if first_run and n_raw > GPU_INFLATE_MAX // 8 and int(isz.sum()) > GPU_INFLATE_MAX:
                    engine = default_engine()
                    members = _Members(engine, BAM_CHUNK_BYTES, pos, isz)
                    if before is not None:
                        while not before.last_sent.wait(0.05):            # (the ring of pinned buffers is the file's in front until then)
                            if _QUIESCE.is_set():
                                break
                    before = _RunUploads(engine, raw, members)
                    fut.set_result((members, before))
                else:
                    fut.set_result(((pos, isz), None))
            except BaseException as e:                    # noqa: BLE001  (handed to the thread that asks for the table)
                if not fut.done():
                    fut.set_exception(e)
    finally:
        if later_pool is not None:
            later_pool.shutdown(wait=True)


_CHAINS: List[threading.Thread] = []    # the helper threads of prefetch_member_tables (quiesce_ahead joins them)
_QUIESCE = threading.Event()             # set: a chain stops in front of its next file
_INGEST_AHEAD: Dict[str, tuple] = {}   # path -> (key, future of its JoinInput): start_ingest_ahead
_SIDE_ENGINE = None


def _targets_of(first, chrs_list) -> Dict[str, int]:
    return {r: l for r, l in zip(first.references, first.lengths) if (len(chrs_list) == 0 or r in chrs_list)}


def start_ingest_ahead(bam_files: Sequence[str], chrs_list, filt: Tuple[int, int, float, float], threads: int) -> None:
    """The ingestion of the run's FIRST BAM file -- upload, inflate, record walk, pages, K1: bam_join_input() as filter() will
    call it -- started on a helper thread before the command line turns to the assembly's N runs: at genome size the device
    inflates for four seconds per file and used to idle through the 0.6 s the assembly takes to cross PCIe and be scanned.
    The helper is the ONLY user of the default engine's context until filter() has taken its result (filter() asks for it
    before it touches the context; the N scan meanwhile runs on a context and stream of its own: get_Ns_ref).  Whatever the
    ingestion raises is raised by filter() where bam_join_input() would have raised it."""
    if (os.environ.get("GCI_INGEST_AHEAD", "1") == "0" or _ingest_mode() != "gpu" or _sharded()
            or not bam_files or bam_files[0] in _INGEST_AHEAD):
        return
    path = bam_files[0]
    try:
        targets = list(_targets_of(bamfmt.read_header(path), chrs_list).keys())
    except Exception:                                     # noqa: BLE001  (filter() meets the same error itself)
        return
    fut = Future()
    engine = default_engine()
    key = (id(engine), tuple(targets), tuple(filt), threads)

    def run():
        try:
            fut.set_result(bam_join_input(engine, path, targets, filt, threads))
        except BaseException as e:                        # noqa: BLE001
            fut.set_exception(e)

    _INGEST_AHEAD[path] = (key, fut)
    threading.Thread(target=run, daemon=True).start()


def quiesce_ahead() -> None:
    """Nothing started ahead is left running or waiting: ingestions not taken by a filter() are waited for (their helper threads
    own the default context until they are done), tables and first-run uploads nobody asked for are dropped."""
    for path in list(_INGEST_AHEAD):
        _, fut = _INGEST_AHEAD.pop(path)
        fut.exception()                                   # (waits; the outcome is nobody's any more)
    # the threads that make tables and first uploads ahead: told to stop in front of their next file, their uploaders (a later
    # file's waits for the ring until the one in front has sent its last run) closed, and waited for -- so that the interpreter never
    # finalises under a thread that is inside HIP or torch (an early sys.exit would otherwise race it)
    _QUIESCE.set()
    for path in list(_TABLES):
        _drop_ahead(_TABLES.pop(path))
    for th in list(_CHAINS):
        if th is not threading.current_thread():
            th.join(timeout=30.0)
    del _CHAINS[:]
    _QUIESCE.clear()


def _side_engine() -> Engine:
    """A second context on a stream of its own (sharing the default engine's ring of pinned buffers): what the main thread works
    with while a helper thread owns the default one (start_ingest_ahead)."""
    global _SIDE_ENGINE
    if _SIDE_ENGINE is None:
        main = default_engine()
        _SIDE_ENGINE = Engine(main.device.index, stream=main.T.Stream(main.device))
        _SIDE_ENGINE._staging = main.staging()
    return _SIDE_ENGINE


def _drop_ahead(ahead) -> None:
    """A prefetched table nobody will use: its uploader (if one was started) is closed once it exists."""
    def done(fut):
        try:
            up = fut.result()[1]
            if up is not None:
                up.close()
        except BaseException:                             # noqa: BLE001
            pass
    ahead[1].add_done_callback(done)


class SeqNeeded(ValueError):
    """bam_join_input(need_seq=True) with the `heads` ingest."""


def _ingest_mode() -> str:                                      # (bam_join_input's `ingest`, where the caller does not say)
    return os.environ.get("GCI_BAM_INGEST", "gpu")


def _ref_sel(engine: Engine, hdr, targets: Sequence[str], own: Optional[Sequence[str]] = None) -> Buffer:
    """refID of the file -> index in `targets` (-1: not selected -- or, with `own`, not one of this rank's contigs), on the device."""
    for t in targets:
        if t not in hdr.references:
            raise ValueError(f"invalid contig `{t}`")          # what pysam's fetch() raises
    tindex = {t: i for i, t in enumerate(targets)}
    keep = tindex if own is None else set(own)
    return engine.to_device(np.asarray([tindex[r] if r in keep else -1 for r in hdr.references], dtype=np.int32))


def bam_join_input(engine: Engine, path: str, targets: Sequence[str], filt: Tuple[int, int, float, float],
                   threads: int = 1, chunk_bytes: Optional[int] = None, ingest: Optional[str] = None, need_seq: bool = False) -> JoinInput:
    """K1 over one BAM file -> the file's join input (compact records + where their names are).

    ingest = "gpu" (default; GCI_BAM_INGEST overrides): the file's bytes are uploaded as they are and inflated on the
    device, the record offsets come from the parallel walk (_ingest_gpu); a stream that walk cannot follow takes the next
    path.
    ingest = "heads": the native host pipeline (gci_bam_heads) inflates the file group by group and keeps every record
    without its SEQ / QUAL bytes; only that heads stream (about 400 B of a 27 KB HiFi record) is uploaded and filtered
    through its record pages; names stay addressable inside those (_ingest_heads).
    ingest = "full" (or an explicit chunk_bytes): the whole stream, inflated on the host, goes to the device (_ingest_full).
    need_seq: the visitor reads the records' SEQ bytes, which a heads stream does not hold: "heads" is refused (SeqNeeded), and a
    "gpu" ingest that declines falls to "full"."""
    ingest = ingest or ("full" if chunk_bytes else _ingest_mode())
    if ingest not in ("heads", "full", "gpu"):
        raise ValueError("ingest must be 'heads', 'full' or 'gpu'")
    if need_seq and ingest == "heads":
        raise SeqNeeded("the reads' bases are needed and the `heads` ingest drops them: use GCI_BAM_INGEST=gpu or full")
    chunk_bytes = int(chunk_bytes or BAM_CHUNK_BYTES)
    nthreads = hostio.pick_threads(threads)
    ahead = _TABLES.pop(path, None)
    if ahead is not None and ingest != "gpu":
        _drop_ahead(ahead)
        ahead = None
    raw = ahead[0] if ahead is not None else (np.memmap(path, dtype=np.uint8, mode="r") if os.path.getsize(path) else np.zeros(0, np.uint8))
    ref_sel_for = lambda hdr: _ref_sel(engine, hdr, targets)      # noqa: E731
    ji = None
    if ingest == "gpu":
        ji = _ingest_gpu(engine, path, raw, ahead, chunk_bytes, ref_sel_for, filt)
        if ji is not None:
            _drop_later(raw)                                  # (the unmapping, off this thread)
            return ji
    if ingest != "full" and not need_seq:
        ji = _ingest_heads(engine, raw, nthreads, ref_sel_for, filt)
    return ji if ji is not None else _ingest_full(engine, path, raw, nthreads, chunk_bytes, ref_sel_for, filt)


def _ingest_gpu(engine: Engine, path: str, raw, ahead, chunk_bytes: int, ref_sel_for, filt) -> Optional[JoinInput]:
    """N1 on the device: the file's bytes are uploaded as they are, the BGZF members are inflated there (gci_bgzf_inflate_device, CRC
    verified), the record offsets come from a parallel walk (gci_bam_record_offsets_device) and K1 runs over the inflated stream.  The
    member table is made on the host while the file's bytes are on their way to the device; a file that may not fit -- BGZF deflates BAM
    2.4 - 4 : 1 -- is uploaded run by run instead.  `ahead`: from prefetch_member_tables.  None: the members are empty, or the walk lost the chain."""
    upload = uploads = None
    try:
        if 0 < raw.shape[0] <= GPU_INFLATE_MAX // 8:
            upload = engine.start_upload(raw, parts=2 if raw.shape[0] >= (256 << 20) else 1)
        with phases.wall("bgzf_member_table"):
            if ahead is not None:
                members, uploads = ahead[1].result()
            else:
                members = hostio.bgzf_blocks(np.asarray(raw))
        if isinstance(members, _Members) and (members.engine is not engine or members.chunk_bytes != chunk_bytes):
            if uploads is not None:
                uploads.close()                               # (made for another engine or other runs: not this call's)
            members, uploads = members.whole(), None
        if not isinstance(members, _Members):
            members = _Members(engine, chunk_bytes, members[0], members[1])
        if not members.lazy() and int(members.isz.sum()) == 0:
            return None
        with phases.wall("bam_ingest (upload | inflate + crc | record walk | pages | filter, overlapped)"):
            ji = _bam_join_input_gpu(engine, path, raw, members, ref_sel_for, filt, upload, uploads)
            if phases.on():
                engine.T.synchronize()
        if phases.on():
            isz = members.whole()[1]
            phases.add("bgzf_bytes", int(raw.shape[0]))
            phases.add("bgzf_members", int(isz.shape[0]))
            phases.add("inflated_bytes", int(isz.sum()))
        return ji
    finally:                                                  # every way out, a failure in front of the first run included
        if upload is not None:
            upload.close()
        if uploads is not None:
            uploads.close()                                   # (idempotent)


def _ingest_heads(engine: Engine, raw, nthreads: int, ref_sel_for, filt) -> Optional[JoinInput]:
    """The heads stream of the host pipeline, uploaded and filtered.  None: gci_bam_heads was refused its address space (strict overcommit)."""
    try:
        heads = hostio.bam_heads(np.asarray(raw), threads=nthreads, check_crc=BGZF_CRC)
    except GciError as e:
        if e.status != _lib.GCI_E_NOMEM:
            raise
        return None
    with heads:
        hdr = bamfmt.parse_header(heads.stream)
        d_bam, d_off = engine.to_device(heads.stream), engine.to_device(heads.offsets)
    return _filter_stream(engine, d_bam, d_off, False, ref_sel_for(hdr), filt)


def _ingest_full(engine: Engine, path: str, raw, nthreads: int, chunk_bytes: int, ref_sel_for, filt) -> JoinInput:
    """The stream inflated on the host.  Up to chunk_bytes: one upload.  Larger: groups of BGZF members are inflated into a host buffer
    (the next group on a background thread while the GPU works on the current one), the partial record at the end of a group is
    carried over, K1 runs per chunk and only the 32-byte records and the packed names (gci_pack_names) are kept on the device."""
    pos, isz = hostio.bgzf_blocks(np.asarray(raw))
    if int(isz.sum()) <= chunk_bytes:
        stream = hostio.bgzf_inflate(np.asarray(raw), threads=nthreads, check_crc=BGZF_CRC)
        hdr = bamfmt.parse_header(stream)
        offs, _ = hostio.bam_record_offsets(stream)
        d_bam, d_off = engine.to_device(stream), engine.to_device(offs)
        return _filter_stream(engine, d_bam, d_off, True, ref_sel_for(hdr), filt)
    groups = _runs_of_members(engine, isz, chunk_bytes, whole_rounds=False)

    def inflate(g):
        lo, hi = g
        return hostio.bgzf_inflate(np.asarray(raw[int(pos[lo]):int(pos[hi])]), threads=nthreads, check_crc=BGZF_CRC)

    carry = np.zeros(0, dtype=np.uint8)
    hdr = parts = None
    with ThreadPoolExecutor(1) as ex:
        nxt = ex.submit(inflate, groups[0])
        for k in range(len(groups)):
            data = nxt.result()
            if k + 1 < len(groups):
                nxt = ex.submit(inflate, groups[k + 1])
            buf = np.concatenate([carry, data]) if carry.shape[0] else data
            start = 0
            if hdr is None:
                try:
                    hdr = bamfmt.parse_header(buf)
                except Exception:                              # header longer than one chunk: keep accumulating
                    carry = buf
                    continue
                start, parts = hdr.first_record, _Parts(engine, ref_sel_for(hdr), filt)
            offs, used = hostio.bam_chunk_offsets(buf, start)
            carry = buf[used:].copy()
            if offs.shape[0] == 0:
                continue
            d_buf, d_off = engine.to_device(buf[:used]), engine.to_device(offs)
            parts.add(d_buf, d_off)
            del d_buf, d_off
    if carry.shape[0]:
        raise bamfmt.BAMError("truncated BAM: %d trailing bytes do not form a record" % carry.shape[0])
    if hdr is None:
        raise bamfmt.BAMError("no BAM header in %s" % path)
    return parts.result()


def filter(paf_files=[], bam_files=[], prefix="GCI", map_qual=30, mq_cutoff=50, iden_percent=0.9,  # noqa: A001
           clip_percent=0.1, ovlp_percent=0.9, flank_len=15, directory=".", force=False, log_reads_type="",
           chrs_list=[], threads=1, engine: Optional[Engine] = None, write=True, issue_hint=None):
    """Filter the PAF and BAM file(s), build the per-base depth in HBM and write
    `{prefix}.depth.gz`.  Returns (depths, targets_length) like the reference.

    `issue_hint` = (leftmost, rightmost, flank_len) of the collapse_depth_range() call that will follow:
    its run boundaries are then detected in the same pass that builds the depth (used as long as no gap
    mask modifies the track first)."""
    engine = engine or default_engine()
    if write:
        refuse_overwrite(f"{directory}/{prefix}.depth.gz", force)
    print(f"Filtering {log_reads_type} alignment files ...")
    if _sharded():
        return _filter_sharded(paf_files, bam_files, prefix, map_qual, mq_cutoff, iden_percent, clip_percent, ovlp_percent,
                               flank_len, directory, log_reads_type, chrs_list, threads, engine, write, issue_hint)

    first = bamfmt.read_header(bam_files[0])
    targets_length = _targets_of(first, chrs_list)
    targets = list(targets_length.keys())
    filt = (map_qual, mq_cutoff, clip_percent, iden_percent)
    # The depth track is asked for NOW, while the first file is still being ingested on its helper thread (this thread would only
    # wait for it): a driver allocation costs by the GB on this chip -- the kernel driver clears VRAM it does not know to be clean,
    # 35 - 45 ms per GB (tools/hwtests/reserve_timing.py) -- and the 12.5 GB of a human genome's track, asked for behind the last
    # file's last byte, were half a second of the command line with nothing beside them.
    early_track = None
    total_elems = sum((int(targets_length[t]) + _lib.GCI_TILE - 1) // _lib.GCI_TILE * _lib.GCI_TILE for t in targets)
    if total_elems >= (1 << 26):
        early_track = engine.T.empty(max(total_elems, 1), engine.T.int32, engine.device)
    # the first file may have been started on already (start_ingest_ahead): its helper thread owns this context until it is done
    first_ahead = None
    for path in [p for p in _INGEST_AHEAD if p != bam_files[0]] + ([bam_files[0]] if bam_files[0] in _INGEST_AHEAD else []):
        key, fut = _INGEST_AHEAD.pop(path)
        try:
            res = ("ok", fut.result())
        except BaseException as e:                        # noqa: BLE001  (raised below, where bam_join_input() would have)
            res = ("err", e)
        if path == bam_files[0] and key == (id(engine), tuple(targets), filt, threads):
            first_ahead = res
    engine.set_layout([targets_length[t] for t in targets])

    inputs: List[JoinInput] = []
    high_qual: Set[str] = set()
    if len(paf_files) != 0:
        try:
            if PAF_FILTER == "host":                          # the native host filter (host_io.cpp), kept as a switch
                native = hostio.paf_filter(paf_files, targets, map_qual, mq_cutoff, iden_percent, threads=hostio.pick_threads(threads))
                inputs += [JoinInput(engine.to_device(r), engine.to_device(nm), engine.to_device(off), 0) for r, nm, off in native]
            else:                                             # K2: tokeniser, grouping and scoring on the GPU
                inputs += engine.paf_filter(paf_files, targets, map_qual, mq_cutoff, iden_percent)
                if bam_files and os.environ.get("GCI_PAF_POOL_KEEP_GB") is None:
                    # the PAF stage is over: its pooled scratch (raw device memory, outside torch's allocator) back to the driver before
                    # the BAM ingestion, the join and the depth build ask for theirs (a harness that repeats the stage says KEEP)
                    engine.lib.gci_paf_pool_release(engine.ctx)
        except GciError as e:
            e.paf_replay = (paf_files, targets)               # a bad LINE: Python's own exception for it, as the reference dies
            _reraise_like_reference(e)
    for k, path in enumerate(bam_files):
        try:
            if k == 0 and first_ahead is not None:
                if first_ahead[0] == "err":
                    raise first_ahead[1]
                inputs.append(first_ahead[1])
                first_ahead = None
            else:
                inputs.append(bam_join_input(engine, path, targets, filt, threads))
        except GciError as e:
            _reraise_like_reference(e)
    try:
        with phases.wall("name_join"), phases.gpu("name join"):
            ivl, count = engine.name_join(inputs, ovlp_percent, count_flank=flank_len)     # + the build's counting pass
    except GciError as e:
        _reraise_like_reference(e)
    track = early_track if (early_track is not None and int(early_track.shape[0]) == max(engine.total, 1)) else engine.new_track()
    with phases.wall("depth_build"), phases.gpu("depth build"):
        fused = engine.depth_build_fused(ivl, count, flank_len, track, want_text=False, want_sums=True,
                                         issue=issue_hint, counted=True, want_runs=bool(write))
    depths = _depths_of_build(engine, targets_length, targets, track, fused, issue_hint, log_reads_type, directory, prefix, write, from_build=True)
    return depths, targets_length


def _depths_of_build(engine: Engine, tl: Dict[str, int], all_targets: List[str], track: Buffer, fused: dict, issue_hint, log_reads_type,
                     directory, prefix, write, from_build: bool) -> DepthTracks:
    """The tail of filter(): the track a fused build has just written, with the build's by-products, and its file.  from_build: the
    build kept its run lists for the writer (the single-process filter(), which also puts the write in the phase log)."""
    depths = DepthTracks(engine, tl, track)
    depths.all_targets = all_targets
    depths._fresh_sums = fused["sums"]
    if issue_hint is not None:
        depths._fresh_runs = (tuple(float(x) for x in issue_hint[:2]) + (int(issue_hint[2]),), fused["runs"])
    print(f"Filtering {log_reads_type} alignment files done!!!")
    if write:
        print(f'Writing depths into "{directory}/{prefix}.depth.gz" ...')
        with phases.wall("write_depth_gz (deflate on the device, D2H, file)") if from_build else contextlib.nullcontext():
            _write_depth_members(directory, prefix, depths, from_build=from_build)
        print("Writing depths done!!!\n\n")
    return depths


# ==============================================================================================
# bam_depth.py: the unfiltered per-base depth of BAM files (`samtools depth -a`)
# ==============================================================================================

COVER_EXCL_DEFAULT = 0x704                 # UNMAP, SECONDARY, QCFAIL, DUP: samtools depth's default
COVER_IVL_BUDGET = 1 << 27                 # intervals collected before they are built into the track: 2 GiB of them, a count below 2^31


class CoverOpts:
    """`samtools depth -a`'s record options: excl (flag bits that skip a record; -G adds, -g removes), min_mapq (-Q), count_del (-J)."""

    def __init__(self, excl: int = COVER_EXCL_DEFAULT, min_mapq: int = 0, count_del: bool = False):
        self.excl, self.min_mapq, self.count_del = int(excl), int(min_mapq), bool(count_del)


class SqMismatch(ValueError):
    """A later BAM file whose @SQ table (names, lengths, order) is not the first file's."""


def same_sq_table(bam_files: Sequence[str]):
    """The first file's header; SqMismatch when a later file's @SQ table (names, lengths, order) is another."""
    first = bamfmt.read_header(bam_files[0])
    for path in bam_files[1:]:
        hdr = bamfmt.read_header(path)
        if (tuple(hdr.references), tuple(hdr.lengths)) != (tuple(first.references), tuple(first.lengths)):
            raise SqMismatch(f'The @SQ table of "{path}" differs from that of "{bam_files[0]}"')
    return first


class _IntervalCollector:
    """Intervals of one file on their way into a track: the parts of every piece collect on the device; flush() builds them into a
    scratch track that is added to the file's (gci_track_add); finish() turns what is left into the file's track."""

    def __init__(self):
        self.flushes = 0
        self.reset()

    def reset(self) -> None:
        self.parts: List[Buffer] = []
        self.n_ivl = 0
        self.track: Optional[Buffer] = None

    def add(self, ivl: Buffer) -> None:
        if int(ivl.shape[0]):
            self.parts.append(ivl)
            self.n_ivl += int(ivl.shape[0])

    def _build(self, engine: Engine) -> Optional[Buffer]:
        """The collected intervals as depths in a new track; None when there is nothing to build."""
        parts, self.parts, self.n_ivl = self.parts, [], 0
        if not parts:
            return None
        ivl = parts[0] if len(parts) == 1 else engine.T.cat(parts)
        track = engine.new_track()
        with phases.gpu("depth build"):
            engine.depth_build(ivl, None, 0, track)
        return track

    def flush(self, engine: Engine) -> None:
        built = self._build(engine)
        if built is None:
            return
        self.flushes += 1
        if self.track is None:
            self.track = built
        else:
            engine.track_add(self.track, built)

    def hand_over(self, stream) -> None:
        """What was made in another engine's stream order is used in `stream` from finish() on."""
        for t in self.parts + ([self.track] if self.track is not None else []):
            t.record_stream(stream)

    def finish(self, engine: Engine) -> Buffer:
        """The file's track: a file that needed no flush is built straight into a new one."""
        if self.track is None:
            track = self._build(engine)
            if track is None:                              # no interval at all
                track = engine.new_track()
                track.zero_()
        else:
            self.flush(engine)
            track = self.track
        self.reset()
        return track


def _file_record_error(engine: Engine, e: GciError, what: str, rec_idx_base: int) -> GciError:
    """e.rec counts inside the piece (the ingestion adds what lies in front: _rebased); the text names the record of the FILE."""
    return GciError(e.status, "%s: %s (record %d of the file)" % (what, engine.lib.gci_strerror(e.status).decode(), e.rec + rec_idx_base), rec=e.rec)


class _CoverVisitor(StreamVisitor):
    """The covered bases of one file after another: the intervals of every piece (gci_bam_cover_*) collect on the device; beyond
    `budget` of them they are built into a scratch track that is added to the file's (_IntervalCollector).  All of that runs on the
    engine, and in the stream, of the piece; file_done() -- on the caller's engine, when the ingestion has ordered the two -- turns
    what is left into the file's track."""

    def __init__(self, main: Engine, opts: CoverOpts, budget: int):
        self.main, self.opts, self.budget = main, opts, max(int(budget), 1)
        self.collector = _IntervalCollector()

    flushes = property(lambda self: self.collector.flushes)
    track = property(lambda self: self.collector.track)

    def begin_file(self) -> None:
        self.collector.reset()

    abort_file = begin_file

    def visit(self, engine, d_stream, d_off, has_seq, ref_sel, rec_idx_base) -> None:
        if engine.lengths != self.main.lengths:            # (the walk engine: a context of its own)
            engine.set_layout(self.main.lengths)
        try:
            with phases.gpu("record cover"):
                ivl = engine.bam_cover(d_stream, d_off, has_seq, ref_sel, self.opts.excl, self.opts.min_mapq, self.opts.count_del)
        except GciError as e:
            if e.rec < 0:
                raise
            raise _file_record_error(engine, e, "gci_bam_cover_size", rec_idx_base) from None
        self.collector.add(ivl)
        if self.collector.n_ivl > self.budget:
            self.collector.flush(engine)
        if engine is not self.main:                        # (made in that engine's stream order, used in the caller's from file_done on)
            self.collector.hand_over(self.main.stream)

    def file_done(self) -> Buffer:
        """The file's track (the caller's engine and stream)."""
        return self.collector.finish(self.main)


def bam_raw_depth(engine: Engine, bam_files: Sequence[str], chrs: Sequence[str] = (), opts: Optional[CoverOpts] = None, threads: int = 1,
                  ivl_budget: Optional[int] = None) -> DepthTracks:
    """The per-base read-mapping depth of `bam_files` as `samtools depth -a` counts it (include/gci_hip.h: gci_bam_cover_size), added
    over the files.  Contig names, lengths and order are the first file's header's (restricted by `chrs`); a file with another @SQ
    table raises SqMismatch.  The files go through bam_join_input with a visitor for a filter: every ingest mode serves."""
    opts = opts or CoverOpts()
    first = same_sq_table(bam_files)
    targets_length = _targets_of(first, list(chrs))
    targets = list(targets_length.keys())
    if not targets:
        raise ValueError("no contig selected")
    engine.set_layout([targets_length[t] for t in targets])
    visitor = _CoverVisitor(engine, opts, COVER_IVL_BUDGET if ivl_budget is None else ivl_budget)
    total = None
    for k, path in enumerate(bam_files):
        visitor.begin_file()
        try:
            with phases.wall("bam_cover[%s]" % os.path.basename(path)):
                bam_join_input(engine, path, targets, visitor, threads)
        except BaseException as e:
            visitor.abort_file()
            if isinstance(e, GciError):
                e.path = path                             # (which file the record index counts in: the command line says so)
            raise
        track = visitor.file_done()
        if total is None:
            total = track
        else:
            engine.track_add(total, track)
    depths = DepthTracks(engine, targets_length, total)
    depths.cover_flushes = visitor.flushes
    return depths


# ==============================================================================================
# clip_sites.py: where alignments break off, base by base
# ==============================================================================================

CLIP_MIN_CLIP = 100                        # a choice for long reads, not a measurement
CLIP_MIN_READS = 3
_CLIP_TRACKS = ("left", "right", "depth")


class ClipSites:
    """What bam_clip_sites returns: left / right / depth = the three DepthTracks (per base the records whose alignment begins / ends
    there with a clip beyond it; the read-mapping depth), sites = device.SITE_DTYPE [n] in contig order and then by position, counts[k]
    = [records counted, left events, right events] of file k, flushes = how often intervals were built into a track before their file
    was through."""

    def __init__(self, left: DepthTracks, right: DepthTracks, depth: DepthTracks, sites: np.ndarray, counts: List[List[int]], flushes: int):
        self.left, self.right, self.depth, self.sites, self.counts, self.flushes = left, right, depth, sites, counts, flushes


class _ClipVisitor(StreamVisitor):
    """_CoverVisitor with two more tracks: every piece goes through gci_bam_cover_* (the depth) and gci_bam_clip_* (the left and the
    right events), so a file is read once; three _IntervalCollectors with the flush and hand-over rules of _CoverVisitor."""

    TRACKS = _CLIP_TRACKS                              # the parts of the event call (two halves here), then the depth
    NEED_SEQ = False                                   # the event call reads SEQ: bam_join_input(need_seq=True)
    PHASE, CALL = "record clips", "gci_bam_clip_size"

    def __init__(self, main: Engine, opts: CoverOpts, min_bases: int, budget: int):
        self.main, self.opts, self.min_bases, self.budget = main, opts, int(min_bases), max(int(budget), 1)
        self.collectors = {name: _IntervalCollector() for name in self.TRACKS}
        self.counts = [0, 0, 0]

    flushes = property(lambda self: sum(c.flushes for c in self.collectors.values()))

    def begin_file(self) -> None:
        for c in self.collectors.values():
            c.reset()
        self.counts = [0, 0, 0]

    abort_file = begin_file

    def events(self, engine, d_stream, d_off, has_seq, ref_sel):
        """-> (the parts of the piece, one per track in front of the depth, ..., the three counts)."""
        return engine.bam_clip(d_stream, d_off, has_seq, ref_sel, self.opts.excl, self.opts.min_mapq, self.min_bases)

    def visit(self, engine, d_stream, d_off, has_seq, ref_sel, rec_idx_base) -> None:
        if engine.lengths != self.main.lengths:            # (the walk engine: a context of its own)
            engine.set_layout(self.main.lengths)
        try:
            with phases.gpu("record cover"):
                ivl = engine.bam_cover(d_stream, d_off, has_seq, ref_sel, self.opts.excl, self.opts.min_mapq, self.opts.count_del)
        except GciError as e:
            if e.rec < 0:
                raise
            raise _file_record_error(engine, e, "gci_bam_cover_size", rec_idx_base) from None
        try:
            with phases.gpu(self.PHASE):
                *parts, counts = self.events(engine, d_stream, d_off, has_seq, ref_sel)
        except GciError as e:
            if e.rec < 0:
                raise
            raise _file_record_error(engine, e, self.CALL, rec_idx_base) from None
        self.counts = [a + b for a, b in zip(self.counts, counts)]
        for name, part in zip(self.TRACKS, (*parts, ivl)):
            c = self.collectors[name]
            c.add(part)
            if c.n_ivl > self.budget:
                c.flush(engine)
            if engine is not self.main:                    # (made in that engine's stream order, used in the caller's from file_done on)
                c.hand_over(self.main.stream)

    def file_done(self) -> Dict[str, Buffer]:
        """The file's tracks by name (the caller's engine and stream)."""
        return {name: self.collectors[name].finish(self.main) for name in self.TRACKS}


def _event_tracks(engine: Engine, bam_files: Sequence[str], chrs: Sequence[str], make_visitor, threads: int, wall: str,
                  regions: Optional[Sequence[Tuple[str, int, int]]], tracks: int = 3, bytes_per_base: int = 0):
    """What bam_clip_sites, bam_indel_sites, bam_mismatch_sites and bam_allele_sites share: the layout of the first file's contigs (restricted by `chrs`),
    the TracksDoNotFit check before anything is read, make_visitor(engine) behind that check and in front of the first file, every
    file once through the visitor's collectors (one per track), the files' tracks added up.  `tracks`: how many tracks the visitor
    builds; `bytes_per_base`: what the run keeps per layout element next to them (the code array of bam_mismatch_sites), as the
    check counts it
    -> (targets_length, the summed tracks by name, counts per file, the visitor, the windows of `regions` in flat track elements
    -- None: `regions` holds no window of a selected contig)."""
    first = same_sq_table(bam_files)
    targets_length = _targets_of(first, list(chrs))
    targets = list(targets_length.keys())
    if not targets:
        raise ValueError("no contig selected")
    engine.set_layout([targets_length[t] for t in targets])
    # the visitor's tracks, one more while intervals are built in parts -- and with several files a second set, the file's next to the
    # sum of the files before it.  The FASTA text of reference_codes is not counted: it is on the device next to the code array only
    # while no track exists yet and is about one byte per base, less than the tracks that follow it
    n_tracks = tracks * (2 if len(bam_files) > 1 else 1) + 1
    track_bytes, free = 4 * int(engine.total), device_memory_free(engine)
    if n_tracks * track_bytes + bytes_per_base * int(engine.total) > free:
        raise TracksDoNotFit(n_tracks, track_bytes, free)
    visitor = make_visitor(engine)
    totals: Dict[str, Buffer] = {}
    counts = []
    for path in bam_files:
        visitor.begin_file()
        try:
            with phases.wall("%s[%s]" % (wall, os.path.basename(path))):
                bam_join_input(engine, path, targets, visitor, threads, need_seq=visitor.NEED_SEQ)
        except BaseException as e:
            visitor.abort_file()
            if isinstance(e, GciError):
                e.path = path                             # (which file the record index counts in: the command line says so)
            raise
        counts.append(list(visitor.counts))
        for name, track in visitor.file_done().items():
            if name in totals:
                engine.track_add(totals[name], track)
            else:
                totals[name] = track
    windows: Optional[List[Tuple[int, int]]] = []
    if regions is not None:
        win, win0 = merge_windows(regions, targets_length)
        for c in range(len(targets)):
            o = int(engine.offsets[c])
            windows += [(o + int(a), o + int(b)) for a, b in win[int(win0[c]):int(win0[c + 1])].tolist()]
        if not windows:
            windows = None
    return targets_length, totals, counts, visitor, windows


def bam_clip_sites(engine: Engine, bam_files: Sequence[str], chrs: Sequence[str] = (), cover_opts: Optional[CoverOpts] = None, threads: int = 1,
                   min_clip: int = CLIP_MIN_CLIP, min_reads: int = CLIP_MIN_READS, regions: Optional[Sequence[Tuple[str, int, int]]] = None,
                   ivl_budget: Optional[int] = None) -> ClipSites:
    """Where the alignments of `bam_files` break off (include/gci_hip.h: gci_bam_clip_size, gci_clip_sites_size): per base the counted
    records whose alignment begins (left) or ends (right) there with a clip of at least `min_clip` bases beyond it, the read-mapping
    depth as bam_raw_depth counts it with the same options, and the bases where left or right reaches `min_reads`.  Several files add;
    the contigs are the first file's (restricted by `chrs`), a file with another @SQ table raises SqMismatch.  regions: only the sites
    inside these (contig, start, end) rows are listed (merge_windows' rules); the tracks are whole.
    Raises TracksDoNotFit before anything is read when the tracks of the run are more than the device has free."""
    opts = cover_opts or CoverOpts()
    if int(min_clip) < 1 or int(min_reads) < 1:
        raise ValueError("min_clip and min_reads are at least 1")
    budget = COVER_IVL_BUDGET if ivl_budget is None else ivl_budget
    targets_length, totals, counts, visitor, windows = _event_tracks(engine, bam_files, chrs, lambda e: _ClipVisitor(e, opts, min_clip, budget),
                                                                     threads, "bam_clip", regions)
    with phases.gpu("clip sites"):
        if windows is None:
            sites = np.zeros(0, dtype=SITE_DTYPE)
        else:
            sites = engine.clip_sites(totals["left"], totals["right"], totals["depth"], int(min_reads), windows)
    tracks = {name: DepthTracks(engine, targets_length, totals[name]) for name in _CLIP_TRACKS}
    return ClipSites(tracks["left"], tracks["right"], tracks["depth"], sites, counts, visitor.flushes)


def clip_sites_bed(sites: np.ndarray, targets: Sequence[str]) -> str:
    """`contig\\tpos\\tpos+1\\tleft\\tright\\tdepth\\n` per site, no header line: a BED file bedgraph_cli.parse_regions reads."""
    return "".join("%s\t%d\t%d\t%d\t%d\t%d\n" % (targets[c], p, p + 1, l, r, d)
                   for c, p, l, r, d in zip(sites["contig"].tolist(), sites["pos"].tolist(), sites["left"].tolist(), sites["right"].tolist(),
                                            sites["depth"].tolist()))


def clip_summary_text(bam_files: Sequence[str], counts: Sequence[Sequence[int]], n_sites: int, options: Sequence[Tuple[str, object]]) -> str:
    """The text of {PREFIX}.clip.txt: per file and in total the records counted, the left and the right events; the sites; the options."""
    lines = ["#file\trecords\tleft_events\tright_events\tpath"]
    for k, (path, row) in enumerate(zip(bam_files, counts), 1):
        lines.append("%d\t%d\t%d\t%d\t%s" % (k, row[0], row[1], row[2], path))
    lines.append("total\t%d\t%d\t%d\t." % tuple(sum(int(row[j]) for row in counts) for j in range(3)))
    lines.append("sites\t%d" % n_sites)
    lines += ["%s\t%s" % (name, value) for name, value in options]
    return "\n".join(lines) + "\n"


# ==============================================================================================
# indel_sites.py: long insertions and deletions in reads, base by base
# ==============================================================================================

INDEL_MIN_LEN = 50                         # the conventional floor of a structural variant: a choice, not a measurement
INDEL_MIN_READS = 3
_INDEL_TRACKS = ("del", "ins", "depth")


class IndelSites:
    """What bam_indel_sites returns: dele / ins / depth = the three DepthTracks (per base the counted records that delete it with one
    long D; the long insertions anchored at it; the read-mapping depth), sites = device.INDEL_SITE_DTYPE [n] in contig order and then
    by position, counts[k] = [records counted, deletions, insertions] of file k, flushes = how often intervals were built into a track
    before their file was through."""

    def __init__(self, dele: DepthTracks, ins: DepthTracks, depth: DepthTracks, sites: np.ndarray, counts: List[List[int]], flushes: int):
        self.dele, self.ins, self.depth, self.sites, self.counts, self.flushes = dele, ins, depth, sites, counts, flushes


class _IndelVisitor(_ClipVisitor):
    """_ClipVisitor with gci_bam_indel_* as the event call: the deletions and the insertions of every piece next to its cover."""

    TRACKS = _INDEL_TRACKS
    PHASE, CALL = "record indels", "gci_bam_indel_size"

    def events(self, engine, d_stream, d_off, has_seq, ref_sel):
        return engine.bam_indel(d_stream, d_off, has_seq, ref_sel, self.opts.excl, self.opts.min_mapq, self.min_bases)


def bam_indel_sites(engine: Engine, bam_files: Sequence[str], chrs: Sequence[str] = (), cover_opts: Optional[CoverOpts] = None, threads: int = 1,
                    min_len: int = INDEL_MIN_LEN, min_reads: int = INDEL_MIN_READS, regions: Optional[Sequence[Tuple[str, int, int]]] = None,
                    ivl_budget: Optional[int] = None) -> IndelSites:
    """The long insertions and deletions the reads of `bam_files` carry (include/gci_hip.h: gci_bam_indel_size, gci_indel_sites_size):
    per base the counted records that delete it with one D operation of at least `min_len` bases, the I operations of at least
    `min_len` bases anchored at it (the base in front of the inserted bases), the read-mapping depth as bam_raw_depth counts it with
    the same options -- without count_del it does not count a read over the bases it deletes: the reads that span a deleted base are
    depth + del --, and the runs of bases where del or ins reaches `min_reads`.  Files, contigs, regions and TracksDoNotFit as in
    bam_clip_sites."""
    opts = cover_opts or CoverOpts()
    if int(min_len) < 1 or int(min_reads) < 1:
        raise ValueError("min_len and min_reads are at least 1")
    budget = COVER_IVL_BUDGET if ivl_budget is None else ivl_budget
    targets_length, totals, counts, visitor, windows = _event_tracks(engine, bam_files, chrs, lambda e: _IndelVisitor(e, opts, min_len, budget),
                                                                     threads, "bam_indel", regions)
    with phases.gpu("indel sites"):
        if windows is None:
            sites = np.zeros(0, dtype=INDEL_SITE_DTYPE)
        else:
            sites = engine.indel_sites(totals["del"], totals["ins"], totals["depth"], int(min_reads), windows)
    tracks = {name: DepthTracks(engine, targets_length, totals[name]) for name in _INDEL_TRACKS}
    return IndelSites(tracks["del"], tracks["ins"], tracks["depth"], sites, counts, visitor.flushes)


def indel_sites_bed(sites: np.ndarray, targets: Sequence[str]) -> str:
    """`contig\\tstart\\tend\\tdel\\tins\\tdepth\\n` per site, no header line: a BED file bedgraph_cli.parse_regions reads."""
    return "".join("%s\t%d\t%d\t%d\t%d\t%d\n" % (targets[c], a, b, d, i, x)
                   for c, a, b, d, i, x in zip(*(sites[f].tolist() for f in ("contig", "start", "end", "del", "ins", "depth"))))


def indel_summary_text(bam_files: Sequence[str], counts: Sequence[Sequence[int]], n_sites: int, options: Sequence[Tuple[str, object]]) -> str:
    """The text of {PREFIX}.indel.txt: per file and in total the records counted, the deletions and the insertions; the sites; the
    options."""
    lines = ["#file\trecords\tdeletions\tinsertions\tpath"]
    for k, (path, row) in enumerate(zip(bam_files, counts), 1):
        lines.append("%d\t%d\t%d\t%d\t%s" % (k, row[0], row[1], row[2], path))
    lines.append("total\t%d\t%d\t%d\t." % tuple(sum(int(row[j]) for row in counts) for j in range(3)))
    lines.append("sites\t%d" % n_sites)
    lines += ["%s\t%s" % (name, value) for name, value in options]
    return "\n".join(lines) + "\n"


# ==============================================================================================
# mismatch_sites.py: bases where the reads disagree with the assembly
# ==============================================================================================

MISMATCH_MIN_READS = 3
MISMATCH_MIN_FRAC = "0.5"                  # of the reads over the base: a choice, not a measurement
_MISMATCH_TRACKS = ("mismatch", "depth")


def parse_fraction_ppm(text: str) -> int:
    """A decimal fraction between 0 and 1 with at most six digits behind the point -> parts per million, exactly (no float on the
    way).  ValueError otherwise."""
    import re
    m = re.fullmatch(r"([0-9]+)(?:\.([0-9]{0,6}))?|\.([0-9]{1,6})", text.strip())
    if not m:
        raise ValueError("not a decimal fraction with at most six digits behind the point: `%s`" % text)
    whole, frac = int(m.group(1) or 0), (m.group(2) or m.group(3) or "")
    ppm = whole * 1000000 + int(frac.ljust(6, "0") or 0)
    if ppm > 1000000:
        raise ValueError("a fraction between 0 and 1 is needed: `%s`" % text)
    return ppm


class MismatchSites:
    """What bam_mismatch_sites returns: mismatch / depth = the two DepthTracks (per base the counted records that carry another base
    than the assembly there; the read-mapping depth), sites = device.MISMATCH_SITE_DTYPE [n] in contig order and then by position,
    counts[k] = [records counted, mismatches, pairs compared] of file k, flushes as in ClipSites."""

    def __init__(self, mismatch: DepthTracks, depth: DepthTracks, sites: np.ndarray, counts: List[List[int]], flushes: int):
        self.mismatch, self.depth, self.sites, self.counts, self.flushes = mismatch, depth, sites, counts, flushes


class ReferenceMismatch(ValueError):
    """reference_codes: the FASTA file does not fit the @SQ table."""


def reference_codes(engine: Engine, reference: str, targets_length: Dict[str, int]) -> Buffer:
    """The assembly of `reference` as gci_fasta_codes lays it out for the engine's layout (the contigs of targets_length, in order).  The
    FASTA ids are matched to the contigs by name: ReferenceMismatch (a ValueError) for an id that occurs twice, a contig the FASTA
    does not hold, and a contig whose sequence is not as long as its @SQ LN -- the lengths come from the tile counts and are checked
    before a code is written.  The FASTA text is on the device only inside this call."""
    from .formats import fasta
    buf, spans = fasta.indexed(reference)
    index = {t: k for k, t in enumerate(targets_length)}
    seen, dst = set(), []
    for rid, _, _ in spans:
        if rid in seen:
            raise ReferenceMismatch(f"the id `{rid}` occurs twice in {reference}")
        seen.add(rid)
        dst.append(int(engine.offsets[index[rid]]) if rid in index else -1)
    for t in targets_length:
        if t not in seen:
            raise ReferenceMismatch(f"contig `{t}` is not in {reference}")
    bodies = np.array([(b, e) for _, b, e in spans], dtype=np.int64).reshape(-1, 2)

    def check_lengths(kept: np.ndarray) -> None:           # (between the tile counts and the codes: what gci_fasta_codes leaves to its caller)
        for (rid, _, _), n in zip(spans, fasta.body_lengths(buf, bodies, kept)):
            if rid in index and n != int(targets_length[rid]):
                raise ReferenceMismatch(f"contig `{rid}` has {n} bases in {reference} and LN:{int(targets_length[rid])} in the BAM header")

    with phases.gpu("fasta codes"):
        codes, _ = engine.fasta_codes(buf, bodies, np.asarray(dst, dtype=np.int64), before_codes=check_lengths)
        engine.sync()                                      # (the walk engines read the codes in their own stream order)
    return codes


class _MismatchVisitor(_ClipVisitor):
    """_ClipVisitor with gci_bam_mismatch_* as the event call: one event track next to the cover; the third count is the pairs compared."""

    TRACKS = _MISMATCH_TRACKS
    NEED_SEQ = True
    PHASE, CALL = "record mismatches", "gci_bam_mismatch_size"

    def __init__(self, main: Engine, opts: CoverOpts, codes: Buffer, budget: int):
        super().__init__(main, opts, 1, budget)
        self.codes = codes

    def events(self, engine, d_stream, d_off, has_seq, ref_sel):
        return engine.bam_mismatch(d_stream, d_off, has_seq, ref_sel, self.codes, self.opts.excl, self.opts.min_mapq)


def bam_mismatch_sites(engine: Engine, reference: str, bam_files: Sequence[str], chrs: Sequence[str] = (), cover_opts: Optional[CoverOpts] = None,
                       threads: int = 1, min_reads: int = MISMATCH_MIN_READS, min_frac: str = MISMATCH_MIN_FRAC,
                       regions: Optional[Sequence[Tuple[str, int, int]]] = None, ivl_budget: Optional[int] = None) -> MismatchSites:
    """The bases where the reads of `bam_files` carry another base than the assembly `reference` (include/gci_hip.h: gci_fasta_codes,
    gci_bam_mismatch_size, gci_mismatch_sites_size): per base the counted records whose base there and the assembly's are both one of
    A, C, G, T and differ, the read-mapping depth as bam_raw_depth counts it with the same options, and the runs of bases where the
    mismatches reach `min_reads` and the share `min_frac` of the depth (a decimal text, or parts per million as an int).  Files,
    contigs, regions and TracksDoNotFit as in bam_clip_sites; the assembly is checked against the @SQ table before a record is read
    (reference_codes).  The reads' bases are needed: SeqNeeded with GCI_BAM_INGEST=heads."""
    opts = cover_opts or CoverOpts()
    frac_ppm = int(min_frac) if isinstance(min_frac, (int, np.integer)) else parse_fraction_ppm(str(min_frac))
    if int(min_reads) < 1 or not 0 <= frac_ppm <= 1000000:
        raise ValueError("min_reads is at least 1, min_frac between 0 and 1")
    if _ingest_mode() == "heads":
        raise SeqNeeded("the reads' bases are needed and the `heads` ingest drops them: use GCI_BAM_INGEST=gpu or full")
    budget = COVER_IVL_BUDGET if ivl_budget is None else ivl_budget
    first = same_sq_table(bam_files)

    def make_visitor(e):
        return _MismatchVisitor(e, opts, reference_codes(e, reference, _targets_of(first, list(chrs))), budget)

    targets_length, totals, counts, visitor, windows = _event_tracks(engine, bam_files, chrs, make_visitor, threads, "bam_mismatch", regions,
                                                                     tracks=2, bytes_per_base=1)
    with phases.gpu("mismatch sites"):
        if windows is None:
            sites = np.zeros(0, dtype=MISMATCH_SITE_DTYPE)
        else:
            sites = engine.mismatch_sites(totals["mismatch"], totals["depth"], int(min_reads), frac_ppm, windows)
    tracks = {name: DepthTracks(engine, targets_length, totals[name]) for name in _MISMATCH_TRACKS}
    return MismatchSites(tracks["mismatch"], tracks["depth"], sites, counts, visitor.flushes)


def mismatch_sites_bed(sites: np.ndarray, targets: Sequence[str]) -> str:
    """`contig\\tstart\\tend\\tmismatch\\tdepth\\n` per site, no header line: a BED file bedgraph_cli.parse_regions reads."""
    return "".join("%s\t%d\t%d\t%d\t%d\n" % (targets[c], a, b, m, d)
                   for c, a, b, m, d in zip(*(sites[f].tolist() for f in ("contig", "start", "end", "mismatch", "depth"))))


def mismatch_summary_text(bam_files: Sequence[str], counts: Sequence[Sequence[int]], n_sites: int, options: Sequence[Tuple[str, object]]) -> str:
    """The text of {PREFIX}.mismatch.txt: per file and in total the records counted, the pairs compared, the mismatches and their
    quotient; the sites; the options."""
    def row(head, c, path):
        return "%s\t%d\t%d\t%d\t%s\t%s" % (head, c[0], c[2], c[1], ("%.6f" % (c[1] / c[2])) if c[2] else "nan", path)
    lines = ["#file\trecords\tcompared\tmismatches\trate\tpath"]
    for k, (path, c) in enumerate(zip(bam_files, counts), 1):
        lines.append(row(str(k), [int(x) for x in c], path))
    lines.append(row("total", [sum(int(c[j]) for c in counts) for j in range(3)], "."))
    lines.append("sites\t%d" % n_sites)
    lines += ["%s\t%s" % (name, value) for name, value in options]
    return "\n".join(lines) + "\n"


# ==============================================================================================
# allele_sites.py: which base the reads carry where they disagree with the assembly
# ==============================================================================================

ALLELE_MIN_READS = 3
ALLELE_MIN_FRAC = "0.5"                    # of the reads over the base, for ONE allele: a choice, not a measurement
_ALLELE_TRACKS = ("A", "C", "G", "T", "depth")
_CODE_LETTER = "=ACMGRSVTWYHKDBN"          # BAM's 4-bit codes, as gci_fasta_codes writes them


class AlleleSites:
    """What bam_allele_sites returns: tracks = the five DepthTracks by name ("A", "C", "G", "T": per base the counted records that
    carry that base where the assembly holds another of A, C, G, T; "depth": the read-mapping depth), sites =
    device.ALLELE_SITE_DTYPE [n] in contig order and then by position, counts[k] = [records counted, A, C, G, T events, pairs compared]
    of file k, flushes as in ClipSites."""

    def __init__(self, tracks: Dict[str, DepthTracks], sites: np.ndarray, counts: List[List[int]], flushes: int):
        self.tracks, self.sites, self.counts, self.flushes = tracks, sites, counts, flushes
        self.depth = tracks["depth"]


class _AlleleVisitor(_ClipVisitor):
    """_ClipVisitor with gci_bam_allele_* as the event call: four event tracks next to the cover, six counts."""

    TRACKS = _ALLELE_TRACKS
    NEED_SEQ = True
    PHASE, CALL = "record alleles", "gci_bam_allele_size"

    def __init__(self, main: Engine, opts: CoverOpts, codes: Buffer, budget: int):
        super().__init__(main, opts, 1, budget)
        self.codes = codes
        self.counts = [0] * 6

    def begin_file(self) -> None:
        super().begin_file()
        self.counts = [0] * 6

    abort_file = begin_file

    def events(self, engine, d_stream, d_off, has_seq, ref_sel):
        return engine.bam_allele(d_stream, d_off, has_seq, ref_sel, self.codes, self.opts.excl, self.opts.min_mapq)


def bam_allele_sites(engine: Engine, reference: str, bam_files: Sequence[str], chrs: Sequence[str] = (), cover_opts: Optional[CoverOpts] = None,
                     threads: int = 1, min_reads: int = ALLELE_MIN_READS, min_frac: str = ALLELE_MIN_FRAC,
                     regions: Optional[Sequence[Tuple[str, int, int]]] = None, ivl_budget: Optional[int] = None) -> AlleleSites:
    """Which base the reads of `bam_files` carry where they disagree with the assembly `reference` (include/gci_hip.h: gci_fasta_codes,
    gci_bam_allele_size, gci_allele_sites_size): bam_mismatch_sites' events dealt to four tracks by the read's base, the read-mapping
    depth, and the single bases where ONE allele reaches `min_reads` and the share `min_frac` of the depth (a decimal text, or parts per
    million as an int) -- two alleles at 30 % each are a mismatch site at 0.5 and no site here.  Files, contigs, regions, TracksDoNotFit,
    the check of the assembly and SeqNeeded as in bam_mismatch_sites.  The code array stays on the device until the sites are listed:
    they carry the assembly's base."""
    opts = cover_opts or CoverOpts()
    frac_ppm = int(min_frac) if isinstance(min_frac, (int, np.integer)) else parse_fraction_ppm(str(min_frac))
    if int(min_reads) < 1 or not 0 <= frac_ppm <= 1000000:
        raise ValueError("min_reads is at least 1, min_frac between 0 and 1")
    if _ingest_mode() == "heads":
        raise SeqNeeded("the reads' bases are needed and the `heads` ingest drops them: use GCI_BAM_INGEST=gpu or full")
    budget = COVER_IVL_BUDGET if ivl_budget is None else ivl_budget
    first = same_sq_table(bam_files)

    def make_visitor(e):
        return _AlleleVisitor(e, opts, reference_codes(e, reference, _targets_of(first, list(chrs))), budget)

    targets_length, totals, counts, visitor, windows = _event_tracks(engine, bam_files, chrs, make_visitor, threads, "bam_allele", regions,
                                                                     tracks=5, bytes_per_base=1)
    with phases.gpu("allele sites"):
        if windows is None:
            sites = np.zeros(0, dtype=ALLELE_SITE_DTYPE)
        else:
            sites = engine.allele_sites(*(totals[name] for name in _ALLELE_TRACKS), visitor.codes, int(min_reads), frac_ppm, windows)
    return AlleleSites({name: DepthTracks(engine, targets_length, totals[name]) for name in _ALLELE_TRACKS}, sites, counts, visitor.flushes)


def _site_columns(sites: np.ndarray):
    """-> per site (contig, pos, REF letter, ALT letter, the count of ALT, the four counts, depth)."""
    n = sites["n"].reshape(-1, 4).tolist()
    for c, p, r, a, row, d in zip(sites["contig"].tolist(), sites["pos"].tolist(), sites["ref"].tolist(), sites["alt"].tolist(), n,
                                  sites["depth"].tolist()):
        yield c, p, _CODE_LETTER[r & 15], _CODE_LETTER[a & 15], row[(1, 2, 4, 8).index(a)], row, d


def allele_sites_vcf(sites: np.ndarray, targets_length: Dict[str, int], reference_path: str) -> str:
    """The text of {PREFIX}.allele.sites.vcf: a sites-only VCF 4.2, one line per site with one ALT, in contig order and then by position.
    REF is the assembly's base as the code array holds it (an upper-case IUPAC letter), ALT the listed allele; DP the read-mapping
    depth, AO the records that carry ALT, BC the A, C, G, T counts.  No genotypes, no qualities."""
    targets = list(targets_length)
    lines = ["##fileformat=VCFv4.2", "##source=allele_sites.py", "##reference=%s" % reference_path]
    lines += ["##contig=<ID=%s,length=%d>" % (t, int(targets_length[t])) for t in targets]
    lines += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Read-mapping depth at the base, as bam_depth.py counts it">',
              '##INFO=<ID=AO,Number=1,Type=Integer,Description="Counted records that carry ALT at the base">',
              '##INFO=<ID=BC,Number=4,Type=Integer,Description="Counted records that carry A, C, G, T at the base where the assembly holds another">',
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    lines += ["%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AO=%d;BC=%d,%d,%d,%d" % (targets[c], p + 1, r, a, d, ao, *row)
              for c, p, r, a, ao, row, d in _site_columns(sites)]
    return "\n".join(lines) + "\n"


def allele_sites_bed(sites: np.ndarray, targets: Sequence[str]) -> str:
    """`contig\\tpos\\tpos+1\\tREF\\tALT\\tAO\\tDP\\n` per site, no header line: a BED file bedgraph_cli.parse_regions reads."""
    return "".join("%s\t%d\t%d\t%s\t%s\t%d\t%d\n" % (targets[c], p, p + 1, r, a, ao, d) for c, p, r, a, ao, _, d in _site_columns(sites))


def allele_summary_text(bam_files: Sequence[str], counts: Sequence[Sequence[int]], n_sites: int, options: Sequence[Tuple[str, object]]) -> str:
    """The text of {PREFIX}.allele.txt: per file and in total the records counted, the pairs compared and the events per read base; the
    sites; the options."""
    def row(head, c, path):
        return "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s" % (head, c[0], c[5], c[1], c[2], c[3], c[4], path)
    lines = ["#file\trecords\tcompared\tA\tC\tG\tT\tpath"]
    for k, (path, c) in enumerate(zip(bam_files, counts), 1):
        lines.append(row(str(k), [int(x) for x in c], path))
    lines.append(row("total", [sum(int(c[j]) for c in counts) for j in range(6)], "."))
    lines.append("sites\t%d" % n_sites)
    lines += ["%s\t%s" % (name, value) for name, value in options]
    return "\n".join(lines) + "\n"


# ==============================================================================================
# filter_depth.py: the per-base depth of what the record filter drops, test by test
# ==============================================================================================

FATE_NAMES = _lib.FATE_NAMES
FATE_WANTED = ("secondary", "supplementary", "mapq", "clip", "identity", "kept")      # the classes a run can ask for, in the filter's order


class FateOpts:
    """The record filter's options that decide a record's class (-mq, -cp, -ip) and how coverage is counted (-J)."""

    def __init__(self, map_qual: int = 30, clip_percent: float = 0.1, iden_percent: float = 0.9, count_del: bool = False):
        self.map_qual, self.clip_percent, self.iden_percent, self.count_del = int(map_qual), float(clip_percent), float(iden_percent), bool(count_del)


class TracksDoNotFit(MemoryError):
    """The depth tracks a run of bam_filter_depth needs are more than the device has free."""

    def __init__(self, n_tracks: int, track_bytes: int, free_bytes: int):
        self.n_tracks, self.track_bytes, self.free_bytes = n_tracks, track_bytes, free_bytes
        super().__init__("%d depth tracks of %d bytes each do not fit into the %d bytes the device has free" % (n_tracks, track_bytes, free_bytes))


def device_memory_free(engine: Engine) -> int:
    """What the process can still take on the engine's device: what the driver has free, and what the arena holds but has not handed out."""
    dev = engine.device.index or 0
    free, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
    r, u, n = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    engine._chk(engine.lib.gci_dev_mem_info(dev, ctypes.byref(free), ctypes.byref(total)), "gci_dev_mem_info")
    engine.lib.gci_dev_arena_info(dev, ctypes.byref(r), ctypes.byref(u), ctypes.byref(n))
    return int(free.value) + max(int(r.value) - int(u.value), 0)


class FilterDepth:
    """What bam_filter_depth returns: tracks[class name] = the DepthTracks of every wanted class, counts[k][class id] = the records of
    file k per class (FATE_NAMES), flushes = how often intervals were built into a track before their file was through.  With `join`:
    counts holds the covered file alone, its row running on through the join's classes (ALL_FATE_NAMES), join_files names every file
    of the join in its order (PAF files, then BAM files), join_counts[k] is gci_name_join_fate's row of file k and cover_file the
    covered file's index among them."""

    def __init__(self, tracks: Dict[str, DepthTracks], counts: List[List[int]], flushes: int):
        self.tracks, self.counts, self.flushes = tracks, counts, flushes
        self.join_files: List[str] = []
        self.join_counts: List[List[int]] = []
        self.cover_file = -1


JOIN_FATE_NAMES = _lib.JOIN_FATE_NAMES
ALL_FATE_NAMES = _lib.ALL_FATE_NAMES
_JOIN_FATE_IDS = tuple(range(_lib.JOIN_FATE_FIRST, _lib.JOIN_FATE_FIRST + len(JOIN_FATE_NAMES)))
_JOIN_FATE_MASK = sum(1 << c for c in _JOIN_FATE_IDS)
_KEPT = FATE_NAMES.index("kept")


class JoinFateOpts:
    """bam_filter_depth's `join`: the files are one read set aligned several times (GCI.py's --hifi list), joined by read name as
    filter() joins them -- paf_files in front of the BAM files, mq_cutoff and ovlp_percent as GCI.py's -- and `cover` is the index,
    among the BAM files, of the one whose records give the depth."""

    def __init__(self, paf_files: Sequence[str] = (), mq_cutoff: int = 50, ovlp_percent: float = 0.9, cover: int = 0):
        self.paf_files, self.mq_cutoff, self.ovlp_percent, self.cover = list(paf_files), int(mq_cutoff), float(ovlp_percent), int(cover)


class _FateVisitor(StreamVisitor):
    """Next to _CoverVisitor: per piece ONE gci_bam_fate call (every CIGAR read once for the verdicts), then for every wanted class
    gci_bam_cover_size_sel / _write with that class's mask into that class's collector -- a record that is not selected makes no
    chunk, so the walks of all classes together read every CIGAR once more.  The interval budget is shared: beyond it every collector
    that holds intervals builds them into its track.  join_fate: the file's bytes of gci_name_join_fate, made on the caller's engine;
    every `kept` record of a piece then takes its join class (gci_fate_refine over the piece's slice) before the classes are walked,
    and `kept`, where it is asked for, is the five of them together."""

    def __init__(self, main: Engine, opts: FateOpts, classes: Sequence[int], budget: int, join_fate: Optional[Buffer] = None):
        self.main, self.opts, self.classes, self.budget = main, opts, list(classes), max(int(budget), 1)
        self.collectors = {c: _IntervalCollector() for c in self.classes}
        self.join_fate = join_fate
        self.counts = [0] * _lib.FATE_CLASSES
        self.n_seen = 0

    flushes = property(lambda self: sum(c.flushes for c in self.collectors.values()))

    def begin_file(self) -> None:
        for c in self.collectors.values():
            c.reset()
        self.counts = [0] * _lib.FATE_CLASSES
        self.n_seen = 0

    abort_file = begin_file

    def _refine(self, engine, cls, n: int, rec_idx_base: int):
        """The piece's slice of the join's bytes into its class bytes."""
        total = int(self.join_fate.shape[0])
        if rec_idx_base + n > total:
            raise GciError(_lib.GCI_E_INVALID, "the second pass meets record %d of a file the join saw %d records of" % (rec_idx_base + n - 1, total))
        if engine is not self.main:                        # (made in the caller's stream order -- the export synchronised --, used in this one's)
            self.join_fate.record_stream(engine.stream)
        engine.fate_refine(cls, self.join_fate[rec_idx_base:rec_idx_base + n])

    def visit(self, engine, d_stream, d_off, has_seq, ref_sel, rec_idx_base) -> None:
        if engine.lengths != self.main.lengths:            # (the walk engine: a context of its own)
            engine.set_layout(self.main.lengths)
        o = self.opts
        what = "gci_bam_fate"
        try:
            with phases.gpu("record fate"):
                cls, counts = engine.bam_fate(d_stream, d_off, has_seq, ref_sel, o.map_qual, o.clip_percent, o.iden_percent)
                if self.join_fate is not None:
                    what = "gci_fate_refine"
                    self._refine(engine, cls, int(d_off.shape[0]), rec_idx_base)
            what = "gci_bam_cover_size_sel"
            for c in self.classes:
                joined = self.join_fate is not None and (c == _KEPT or c in _JOIN_FATE_IDS)
                if counts[_KEPT if joined else c]:         # (`none` is never asked for: 0x4 stays among the excluded flags)
                    mask = _JOIN_FATE_MASK if (joined and c == _KEPT) else 1 << c
                    with phases.gpu("record cover"):
                        self.collectors[c].add(engine.bam_cover(d_stream, d_off, has_seq, ref_sel, 0x4, 0, o.count_del, classes=cls, mask=mask))
        except GciError as e:
            if e.rec < 0:
                raise
            raise _file_record_error(engine, e, what, rec_idx_base) from None
        self.n_seen += int(d_off.shape[0])
        self.counts = [a + b for a, b in zip(self.counts, counts)]
        if sum(c.n_ivl for c in self.collectors.values()) > self.budget:
            for c in self.collectors.values():
                c.flush(engine)
        if engine is not self.main:                        # (made in that engine's stream order, used in the caller's from file_done on)
            for c in self.collectors.values():
                c.hand_over(self.main.stream)

    def file_done(self) -> Dict[int, Buffer]:
        """The file's track of every wanted class (the caller's engine and stream)."""
        return {c: col.finish(self.main) for c, col in self.collectors.items()}


def _zero_qlen_file(inputs: Sequence[JoinInput], rec: int) -> int:
    """Which file of the join holds the passing record `rec` (its rec_idx) with a zero query length: the first one behind file 0."""
    for f in range(1, len(inputs)):
        r = np.ascontiguousarray(inputs[f].recs.cpu().numpy()).view(REC_DTYPE).reshape(-1)
        if (((r["flags"] & REC_PASS) != 0) & (r["rec_idx"] == rec) & (r["qlen"] == 0)).any():
            return f
    return -1


def _join_fates(engine: Engine, bam_files: Sequence[str], targets: List[str], opts: FateOpts, join: JoinFateOpts, threads: int):
    """The first pass of bam_filter_depth(join=...): every PAF through the PAF filter, every BAM through the record filter, one
    gci_name_join_fate over them in the reference's order -> (the covered file's bytes, the records the join saw of it, every file's
    row of counts).  The records and names of all files are released on the way out."""
    filt = (opts.map_qual, join.mq_cutoff, opts.clip_percent, opts.iden_percent)
    inputs: List[JoinInput] = []
    if join.paf_files:
        with phases.wall("paf_filter"):
            inputs += engine.paf_filter(join.paf_files, targets, opts.map_qual, join.mq_cutoff, opts.iden_percent)
        if os.environ.get("GCI_PAF_POOL_KEEP_GB") is None:
            engine.lib.gci_paf_pool_release(engine.ctx)
    for path in bam_files:
        try:
            with phases.wall("bam_join_input[%s]" % os.path.basename(path)):
                inputs.append(bam_join_input(engine, path, targets, filt, threads))
        except GciError as e:
            e.path = path
            raise
    names = list(join.paf_files) + list(bam_files)
    try:
        with phases.wall("name_join_fate"), phases.gpu("name join fate"):
            fates, counts = engine.name_join_fate(inputs, join.ovlp_percent)
    except GciError as e:
        if e.status == _lib.GCI_E_ZERO_DIV and e.rec >= 0:
            f = _zero_qlen_file(inputs, e.rec)
            e.path, e.in_join = (names[f] if f >= 0 else "?"), True
        raise
    k = len(join.paf_files) + join.cover
    return fates[k], int(inputs[k].recs.shape[0]), counts


def _join_row(bam_files: Sequence[str], join: JoinFateOpts, join_counts, join_n_rec: int, n_seen: int, n_kept: int) -> List[int]:
    """The covered file's records per join class, once both passes saw the same records of it and agree on which of them pass
    (gci_fate_refine checked each one)."""
    row = join_counts[len(join.paf_files) + join.cover][_lib.JOIN_FATE_FIRST:_lib.JOIN_FATE_FIRST + len(JOIN_FATE_NAMES)]
    if n_seen != join_n_rec or sum(row) != n_kept:
        raise GciError(_lib.GCI_E_INVALID, 'the two passes over "%s" disagree: %d records and %d kept in the join, %d and %d in the walk'
                       % (bam_files[join.cover], join_n_rec, sum(row), n_seen, n_kept))
    return row


def bam_filter_depth(engine: Engine, bam_files: Sequence[str], chrs: Sequence[str], opts: Optional[FateOpts], threads: int,
                     classes: Sequence[str], ivl_budget: Optional[int] = None, join: Optional[JoinFateOpts] = None) -> FilterDepth:
    """Per wanted class of the record filter (FATE_WANTED: the first test of read_sam a record fails, or `kept`) the per-base depth of
    that class's records over `bam_files`, counted as bam_raw_depth counts it (CIGAR-aware, no flank; opts.count_del for deletions), so
    that the six tracks add up, base for base, to bam_raw_depth with excl = 0x4.  Several files add per class; the contigs are the
    first file's (restricted by `chrs`), a file with another @SQ table raises SqMismatch.  A record the reference would have raised on
    (no NM tag, a zero denominator) or a malformed one raises GciError with .path and the record's index in the file.
    Raises TracksDoNotFit before anything is read when the tracks of the run are more than the device has free.

    join (JoinFateOpts): the files are ONE read set aligned several times and are joined, not added.  A first pass filters every file
    and asks gci_name_join_fate what the cross-file join does with every record; the second pass walks the BAM file join.cover alone,
    as above, with every `kept` record moved to its join class -- shadowed, unpaired, contig, overlap, joined (JOIN_FATE_NAMES), which
    `classes` may then name; `kept` stays their sum.  The covered file is read twice.  A zero query length the join divides by raises
    GciError with .path, .rec and .in_join."""
    opts = opts or FateOpts()
    wanted = FATE_WANTED + (JOIN_FATE_NAMES if join is not None else ())
    ids = []
    for name in classes:
        if name not in wanted:
            raise ValueError('"%s" is not one of %s' % (name, ", ".join(wanted)))
        if ALL_FATE_NAMES.index(name) not in ids:
            ids.append(ALL_FATE_NAMES.index(name))
    if not ids:
        raise ValueError("no class selected")
    if join is not None and not 0 <= join.cover < len(bam_files):
        raise ValueError("cover = %d: there are %d BAM files" % (join.cover, len(bam_files)))
    first = same_sq_table(bam_files)
    targets_length = _targets_of(first, list(chrs))
    targets = list(targets_length.keys())
    if not targets:
        raise ValueError("no contig selected")
    engine.set_layout([targets_length[t] for t in targets])
    # a track per class, one more while intervals are built in parts -- and with several files a second one per class, the file's next
    # to the sum of the files before it
    n_tracks = len(ids) * (2 if (len(bam_files) > 1 and join is None) else 1) + 1      # (with join one file alone is covered)
    track_bytes, free = 4 * int(engine.total), device_memory_free(engine)
    if n_tracks * track_bytes > free:
        raise TracksDoNotFit(n_tracks, track_bytes, free)
    join_fate, join_n_rec, join_counts = _join_fates(engine, bam_files, targets, opts, join, threads) if join is not None else (None, 0, [])
    visitor = _FateVisitor(engine, opts, ids, COVER_IVL_BUDGET if ivl_budget is None else ivl_budget, join_fate)
    totals: Dict[int, Buffer] = {}
    counts = []
    for path in (bam_files if join is None else [bam_files[join.cover]]):
        visitor.begin_file()
        try:
            with phases.wall("bam_fate[%s]" % os.path.basename(path)):
                bam_join_input(engine, path, targets, visitor, threads)
        except BaseException as e:
            visitor.abort_file()
            if isinstance(e, GciError):
                e.path = path                             # (which file the record index counts in: the command line says so)
            raise
        counts.append(list(visitor.counts))
        for c, track in visitor.file_done().items():
            if c in totals:
                engine.track_add(totals[c], track)
            else:
                totals[c] = track
    result = FilterDepth({ALL_FATE_NAMES[c]: DepthTracks(engine, targets_length, totals[c]) for c in ids}, counts, visitor.flushes)
    if join is not None:
        counts[0] = counts[0] + _join_row(bam_files, join, join_counts, join_n_rec, visitor.n_seen, counts[0][_KEPT])
        result.join_files, result.join_counts, result.cover_file = list(join.paf_files) + list(bam_files), join_counts, len(join.paf_files) + join.cover
    return result


# ==============================================================================================
# filter_reads.py: the reads over a set of regions, one row each, and what the record filter does with them
# ==============================================================================================

READS_COLUMNS = ("file", "name", "contig", "start", "end", "strand", "flag", "mapq", "M", "I", "D", "S", "NM", "clip", "identity", "class")


def merge_windows(regions: Sequence[Tuple[str, int, int]], targets_length: Dict[str, int]) -> Tuple[np.ndarray, np.ndarray]:
    """BED rows (contig, start, end) as the windows of gci_bam_reads_size -> (int64 [n, 2]: [begin, end) in contig coordinates, contig
    after contig in the order of `targets_length`, per contig sorted, disjoint and not abutting; uint32 [n_sel + 1]: every contig's
    first window, then n).  A row is clamped to its contig; a row on a contig that is not selected, and one that is empty after the
    clamp, is dropped; rows that overlap or abut are merged."""
    per = {t: [] for t in targets_length}
    for name, start, end in regions:
        if name in per:
            a, b = max(int(start), 0), min(int(end), int(targets_length[name]))
            if a < b:
                per[name].append((a, b))
    win, win0 = [], [0]
    for t in targets_length:
        for a, b in sorted(per[t]):
            if len(win) > win0[-1] and a <= win[-1][1]:
                win[-1][1] = max(win[-1][1], b)
            else:
                win.append([a, b])
        win0.append(len(win))
    return np.asarray(win, dtype=np.int64).reshape(-1, 2), np.asarray(win0, dtype=np.uint32)


class FilterReads:
    """What bam_filter_reads returns: files = the BAM files listed, counts[k][class id] = the records of file k per class (as
    FilterDepth.counts; with `join` the covered file's row runs on through the join's classes), rows[k] = the rows written for it."""

    def __init__(self, files: List[str], counts: List[List[int]], rows: List[int]):
        self.files, self.counts, self.rows = files, counts, rows


class _ReadsVisitor(_FateVisitor):
    """Next to _FateVisitor, whose class bytes, join refinement and record counts it shares: per piece gci_bam_fate (+ gci_fate_refine),
    then gci_bam_reads_size / _write over the class bytes, the rows to the host and behind the file `f`.  Only the rows cross the
    link.  A file that is read again from its first record (abort_file) loses the rows written for it."""

    def __init__(self, main: Engine, opts: FateOpts, mask: int, names: Sequence[bytes], windows, f, join_fate: Optional[Buffer] = None):
        super().__init__(main, opts, [], 1, join_fate)
        self.mask, self.names, self.windows, self.f = int(mask), list(names), windows, f
        self.file_no, self.rows, self.mark = 0, 0, f.tell()
        self._on_device: Dict[int, tuple] = {}

    def begin_file(self) -> None:
        super().begin_file()
        self.rows, self.mark = 0, self.f.tell()

    def abort_file(self) -> None:
        self.f.seek(self.mark)
        self.f.truncate()
        self.begin_file()

    def _tables(self, engine):
        """The contig names and the windows on the engine's device, uploaded once."""
        if id(engine) not in self._on_device:
            d_names = engine.to_device(np.frombuffer(b"".join(self.names) + b"\0", dtype=np.uint8))
            d_win = d_win0 = None
            if self.windows is not None:
                win, win0 = self.windows
                d_win = engine.to_device(np.ascontiguousarray(win if win.shape[0] else np.zeros((1, 2), dtype=np.int64)))
                d_win0 = engine.to_device(win0)
            self._on_device[id(engine)] = (d_names, d_win, d_win0)
        return self._on_device[id(engine)]

    def visit(self, engine, d_stream, d_off, has_seq, ref_sel, rec_idx_base) -> None:
        if engine.lengths != self.main.lengths:            # (the walk engine: a context of its own)
            engine.set_layout(self.main.lengths)
        o = self.opts
        d_names, d_win, d_win0 = self._tables(engine)
        what = "gci_bam_fate"
        try:
            with phases.gpu("record fate"):
                cls, counts = engine.bam_fate(d_stream, d_off, has_seq, ref_sel, o.map_qual, o.clip_percent, o.iden_percent)
                if self.join_fate is not None:
                    what = "gci_fate_refine"
                    self._refine(engine, cls, int(d_off.shape[0]), rec_idx_base)
            what = "gci_bam_reads_size"
            with phases.gpu("record rows"):
                text, n_rows = engine.bam_reads(d_stream, d_off, has_seq, ref_sel, cls, self.mask, self.names, d_names, d_win, d_win0, self.file_no)
        except GciError as e:
            if e.rec < 0:
                raise
            raise _file_record_error(engine, e, what, rec_idx_base) from None
        self.f.write(text)
        self.rows += n_rows
        self.n_seen += int(d_off.shape[0])
        self.counts = [a + b for a, b in zip(self.counts, counts)]


def bam_filter_reads(engine: Engine, bam_files: Sequence[str], chrs: Sequence[str], opts: Optional[FateOpts], threads: int, classes: Sequence[str],
                     regions: Optional[Sequence[Tuple[str, int, int]]], out: str, join: Optional[JoinFateOpts] = None) -> FilterReads:
    """`out`: one row per record of `bam_files` whose class (bam_filter_depth's: FATE_WANTED, with `join` JOIN_FATE_NAMES too, where
    `kept` stands for the five of them) is among `classes` and whose reference span overlaps a row of `regions` (BED rows; None:
    every such record), in the files' record order, file after file -- the columns READS_COLUMNS as include/gci_hip.h
    (gci_bam_reads_size) states them, behind one `#file` line per listed file and the line of column names.  Contigs, @SQ check,
    `join` and the errors raised are bam_filter_depth's; with `join` the file join.cover alone is listed."""
    opts = opts or FateOpts()
    wanted = FATE_WANTED + (JOIN_FATE_NAMES if join is not None else ())
    mask = 0
    for name in classes:
        if name not in wanted:
            raise ValueError('"%s" is not one of %s' % (name, ", ".join(wanted)))
        mask |= _JOIN_FATE_MASK if (join is not None and name == "kept") else 1 << ALL_FATE_NAMES.index(name)
    if not mask:
        raise ValueError("no class selected")
    if join is not None and not 0 <= join.cover < len(bam_files):
        raise ValueError("cover = %d: there are %d BAM files" % (join.cover, len(bam_files)))
    first = same_sq_table(bam_files)
    targets_length = _targets_of(first, list(chrs))
    targets = list(targets_length.keys())
    if not targets:
        raise ValueError("no contig selected")
    engine.set_layout([targets_length[t] for t in targets])
    join_fate, join_n_rec, join_counts = _join_fates(engine, bam_files, targets, opts, join, threads) if join is not None else (None, 0, [])
    listed = list(bam_files) if join is None else [bam_files[join.cover]]
    windows = None if regions is None else merge_windows(regions, targets_length)
    counts, rows = [], []
    try:
        with open(out, "wb") as f:
            for k, path in enumerate(listed):
                f.write(b"#file\t%d\t%s\n" % (k + 1, os.fsencode(path)))
            f.write(b"#" + "\t".join(READS_COLUMNS).encode() + b"\n")
            visitor = _ReadsVisitor(engine, opts, mask, [t.encode() for t in targets], windows, f, join_fate)
            for k, path in enumerate(listed):
                visitor.file_no = k + 1
                visitor.begin_file()
                try:
                    with phases.wall("bam_reads[%s]" % os.path.basename(path)):
                        bam_join_input(engine, path, targets, visitor, threads)
                except GciError as e:
                    e.path = path                         # (which file the record index counts in: the command line says so)
                    raise
                counts.append(list(visitor.counts))
                rows.append(visitor.rows)
    except BaseException:
        if os.path.exists(out):                           # (no half a table is left behind)
            os.remove(out)
        raise
    if join is not None:
        counts[0] = counts[0] + _join_row(bam_files, join, join_counts, join_n_rec, visitor.n_seen, counts[0][_KEPT])
    return FilterReads(listed, counts, rows)


# ==============================================================================================
# filter_sweep.py: how the record filter's three thresholds cut a BAM file
# ==============================================================================================

SWEEP_COLUMNS = ("value",) + _lib.SWEEP_COLUMNS + ("kept_at", "kept_bases_at")


class FilterSweep:
    """What bam_filter_sweep returns: files = the BAM files, tables[k] = file k's table uint64 [GCI_SWEEP_ROWS(digits), 4] (records,
    bases, records_others, bases_others; the rows as _lib.SweepRows(digits) numbers them)."""

    def __init__(self, files: List[str], tables: List[np.ndarray], digits: int):
        self.files, self.tables, self.digits = files, tables, digits


class _SweepVisitor(StreamVisitor):
    """Per piece of a file ONE gci_bam_sweep call; the pieces' tables add on the host (a table is 72 KB at three digits)."""

    def __init__(self, main: Engine, opts: FateOpts, digits: int, windows):
        self.main, self.opts, self.digits, self.windows = main, opts, int(digits), windows
        self.table = np.zeros((_lib.SweepRows(self.digits).rows, _lib.SWEEP_COLS), dtype=np.uint64)
        self._on_device: Dict[int, tuple] = {}

    def begin_file(self) -> None:
        self.table[:] = 0

    abort_file = begin_file

    def _windows(self, engine):
        """The windows on the engine's device, uploaded once."""
        if self.windows is None:
            return None, None
        if id(engine) not in self._on_device:
            win, win0 = self.windows
            self._on_device[id(engine)] = (engine.to_device(np.ascontiguousarray(win if win.shape[0] else np.zeros((1, 2), dtype=np.int64))),
                                           engine.to_device(win0))
        return self._on_device[id(engine)]

    def visit(self, engine, d_stream, d_off, has_seq, ref_sel, rec_idx_base) -> None:
        if engine.lengths != self.main.lengths:            # (the walk engine: a context of its own)
            engine.set_layout(self.main.lengths)
        o = self.opts
        d_win, d_win0 = self._windows(engine)
        try:
            with phases.gpu("record sweep"):
                self.table += engine.bam_sweep(d_stream, d_off, has_seq, ref_sel, o.map_qual, o.clip_percent, o.iden_percent, self.digits, d_win, d_win0)
        except GciError as e:
            if e.rec < 0:
                raise
            raise _file_record_error(engine, e, "gci_bam_sweep", rec_idx_base) from None


def bam_filter_sweep(engine: Engine, bam_files: Sequence[str], chrs: Sequence[str], opts: Optional[FateOpts], threads: int, digits: int = 3,
                     regions: Optional[Sequence[Tuple[str, int, int]]] = None) -> FilterSweep:
    """Per file of `bam_files` the distribution of MAPQ, clip quotient and identity quotient over its primary records (those
    bam_filter_depth puts into mapq, clip, identity or kept), `digits` decimal digits a quotient, weighted by records and by covered
    bases, and beside both what passes the other two tests at `opts`' thresholds (include/gci_hip.h: gci_bam_sweep).  regions (BED
    rows; None: every primary record): only the records whose reference span overlaps one.  Contigs and @SQ check are
    bam_filter_depth's.  A malformed record raises GciError with .path and the record's index in the file; a record GCI.py would raise on
    (no NM tag, a zero denominator) is counted on an `undefined` row."""
    opts = opts or FateOpts()
    rows = _lib.SweepRows(int(digits))                     # (digits outside 1 .. 3: ValueError)
    first = same_sq_table(bam_files)
    targets_length = _targets_of(first, list(chrs))
    targets = list(targets_length.keys())
    if not targets:
        raise ValueError("no contig selected")
    engine.set_layout([targets_length[t] for t in targets])
    windows = None if regions is None else merge_windows(regions, targets_length)
    visitor = _SweepVisitor(engine, opts, rows.digits, windows)
    tables = []
    for path in bam_files:
        visitor.begin_file()
        try:
            with phases.wall("bam_sweep[%s]" % os.path.basename(path)):
                bam_join_input(engine, path, targets, visitor, threads)
        except GciError as e:
            e.path = path                                 # (which file the record index counts in: the command line says so)
            raise
        tables.append(visitor.table.copy())
    return FilterSweep(list(bam_files), tables, rows.digits)


def sweep_value(rows, row: int) -> str:
    """The `value` column of row `row` of a sweep table: the MAPQ, the quotient 0.000 .. 1.000 rendered from the integer row, or the
    name of a special row."""
    if row < rows.clip0:
        return str(row)
    if row in (rows.clip_undef, rows.iden_undef):
        return "undefined"
    if row == rows.iden_below:
        return "<0"
    if row == rows.iden_above:
        return ">1"
    b = row - (rows.clip0 if row < rows.clip_undef else rows.iden0)
    return "%d.%0*d" % (b // rows.bins, rows.digits, b % rows.bins)


def sweep_text(table: np.ndarray, digits: int) -> str:
    """The three tables `#mapq`, `#clip`, `#identity` of one file as filter_sweep.py writes them: every row, in table order, with the
    columns SWEEP_COLUMNS.  kept_at / kept_bases_at: what would be `kept` if this one threshold were set to the row's value while the
    other two stay -- the sum of the _others columns over the rows that pass then (mapq: rows >= v; clip: numeric rows <= v; identity:
    numeric rows >= v, plus `>1`); `-` on the special rows."""
    rows = _lib.SweepRows(digits)
    t = [[int(x) for x in r] for r in np.asarray(table).tolist()]
    kept = {}                                             # row -> (records, bases)
    acc = [0, 0]
    for r in range(rows.clip0 - 1, -1, -1):               # mapq: from 255 down
        acc = [acc[0] + t[r][2], acc[1] + t[r][3]]
        kept[r] = tuple(acc)
    acc = [0, 0]
    for r in range(rows.clip0, rows.clip_undef):          # clip: from 0 up
        acc = [acc[0] + t[r][2], acc[1] + t[r][3]]
        kept[r] = tuple(acc)
    acc = [t[rows.iden_above][2], t[rows.iden_above][3]]
    for r in range(rows.iden_above - 1, rows.iden0 - 1, -1):      # identity: from 1 down, behind `>1`
        acc = [acc[0] + t[r][2], acc[1] + t[r][3]]
        kept[r] = tuple(acc)
    out = []
    for name, a, b in (("mapq", 0, rows.clip0), ("clip", rows.clip0, rows.iden_below), ("identity", rows.iden_below, rows.rows)):
        out.append("#%s\n%s\n" % (name, "\t".join(SWEEP_COLUMNS)))
        for r in range(a, b):
            k = kept.get(r, ("-", "-"))
            out.append("\t".join([sweep_value(rows, r)] + [str(x) for x in t[r]] + [str(k[0]), str(k[1])]) + "\n")
    return "".join(out)


# ==============================================================================================
# contig-sharded run (one process per GPU)
# ==============================================================================================

def bam_records_of_contigs(engine: Engine, path: str, targets: Sequence[str], own: Sequence[str], filt, threads: int = 1) -> JoinInput:
    """K1 over the records of the contigs `own` of one BAM file -- the part of the reference's fan-out over contigs
    (GCI.py:257-270) that falls to this rank.  gci_rec.contig is the index in `targets` (all selected contigs).

    With an index next to the file (`<bam>.bai`; the reference needs one for pysam's fetch) only the BGZF members
    that hold those records are read and inflated: the pseudo-bin samtools writes per reference (or the hull of its
    chunks) gives the virtual offsets of the contig's first record and of the end of its last one; that run of members
    is inflated and walked on the device (GCI_BAM_INGEST=gpu, the default) or on host threads.  Without an index the
    whole file is ingested and K1 drops the records of the other contigs."""
    hdr = bamfmt.read_header(path)
    ref_sel = _ref_sel(engine, hdr, targets, own)
    own_set = set(own)
    index = bamfmt.read_bai(path + ".bai")
    nthreads = hostio.pick_threads(threads)
    if index is None or len(index) != len(hdr.references):
        raw = np.fromfile(path, dtype=np.uint8)
        with hostio.bam_heads(raw, threads=nthreads, check_crc=BGZF_CRC) as heads:
            d_bam, d_off = engine.to_device(heads.stream), engine.to_device(heads.offsets)
        return _filter_stream(engine, d_bam, d_off, False, ref_sel, filt)
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    n_raw = int(raw.shape[0])
    on_device = _ingest_mode() == "gpu"
    parts = _Parts(engine, ref_sel, filt)
    for r, name in enumerate(hdr.references):
        if name not in own_set or index[r] is None:
            continue
        beg, end = index[r]
        # the member table of THIS contig's run only: from the member of its first record (beg >> 16) to the member its range
        # ends in (end >> 16), hopping BSIZE from header to header -- a rank never touches the members of the other ranks'
        # contigs (round 2 scanned the whole file on every rank: N x the file's pages through the page cache)
        c_beg, c_end = beg >> 16, end >> 16
        if not (0 <= c_beg <= c_end and c_end + 18 <= n_raw):
            raise bamfmt.BAMError("index of %s does not match its BGZF members" % path)
        try:
            run_end = c_end + bgzf.member_size(raw, c_end)                           # (the BC sub-field wherever it stands)
        except bgzf.BGZFError as e:
            raise bamfmt.BAMError("index of %s does not match its BGZF members" % path) from e
        try:
            pos, isz = hostio.bgzf_blocks(np.asarray(raw[c_beg:min(run_end, n_raw)]))
        except Exception as e:                                                    # noqa: BLE001
            raise bamfmt.BAMError("index of %s does not match its BGZF members" % path) from e
        pos = pos + np.uint64(c_beg)
        cpos = pos[:isz.shape[0]].astype(np.int64)
        a, b = 0, int(isz.shape[0]) - 1
        if b < 0 or cpos[a] != c_beg or cpos[b] != c_end:
            raise bamfmt.BAMError("index of %s does not match its BGZF members" % path)
        last = b if (end & 0xFFFF) else b - 1                                    # (a range ending at offset 0 of a member stops before it)
        if last < a:
            continue
        stop = int(isz[a:b].sum()) + (end & 0xFFFF)                              # end of the contig's last record inside the run
        d_buf = d_off = None
        if on_device and int(isz[a:last + 1].sum()) <= GPU_INFLATE_MAX:
            # the run's members inflated and walked on the device (N1, as in bam_join_input)
            p0 = int(pos[a])
            with _rebased(a):
                d_run = engine.bgzf_inflate(raw[p0:int(pos[last + 1])], pos[a:last + 2] - np.uint64(p0), isz[a:last + 1], check_crc=BGZF_CRC)
            d_off, used, ok = engine.bam_record_offsets(d_run[:stop], beg & 0xFFFF, len(hdr.references))
            if ok and used == stop:
                d_buf = d_run[:stop]
            del d_run
        if d_buf is None:
            buf = hostio.bgzf_inflate(np.asarray(raw[int(pos[a]):int(pos[last + 1])]), threads=nthreads, check_crc=BGZF_CRC)
            offs, _ = hostio.bam_chunk_offsets(buf[:stop], beg & 0xFFFF)
            d_buf, d_off = engine.to_device(buf[:stop]), engine.to_device(offs)
        if d_off.shape[0] == 0:
            continue
        try:
            parts.add(d_buf, d_off)
        except GciError as e:
            e.contig = targets.index(name)          # (the ranks agree on the error of the earliest contig: _agree_on_error)
            raise
        del d_buf, d_off
    return parts.result()


def _replicate(engine: Engine, ji: JoinInput) -> JoinInput:
    """One file's compact records + names of every rank, on every rank (all-gather; RCCL over xGMI).  Rank r's records
    keep their order and sit behind those of ranks < r: a contig's records come from one rank, so "the last record of a
    name wins" (contig order first, then file order; GCI.py:269) is decided as in a single process."""
    from . import shard
    n = int(ji.recs.shape[0])
    if n:
        blob, off = engine.pack_names(ji)
    else:
        blob, off = engine.T.zeros(0, engine.T.uint8, engine.device), engine.T.zeros(1, engine.T.int64, engine.device)
    ex = shard.RecordExchange(n, int(blob.shape[0]), engine.device, via_host=SHARD.backend != "nccl")
    ex.send_recs[:n] = ji.recs
    ex.send_recs[:n, 29] &= 3                          # the names travel packed: no longer GCI_REC_NAME16
    ex.send_names[:blob.shape[0]] = blob
    ex.send_off[:n + 1] = off
    g = ex.gather()
    return JoinInput(g.recs, g.names, g.name_index, 0)


def _own_names_only(engine: Engine, ji: JoinInput, world: int, rank: int) -> JoinInput:
    """Records every rank holds alike (PAF files are filtered whole on every rank): keep those whose NAME this rank owns --
    (hash >> 33) % world, the rule of gci_route_records -- so that they meet the routed BAM records of the same names."""
    if int(ji.recs.shape[0]) == 0:
        return ji
    import torch                                       # (a contig-sharded run: the torch provider)
    h = ji.recs[:, 0:8].contiguous().view(torch.int64).reshape(-1)
    dest = ((h >> 33) & 0x7FFFFFFF) % world
    recs = ji.recs.clone()
    recs[dest != rank, 29] = 0                       # gci_rec.flags
    return JoinInput(recs, ji.name_base, ji.name_off, ji.name_delta)


def _agree_on_error(err: Optional[GciError], contig: int = 1 << 30) -> None:
    """A contig-sharded run fails as ONE run: every rank learns whether any rank's record filter / join raised, and all of them
    raise the error of the earliest contig (the one the reference's loop over contigs would have met first) -- a rank that
    went on alone would wait in the next collective for ever."""
    code = 0 if err is None else -int(err.status)
    key = (min(int(contig), (1 << 30)) << 8 | code) if code else (1 << 40)
    best = -SHARD.all_reduce_max([-key])[0]
    if best >= (1 << 40):
        return
    _reraise_like_reference(err if (err is not None and key == best) else GciError(-(best & 0xFF), "record filter / join failed on another rank"))


def _filter_sharded(paf_files, bam_files, prefix, map_qual, mq_cutoff, iden_percent, clip_percent, ovlp_percent, flank_len,
                    directory, log_reads_type, chrs_list, threads, engine: Engine, write, issue_hint):
    """filter() of a contig-sharded run.  Contigs are dealt to the ranks (longest first onto the least loaded); depth
    build, gap mask, two-type max, issue scan and depth text are contig-local.  The read-name join is not -- a read
    aligned to contigs of two ranks must be dropped, a name repeated across contigs keeps its last record
    (GCI.py:269, 296-297) -- but it is independent per NAME: every rank filters the records of ITS contigs (K1), routes them
    by name hash to the rank that owns the name (two all-to-alls per file), joins the names it owns and routes the surviving
    intervals to the owners of their contigs (shard.ShardedJoin; round 2 replicated every record on every rank).
    PAF files are sharded by byte range (shard.paf_by_byte_range: every rank tokenises the lines of its range, the hits travel to
    the rank that owns their query name and are scored there); when a line raises, every rank filters the whole files and keeps
    the names it owns (round 2's way)."""
    from . import shard
    first = bamfmt.read_header(bam_files[0])
    targets_length = _targets_of(first, chrs_list)
    targets = list(targets_length.keys())
    mine = SHARD.assign([targets_length[t] for t in targets])
    if SHARD.world > len(targets):                  # (every rank sees this: rank 0 says it)
        sys.exit(f"ERROR!!! {SHARD.world} GPUs for {len(targets)} contig(s): use at most one GPU per contig")
    local_tl = {targets[c]: targets_length[targets[c]] for c in mine}
    engine.set_layout(list(local_tl.values()))
    filt = (map_qual, mq_cutoff, clip_percent, iden_percent)
    paf_inputs: List[JoinInput] = []
    local: List[JoinInput] = []
    err, err_contig = None, 1 << 30
    try:
        if len(paf_files) != 0:
            # every rank tokenises 1 / world of the files' bytes; the hits are scored on the rank that owns their query name
            # (None: a line the reference raises on -- then every rank reads the whole files, and the exception comes out exact)
            by_range = shard.paf_by_byte_range(engine, paf_files, targets, map_qual, mq_cutoff, iden_percent, SHARD.world, SHARD.rank,
                                               SHARD.all_reduce_max, engine.device, via_host=SHARD.backend != "nccl")
            try:
                paf_inputs = by_range if by_range is not None else [
                    _own_names_only(engine, ji, SHARD.world, SHARD.rank)
                    for ji in engine.paf_filter(paf_files, targets, map_qual, mq_cutoff, iden_percent)]
            except GciError as e:
                e.paf_replay = (paf_files, targets)
                raise
        for path in bam_files:
            local.append(bam_records_of_contigs(engine, path, targets, list(local_tl), filt, threads))
    except GciError as e:
        err, err_contig = e, getattr(e, "contig", 0)
    _agree_on_error(err, err_contig)
    # routed name slots: as long as the longest query name of the run (a multiple of 16, the same on every rank)
    import torch                                       # (a contig-sharded run: the torch provider)
    longest = max([int(ji.recs[:, 30:32].contiguous().view(torch.int16).max().item()) if int(ji.recs.shape[0]) else 0 for ji in local] + [1])
    slot = (SHARD.all_reduce_max([longest])[0] + 15) // 16 * 16
    sj = shard.ShardedJoin(engine, [int(ji.recs.shape[0]) for ji in local], SHARD.owner, engine.device,
                           via_host=SHARD.backend != "nccl", name_slot=max(16, slot),
                           extra_records=sum(int(ji.recs.shape[0]) for ji in paf_inputs))
    classic = False
    try:
        while True:
            inputs = paf_inputs + sj.exchange_files(local)          # (ONE all-to-all for the records and names of every file)
            ivl, n_slots = sj.join(inputs, ovlp_percent)
            err = None
            try:
                def decode(w, what):
                    rec = ctypes.c_uint32(0)
                    st = engine.lib.gci_decode_status(w, ctypes.byref(rec))
                    if st != 0:
                        e = GciError(st, "%s: %s" % (what, engine.lib.gci_strerror(st).decode()), rec=int(rec.value))
                        e.what = what
                        raise e
                sj.check(decode)
            except GciError as e:
                err = e
            cap = err is not None and err.status == _lib.GCI_E_CAPACITY
            # GCI_E_CAPACITY has two senders.  The partitioned JOIN refuses what its 32-byte entries / LDS tables cannot hold
            # (adversarial names): every rank then joins on the classic table, once -- larger buckets would change nothing.
            # A ROUTE / SEAL step reports a bucket that overflowed (names hash unevenly): larger buckets, again.
            from_join = cap and getattr(err, "what", "") == "gci_name_join"
            refuse, grow = SHARD.all_reduce_max([1 if from_join else 0, 1 if (cap and not from_join) else 0])
            if grow:
                sj.grow()
                continue
            if refuse and not classic:
                classic = True
                engine._chk(engine.lib.gci_join_mode(engine.ctx, 1), "gci_join_mode")
                continue
            _agree_on_error(err)
            break
    finally:
        if classic:
            engine._chk(engine.lib.gci_join_mode(engine.ctx, engine.join_mode), "gci_join_mode")
    track = engine.new_track()
    fused = engine.depth_build_fused(ivl, None, flank_len, track, want_text=False, want_sums=True, issue=issue_hint, counted=False)
    depths = _depths_of_build(engine, local_tl, targets, track, fused, issue_hint, log_reads_type, directory, prefix, write, from_build=False)
    return depths, targets_length


def _paf_line_exception(paf_files: Sequence[str], targets: Sequence[str]) -> Optional[BaseException]:
    """ERROR PATH ONLY.  The device PAF filter has reported a line the reference raises on (GCI_E_MALFORMED / GCI_E_ZERO_DIV with a
    line number); the reference would die with Python's own exception for that line -- IndexError for a missing column,
    ValueError with int()'s message for a bad number, ZeroDivisionError for a zero alignment length -- and which one depends on
    the order GCI.py:217-229 touches the columns in.  This replays exactly those statements over the files in order and returns
    the first exception they raise (None if no line raises).  It computes nothing that is used: no dict, no score."""
    tset = set(targets)
    for path in paf_files:
        with open(path, "r") as f:
            for line in f:
                try:
                    paf = line.strip().split("\t")
                    if paf[5] in tset:
                        int(paf[1]), int(paf[2]), int(paf[3]), int(paf[7]), int(paf[8])
                        num_match_res, len_aln = int(paf[9]), int(paf[10])
                        int(paf[11])
                        num_match_res / len_aln
                except (IndexError, ValueError, ZeroDivisionError) as exc:
                    return exc
    return None


def _reraise_like_reference(e: GciError):
    from . import _lib
    replay = getattr(e, "paf_replay", None)
    if replay is not None and e.status in (_lib.GCI_E_MALFORMED, _lib.GCI_E_ZERO_DIV) and getattr(e, "rec", 0) > 0:
        exc = _paf_line_exception(*replay)
        if exc is not None:
            raise exc from e
    if e.status == _lib.GCI_E_NO_NM:
        raise KeyError("tag 'NM' not present") from e
    if e.status == _lib.GCI_E_ZERO_DIV:
        raise ZeroDivisionError("division by zero") from e
    raise e


# `{prefix}.depth.gz` is written by the device: gzip members straight from the track or from the run lists the build kept
# (gci_depth_deflate_*: no text buffer, a few MB cross PCIe).  (Rounds 1 - 5 kept the older way -- text rendered on the device, gzip on
# host threads -- behind GCI_DEPTH_GZ=host; the text seam itself, gci_depth_text_*, stays in the library and in bench.py's step.)


def write_depth(directory=".", prefix="GCI", depths: DepthTracks = None, threads=1) -> None:
    """`{directory}/{prefix}.depth.gz`: '>contig' line then one decimal per line (GCI.py:99-143), as a multi-member
    gzip (any gzip whose payload equals the reference's text is a valid .depth.gz)."""
    depths._bind()
    _write_depth_members(directory, prefix, depths)


def _write_depth_members(directory, prefix, depths: DepthTracks, from_build: bool = False) -> None:
    """'>contig' member (host), then the contig's lines as the members the device wrote.  Contig-sharded run: every rank
    deflates the contigs it owns, rank 0 gathers the members and writes them in header order.  from_build: only filter() says
    so, for the track its own build has just written (Engine.depth_deflate)."""
    blobs = depths.engine.depth_deflate(depths.track, from_build=from_build)               # views of the engine's pinned staging buffer
    items = list(zip(depths.targets, depths.lengths, blobs))
    if _sharded():
        # to rank 0 only (the members of a genome are GBs), as bytes: a sized gather of one uint8 tensor per rank -- which contigs a
        # rank owns every rank knows (SHARD.owner), so names and lengths need not travel
        order = {t: i for i, t in enumerate(depths.all_targets)}
        parts = SHARD.gather_bytes_to_root([np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for _, _, b in items])
        if not SHARD.root:
            return
        all_t = depths.all_targets
        items = []
        for r, blobs_r in enumerate(parts):
            owned = [c for c, o in enumerate(SHARD.owner) if o == r]
            assert len(owned) == len(blobs_r), (r, len(owned), len(blobs_r))
            # (a contig of length 0 has no members: its empty blob stands for "L == 0" below)
            items += [(all_t[c], int(b.shape[0]), b.tobytes()) for c, b in zip(owned, blobs_r)]
        items.sort(key=lambda x: order[x[0]])
    path = f"{directory}/{prefix}.depth.gz"
    if os.path.exists(path):
        os.remove(path)
    layout = {}
    with open(path, "wb") as f:
        for t, L, blob in items:
            if L == 0:
                continue              # the reference's chunk loop never runs for an empty contig: not even the '>' line
            at = f.tell()
            f.write(hostio.gzip_members((">%s\n" % t).encode(), threads=1))
            f.write(blob)
            layout[t] = (at, f.tell())
    phases.note("depth_gz_layout:" + path, layout)    # (a harness that checks single contigs of a genome-size file reads this)


def merge_two_type_depth(hifi_depths: DepthTracks = None, nano_depths: DepthTracks = None, prefix="GCI_two_type",
                         directory=".", force=False, threads=1, write=True, issue_hint=None) -> DepthTracks:
    """issue_hint = (leftmost, rightmost, flank_len) of the collapse_depth_range() calls that follow (as for filter()): the merge
    is then ONE pass over the two tracks that also applies their pending N-run masks (merge_gaps_depths(lazy=True)) and finds the
    issue runs of the HiFi, the ONT and the merged track (gci_two_type_tail) -- 12 bytes per base instead of 24."""
    print("Merging HiFi and ONT depth file ...")
    if write:
        refuse_overwrite(f"{directory}/{prefix}.depth.gz", force)
    if nano_depths.targets != hifi_depths.targets or nano_depths.lengths != hifi_depths.lengths:
        # the reference indexes nano by the HiFi dict's keys; GCI() has already checked both headers agree
        raise KeyError("HiFi and ONT depth tracks cover different contigs")
    engine = hifi_depths.engine
    pend = [d._pending_gaps for d in (hifi_depths, nano_depths)]
    same_pending = (pend[0] is None and pend[1] is None) or (pend[0] is not None and pend[1] is not None and
                                                             pend[0].tobytes() == pend[1].tobytes())
    if issue_hint is not None and nano_depths.engine is engine and same_pending:
        hifi_depths._bind_layout()
        lo, hi, fl = float(issue_hint[0]), float(issue_hint[1]), int(issue_hint[2])
        d_sums = engine.T.zeros((3, max(len(hifi_depths.targets), 1)), engine.T.int64, engine.device)
        two, runs = engine.two_type_tail(hifi_depths.track, nano_depths.track, pend[0], lo, hi, fl, sums=d_sums)
        merged = DepthTracks(engine, hifi_depths.targets_length, two)
        h_sums = d_sums.cpu().numpy()[:, :len(hifi_depths.targets)]
        for k, (d, r) in enumerate(zip((hifi_depths, nano_depths, merged), runs)):
            if pend[0] is not None:
                d._pending_gaps, d._masked_with = None, pend[0].tobytes()
            d._fresh_sums = h_sums[k].copy()                     # (the numerator of the mean depth of a `-p` run: no pass of its own)
            d._fresh_runs = ((lo, hi, fl), r)
    else:
        hifi_depths._bind()
        nano_depths._bind()
        merged = DepthTracks(engine, hifi_depths.targets_length, engine.max2(hifi_depths.track, nano_depths.track))
    merged.all_targets = hifi_depths.all_targets
    if write:
        write_depth(directory, prefix, merged, threads)
    print("Merging HiFi and ONT depth file done!!!\n\n")
    return merged


# ==============================================================================================
# issue scan
# ==============================================================================================

def _issues_from_runs(runs: np.ndarray, n_slice: int, chr_len: int, flank_len: int, start_pos: int
                      ) -> List[Tuple[int, int]]:
    """Apply the reference's closing rules (GCI.py:380-388) to raw maximal runs given relative to
    the scanned slice: a run that ends at an out-of-range base at relative index i is reported
    only if i > flank_len; a run reaching the last scanned base is reported iff that base has
    relative index chr_len - 2 * flank_len - 1."""
    out: List[Tuple[int, int]] = []
    for rs, re_ in runs.tolist():
        if re_ == n_slice:
            if n_slice - 1 != chr_len - 2 * flank_len - 1:
                continue
        elif not (re_ > flank_len):
            continue
        out.append((rs + flank_len + start_pos, re_ + flank_len + start_pos))
    return out


def collapse_depth_range(depths: DepthTracks = None, leftmost=-1, rightmost=0, flank_len=15, start_pos=0
                         ) -> Dict[str, List[Tuple[int, int]]]:
    depths._bind()
    key = (float(leftmost), float(rightmost), int(flank_len))
    if depths._fresh_runs is not None and depths._fresh_runs[0] == key:
        runs = depths._fresh_runs[1]
    else:
        runs = depths.engine.issue_scan(depths.track, leftmost, rightmost, flank_len)
    out = {}
    for c, t in enumerate(depths.targets):
        L = depths.lengths[c]
        a, b = _slice_bound(flank_len, L), _slice_bound(L - flank_len, L)
        out[t] = _issues_from_runs(runs[c], max(0, b - a), L, flank_len, start_pos)
    return out


def collapse_regions(depths: DepthTracks, regions: Sequence[Tuple[str, int, int]], leftmost, rightmost
                     ) -> List[List[Tuple[int, int]]]:
    depths._bind()
    wins, meta = [], []
    for target, start, end in regions:
        c = depths.targets.index(target)
        L = depths.lengths[c]
        a, b = _slice_bound(start, L), _slice_bound(end, L)
        b = max(a, b)
        o = depths.engine.offsets[c]
        wins.append((o + a, o + b))
        meta.append((b - a, start))
    runs = depths.engine.issue_scan_windows(depths.track, wins, leftmost, rightmost)
    return [_issues_from_runs(r, n, n, 0, sp) for r, (n, sp) in zip(runs, meta)]


def merge_depth(depths: DepthTracks = None, prefix="GCI", threshold=0, flank_len=15, directory=".", force=False,
                log_reads_type=""):
    print(f"Getting {log_reads_type} issues bed file detected by GCI ...")
    path = f"{directory}/{prefix}.{threshold}.depth.bed"
    refuse_overwrite(path, force)
    merged = collapse_depth_range(depths, -1, threshold, flank_len, 0)
    if _sharded():                      # every rank scanned its contigs; the lists (<= 10^4 items) travel as objects
        union = {}
        for part in SHARD.gather_objects(merged):
            union.update(part)
        merged = {t: union[t] for t in depths.all_targets}          # header order
    if _is_root():
        with open(path, "w") as f:
            for target, segments in merged.items():
                for s, e in segments:
                    f.write(f"{target}\t{s}\t{e}\n")
    print(f"Getting {log_reads_type} issues bed file done!!!\n\n")
    return merged


# ==============================================================================================
# N3: the `-p` numeric front-end
# ==============================================================================================

def sliding_window_average_depth_many(depths: DepthTracks, items: Sequence[Tuple[str, int, Optional[int]]], window_size=50000,
                                      max_depth=None):
    """sliding_window_average_depth(depths[target][start:end], window_size, max_depth, start, target) of the reference
    (GCI.py:660-705) for every (target, start, end) of `items` over a track in HBM, in TWO device calls for all of them:
    -> [(positions in Mb: list of float, values: float64 array, the reference's warning line or None)].

    The reference walks the bases one by one and restarts its window at every zero-depth base.  Which bases emit a value follows
    from the zero runs and the window size alone, so the device finds the zero runs of all items (ONE gci_issue_scan_windows)
    and sums all their windows (ONE gci_range_sums); the few thousand windows per contig are assembled here."""
    depths._bind()
    geo = []
    for target, start, end in items:
        c = depths.targets.index(target)
        L = depths.lengths[c]
        a = _slice_bound(start, L)
        b = max(a, _slice_bound(L if end is None else end, L))
        n = b - a
        w, warn = window_size, None
        if n < window_size:
            warn = (f'Warning!!! The length ({n}) of plotting region ({target}:{start}-{start + n}) is less than the window size '
                    f'({window_size}), and therefore the window size will be 1 bp')
            w = 1
        geo.append((depths.engine.offsets[c] + a, n, w, warn, start))
    live = [k for k, g in enumerate(geo) if g[1] > 0]
    zeros = depths.engine.issue_scan_windows(depths.track, [(geo[k][0], geo[k][0] + geo[k][1]) for k in live], -1, 0) if live else []
    plans, ranges = {}, []
    for k, z in zip(live, zeros):
        o, n, w, _, _ = geo[k]
        zero = z.reshape(-1, 2)                                  # runs of depth 0, relative to the item's first base
        edges = np.concatenate([[0], zero.reshape(-1), [n]]).astype(np.int64)       # the non-zero runs in between
        p, q = edges[0::2], edges[1::2]
        keep = q > p
        p, q = p[keep], q[keep]
        full = (q - p) // w                                      # whole windows per run, then one partial flush
        rem = (q - p) - full * w
        # window k of run r: [p + k w, p + (k + 1) w); emitted at its last base
        run_of = np.repeat(np.arange(p.shape[0]), full)
        kk = np.arange(int(full.sum()), dtype=np.int64) - np.repeat(np.cumsum(full) - full, full)
        wb = p[run_of] + kk * w
        has_rem = rem > 0
        begins = np.concatenate([wb, (q - rem)[has_rem]])
        ends = np.concatenate([wb + w, q[has_rem]])
        plans[k] = (zero, begins, ends, len(ranges), begins.shape[0])
        ranges.append(np.stack([begins + o, ends + o], axis=1))
    sums = depths.engine.range_sums(depths.track, np.concatenate(ranges)) if ranges else np.zeros(0, dtype=np.int64)
    at = np.concatenate([[0], np.cumsum([r.shape[0] for r in ranges])]).astype(np.int64) if ranges else np.zeros(1, np.int64)
    out = []
    for k, (o, n, w, warn, start) in enumerate(geo):
        if n == 0:
            out.append(([], np.array([], dtype=np.float64), warn))
            continue
        zero, begins, ends, slot, cnt = plans[k]
        s = sums[int(at[slot]):int(at[slot]) + cnt]
        means = s.astype(np.float64) / (ends - begins).astype(np.float64)   # int / int, both < 2^53: as Python's true division
        means = np.where(means > max_depth, np.float64(max_depth), means)
        zlen = zero[:, 1] - zero[:, 0]
        zidx = np.repeat(zero[:, 0] - (np.cumsum(zlen) - zlen), zlen) + np.arange(int(zlen.sum()), dtype=np.int64)
        idx = np.concatenate([ends - 1, zidx])
        val = np.concatenate([means, np.zeros(zidx.shape[0], dtype=np.float64)])
        order = np.argsort(idx, kind="stable")
        idx, val = idx[order], val[order]
        out.append((((idx + start) / 1e6).tolist(), val, warn))
    return out


def sliding_window_average_depth(depths: DepthTracks, target: str, window_size=50000, max_depth=None, start=0, end=None):
    """One (target, start, end): -> (positions in Mb: list of float, values: float64 array); the reference's warning for a region
    shorter than the window goes to stderr (GCI.py:675-677)."""
    pos, val, warn = sliding_window_average_depth_many(depths, [(target, start, end)], window_size, max_depth)[0]
    if warn:
        print(warn, file=sys.stderr)
    return pos, val


def depth_profile_v2(tracks: DepthTracks, items: Sequence[Tuple[str, int, int]], window_size: int, low_below: int = 5):
    """What utility/depth_plotter_v2.py computes from depths[target][start:end + 1] for every (target, start, end INCLUSIVE) of
    `items` (0 <= start <= end < length), over a track in HBM, in TWO device calls for all of them: ONE gci_depth_classes (the zero
    runs, the low runs, the sum and the number of the bases with depth > 0) and ONE gci_range_sums (the window sums).  Per item a
    dict, positions relative to `start`:
        zero, low   int64 [k, 2]: inclusive (first, last) of every run of depth == 0 / of 0 < depth < low_below
        means, starts, ends   the utility's windows -- a stretch between two zero runs is cut into pieces of window_size from its
                    first base on, the last piece shorter; no window is empty -- as float64 means (sum / bases, both below 2^53:
                    np.mean of the int64 slice) and inclusive int64 bounds
        sum_pos, n_pos   the sum of the depths > 0 and how many there are.
    The utility walks every base three times in Python for the same."""
    tracks._bind()
    w = int(window_size)
    wins = []
    for target, start, end in items:
        o = int(tracks.engine.offsets[tracks.targets.index(target)])
        wins.append((o + int(start), o + int(end) + 1))
    if not wins:
        return []
    zeros, lows, stats = tracks.engine.depth_classes(tracks.track, wins, low_below)
    plans, ranges = [], []
    for (a, b), zero in zip(wins, zeros):
        edges = np.concatenate([[0], zero.reshape(-1), [b - a]]).astype(np.int64)      # the stretches between the zero runs
        p, q = edges[0::2], edges[1::2]
        keep = q > p
        p, q = p[keep], q[keep]
        per = (q - p + w - 1) // w                                                     # windows per stretch
        of = np.repeat(np.arange(p.shape[0]), per)
        k = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
        begins = p[of] + k * w
        ends = np.minimum(begins + w, q[of])
        plans.append((begins, ends))
        ranges.append(np.stack([begins + a, ends + a], axis=1))
    sums = tracks.engine.range_sums(tracks.track, np.concatenate(ranges))
    out, at = [], 0
    for (begins, ends), zero, low, st in zip(plans, zeros, lows, stats):
        n = begins.shape[0]
        means = sums[at:at + n].astype(np.float64) / (ends - begins).astype(np.float64)
        at += n
        incl = np.array([0, -1], dtype=np.int64)
        out.append({"zero": zero.reshape(-1, 2) + incl, "low": low.reshape(-1, 2) + incl, "means": means, "starts": begins,
                    "ends": ends - 1, "sum_pos": int(st[0]), "n_pos": int(st[1])})
    return out


def pre_plot_base(depths_list: Sequence[DepthTracks], max_depths: Sequence[float], window_size=50000, start=0,
                  region: Optional[Tuple[str, int, int]] = None):
    """pre_plot_base of the reference (GCI.py:708-739).  region = (target, start, end) is the reference's
    `{target: depths[start:end]}` input of the regions loop (GCI.py:887-892); None = every contig, whole.  Per track all its
    contigs go through the device together (two calls); the warnings come out in the reference's order (target by target)."""
    targets = [region[0]] if region else depths_list[0].targets
    items = [(t, region[1] if region else start, region[2] if region else None) for t in targets]
    per_track = [sliding_window_average_depth_many(tr, items, window_size, max_depths[i]) for i, tr in enumerate(depths_list)]
    averaged = [{} for _ in depths_list]
    maxima = [[] for _ in depths_list]
    for k, target in enumerate(targets):
        for i in range(len(depths_list)):
            pos, val, warn = per_track[i][k]
            if warn:
                print(warn, file=sys.stderr)
            averaged[i][target] = (pos, val)
            maxima[i].append(max(val))
    if _sharded() and region is None:            # the axis limits span every contig: the few maxima of all ranks
        maxima = [[x for part in parts for x in part] for parts in zip(*SHARD.gather_objects(maxima))]
    y_max = max(maxima[0]) + 10
    y_min = 0 if len(depths_list) == 1 else max(maxima[1]) + 10
    return averaged, y_min / (y_max + y_min), y_min, y_max


# ==============================================================================================
# score files
# ==============================================================================================

complement_merged_depth = score.complement_merged_depth
compute_n50 = score.compute_n50
merge_merged_depth_bed = score.merge_merged_depth_bed


def compute_index(targets_length={}, prefix="GCI", directory=".", force=False, merged_depths_bed_list=[],
                  type_list=[], flank_len=15, dist_percent=0.005, regions_bed={}, depths_list=[], threshold=0,
                  chrs_list=[]):
    gci_path = f"{directory}/{prefix}.gci"
    refuse_overwrite(gci_path, force)
    if _is_root():
        with open(gci_path, "w"):
            pass
    reg_path = f"{directory}/{prefix}.regions.gci"
    if len(regions_bed) > 0:
        refuse_overwrite(reg_path, force)
    # progress lines are printed where the work happens (same lines, same order as GCI.py:553-607)
    print("Computing Theoretical minimum N50 and contigs number ...")
    rows, exp_n50, exp_ctg = score.expected_table(targets_length, chrs_list)
    print("Computing Theoretical minimum N50 and contigs number done!!!")
    for t, bed in zip(type_list, merged_depths_bed_list):
        print(f"Computing Curated N50 and contigs number for {t} ...")
        obs_n50, obs_ctg = score.curated_table(bed, targets_length, flank_len, dist_percent, rows[-1])
        print(f"Computing Curated N50 and contigs number for {t} done!!!")
        print(f"Writing results to {gci_path} ...")
        if _is_root():
            with open(gci_path, "a") as f:
                f.write(score.section_text(t, rows, exp_n50, exp_ctg, obs_n50, obs_ctg))
        print(f"Writing results to {gci_path} done!!!\n\n")
    if len(regions_bed) > 0:
        print("Computing GCI scores for regions ...")
        flat = [(t, s, e) for t, segs in regions_bed.items() for s, e in segs]
        mine = [r for r in flat if r[0] in depths_list[0]]                      # the regions on contigs this rank holds
        per_track = [collapse_regions(d, mine, -1, threshold) for d in depths_list]
        lookup = {(i, r): per_track[i][k] for i in range(len(depths_list)) for k, r in enumerate(mine)}
        if _sharded():
            merged_lookup = {}
            for part in SHARD.gather_objects(lookup):
                merged_lookup.update(part)
            lookup = merged_lookup
        if _is_root():
            text = score.regions_text(regions_bed, type_list, len(depths_list),
                                      lambda i, t, s, e: lookup[(i, (t, s, e))], dist_percent,
                                      warn=lambda m: print(m, file=sys.stderr))
            with open(reg_path, "w") as f:
                f.write(text)
        print("Computing GCI scores for regions done!!!\n\n")


# ==============================================================================================
# GCI_score.py: a saved .depth.gz back to a track in HBM (utility/GCI_score.py:11-39)
# ==============================================================================================

def _upload_depths(engine: Engine, depths: Dict[str, np.ndarray]) -> Tuple[DepthTracks, Dict[str, int]]:
    targets_length = {t: int(a.shape[0]) for t, a in depths.items()}
    engine.set_layout(list(targets_length.values()))
    host = np.zeros(max(engine.total, 1), dtype=np.int32)
    for o, a in zip(engine.offsets, depths.values()):
        host[o:o + a.shape[0]] = a
    return DepthTracks(engine, targets_length, engine.to_device(host)), targets_length


def depth_read_mode() -> str:
    """GCI_DEPTH_READ: "members" (the default: this project's own files are read in the compressed domain, every other file as
    text) or "text" (today's path for every file)."""
    mode = os.environ.get("GCI_DEPTH_READ", "") or "members"
    if mode not in ("members", "text"):
        raise ValueError("GCI_DEPTH_READ=%s: members or text" % mode)
    return mode


def depth_members_plan(engine, path: str, buf, to_engine):
    """The first half of the compressed-domain read of a `.depth.gz`: every ten-byte member header of `buf`
    is a candidate, the engine decodes them all side by side (gci_depth_gz_scan over to_engine(buf), the same bytes in the engine's
    memory -- asked for only once the file begins with a '>name' member and has candidates) and the host follows the chain from
    byte 0 (depthfile.member_chain).  -> ((names, lengths, members), the bytes in the engine's memory) when the whole file is this
    project's writer's, else None: the text path takes all of it.  Which one it is goes to the phase log as "depth_read:<path>"."""
    from .formats import depthfile
    plan = None
    if depth_read_mode() == "members" and depthfile.header_member(memoryview(buf), 0) is not None:
        cand = depthfile.member_candidates(buf)
        if cand.shape[0]:
            d_raw = to_engine(buf)
            chain = depthfile.member_chain(buf, cand, engine.depth_gz_scan(d_raw, cand))
            plan = None if chain is None else (chain, d_raw)
    phases.note("depth_read:" + path, "members" if plan is not None else "text")
    return plan


def _depth_file_track(engine: Engine, names, lengths, ref_lengths):
    """The contigs of a depth file laid out on the device -> ({contig: length}, the zeroed track).  The track is None, and nothing
    is laid out, when ref_lengths is given and lacks one of the contigs; a contig an int32 index cannot span is refused."""
    from .formats import depthfile
    targets_length = dict(zip(names, lengths))
    if ref_lengths is not None and any(t not in ref_lengths for t in targets_length):
        return targets_length, None
    if any(L > depthfile.INT32_MAX for L in lengths):
        sys.exit("ERROR!!! A contig of the depth file is longer than 2^31 - 1 bases, which is not supported")
    engine.set_layout(lengths)
    return targets_length, engine.T.zeros(max(engine.total, 1), engine.T.int32, engine.device)     # (the padding behind every contig too)


def _read_depth_members(engine: Engine, path: str, buf: bytearray, ref_lengths):
    """read_depth_tracks for a file of this project's own writer: its bytes to HBM as they are, the members decoded into runs and
    the runs expanded into the track (k_depth_gz.hip).  No text on the host or the device.  -> None: not such a file."""
    from .formats import depthfile

    def upload(b):
        raw = np.frombuffer(b, dtype=np.uint8)
        return engine.upload_staged(raw) if raw.shape[0] >= (256 << 20) else engine.to_device(raw)

    plan = depth_members_plan(engine, path, buf, upload)
    if plan is None:
        return None
    (names, lengths, members), d_raw = plan
    targets_length, track = _depth_file_track(engine, names, lengths, ref_lengths)
    if track is None:
        return None, targets_length
    engine.depth_gz_track(d_raw, depthfile.place_members(members, engine.offsets), track)
    return DepthTracks(engine, targets_length, track), targets_length


def read_depth_tracks(engine: Engine, path: str, ref_lengths: Optional[Dict[str, int]] = None, plotter_v2: bool = False
                      ) -> Tuple[Optional[DepthTracks], Dict[str, int]]:
    """parse_depth of the reference's GCI_score.py for a `.depth.gz` file -> (DepthTracks, {contig: length}).  A file this project
    wrote itself is read in the compressed domain (_read_depth_members; GCI_DEPTH_READ=text switches that off).  Any other file is inflated
    on host threads (hostio.GzipText), its text goes to HBM through the staging ring, the device checks the grammar and ranks the
    lines (gci_depth_text_index), the host resolves the header lines into contigs and the device writes the track
    (gci_depth_text_parse).  Text outside the strict grammar, and a file the native inflate refuses, take the reference's own
    statements on the host (rare: hand-made files).  ref_lengths: when a contig of the file is not among them nothing is
    uploaded and the tracks are None (the caller refuses the file).
    plotter_v2: the reader of depth_plotter_v2.py -- a path that does not end in `.gz` is plain text (its bytes are the text, and from
    there on it is the text path; every other caller gunzips the file whatever its name, as its utility does), the names by that
    utility's expression, and (None, {}) instead of the host
    statements of GCI_score.py wherever the file is not wholly inside the strict grammar with every name once (the caller then
    reads it line by line, depthfile.lockstep_sequences)."""
    from .formats import depthfile
    with open(path, "rb") as f:
        buf = bytearray(os.path.getsize(path))
        f.readinto(buf)
    plain = plotter_v2 and not path.endswith(".gz")          # (that utility alone goes by the name; the others gunzip whatever it is)
    if plain:
        phases.note("depth_read:" + path, "text")
        text = np.frombuffer(buf, dtype=np.uint8)
    else:
        with phases.wall("depth_gz_members"):
            got = _read_depth_members(engine, path, buf, ref_lengths)
        if got is not None:
            return got
        raw = np.frombuffer(buf, dtype=np.uint8)
        del buf
        try:
            with phases.wall("depth_gz_inflate"):
                gz = hostio.GzipText(raw, hostio.pick_threads(1))
        except GciError:
            if plotter_v2:
                return None, {}
            import gzip
            with gzip.open(path, "rb") as f:                 # raises what the reference's read raises (BadGzipFile, EOFError, zlib.error)
                depths = depthfile.parse_depth_lines(f)
            return _checked_upload(engine, depths, ref_lengths)
        del raw
        with phases.wall("depth_gz_export"), gz:                 # (the members' text into one host array; the members freed)
            text = gz.export()
    if plotter_v2 and text.shape[0] == 0:
        return None, {}
    with phases.wall("depth_text_upload"):
        d_text = engine.upload_staged(text) if text.shape[0] >= (256 << 20) else engine.to_device(text)
    with phases.wall("depth_text_parse"):
        d_line0, line0, keys, bad = engine.depth_text_index(d_text)
        found = depthfile.header_segments(text, keys, line0, plotter_v2) if bad == (1 << 64) - 1 else None
        if found is None:
            del d_text, d_line0
            if plotter_v2:
                return None, {}
            import io
            return _checked_upload(engine, depthfile.parse_depth_lines(io.BytesIO(text.tobytes())), ref_lengths)
        names, lengths, segs = found
        targets_length, track = _depth_file_track(engine, names, lengths, ref_lengths)
        if track is None:
            return None, targets_length
        engine.depth_text_parse(d_text, d_line0, segs(engine.offsets), track)
        del d_text, d_line0
    return DepthTracks(engine, targets_length, track), targets_length


def _checked_upload(engine: Engine, depths: Dict[str, np.ndarray], ref_lengths) -> Tuple[Optional[DepthTracks], Dict[str, int]]:
    """The slow path's dict to the device, after the contig check -- and the one thing an int32 track cannot hold refused: a depth
    outside the int32 range (GCI_score.py)."""
    from .formats import depthfile
    targets_length = {t: len(a) for t, a in depths.items()}
    if ref_lengths is not None and any(t not in ref_lengths for t in targets_length):
        return None, targets_length
    for target, arr in depths.items():
        if not isinstance(arr, np.ndarray):
            sys.exit('ERROR!!! A header line of the depth file names the contig "" and is not the last one, which is not supported')
        if arr.size and (int(arr.min()) < depthfile.INT32_MIN or int(arr.max()) > depthfile.INT32_MAX):
            sys.exit(f'ERROR!!! The depth file holds a depth of "{target}" outside the 32-bit range (-2^31 .. 2^31 - 1), which is not supported')
    return _upload_depths(engine, depths)


# ==============================================================================================
# convert_samtools_depth.py: the text of `samtools depth -a` to a .depth.gz (k_sdepth.hip)
# ==============================================================================================

def convert_samtools_depth(engine: Optional[Engine], path: str, prefix: str) -> str:
    """utility/convert_samtools_depth.py for `path` -> `{prefix}.depth.gz`, a multi-member gzip whose payload is the reference's.
    The file is mapped, its text goes to HBM through the staging ring, the device checks the grammar, counts the lines and marks
    the lines where the name changes (gci_sdepth_index), the host turns those into segments -- one per run of a name, in file
    order -- and lays out the track, the device writes the depths (gci_sdepth_parse) and deflates them (Engine.depth_deflate).
    A file larger than GCI_SDEPTH_RESIDENT_MAX bytes (default 64 GiB) goes through in pieces of GCI_SDEPTH_CHUNK_BYTES cut at line
    ends, twice: once to index, once to parse.  Text outside the strict grammar, and an empty file, take the reference's own
    statements on the host (formats.depthfile.convert_samtools_host).  -> the path taken: "device", "device-chunked" or "host"."""
    from .formats import depthfile
    out = f"{prefix}.depth.gz"
    open(out, "wb").close()                                    # (the reference opens its output first: it exists when the input does not)
    n = os.stat(path).st_size if os.path.exists(path) else -1
    if n < 0:
        open(path, "r").close()                                # raises the reference's FileNotFoundError
    taken = "host"
    segs = None
    if n > 0:
        engine = engine if engine is not None else default_engine()
        raw = np.memmap(path, dtype=np.uint8, mode="r")
        resident = n <= int(os.environ.get("GCI_SDEPTH_RESIDENT_MAX", str(64 << 30)))
        pieces = [(0, n, b"")] if resident else depthfile.sdepth_chunks(raw, int(os.environ.get("GCI_SDEPTH_CHUNK_BYTES", str(8 << 30))))

        def upload(a, b):
            with phases.wall("sdepth_text_upload"):
                return engine.upload_staged(raw[a:b]) if b - a >= (256 << 20) else engine.to_device(np.asarray(raw[a:b]))

        with phases.wall("sdepth_index"):
            found, lines_of, keys_of, kept, line_base, valid = [], [], [], None, 0, True
            for a, b, prev in pieces:
                d_text = upload(a, b)
                d_line0, line0, keys, bad = engine.sdepth_index(d_text, prev)
                if bad != (1 << 64) - 1:
                    valid = False
                    break
                found += depthfile.sdepth_segments(raw, keys, line0, a, line_base)
                lines_of.append(int(line0[-1]))
                keys_of.append(int(keys.shape[0]))
                line_base += int(line0[-1])
                kept = (d_text, d_line0) if resident else None
                del d_text, d_line0
        if valid:
            first = np.array([g for _, g in found] + [line_base], dtype=np.int64)
            lengths = np.diff(first)
            if lengths.size and int(lengths.max()) > depthfile.INT32_MAX:
                sys.exit("ERROR!!! A contig of the samtools depth file is longer than 2^31 - 1 bases, which is not supported")
            engine.set_layout(lengths.tolist())
            segs = np.stack([first[:-1], lengths, np.asarray(engine.offsets, dtype=np.int64)], axis=1) if lengths.size else np.zeros((0, 3), np.int64)
            with phases.wall("sdepth_parse"):
                track = engine.T.zeros(max(engine.total, 1), engine.T.int32, engine.device)     # (the padding behind every segment too)
                line_base = 0
                for k, (a, b, prev) in enumerate(pieces):
                    if kept is not None:
                        d_text, d_line0 = kept
                    else:
                        d_text = upload(a, b)
                        d_line0 = engine.sdepth_index(d_text, prev, cap=max(keys_of[k], 1))[0]
                    engine.sdepth_parse(d_text, d_line0, segs, track, line_base)
                    line_base += lines_of[k]
                    del d_text, d_line0
                kept = None
            taken = "device" if resident else "device-chunked"
            with phases.wall("sdepth_deflate"):
                blobs = engine.depth_deflate(track)                # views of the engine's pinned staging buffer
            with phases.wall("depth_gz_write"), open(out, "wb") as f:
                for (name, _), blob in zip(found, blobs):
                    f.write(hostio.gzip_members(b">" + name + b"\n", threads=1))
                    f.write(blob)
        del raw
    if taken == "host":
        with phases.wall("sdepth_host_convert"):
            depthfile.convert_samtools_host(path, out)
    phases.note("convert_samtools_depth_path", taken)
    return taken


# ==============================================================================================
# depth_to_bedgraph.py: a track in HBM as bedGraph lines (k_bedgraph.hip)
# ==============================================================================================

def depth_bedgraph(tracks: DepthTracks, items: Optional[Sequence[Tuple[str, int, int]]] = None, out=None):
    """The bedGraph text of `tracks`: per (target, start, end) of `items` -- end EXCLUSIVE, 0 <= start <= end <= length; None: every
    contig whole, in the track's order --, in the order given, one line `name\\tstart\\tend\\tdepth\\n` per maximal run of equal depth
    inside [start, end), ascending, in 0-based half-open contig coordinates.  A run never crosses an item's edge, an empty item gives
    no line, zero-depth runs are written like any other; no `track` line, no header.  One device round (Engine.bedgraph_runs, then
    Engine.bedgraph_text).  The text goes to the open binary file `out`, or comes back as bytes."""
    tracks._bind()
    if items is None:
        items = [(t, 0, L) for t, L in zip(tracks.targets, tracks.lengths)]
    at = {t: (int(o), int(L)) for t, o, L in zip(tracks.targets, tracks.engine.offsets, tracks.lengths)}
    wins, names, coord0 = [], [], []
    for target, start, end in items:
        o, L = at[target]
        start, end = int(start), int(end)
        if not 0 <= start <= end <= L:
            raise ValueError(f"depth_bedgraph: [{start}, {end}) is not inside {target} (length {L})")
        wins.append((o + start, o + end))
        names.append(target.encode())
        coord0.append(start)
    with phases.wall("bedgraph_runs"):
        held = tracks.engine.bedgraph_runs(tracks.track, wins)
    with phases.wall("bedgraph_text"):
        text, _ = tracks.engine.bedgraph_text(held, names, coord0)
    del held
    if out is None:
        return bytes(text)
    with phases.wall("bedgraph_write_file"):
        out.write(text)
    return None


# ==============================================================================================
# depth_dist.py: the depth histogram and the statistics of a track in HBM (k_hist.hip)
# ==============================================================================================

DIST_HIST_BUDGET = 256 << 20          # bytes of histogram (items x (n_bins + 2) x 8) one device round may hold; more items: more rounds


def _dist_batches(n_items: int, cols: int):
    per = max(1, DIST_HIST_BUDGET // (cols * 8))
    return [(a, min(n_items, a + per)) for a in range(0, n_items, per)]


def depth_distribution(tracks: DepthTracks, items: Optional[Sequence[Tuple[str, int, int]]] = None, max_depth: int = 65535
                       ) -> Tuple[np.ndarray, np.ndarray]:
    """The depth distribution of `tracks` per (target, start, end) of `items` -- as in depth_bedgraph: end EXCLUSIVE, None: every contig
    whole -> (hist uint64 [n, n_bins + 2], stats int64 [n, 4]) as Engine.depth_hist gives them: column d < n_bins the bases of depth d,
    column n_bins those of depth >= n_bins, column n_bins + 1 those of depth < 0; sum, min, max, bases.  Two device rounds: a
    statistics-only one for the largest depth, then the histogram with n_bins = min(largest max + 1, max_depth + 1) (1 if every item
    is empty).  A round's items go in batches whose histogram stays under DIST_HIST_BUDGET bytes.  No formatting here."""
    if not 0 <= int(max_depth) < _lib.HIST_MAX_BINS:
        raise ValueError(f"depth_distribution: max_depth {max_depth} is not in [0, {_lib.HIST_MAX_BINS - 1}]")
    tracks._bind()
    if items is None:
        items = [(t, 0, L) for t, L in zip(tracks.targets, tracks.lengths)]
    at = {t: (int(o), int(L)) for t, o, L in zip(tracks.targets, tracks.engine.offsets, tracks.lengths)}
    wins = []
    for target, start, end in items:
        o, L = at[target]
        start, end = int(start), int(end)
        if not 0 <= start <= end <= L:
            raise ValueError(f"depth_distribution: [{start}, {end}) is not inside {target} (length {L})")
        wins.append((o + start, o + end))
    n = len(wins)
    with phases.wall("dist_stats"):
        stats = [tracks.engine.depth_hist(tracks.track, wins[a:b], 0)[1] for a, b in _dist_batches(n, 2)]
    stats = np.concatenate(stats) if stats else np.zeros((0, 4), dtype=np.int64)
    full = stats[:, 3] > 0
    n_bins = max(1, min(int(stats[full, 2].max()) + 1, int(max_depth) + 1)) if full.any() else 1
    with phases.wall("dist_hist"):
        parts = [tracks.engine.depth_hist(tracks.track, wins[a:b], n_bins) for a, b in _dist_batches(n, n_bins + 2)]
    if not parts:
        return np.zeros((0, n_bins + 2), dtype=np.uint64), stats
    return np.concatenate([h for h, _ in parts]), np.concatenate([s for _, s in parts])
