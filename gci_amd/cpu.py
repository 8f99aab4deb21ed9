"""libgci_cpu.so: the function seams of include/gci_hip.h on host memory and host threads (gci_amd/csrc/cpu/gci_cpu.cpp),
bound with ctypes over NumPy arrays.

What it is for: the CPU baseline behind the same C-ABI (bench.py: `cpu_baseline.kind = "libgci_cpu"`, every core of the
host) and running the seam tests without a GPU (tests/test_cpu_seams.py holds it against the oracle).  It is NOT a fall-back
of the product: gci_amd.pipeline / gci_amd.cli / GCI.py never import this module -- without an MI355X they refuse.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from ctypes import c_char_p, c_int, c_uint32, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib                         # (prototypes and structs alone: importing it loads no library)
from ._lib import JoinFile as _JoinFile, Window as _Window

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "cpu", "gci_cpu.cpp")
LIB_PATH = os.path.join(_HERE, "csrc", "libgci_cpu.so")

REC_DTYPE = np.dtype([("name_hash", "<u8"), ("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("qlen", "<i4"),
                      ("rec_idx", "<u4"), ("mapq", "u1"), ("flags", "u1"), ("name_len", "<u2")])
IVL_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("pad", "<i4")])
RUN_DTYPE = np.dtype([("start", "<u4"), ("depth", "<i4")])          # gci_depth_run
SITE_DTYPE = np.dtype([("contig", "<i4"), ("pos", "<i4"), ("left", "<i4"), ("right", "<i4"), ("depth", "<i4"), ("pad", "<i4")])      # gci_clip_site
INDEL_SITE_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("del", "<i4"), ("ins", "<i4"), ("depth", "<i4")])      # gci_indel_site
MISMATCH_SITE_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("mismatch", "<i4"), ("depth", "<i4")])      # gci_mismatch_site
ALLELE_SITE_DTYPE = np.dtype([("contig", "<i4"), ("pos", "<i4"), ("ref", "<i4"), ("alt", "<i4"), ("n", "<i4", (4,)), ("depth", "<i4")])      # gci_allele_site
GCI_TILE = 4096


class CpuError(RuntimeError):
    def __init__(self, status: int, msg: str, rec: int = -1):
        super().__init__(msg)
        self.status, self.rec = status, rec


# the seam set: the argument lists are those of gci_amd/_lib.py (include/gci_hip.h), looked up by name; + gci_cpu_option
_SEAMS = """gci_abi_version gci_ctx_create gci_ctx_destroy gci_sync gci_strerror gci_last_error gci_malloc gci_free gci_memcpy_h2d
gci_memcpy_d2h gci_memset gci_layout_set gci_layout_total gci_layout_offsets gci_name_hash gci_decode_status gci_bam_filter gci_name_join
gci_depth_build gci_gap_mask gci_max2 gci_issue_scan gci_issue_scan_windows gci_depth_classes gci_depth_text_size gci_depth_text_write
gci_depth_sum gci_range_sums gci_depth_deflate_from_build gci_depth_deflate_size gci_depth_deflate_write gci_depth_text_index
gci_depth_text_parse gci_sdepth_index gci_sdepth_parse gci_depth_gz_scan gci_depth_gz_runs gci_depth_gz_expand gci_depth_runs_count
gci_depth_runs_write gci_bedgraph_size gci_bedgraph_write gci_depth_hist gci_bam_cover_size gci_bam_cover_write gci_track_add
gci_bam_fate gci_bam_cover_size_sel gci_name_join_fate gci_fate_refine gci_bam_reads_size gci_bam_reads_write gci_bam_sweep gci_bam_clip_size gci_bam_clip_write gci_clip_sites_size gci_clip_sites_write
gci_bam_indel_size gci_bam_indel_write gci_indel_sites_size gci_indel_sites_write
gci_fasta_codes gci_bam_mismatch_size gci_bam_mismatch_write gci_mismatch_sites_size gci_mismatch_sites_write
gci_bam_allele_size gci_bam_allele_write gci_allele_sites_size gci_allele_sites_write""".split()
_PROTO = {name: (name, res, args) for name, res, args in _lib.EXPORTS}
EXPORTS = [_PROTO[name] for name in _SEAMS] + [("gci_cpu_option", c_int, [c_void_p, c_char_p, c_int])]


def needs_build() -> bool:
    return not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(
        os.path.getmtime(p) for p in (SRC, os.path.join(_HERE, "csrc", "gci_common.h"), os.path.join(_HERE, "..", "include", "gci_hip.h")))


def build(force: bool = False) -> str:
    """g++ over the one source file: include/gci_hip.h a second time."""
    if force or needs_build():
        subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", "-fno-fast-math", "-ffp-contract=off", "-Wall", "-o", LIB_PATH, SRC], check=True)
    return LIB_PATH


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        if needs_build():
            build()
        lib = ctypes.CDLL(LIB_PATH)
        for name, res, args in EXPORTS:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _LIB = lib
    return _LIB


def _p(a: Optional[np.ndarray]):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class CpuEngine:
    """The seam calls over NumPy arrays (host memory is this library's "device" memory)."""

    def __init__(self, threads: Optional[int] = None):
        self.lib = load()
        h = c_void_p()
        self._chk(self.lib.gci_ctx_create(0, None, 0, ctypes.byref(h)), "gci_ctx_create")
        self.ctx = h
        if threads:
            self.lib.gci_cpu_option(self.ctx, b"threads", int(threads))
        self.lengths: List[int] = []
        self.offsets = np.zeros(0, dtype=np.int64)
        self.total = 0

    def close(self):
        if self.ctx:
            self.lib.gci_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def threads(self) -> int:
        return int(self.lib.gci_cpu_option(self.ctx, b"threads", 0))

    def heads(self, on: bool):
        """gci_bam_filter over a heads stream (records without SEQ / QUAL) from now on."""
        self.lib.gci_cpu_option(self.ctx, b"heads", 1 if on else 0)

    def _chk(self, st: int, what: str):
        if st != 0:
            raise CpuError(st, "%s: %s" % (what, self.lib.gci_strerror(st).decode()))

    def _status(self, word: np.ndarray, what: str):
        rec = c_uint32()
        st = self.lib.gci_decode_status(int(word[0]), ctypes.byref(rec))
        if st != 0:
            raise CpuError(st, "%s: %s at record %d" % (what, self.lib.gci_strerror(st).decode(), rec.value), rec.value)

    def set_layout(self, lengths: Sequence[int]):
        self.lengths = [int(l) for l in lengths]
        a = np.asarray(self.lengths, dtype=np.int64)
        self._chk(self.lib.gci_layout_set(self.ctx, len(self.lengths), _p(a)), "gci_layout_set")
        self.total = int(self.lib.gci_layout_total(self.ctx))
        self.offsets = np.zeros(len(self.lengths), dtype=np.int64)
        self._chk(self.lib.gci_layout_offsets(self.ctx, _p(self.offsets)), "gci_layout_offsets")

    def new_track(self) -> np.ndarray:
        return np.zeros(self.total, dtype=np.int32)

    def contig(self, track: np.ndarray, c: int) -> np.ndarray:
        o = int(self.offsets[c])
        return track[o:o + self.lengths[c]]

    # ---- R1
    def bam_filter(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, mq: int, cut: int, cp: float, ip: float,
                   rec_idx_base: int = 0, check: bool = True) -> np.ndarray:
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        out = np.zeros(offs.shape[0], dtype=REC_DTYPE)
        self.last_status = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_bam_filter(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], _p(ref_sel), ref_sel.shape[0], mq, cut, cp, ip,
                                          rec_idx_base, _p(out), _p(self.last_status)), "gci_bam_filter")
        if check:
            self._status(self.last_status, "gci_bam_filter")
        return out

    # ---- bam_depth.py (k_cover.hip's twins)
    def bam_cover(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, has_seq: bool = True, excl_flags: int = 0x704,
                  min_mapq: int = 0, count_del: bool = False, check: bool = True, cap: Optional[int] = None,
                  classes: Optional[np.ndarray] = None, mask: int = 0) -> np.ndarray:
        """device.Engine.bam_cover's twin: the covered reference bases of every record as IVL_DTYPE (`end` = the last covered base).
        cap: the room offered to the write call (default: what the size call asked for).  classes (bam_fate's bytes) and mask: only the
        records whose class is a bit of the mask (gci_bam_cover_size_sel)."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        n = ctypes.c_uint64(0)
        self.last_status = np.zeros(1, dtype=np.uint64)
        head = (self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(ref_sel), ref_sel.shape[0], int(excl_flags),
                int(min_mapq), int(count_del))
        if classes is None:
            self._chk(self.lib.gci_bam_cover_size(*head, ctypes.byref(n), _p(self.last_status)), "gci_bam_cover_size")
        else:
            classes = np.ascontiguousarray(classes, dtype=np.uint8)
            self._chk(self.lib.gci_bam_cover_size_sel(*head, _p(classes), int(mask), ctypes.byref(n), _p(self.last_status)), "gci_bam_cover_size_sel")
        if check:
            self._status(self.last_status, "gci_bam_cover_size")
        room = int(n.value) if cap is None else int(cap)
        out = np.zeros(max(room, 1), dtype=IVL_DTYPE)
        self._chk(self.lib.gci_bam_cover_write(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(out), room,
                                               _p(self.last_status)), "gci_bam_cover_write")
        return out[:int(n.value)]

    def bam_fate(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, map_qual: int, clip_percent: float, iden_percent: float,
                 has_seq: bool = True, check: bool = True):
        """device.Engine.bam_fate's twin -> (class byte per record, records per class)."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        cls = np.zeros(max(offs.shape[0], 1), dtype=np.uint8)
        counts = np.zeros(_lib.FATE_CLASSES, dtype=np.uint64)
        self.last_status = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_bam_fate(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(ref_sel), ref_sel.shape[0],
                                        int(map_qual), float(clip_percent), float(iden_percent), _p(cls), _p(counts), _p(self.last_status)),
                  "gci_bam_fate")
        if check:
            self._status(self.last_status, "gci_bam_fate")
        return cls[:offs.shape[0]], counts

    def bam_reads(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, classes: np.ndarray, mask: int, names: Sequence[bytes],
                  win: Optional[np.ndarray] = None, win0: Optional[np.ndarray] = None, file_no: int = 1, has_seq: bool = True,
                  check: bool = True, cap: Optional[int] = None, guard: int = 0) -> Tuple[bytes, int]:
        """device.Engine.bam_reads's twin -> (the rows of the records whose class is a bit of the mask and that overlap a window, the
        number of rows).  names: the selected contigs' names; win int64 [n, 2] and win0 uint32 [n_sel + 1] as pipeline.merge_windows
        makes them (None: no window test).  cap: the room offered to the write call; guard: bytes of 0xA5 behind it that must stay."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        classes = np.ascontiguousarray(classes, dtype=np.uint8)
        if win0 is not None:
            win, win0 = np.ascontiguousarray(win, dtype=np.int64).reshape(-1, 2), np.ascontiguousarray(win0, dtype=np.uint32)
        blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        name_len = np.asarray([len(x) for x in names], dtype=np.uint32)
        name_off = np.concatenate(([0], np.cumsum(name_len[:-1], dtype=np.uint64))).astype(np.uint64)
        rows, size = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.last_status = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_bam_reads_size(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(ref_sel), ref_sel.shape[0],
                                              _p(classes), int(mask), _p(win) if win0 is not None else None, _p(win0), _p(name_len), int(file_no),
                                              ctypes.byref(rows), ctypes.byref(size), _p(self.last_status)), "gci_bam_reads_size")
        if check:
            self._status(self.last_status, "gci_bam_reads_size")
        room = int(size.value) if cap is None else int(cap)
        out = np.full(room + guard + 1, 0xA5, dtype=np.uint8)
        self._chk(self.lib.gci_bam_reads_write(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], _p(blob), _p(name_off), _p(name_len),
                                               _p(out), room), "gci_bam_reads_write")
        if (out[int(size.value):] != 0xA5).any():
            raise CpuError(-1, "gci_bam_reads_write wrote behind its rows")
        return out[:int(size.value)].tobytes(), int(rows.value)

    def bam_sweep(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, map_qual: int, clip_percent: float, iden_percent: float,
                  digits: int = 3, win: Optional[np.ndarray] = None, win0: Optional[np.ndarray] = None, has_seq: bool = True, check: bool = True,
                  guard: int = 0) -> np.ndarray:
        """device.Engine.bam_sweep's twin -> the table uint64 [GCI_SWEEP_ROWS(digits), 4]; win / win0 as for bam_reads.  guard: entries
        of a pattern behind the table that must stay (the table itself is pre-filled with it)."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        if win0 is not None:
            win, win0 = np.ascontiguousarray(win, dtype=np.int64).reshape(-1, 2), np.ascontiguousarray(win0, dtype=np.uint32)
        cells = _lib.SWEEP_COLS * _lib.SweepRows(digits).rows
        table = np.full(cells + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        self.last_status = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_bam_sweep(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(ref_sel), ref_sel.shape[0],
                                         _p(win) if win0 is not None else None, _p(win0), int(map_qual), float(clip_percent), float(iden_percent),
                                         int(digits), _p(table), _p(self.last_status)), "gci_bam_sweep")
        if (table[cells:] != 0xA5A5A5A5A5A5A5A5).any():
            raise CpuError(-1, "gci_bam_sweep wrote behind its table")
        if check:
            self._status(self.last_status, "gci_bam_sweep")
        return table[:cells].reshape(-1, _lib.SWEEP_COLS)

    # ---- clip_sites.py (k_clips.hip's twins)
    def bam_clip(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, has_seq: bool = True, excl_flags: int = 0x704, min_mapq: int = 0,
                 min_clip: int = 100, check: bool = True, cap: Optional[int] = None, guard: int = 0):
        """device.Engine.bam_clip's twin -> (the left events, the right events as IVL_DTYPE, [records counted, left events, right events]).
        cap: the room offered to the write call (default: what the size call asked for); guard: entries of a pattern behind it that must
        stay (the buffer itself is pre-filled with it)."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        counts = np.zeros(3, dtype=np.uint64)
        self.last_status = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_bam_clip_size(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(ref_sel), ref_sel.shape[0],
                                             int(excl_flags), int(min_mapq), int(min_clip), _p(counts), _p(self.last_status)), "gci_bam_clip_size")
        if check:
            self._status(self.last_status, "gci_bam_clip_size")
        n_left, n_right = int(counts[1]), int(counts[2])
        room = n_left + n_right if cap is None else int(cap)
        out = np.full((max(room, n_left + n_right) + guard + 1, 4), -0x5A5A5A5B, dtype=np.int32)
        self.last_out = out
        self._chk(self.lib.gci_bam_clip_write(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(out), room,
                                              _p(self.last_status)), "gci_bam_clip_write")
        if (out[n_left + n_right:] != -0x5A5A5A5B).any():
            raise CpuError(-1, "gci_bam_clip_write wrote behind its events")
        ivl = out.view(IVL_DTYPE).reshape(-1)
        return ivl[:n_left], ivl[n_left:n_left + n_right], [int(c) for c in counts]

    def clip_sites(self, left: np.ndarray, right: np.ndarray, depth: Optional[np.ndarray], min_reads: int,
                   windows: Sequence[Tuple[int, int]] = (), cap: Optional[int] = None) -> np.ndarray:
        """device.Engine.clip_sites's twin -> SITE_DTYPE [n].  cap: the room offered to the write call."""
        nw = len(windows)
        w = (_Window * max(nw, 1))()
        for i, (a, b) in enumerate(windows):
            w[i].begin, w[i].end = int(a), int(b)
        n = ctypes.c_uint64(0)
        head = (self.ctx, _p(left), _p(right), _p(depth), int(min_reads), w, nw)
        self._chk(self.lib.gci_clip_sites_size(*head, ctypes.byref(n)), "gci_clip_sites_size")
        total = int(n.value)
        room = total if cap is None else int(cap)
        out = np.full((max(room, total) + 1, 6), -0x5A5A5A5B, dtype=np.int32)
        self.last_out = out
        self._chk(self.lib.gci_clip_sites_write(*head, _p(out), room), "gci_clip_sites_write")
        if (out[total:] != -0x5A5A5A5B).any():
            raise CpuError(-1, "gci_clip_sites_write wrote behind its sites")
        return out.view(SITE_DTYPE).reshape(-1)[:total]

    # ---- indel_sites.py (k_indels.hip's twins)
    def bam_indel(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, has_seq: bool = True, excl_flags: int = 0x704, min_mapq: int = 0,
                  min_len: int = 50, check: bool = True, cap: Optional[int] = None, guard: int = 0):
        """device.Engine.bam_indel's twin -> (the deletions, the insertions as IVL_DTYPE, [records counted, deletions, insertions]).
        cap: the room offered to the write call (default: what the size call asked for); guard: entries of a pattern behind it that must
        stay (the buffer itself is pre-filled with it)."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        counts = np.zeros(3, dtype=np.uint64)
        self.last_status = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_bam_indel_size(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(ref_sel), ref_sel.shape[0],
                                              int(excl_flags), int(min_mapq), int(min_len), _p(counts), _p(self.last_status)), "gci_bam_indel_size")
        if check:
            self._status(self.last_status, "gci_bam_indel_size")
        n_del, n_ins = int(counts[1]), int(counts[2])
        room = n_del + n_ins if cap is None else int(cap)
        out = np.full((max(room, n_del + n_ins) + guard + 1, 4), -0x5A5A5A5B, dtype=np.int32)
        self.last_out = out
        self._chk(self.lib.gci_bam_indel_write(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(out), room,
                                               _p(self.last_status)), "gci_bam_indel_write")
        if (out[n_del + n_ins:] != -0x5A5A5A5B).any():
            raise CpuError(-1, "gci_bam_indel_write wrote behind its events")
        ivl = out.view(IVL_DTYPE).reshape(-1)
        return ivl[:n_del], ivl[n_del:n_del + n_ins], [int(c) for c in counts]

    def indel_sites(self, dele: np.ndarray, ins: np.ndarray, depth: Optional[np.ndarray], min_reads: int,
                    windows: Sequence[Tuple[int, int]] = (), cap: Optional[int] = None) -> np.ndarray:
        """device.Engine.indel_sites's twin -> INDEL_SITE_DTYPE [n].  cap: the room offered to the write call."""
        nw = len(windows)
        w = (_Window * max(nw, 1))()
        for i, (a, b) in enumerate(windows):
            w[i].begin, w[i].end = int(a), int(b)
        n = ctypes.c_uint64(0)
        head = (self.ctx, _p(dele), _p(ins), _p(depth), int(min_reads), w, nw)
        self._chk(self.lib.gci_indel_sites_size(*head, ctypes.byref(n)), "gci_indel_sites_size")
        total = int(n.value)
        room = total if cap is None else int(cap)
        out = np.full((max(room, total) + 1, 6), -0x5A5A5A5B, dtype=np.int32)
        self.last_out = out
        self._chk(self.lib.gci_indel_sites_write(*head, _p(out), room), "gci_indel_sites_write")
        if (out[total:] != -0x5A5A5A5B).any():
            raise CpuError(-1, "gci_indel_sites_write wrote behind its sites")
        return out.view(INDEL_SITE_DTYPE).reshape(-1)[:total]

    # ---- mismatch_sites.py (k_mismatch.hip's twins)
    def fasta_codes(self, text: np.ndarray, bodies: np.ndarray, dst: np.ndarray, codes: Optional[np.ndarray] = None,
                    before_codes=None) -> Tuple[np.ndarray, np.ndarray]:
        """device.Engine.fasta_codes's twin -> (the uint8 code array of the layout, the uint32 sequence-byte count of every 4096-byte tile).
        codes: the array to write into (default: a new one filled with 15)."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        n = text.shape[0]
        if text.ctypes.data & 15:                                              # (the call wants the text 16-byte aligned)
            room = np.zeros(n + 16, dtype=np.uint8)
            shift = (-room.ctypes.data) & 15
            room[shift:shift + n] = text
            text = room[shift:shift + n]
        bodies = np.ascontiguousarray(bodies, dtype=np.int64).reshape(-1, 2)
        dst = np.ascontiguousarray(dst, dtype=np.int64)
        seq = np.zeros(n + 1, dtype=np.int64)                                  # gci_fasta_n_scan's tile counts: in a body, not dropped
        for a, b in bodies.tolist():
            seq[a] += 1
            seq[min(b, n)] -= 1
        is_seq = (np.cumsum(seq[:n]) > 0) & (text != 10) & (text != 13) & (text != 32)
        kept = np.add.reduceat(is_seq.astype(np.uint32), np.arange(0, n, 4096)).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
        kept0 = np.concatenate(([0], np.cumsum(kept, dtype=np.uint64))).astype(np.uint64)
        if before_codes is not None:
            before_codes(kept)
        if codes is None:
            codes = np.full(max(self.total, 1), 15, dtype=np.uint8)
        self._chk(self.lib.gci_fasta_codes(self.ctx, _p(text), n, _p(bodies), bodies.shape[0], _p(dst), _p(kept0), _p(codes)), "gci_fasta_codes")
        return codes, kept

    def sync(self) -> None:
        pass

    def bam_mismatch(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, codes: np.ndarray, has_seq: bool = True, excl_flags: int = 0x704,
                     min_mapq: int = 0, check: bool = True, cap: Optional[int] = None, guard: int = 0):
        """device.Engine.bam_mismatch's twin -> (the events as IVL_DTYPE, [records counted, mismatches, pairs compared]).  cap, guard: as
        bam_indel takes them."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        counts = np.zeros(3, dtype=np.uint64)
        self.last_status = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_bam_mismatch_size(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(ref_sel),
                                                 ref_sel.shape[0], int(excl_flags), int(min_mapq), _p(codes), _p(counts), _p(self.last_status)),
                  "gci_bam_mismatch_size")
        if check:
            self._status(self.last_status, "gci_bam_mismatch_size")
        n = int(counts[1])
        room = n if cap is None else int(cap)
        out = np.full((max(room, n) + guard + 1, 4), -0x5A5A5A5B, dtype=np.int32)
        self.last_out = out
        self._chk(self.lib.gci_bam_mismatch_write(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(codes), _p(out),
                                                  room, _p(self.last_status)), "gci_bam_mismatch_write")
        if (out[n:] != -0x5A5A5A5B).any():
            raise CpuError(-1, "gci_bam_mismatch_write wrote behind its events")
        return out.view(IVL_DTYPE).reshape(-1)[:n], [int(c) for c in counts]

    def mismatch_sites(self, mismatch: np.ndarray, depth: np.ndarray, min_reads: int, frac_ppm: int, windows: Sequence[Tuple[int, int]] = (),
                       cap: Optional[int] = None) -> np.ndarray:
        """device.Engine.mismatch_sites's twin -> MISMATCH_SITE_DTYPE [n].  cap: the room offered to the write call."""
        nw = len(windows)
        w = (_Window * max(nw, 1))()
        for i, (a, b) in enumerate(windows):
            w[i].begin, w[i].end = int(a), int(b)
        n = ctypes.c_uint64(0)
        head = (self.ctx, _p(mismatch), _p(depth), int(min_reads), int(frac_ppm), w, nw)
        self._chk(self.lib.gci_mismatch_sites_size(*head, ctypes.byref(n)), "gci_mismatch_sites_size")
        total = int(n.value)
        room = total if cap is None else int(cap)
        out = np.full((max(room, total) + 1, 5), -0x5A5A5A5B, dtype=np.int32)
        self.last_out = out
        self._chk(self.lib.gci_mismatch_sites_write(*head, _p(out), room), "gci_mismatch_sites_write")
        if (out[total:] != -0x5A5A5A5B).any():
            raise CpuError(-1, "gci_mismatch_sites_write wrote behind its sites")
        return out.view(MISMATCH_SITE_DTYPE).reshape(-1)[:total]

    # ---- allele_sites.py (the twins of k_mismatch.hip's allele calls)
    def bam_allele(self, stream: np.ndarray, offs: np.ndarray, ref_sel: np.ndarray, codes: np.ndarray, has_seq: bool = True, excl_flags: int = 0x704,
                   min_mapq: int = 0, check: bool = True, cap: Optional[int] = None, guard: int = 0):
        """device.Engine.bam_allele's twin -> (the A, C, G, T events as IVL_DTYPE, [records counted, A, C, G, T events, pairs compared]).
        cap, guard: as bam_indel takes them."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        ref_sel = np.ascontiguousarray(ref_sel, dtype=np.int32)
        counts = np.zeros(6, dtype=np.uint64)
        self.last_status = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_bam_allele_size(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(ref_sel),
                                               ref_sel.shape[0], int(excl_flags), int(min_mapq), _p(codes), _p(counts), _p(self.last_status)),
                  "gci_bam_allele_size")
        if check:
            self._status(self.last_status, "gci_bam_allele_size")
        ends = np.cumsum([0] + [int(c) for c in counts[1:5]]).tolist()
        n = ends[4]
        room = n if cap is None else int(cap)
        out = np.full((max(room, n) + guard + 1, 4), -0x5A5A5A5B, dtype=np.int32)
        self.last_out = out
        self._chk(self.lib.gci_bam_allele_write(self.ctx, _p(stream), stream.shape[0], _p(offs), offs.shape[0], int(has_seq), _p(codes), _p(out),
                                                room, _p(self.last_status)), "gci_bam_allele_write")
        if (out[n:] != -0x5A5A5A5B).any():
            raise CpuError(-1, "gci_bam_allele_write wrote behind its events")
        ivl = out.view(IVL_DTYPE).reshape(-1)
        return (*(ivl[ends[k]:ends[k + 1]] for k in range(4)), [int(c) for c in counts])

    def allele_sites(self, a: np.ndarray, c: np.ndarray, g: np.ndarray, t: np.ndarray, depth: np.ndarray, codes: np.ndarray, min_reads: int,
                     frac_ppm: int, windows: Sequence[Tuple[int, int]] = (), cap: Optional[int] = None) -> np.ndarray:
        """device.Engine.allele_sites's twin -> ALLELE_SITE_DTYPE [n].  cap: the room offered to the write call."""
        nw = len(windows)
        w = (_Window * max(nw, 1))()
        for i, (lo, hi) in enumerate(windows):
            w[i].begin, w[i].end = int(lo), int(hi)
        n = ctypes.c_uint64(0)
        head = (self.ctx, _p(a), _p(c), _p(g), _p(t), _p(depth), _p(codes), int(min_reads), int(frac_ppm), w, nw)
        self._chk(self.lib.gci_allele_sites_size(*head, ctypes.byref(n)), "gci_allele_sites_size")
        total = int(n.value)
        room = total if cap is None else int(cap)
        out = np.full((max(room, total) + 1, 9), -0x5A5A5A5B, dtype=np.int32)
        self.last_out = out
        self._chk(self.lib.gci_allele_sites_write(*head, _p(out), room), "gci_allele_sites_write")
        if (out[total:] != -0x5A5A5A5B).any():
            raise CpuError(-1, "gci_allele_sites_write wrote behind its sites")
        return out.view(ALLELE_SITE_DTYPE).reshape(-1)[:total]

    def track_add(self, acc: np.ndarray, add: np.ndarray) -> np.ndarray:
        self._chk(self.lib.gci_track_add(self.ctx, _p(acc), _p(add)), "gci_track_add")
        return acc

    # ---- R5
    def name_join(self, files: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray, int]], ovlp: float,
                  contig_map: Optional[np.ndarray] = None) -> np.ndarray:
        """files: (records, name base bytes, name offsets by record position, name_delta) in reference order -> intervals."""
        arr = (_JoinFile * len(files))()
        keep = []
        cap = 0
        for k, (recs, base, off, delta) in enumerate(files):
            recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
            base = np.ascontiguousarray(base, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            keep += [recs, base, off]
            arr[k] = _JoinFile(recs.ctypes.data, recs.shape[0], int(delta), base.ctypes.data, off.ctypes.data)
            cap += int(recs.shape[0])
        out = np.zeros(max(cap, 1), dtype=IVL_DTYPE)
        n = np.zeros(1, dtype=np.uint32)
        st = np.zeros(1, dtype=np.uint64)
        cm = None if contig_map is None else np.ascontiguousarray(contig_map, dtype=np.int32)
        self._chk(self.lib.gci_name_join(self.ctx, arr, len(files), ovlp, _p(cm), _p(out), out.shape[0], _p(n), _p(st)), "gci_name_join")
        self._status(st, "gci_name_join")
        return out[:int(n[0])]

    def name_join_fate(self, files: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray, int]], ovlp: float, guard: int = 0):
        """device.Engine.name_join_fate's twin; files as for name_join -> (per file the byte of every record, followed by `guard`
        bytes of 0xA5 the call must leave alone; uint64 [n, JOIN_FATE_CLASSES] records per file and byte; the status word)."""
        arr = (_JoinFile * len(files))()
        keep, fate = [], []
        for k, (recs, base, off, delta) in enumerate(files):
            recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
            base = np.ascontiguousarray(base, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            keep += [recs, base, off]
            arr[k] = _JoinFile(recs.ctypes.data, recs.shape[0], int(delta), base.ctypes.data, off.ctypes.data)
            fate.append(np.full(recs.shape[0] + guard, 0xA5, dtype=np.uint8))
        ptrs = (c_void_p * len(files))(*[f.ctypes.data for f in fate])
        counts = np.full((len(files) + 1, _lib.JOIN_FATE_CLASSES), 7, dtype=np.uint64)       # (one row more than the call may write)
        st = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.gci_name_join_fate(self.ctx, arr, len(files), float(ovlp), ptrs, _p(counts), _p(st)), "gci_name_join_fate")
        if (counts[-1] != 7).any():
            raise CpuError(-1, "gci_name_join_fate wrote behind its counts")
        return fate, counts[:-1], int(st[0])

    def fate_refine(self, classes: np.ndarray, join_fate: np.ndarray) -> int:
        """gci_fate_refine over `classes` in place -> the status word."""
        st = np.zeros(1, dtype=np.uint64)
        n = min(classes.shape[0], join_fate.shape[0])
        self._chk(self.lib.gci_fate_refine(self.ctx, _p(classes), _p(join_fate), n, _p(st)), "gci_fate_refine")
        return int(st[0])

    # ---- R6, R8, R9
    def depth_build(self, ivl: np.ndarray, flank: int, track: Optional[np.ndarray] = None) -> np.ndarray:
        ivl = np.ascontiguousarray(ivl, dtype=IVL_DTYPE)
        track = self.new_track() if track is None else track
        self._chk(self.lib.gci_depth_build(self.ctx, _p(ivl), None, ivl.shape[0], flank, _p(track)), "gci_depth_build")
        return track

    def gap_mask(self, track: np.ndarray, gaps: Sequence[Tuple[int, int, int]]):
        g = np.zeros(len(gaps), dtype=IVL_DTYPE)
        for k, (c, a, b) in enumerate(gaps):
            g[k] = (c, a, b, 0)
        self._chk(self.lib.gci_gap_mask(self.ctx, _p(track), _p(g), g.shape[0]), "gci_gap_mask")

    def max2(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        out = self.new_track()
        self._chk(self.lib.gci_max2(self.ctx, _p(a), _p(b), _p(out)), "gci_max2")
        return out

    # ---- R10
    @staticmethod
    def _scan_keys(call, n_arrays: int = 1) -> List[np.ndarray]:
        """call(keys, cap, counters) until every key fitted (n_arrays key arrays of `cap` keys back to back, one counter each), the
        buffer grown to what the counters ask for -> the sorted keys of every array."""
        cap = 1 << 12
        while True:
            keys = np.zeros(n_arrays * cap, dtype=np.uint64)
            n = np.zeros(n_arrays, dtype=np.uint32)
            call(keys, cap, n)
            if int(n.max()) <= cap:
                return [np.sort(keys[x * cap:x * cap + int(n[x])]) for x in range(n_arrays)]
            cap = int(n.max())

    def issue_keys(self, track: np.ndarray, lo: float, hi: float, flank: int, windows: Optional[Sequence[Tuple[int, int]]] = None) -> np.ndarray:
        def call(keys, cap, n):
            if windows is None:
                self._chk(self.lib.gci_issue_scan(self.ctx, _p(track), lo, hi, flank, _p(keys), cap, _p(n)), "gci_issue_scan")
            else:
                w = (_Window * len(windows))(*[_Window(int(a), int(b)) for a, b in windows])
                self._chk(self.lib.gci_issue_scan_windows(self.ctx, _p(track), w, len(windows), lo, hi, _p(keys), cap, _p(n)), "gci_issue_scan_windows")
        return self._scan_keys(call)[0]

    def issue_runs(self, track: np.ndarray, lo: float, hi: float, flank: int, n_windows: Optional[int] = None,
                   windows: Optional[Sequence[Tuple[int, int]]] = None) -> List[List[Tuple[int, int]]]:
        """Sorted keys -> per window the runs (start, end) relative to the window's beginning."""
        keys = self.issue_keys(track, lo, hi, flank, windows)
        nw = len(self.lengths) if windows is None else len(windows)
        runs: List[List[Tuple[int, int]]] = [[] for _ in range(nw)]
        for k in range(0, keys.shape[0], 2):
            a, b = int(keys[k]), int(keys[k + 1])
            assert (a >> 33) == (b >> 33) and not (a & 1) and (b & 1)
            runs[a >> 33].append(((a >> 1) & 0xFFFFFFFF, (b >> 1) & 0xFFFFFFFF))
        return runs

    def depth_classes(self, track: np.ndarray, windows: Sequence[Tuple[int, int]], low_below: int = 5
                      ) -> Tuple[List[np.ndarray], List[np.ndarray], np.ndarray]:
        """gci_depth_classes (device.Engine.depth_classes' twin): per window the runs of depth 0 and of 0 < depth < low_below as int64
        [k, 2] of (start, exclusive end) relative to the window's beginning, and int64 [n, 2] of (sum, count) of the depths > 0."""
        nw = len(windows)
        w = (_Window * max(nw, 1))(*[_Window(int(a), int(b)) for a, b in windows])
        stats = np.zeros((nw, 2), dtype=np.int64)

        def call(keys, cap, n):
            self._chk(self.lib.gci_depth_classes(self.ctx, _p(track), w, nw, int(low_below), _p(keys), cap, _p(n), _p(stats)), "gci_depth_classes")
        out = []
        for k in self._scan_keys(call, 2):
            if (k.shape[0] & 1) or (k[0::2] & np.uint64(1)).any() or not (k[1::2] & np.uint64(1)).all():
                raise CpuError(-1, "gci_depth_classes produced unpaired run boundaries")
            win = (k >> np.uint64(33)).astype(np.int64)
            rel = ((k >> np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
            bounds = np.searchsorted(win, np.arange(nw + 1))
            out.append([np.stack([rel[a:b:2], rel[a + 1:b:2]], axis=1) for a, b in zip(bounds[:-1], bounds[1:])])
        return out[0], out[1], stats

    # ---- depth_to_bedgraph.py (k_bedgraph.hip's twins)
    def _depth_runs(self, track: np.ndarray, w, nw: int) -> Tuple[np.ndarray, np.ndarray]:
        run0 = np.zeros(nw + 1, dtype=np.uint64)
        self._chk(self.lib.gci_depth_runs_count(self.ctx, _p(track), w, nw, _p(run0)), "gci_depth_runs_count")
        runs = np.zeros(max(int(run0[nw]), 1), dtype=RUN_DTYPE)
        self._chk(self.lib.gci_depth_runs_write(self.ctx, _p(track), _p(runs), int(run0[nw])), "gci_depth_runs_write")
        return runs, run0

    def depth_runs(self, track: np.ndarray, windows: Sequence[Tuple[int, int]]) -> Tuple[np.ndarray, np.ndarray]:
        """device.Engine.depth_runs' twin: (RUN_DTYPE [total], uint64 [n + 1] first run of every window, then the total)."""
        nw = len(windows)
        w = (_Window * max(nw, 1))(*[_Window(int(a), int(b)) for a, b in windows])
        runs, run0 = self._depth_runs(track, w, nw)
        return runs[:int(run0[nw])], run0

    def bedgraph(self, track: np.ndarray, windows: Sequence[Tuple[int, int]], names: Sequence[bytes], coord0: Sequence[int]
                 ) -> Tuple[memoryview, np.ndarray]:
        """device.Engine.bedgraph's twin: (the text, uint64 [n + 1] first byte of every window, then the total)."""
        return self.bedgraph_text(self.bedgraph_runs(track, windows), names, coord0)

    def bedgraph_runs(self, track: np.ndarray, windows: Sequence[Tuple[int, int]]):
        nw = len(windows)
        w = (_Window * max(nw, 1))(*[_Window(int(a), int(b)) for a, b in windows])
        return (w, nw) + self._depth_runs(track, w, nw)

    def bedgraph_text(self, held, names: Sequence[bytes], coord0: Sequence[int]) -> Tuple[memoryview, np.ndarray]:
        w, nw, runs, run0 = held
        coord = np.ascontiguousarray(coord0, dtype=np.int64)
        name_len = np.array([len(x) for x in names], dtype=np.uint32)
        if coord.shape[0] != nw or name_len.shape[0] != nw:
            raise CpuError(-1, "bedgraph: one name and one coordinate per window")
        name_off = np.zeros(max(nw, 1), dtype=np.uint64)
        name_off[1:nw] = np.cumsum(name_len[:-1], dtype=np.uint64)
        blob = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8)
        byte0 = np.zeros(nw + 1, dtype=np.uint64)
        self._chk(self.lib.gci_bedgraph_size(self.ctx, _p(runs), _p(run0), w, nw, _p(coord), _p(name_len), _p(byte0)), "gci_bedgraph_size")
        out = np.zeros(max(int(byte0[nw]), 1), dtype=np.uint8)
        self._chk(self.lib.gci_bedgraph_write(self.ctx, _p(runs), _p(run0), w, nw, _p(coord), _p(blob), _p(name_off), _p(name_len), _p(out),
                                              int(byte0[nw])), "gci_bedgraph_write")
        return memoryview(out[:int(byte0[nw])]), byte0

    # ---- depth_dist.py (k_hist.hip's twin)
    HIST_LDS_BINS = _lib.HIST_LDS_BINS

    def depth_hist(self, track: np.ndarray, windows: Sequence[Tuple[int, int]], n_bins: int) -> Tuple[np.ndarray, np.ndarray]:
        """device.Engine.depth_hist's twin: (uint64 [n, n_bins + 2], int64 [n, 4] of sum, min, max, elements)."""
        nw, n_bins = len(windows), int(n_bins)
        w = (_Window * max(nw, 1))(*[_Window(int(a), int(b)) for a, b in windows])
        hist = np.zeros((nw, n_bins + 2), dtype=np.uint64)
        stats = np.zeros((nw, 4), dtype=np.int64)
        self._chk(self.lib.gci_depth_hist(self.ctx, _p(track), w, nw, n_bins, _p(hist), _p(stats)), "gci_depth_hist")
        return hist, stats

    # ---- R7, R15
    def depth_text(self, track: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        off = np.zeros(len(self.lengths) + 1, dtype=np.uint64)
        self._chk(self.lib.gci_depth_text_size(self.ctx, _p(track), _p(off)), "gci_depth_text_size")
        out = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
        self._chk(self.lib.gci_depth_text_write(self.ctx, _p(track), _p(out), out.shape[0]), "gci_depth_text_write")
        return out[:int(off[-1])], off

    MEMBER_BASES = 64 * 4096

    def depth_deflate(self, track: np.ndarray) -> List[bytes]:
        """-> per contig the bytes of the gzip members whose payload is its depth lines (device.Engine.depth_deflate's twin)."""
        elem, cnt, first = [], [], [0]
        for off, length in zip(self.offsets.tolist(), self.lengths):
            for g in range(0, int(length), self.MEMBER_BASES):
                elem.append(int(off) + g)
                cnt.append(min(self.MEMBER_BASES, int(length) - g))
            first.append(len(elem))
        nm = len(elem)
        if nm == 0:
            return [b"" for _ in self.lengths]
        d_elem, d_cnt = np.asarray(elem, dtype=np.uint64), np.asarray(cnt, dtype=np.uint32)
        tile_bytes = np.zeros(nm * 64, dtype=np.uint32)
        mb, crc, isz = (np.zeros(nm, dtype=np.uint32) for _ in range(3))
        self._chk(self.lib.gci_depth_deflate_size(self.ctx, _p(track), _p(d_elem), _p(d_cnt), nm, _p(tile_bytes), _p(mb), _p(crc), _p(isz)),
                  "gci_depth_deflate_size")
        offs = np.zeros(nm + 1, dtype=np.uint64)
        np.cumsum(mb.astype(np.uint64), out=offs[1:])
        out = np.zeros(int(offs[nm]), dtype=np.uint8)
        self._chk(self.lib.gci_depth_deflate_write(self.ctx, _p(track), _p(d_elem), _p(d_cnt), nm, _p(tile_bytes), _p(crc), _p(isz), _p(offs),
                                                   _p(out), out.shape[0]), "gci_depth_deflate_write")
        return [out[int(offs[first[c]]):int(offs[first[c + 1]])].tobytes() for c in range(len(self.lengths))]

    def depth_sum(self, track: np.ndarray) -> np.ndarray:
        s = np.zeros(len(self.lengths), dtype=np.int64)
        self._chk(self.lib.gci_depth_sum(self.ctx, _p(track), _p(s)), "gci_depth_sum")
        return s

    def range_sums(self, track: np.ndarray, ranges: np.ndarray) -> np.ndarray:
        r = np.ascontiguousarray(ranges, dtype=np.int64).reshape(-1, 2)
        s = np.zeros(r.shape[0], dtype=np.int64)
        self._chk(self.lib.gci_range_sums(self.ctx, _p(track), _p(r), r.shape[0], _p(s)), "gci_range_sums")
        return s

    # ---- text back to a track (k_depth_parse.hip's and k_sdepth.hip's twins)
    def _text_index(self, call, text: np.ndarray, cap: int) -> Tuple[np.ndarray, np.ndarray, int]:
        """call(text, tiles, keys, cap, n_keys, bad) until every key fitted -> (uint32 line starts per 4096-byte tile, the sorted keys,
        the smallest offending offset or 2**64 - 1)."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        n_tiles = (text.shape[0] + 4095) // 4096
        tiles = np.zeros(max(n_tiles, 1), dtype=np.uint32)
        while True:
            keys = np.zeros(max(cap, 1), dtype=np.uint64)
            nk, bad = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
            call(text, tiles, keys, cap, nk, bad)
            if int(nk[0]) <= cap:
                return tiles[:n_tiles], np.sort(keys[:int(nk[0])]), int(bad[0])
            cap = int(nk[0])

    def _text_parse(self, fn, what: str, text: np.ndarray, tile_line0: np.ndarray, base: tuple, segs: np.ndarray, track: np.ndarray) -> np.ndarray:
        """fn(ctx, text, n, tile_line0, *base, segs, n_segs, track, track_n)"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        line0 = np.ascontiguousarray(tile_line0, dtype=np.uint64)
        segs = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1, 3)
        self._chk(fn(self.ctx, _p(text), text.shape[0], _p(line0), *base, _p(segs), segs.shape[0], _p(track), track.shape[0]), what)
        return track

    def depth_text_index(self, text: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
        """-> (uint32 line starts per 4096-byte tile, sorted uint64 header keys (offset << 12 | rank in tile), smallest offset of a
        data line outside the strict grammar or 2**64 - 1)."""
        def call(text, tiles, keys, cap, nk, bad):
            self._chk(self.lib.gci_depth_text_index(self.ctx, _p(text), text.shape[0], _p(tiles), _p(keys), cap, _p(nk), _p(bad)),
                      "gci_depth_text_index")
        return self._text_index(call, text, 1 << 10)

    def depth_text_parse(self, text: np.ndarray, tile_line0: np.ndarray, segs: np.ndarray, track: np.ndarray) -> np.ndarray:
        return self._text_parse(self.lib.gci_depth_text_parse, "gci_depth_text_parse", text, tile_line0, (), segs, track)

    def sdepth_index(self, text: np.ndarray, prev_name: bytes = b"", cap: int = 1 << 10) -> Tuple[np.ndarray, np.ndarray, int]:
        """-> (uint32 line starts per 4096-byte tile, sorted uint64 keys (offset << 12 | rank in tile) of the lines whose name differs
        from the line in front -- the first line: from prev_name --, smallest offset of a line outside the strict grammar or 2**64 - 1)."""
        prev = np.frombuffer(bytes(prev_name) or b"\0", dtype=np.uint8)

        def call(text, tiles, keys, cap, nk, bad):
            self._chk(self.lib.gci_sdepth_index(self.ctx, _p(text), text.shape[0], _p(prev), len(prev_name), _p(tiles), _p(keys), cap, _p(nk),
                                                _p(bad)), "gci_sdepth_index")
        return self._text_index(call, text, cap)

    def sdepth_parse(self, text: np.ndarray, tile_line0: np.ndarray, segs: np.ndarray, track: np.ndarray, line_base: int = 0) -> np.ndarray:
        return self._text_parse(self.lib.gci_sdepth_parse, "gci_sdepth_parse", text, tile_line0, (int(line_base),), segs, track)

    # ---- this project's own .depth.gz to a track without inflating it (k_depth_gz.hip's twin)
    def depth_gz_scan(self, raw: np.ndarray, cand_pos: np.ndarray) -> np.ndarray:
        """-> DGZ_INFO_DTYPE per candidate member start: status, end offset, lines, runs, CRC-32 / ISIZE verdicts."""
        from .formats.depthfile import DGZ_INFO_DTYPE
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        cand = np.ascontiguousarray(cand_pos, dtype=np.uint64)
        info = np.zeros(cand.shape[0], dtype=DGZ_INFO_DTYPE)
        self._chk(self.lib.gci_depth_gz_scan(self.ctx, _p(raw), raw.shape[0], _p(cand), cand.shape[0], _p(info)), "gci_depth_gz_scan")
        return info

    def depth_gz_runs(self, raw: np.ndarray, members: np.ndarray) -> np.ndarray:
        """members: DGZ_MEMBER_DTYPE (pos, run0, runs as the scan reported them) -> DGZ_RUN_DTYPE, every member's runs at its run0."""
        from .formats.depthfile import DGZ_MEMBER_DTYPE, DGZ_RUN_DTYPE
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        members = np.ascontiguousarray(members, dtype=DGZ_MEMBER_DTYPE)
        runs = np.zeros(max(int(members["runs"].astype(np.uint64).sum()), 1), dtype=DGZ_RUN_DTYPE)
        self._chk(self.lib.gci_depth_gz_runs(self.ctx, _p(raw), raw.shape[0], _p(members), members.shape[0], _p(runs)), "gci_depth_gz_runs")
        return runs

    def depth_gz_expand(self, runs: np.ndarray, members: np.ndarray, track: np.ndarray) -> np.ndarray:
        from .formats.depthfile import DGZ_MEMBER_DTYPE
        members = np.ascontiguousarray(members, dtype=DGZ_MEMBER_DTYPE)
        self._chk(self.lib.gci_depth_gz_expand(self.ctx, _p(runs), _p(members), members.shape[0], _p(track), track.shape[0]),
                  "gci_depth_gz_expand")
        return track

    def depth_gz_track(self, raw: np.ndarray, members: np.ndarray, track: np.ndarray) -> np.ndarray:
        """The members' lines into `track` at each member's elem0 (device.Engine.depth_gz_track's twin)."""
        return self.depth_gz_expand(self.depth_gz_runs(raw, members), members, track)
