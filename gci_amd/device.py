"""Device side of the path: one `Engine` per GPU wrapping a gci_ctx (include/gci_hip.h).

HBM buffers, streams and events come from a provider (gci_amd/hbm.py): the library's own `gci_dev_*` exports for the single-GPU
command line (no `import torch` in that process), or torch for contig-sharded runs and the test fixtures -- plumbing either way:
every per-record and per-base operation is a hand-written gfx950 kernel reached through the C ABI.  Nothing here computes on
the CPU; a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes
import os
import threading
from concurrent.futures import ThreadPoolExecutor
import warnings
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, hbm
from ._lib import BuildOpts, GciError, JoinFile, Window

REC_DTYPE = np.dtype([("name_hash", "<u8"), ("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("qlen", "<i4"),
                      ("rec_idx", "<u4"), ("mapq", "u1"), ("flags", "u1"), ("name_len", "<u2")])
assert REC_DTYPE.itemsize == 32
IVL_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("pad", "<i4")])
RUN_DTYPE = np.dtype([("start", "<u4"), ("depth", "<i4")])          # gci_depth_run
SITE_DTYPE = np.dtype([("contig", "<i4"), ("pos", "<i4"), ("left", "<i4"), ("right", "<i4"), ("depth", "<i4"), ("pad", "<i4")])      # gci_clip_site
INDEL_SITE_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("del", "<i4"), ("ins", "<i4"), ("depth", "<i4")])      # gci_indel_site
MISMATCH_SITE_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("mismatch", "<i4"), ("depth", "<i4")])      # gci_mismatch_site
ALLELE_SITE_DTYPE = np.dtype([("contig", "<i4"), ("pos", "<i4"), ("ref", "<i4"), ("alt", "<i4"), ("n", "<i4", (4,)), ("depth", "<i4")])      # gci_allele_site

_M64 = (1 << 64) - 1
Buffer = Any                  # a device buffer of the engine's provider: hbm.Buf or Buffer


def name_hash_np(names: Sequence[bytes]) -> np.ndarray:
    """Vectorised twin of gci_name_hash (gci_amd/csrc/gci_common.h) for host-built records."""
    n = len(names)
    lens = np.fromiter((len(x) for x in names), dtype=np.int64, count=n)
    width = int(((lens.max() if n else 0) + 7) // 8 * 8) or 8
    buf = np.zeros((n, width), dtype=np.uint8)
    for i, x in enumerate(names):
        buf[i, :len(x)] = np.frombuffer(x, dtype=np.uint8)
    words = buf.view("<u8")

    def mix(x):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))

    acc = np.zeros(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(width // 8):
            use = (k * 8) < lens
            key = (0x9E3779B97F4A7C15 * (k + 1)) & _M64
            mul = np.uint64(((key >> 1) ^ 0xbf58476d1ce4e5b9) | 1)
            acc = acc + np.where(use, (words[:, k] ^ np.uint64(key)) * mul, np.uint64(0))
        return mix(acc ^ (lens.astype(np.uint64) * np.uint64(0xD6E8FEB86659FD93)))


def _forget_pages(raw, lo: int, hi: int) -> None:
    """The pages [lo, hi) of a memory-mapped input file have been read for the last time BY THE CPU: drop their entries from this
    process's page table (madvise DONTNEED; the page cache keeps the data), so that the final unmap of a 77 GB file does not
    tear down 19 M entries at once under the address-space lock (every hipMalloc and every new mapping of the process waits
    for that: the join's scratch behind the second whole-genome file was measured at 3 s of wall time for 1.5 ms of kernels).
    ONLY for ranges the GPU driver never saw: a pageable host-to-device copy registers the user pages with the driver, and a
    madvise / munmap over registered pages goes through its MMU notifier, which evicts the process's GPU queues while it
    invalidates -- measured: every kernel of the run 1.4 - 8 x slower, the command line at 1/4 genome 9.2 s instead of 5.2 s
    (profiles/r04j_forget_pages_ab.txt).  pipeline._RunUploads therefore stages the file's bytes through pinned memory itself."""
    import mmap as _mmap
    mm = getattr(raw, "_mmap", None)
    if mm is None or hi <= lo or not hasattr(mm, "madvise"):
        return
    a = lo // _mmap.PAGESIZE * _mmap.PAGESIZE
    try:
        mm.madvise(_mmap.MADV_DONTNEED, a, hi - a)
    except (OSError, ValueError, AttributeError):
        pass


class _Staging:
    """A ring of pinned host buffers through which the bytes of a memory-mapped file travel to the device: host threads copy a
    piece of the mapping into a slot (parallel memcpy out of the page cache: the page faults are theirs, not the copy engine's),
    the slot leaves by DMA on the copy stream, and is reused once that copy's event has passed.  One per engine, made once."""
    SLOT = int(os.environ.get("GCI_STAGING_SLOT_MB", "64")) << 20    # (page-locking costs ~0.3 s per GB on these hosts: a ring of 256 MB, not of 1.2 GB)
    SLOTS = int(os.environ.get("GCI_STAGING_SLOTS", "4"))
    # (copying threads: 6, 12 and 24 bring a tmpfs file to the device at 46 - 47 GB/s inside the command line, 48 at 57 GB/s -- the
    #  link's own rate -- on the 256-thread hosts of the pool: profiles/r06e_staging_threads.txt; a quarter of the host's threads, at most 48)
    # As one rank of N on a node (LOCAL_WORLD_SIZE, set by `GCI.py --gpus N` and by torch.distributed.run) a ring takes its share of that.
    _RANKS = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1)) if "RANK" in os.environ else 1
    THREADS = int(os.environ.get("GCI_STAGING_THREADS", str(min(48, max(4, (os.cpu_count() or 24) // (4 * _RANKS))))))

    def __init__(self, engine):
        # the loop over the slots is the library's (staging.cpp: gci_stage_send)
        self.engine = engine
        h = ctypes.c_void_p()
        engine._chk(engine.lib.gci_stage_create(engine.ctx, self.SLOT, self.SLOTS, self.THREADS, ctypes.byref(h)), "gci_stage_create")
        self.native = h

    def close(self):
        """The ring's threads, pinned slots and events (gci_stage_free)."""
        if self.native is not None:
            self.engine.lib.gci_stage_free(self.native)
            self.native = None

    def send(self, raw, p0: int, p1: int, dst: Buffer, stream, urgent: bool = True) -> None:
        """raw[p0:p1] -> dst[:p1 - p0] (device), enqueued on `stream`; returns when the last piece is enqueued.  A sender that is not
        urgent (the assembly, whose N runs nobody waits for) lets the urgent ones (the runs of a BAM file: the device inflates them
        as they arrive) go first, piece by piece."""
        if self.native is not None:
            if p1 <= p0:
                return
            src = raw.ctypes.data + p0                      # (a numpy array / memmap of uint8: its bytes as they lie)
            forget = 1 if getattr(raw, "_mmap", None) is not None else 0
            self.engine._chk(self.engine.lib.gci_stage_send(self.engine.ctx, self.native, ctypes.c_void_p(src), p1 - p0, ctypes.c_void_p(dst.data_ptr()),
                                                            ctypes.c_void_p(stream.cuda_stream), forget, 1 if urgent else 0), "gci_stage_send")
            return
        raise GciError(_lib.GCI_E_INVALID, "the staging ring of this engine has been closed")


@dataclass
class JoinInput:
    """One file of the join: compact records on the device + where its name bytes are."""
    recs: Buffer            # uint8 [n, 32]
    name_base: Buffer       # uint8 blob (BAM: the inflated stream)
    name_off: Buffer        # int64 [*], indexed by rec_idx
    name_delta: int               # 36 for BAM records, 0 for a names blob


@dataclass
class Pages:
    """Record pages of one alignment file on the device (gci_bam_pages_write)."""
    buf: Buffer             # uint8: pages | blob | 16 zero bytes
    n_pages: int
    page_bytes: int
    blob_off: int
    n_rec: int


class _Upload:
    """A file on its way to the device in pieces (Engine.start_upload): the device buffer, where the pieces end, per piece the copy
    stream's event and whether it has been recorded yet, and the helper thread that enqueues the copies (`future`: its outcome)."""

    def __init__(self, d_raw: Buffer, cuts: List[int], events: list, queued: list, stream, run):
        self.d_raw, self.cuts, self.events, self.queued, self.stream = d_raw, cuts, events, queued, stream
        self.pool = ThreadPoolExecutor(1)
        self.future = self.pool.submit(run)

    def close(self) -> None:
        """The helper thread is through and gone.  Idempotent; raises nothing (what the upload raised is future.result()'s to tell)."""
        pool, self.pool = self.pool, None
        if pool is not None:
            pool.shutdown(wait=True)


class Engine:
    """A gci_ctx bound to a stream of its provider (hbm.py) on `device`."""

    def __init__(self, device: int = 0, stream: Optional[Any] = None, backend: Optional[str] = None):
        """`stream`: the provider's stream this context enqueues on (default: the device's current stream).  `backend`: "native"
        (the library's own gci_dev_* exports: no torch in the process) or "torch"; default hbm.provider()'s rule."""
        self.lib = _lib.load()
        self.T = T = hbm.provider_of(stream) if (stream is not None and backend is None) else hbm.provider(backend)
        if not T.is_available():
            raise GciError(_lib.GCI_E_HIP, "no MI355X visible: the HIP path has no CPU fallback")
        self.device = T.device(device)
        T.set_device(self.device)
        self.stream = stream if stream is not None else T.current_stream(self.device)
        from . import phases
        phases.set_provider(T)
        h = ctypes.c_void_p()
        st = self.lib.gci_ctx_create(device, ctypes.c_void_p(self.stream.cuda_stream), 0, ctypes.byref(h))
        if st != 0:
            raise GciError(st, "gci_ctx_create: %s" % self.lib.gci_strerror(st).decode())
        self.ctx = h
        self.lengths: List[int] = []
        self.offsets: List[int] = []
        self.total = 0
        self._status = self.T.zeros(1, self.T.int64, self.device)
        self._count = self.T.zeros(1, self.T.int32, self.device)
        self._members_host = None                 # pinned staging buffer of depth_deflate()
        self._staging = None
        self._copy_stream = None
        self._walk = None
        self._lock = threading.Lock()
        m = os.environ.get("GCI_JOIN", "")
        self.join_mode = 1 if m.startswith("c") else 2 if m.startswith("p") else 0    # what gci_ctx_create read

    def close(self) -> None:
        if getattr(self, "ctx", None):
            walk, self._walk = getattr(self, "_walk", None), None
            if walk is not None:
                walk.close()
            st, self._staging = getattr(self, "_staging", None), None
            if st is not None and getattr(st, "engine", None) is self:     # (a side engine borrows the main engine's ring)
                st.close()                                # before the context it was made with goes
            self.lib.gci_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def _chk(self, st: int, what: str) -> None:
        if st != 0:
            detail = self.lib.gci_last_error(self.ctx).decode() if st == _lib.GCI_E_HIP else ""
            raise GciError(st, "%s: %s %s" % (what, self.lib.gci_strerror(st).decode(), detail))

    def sync(self) -> None:
        self._chk(self.lib.gci_sync(self.ctx), "gci_sync")

    @staticmethod
    def _p(t: Optional[Buffer]):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def to_device(self, a: np.ndarray) -> Buffer:
        return self.T.from_numpy(a, self.device)

    def _host_src(self, a) -> Any:
        """A host array as the source of a buffer's copy_(): numpy for the native provider, a tensor over the same memory for torch."""
        a = np.asarray(a)
        if self.T.name == "torch":
            return self.T.t.from_numpy(a)
        return a

    def upload_staged(self, a: np.ndarray) -> Buffer:
        """A large host array (the 3 GB assembly) to the device through the ring of pinned buffers (`_Staging`) instead of one
        pageable copy: host threads fill a slot while the one before it crosses PCIe.  Ordered before what this engine's stream
        does next."""
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        n = int(a.shape[0])
        staging, copy = self.staging(), self.copy_stream()
        dst = self.T.empty(max(n, 1), self.T.uint8, self.device)
        copy.wait_stream(self.stream)
        staging.send(a, 0, n, dst, copy, urgent=False)
        self.stream.wait_stream(copy)
        return dst[:n]

    def staging(self) -> "_Staging":
        """The engine's ring of pinned buffers (made on first use; a helper thread may be the first)."""
        with self._lock:
            if self._staging is None:
                self._staging = _Staging(self)
            return self._staging

    def copy_stream(self) -> Any:
        with self._lock:
            if self._copy_stream is None:
                self._copy_stream = self.T.Stream(self.device)
            return self._copy_stream

    def walk_engine(self) -> "Engine":
        """The context that walks, pages and filters a run of a large file while this one inflates the next (pipeline.
        _bam_join_input_gpu): a stream and scratch of its own (a gci_ctx is one stream and is not shared between streams), the same
        provider and device.  Made on first use; close() closes it."""
        with self._lock:
            if self._walk is None:
                self._walk = Engine(self.device.index or 0, stream=self.T.Stream(self.device))
            return self._walk

    # ---- per-kernel HIP-event timing (library side, on the ctx stream) -------------------------
    def profile_enable(self, mask: int) -> None:
        self._chk(self.lib.gci_profile_enable(self.ctx, int(mask)), "gci_profile_enable")

    def profile_read(self, reset: bool = True) -> Dict[str, Tuple[float, int]]:
        """-> {kernel name: (total ms, launches)} accumulated since the last reset."""
        out = {}
        for k in range(_lib.PROF_COUNT):
            ms, n = ctypes.c_double(0), ctypes.c_uint64(0)
            self._chk(self.lib.gci_profile_read(self.ctx, k, ctypes.byref(ms), ctypes.byref(n), int(reset)),
                      "gci_profile_read")
            if n.value:
                out[self.lib.gci_profile_name(k).decode()] = (ms.value, int(n.value))
        return out

    # ---- layout ------------------------------------------------------------------------------
    def set_layout(self, lengths: Sequence[int]) -> List[int]:
        arr = np.asarray(lengths, dtype=np.int64)
        self._chk(self.lib.gci_layout_set(self.ctx, arr.shape[0], arr.ctypes.data_as(ctypes.c_void_p)), "gci_layout_set")
        self.lengths = [int(x) for x in arr]
        offs = np.zeros(arr.shape[0], dtype=np.int64)
        self._chk(self.lib.gci_layout_offsets(self.ctx, offs.ctypes.data_as(ctypes.c_void_p)), "gci_layout_offsets")
        self.offsets = [int(x) for x in offs]
        self.total = int(self.lib.gci_layout_total(self.ctx))
        return self.offsets

    def new_track(self) -> Buffer:
        return self.T.empty(max(self.total, 1), self.T.int32, self.device)

    # ---- R1 ----------------------------------------------------------------------------------
    def bam_filter(self, d_bam: Buffer, d_rec_off: Buffer, d_ref_sel: Buffer, map_qual: int,
                   mq_cutoff: int, clip_percent: float, iden_percent: float, out: Optional[Buffer] = None,
                   check: bool = True, rec_idx_base: int = 0) -> Buffer:
        """K1 over the whole inflated stream (the round-1 / 2 kernel, GCI_K1=stream; the product runs bam_pages +
        bam_filter_pages)."""
        n = int(d_rec_off.shape[0])
        if out is None:
            out = self.T.empty((max(n, 1), 32), self.T.uint8, self.device)
        st = self.lib.gci_bam_filter(self.ctx, self._p(d_bam), int(d_bam.shape[0]), self._p(d_rec_off), n, self._p(d_ref_sel),
                int(d_ref_sel.shape[0]), int(map_qual), int(mq_cutoff), float(clip_percent), float(iden_percent),
                int(rec_idx_base), self._p(out), self._p(self._status))
        self._chk(st, "gci_bam_filter")
        if check:
            self.check_status("gci_bam_filter")
        return out[:n]

    # ---- R1 over record pages (include/gci_hip.h: gci_bam_pages_*, gci_bam_filter_pages) -------------------------------
    def bam_pages(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, page_bytes: int = 0) -> "Pages":
        """The records of an inflated BAM stream (has_seq) or of a heads stream laid out as record pages: the bytes read_sam
        looks at, 16-byte aligned, no offset table -- what the record filter is fastest on."""
        page_bytes = int(page_bytes or _lib.PAGE_BYTES_DEFAULT)
        n = int(d_rec_off.shape[0])
        h = (ctypes.c_uint64 * 3)()
        self._chk(self.lib.gci_bam_pages_size(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                              page_bytes, h), "gci_bam_pages_size")
        buf = self.T.empty(int(h[1]), self.T.uint8, self.device)
        self._chk(self.lib.gci_bam_pages_write(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                               self._p(buf), int(h[1])), "gci_bam_pages_write")
        return Pages(buf, int(h[0]), page_bytes, int(h[2]), n)

    def bam_filter_pages(self, pages: "Pages", d_ref_sel: Buffer, map_qual: int, mq_cutoff: int, clip_percent: float,
                         iden_percent: float, out: Optional[Buffer] = None, name_off: Optional[Buffer] = None,
                         check: bool = True, rec_idx_base: int = 0) -> Tuple[Buffer, Buffer]:
        """-> (records uint8 [n, 32], name offsets int64 [n] into pages.buf)."""
        n = pages.n_rec
        if out is None:
            out = self.T.empty((max(n, 1), 32), self.T.uint8, self.device)
        if name_off is None:
            name_off = self.T.empty(max(n, 1), self.T.int64, self.device)
        st = self.lib.gci_bam_filter_pages(self.ctx, self._p(pages.buf), int(pages.buf.shape[0]), pages.page_bytes, pages.n_pages, n,
                                           self._p(d_ref_sel), int(d_ref_sel.shape[0]), int(map_qual), int(mq_cutoff),
                                           float(clip_percent), float(iden_percent), int(rec_idx_base), self._p(out),
                                           self._p(name_off), self._p(self._status))
        self._chk(st, "gci_bam_filter_pages")
        if check:
            self.check_status("gci_bam_filter_pages")
        return out[:n], name_off[:n]

    # ---- bam_depth.py: the reference bases the records cover (include/gci_hip.h: gci_bam_cover_*, gci_track_add) -------
    def bam_cover(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, d_ref_sel: Buffer, excl_flags: int = 0x704,
                  min_mapq: int = 0, count_del: bool = False, check: bool = True, rec_idx_base: int = 0,
                  classes: Optional[Buffer] = None, mask: int = 0) -> Buffer:
        """-> intervals int32 [n, 4] (contig, start, last covered base, 0) of the records of an inflated BAM stream (has_seq) or a
        heads stream: what `samtools depth -a` counts, for depth_build with flank 0.  Needs the layout of the selected contigs.
        classes (bam_fate's bytes) and mask: only the records whose class is a bit of the mask (gci_bam_cover_size_sel)."""
        n = int(d_rec_off.shape[0])
        n_ivl = ctypes.c_uint64(0)
        head = (self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq), self._p(d_ref_sel),
                int(d_ref_sel.shape[0]), int(excl_flags), int(min_mapq), int(bool(count_del)))
        if classes is None:
            self._chk(self.lib.gci_bam_cover_size(*head, ctypes.byref(n_ivl), self._p(self._status)), "gci_bam_cover_size")
        else:
            self._chk(self.lib.gci_bam_cover_size_sel(*head, self._p(classes), int(mask), ctypes.byref(n_ivl), self._p(self._status)),
                      "gci_bam_cover_size_sel")
        if check:
            self._raise_status(self._status.item(), "gci_bam_cover_size", rec_idx_base)
        out = self.T.empty((max(int(n_ivl.value), 1), 4), self.T.int32, self.device)
        self._chk(self.lib.gci_bam_cover_write(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                               self._p(out), int(n_ivl.value), self._p(self._status)), "gci_bam_cover_write")
        return out[:int(n_ivl.value)]

    def bam_fate(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, d_ref_sel: Buffer, map_qual: int, clip_percent: float,
                 iden_percent: float, check: bool = True, rec_idx_base: int = 0):
        """-> (class byte per record uint8 [n] on the device, records per class as a list of FATE_CLASSES ints): which test of read_sam
        drops every record of an inflated BAM stream (has_seq) or a heads stream (include/gci_hip.h: gci_bam_fate)."""
        n = int(d_rec_off.shape[0])
        cls = self.T.empty(max(n, 1), self.T.uint8, self.device)
        counts = (ctypes.c_uint64 * _lib.FATE_CLASSES)()
        self._chk(self.lib.gci_bam_fate(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                        self._p(d_ref_sel), int(d_ref_sel.shape[0]), int(map_qual), float(clip_percent), float(iden_percent),
                                        self._p(cls), counts, self._p(self._status)), "gci_bam_fate")
        if check:
            self._raise_status(self._status.item(), "gci_bam_fate", rec_idx_base)
        return cls[:n], [int(c) for c in counts]

    def bam_reads(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, d_ref_sel: Buffer, classes: Buffer, mask: int, names: Sequence[bytes],
                  d_names: Buffer, d_win: Optional[Buffer] = None, d_win0: Optional[Buffer] = None, file_no: int = 1, check: bool = True,
                  rec_idx_base: int = 0) -> Tuple[bytes, int]:
        """-> (the rows of text of the records whose class -- bam_fate's bytes -- is a bit of the mask and whose span overlaps a window, in
        record order; the number of rows): include/gci_hip.h gci_bam_reads_size / _write.  names: the selected contigs' names, d_names their
        bytes back to back on the device; d_win int64 [n, 2] and d_win0 uint32 [n_sel + 1] as pipeline.merge_windows makes them (None: no
        window test).  Needs the layout of the selected contigs.  Only the rows cross to the host."""
        n = int(d_rec_off.shape[0])
        name_len = np.array([len(x) for x in names], dtype=np.uint32)
        name_off = np.zeros(max(len(names), 1), dtype=np.uint64)
        name_off[1:len(names)] = np.cumsum(name_len[:-1], dtype=np.uint64)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                   # noqa: E731
        rows, size = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._chk(self.lib.gci_bam_reads_size(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq), self._p(d_ref_sel),
                                              int(d_ref_sel.shape[0]), self._p(classes), int(mask), self._p(d_win) if d_win0 is not None else None,
                                              self._p(d_win0), vp(name_len), int(file_no), ctypes.byref(rows), ctypes.byref(size),
                                              self._p(self._status)), "gci_bam_reads_size")
        if check:
            self._raise_status(self._status.item(), "gci_bam_reads_size", rec_idx_base)
        total = int(size.value)
        if total == 0:
            return b"", 0
        out = self.T.empty(total, self.T.uint8, self.device)
        self._chk(self.lib.gci_bam_reads_write(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, self._p(d_names), vp(name_off),
                                               vp(name_len), self._p(out), total), "gci_bam_reads_write")
        return out.cpu().numpy().tobytes(), int(rows.value)

    def bam_sweep(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, d_ref_sel: Buffer, map_qual: int, clip_percent: float, iden_percent: float,
                  digits: int = 3, d_win: Optional[Buffer] = None, d_win0: Optional[Buffer] = None, check: bool = True,
                  rec_idx_base: int = 0) -> np.ndarray:
        """-> the table uint64 [GCI_SWEEP_ROWS(digits), 4] (records, bases, records_others, bases_others; the rows as _lib.SweepRows
        numbers them) of the primary records of an inflated BAM stream (has_seq) or a heads stream: their MAPQ, clip and identity
        quotients, and what passes the other two tests at these thresholds (include/gci_hip.h: gci_bam_sweep).  d_win / d_win0 as for
        bam_reads (None: no window test; with windows the layout of the selected contigs is needed)."""
        n = int(d_rec_off.shape[0])
        table = np.zeros((_lib.SweepRows(digits).rows, _lib.SWEEP_COLS), dtype=np.uint64)
        self._chk(self.lib.gci_bam_sweep(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq), self._p(d_ref_sel),
                                         int(d_ref_sel.shape[0]), self._p(d_win) if d_win0 is not None else None, self._p(d_win0), int(map_qual),
                                         float(clip_percent), float(iden_percent), int(digits), table.ctypes.data_as(ctypes.c_void_p),
                                         self._p(self._status)), "gci_bam_sweep")
        if check:
            self._raise_status(self._status.item(), "gci_bam_sweep", rec_idx_base)
        return table

    # ---- clip_sites.py: where alignments break off (include/gci_hip.h: gci_bam_clip_*, gci_clip_sites_*; k_clips.hip) ----
    def bam_clip(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, d_ref_sel: Buffer, excl_flags: int = 0x704, min_mapq: int = 0,
                 min_clip: int = 100, check: bool = True, rec_idx_base: int = 0) -> Tuple[Buffer, Buffer, List[int]]:
        """-> (the left events, the right events, [records counted, left events, right events]): per counted record of an inflated BAM
        stream (has_seq) or a heads stream one interval int32 [n, 4] (contig, site, site, 0) where its alignment begins / ends with a clip
        of at least min_clip bases beyond it, each half in record order, for depth_build with flank 0.  Needs the layout of the selected
        contigs."""
        n = int(d_rec_off.shape[0])
        counts = (ctypes.c_uint64 * 3)()
        self._chk(self.lib.gci_bam_clip_size(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                             self._p(d_ref_sel), int(d_ref_sel.shape[0]), int(excl_flags), int(min_mapq), int(min_clip), counts,
                                             self._p(self._status)), "gci_bam_clip_size")
        if check:
            self._raise_status(self._status.item(), "gci_bam_clip_size", rec_idx_base)
        n_left, n_right = int(counts[1]), int(counts[2])
        out = self.T.empty((max(n_left + n_right, 1), 4), self.T.int32, self.device)
        self._chk(self.lib.gci_bam_clip_write(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                              self._p(out), n_left + n_right, self._p(self._status)), "gci_bam_clip_write")
        return out[:n_left], out[n_left:n_left + n_right], [int(c) for c in counts]

    def clip_sites(self, left: Buffer, right: Buffer, depth: Optional[Buffer], min_reads: int,
                   windows: Sequence[Tuple[int, int]] = ()) -> np.ndarray:
        """-> SITE_DTYPE [n]: the elements of the tracks `left` / `right` with left >= min_reads or right >= min_reads inside the sorted,
        disjoint [begin, end) windows of track elements (none: every contig), in ascending order, with the depth there (0 without a depth
        track)."""
        nw = len(windows)
        arr = self._window_array(windows)
        n = ctypes.c_uint64(0)
        head = (self.ctx, self._p(left), self._p(right), self._p(depth), int(min_reads), arr, nw)
        self._chk(self.lib.gci_clip_sites_size(*head, ctypes.byref(n)), "gci_clip_sites_size")
        total = int(n.value)
        if total == 0:
            return np.zeros(0, dtype=SITE_DTYPE)
        out = self.T.empty((total, 6), self.T.int32, self.device)
        self._chk(self.lib.gci_clip_sites_write(*head, self._p(out), total), "gci_clip_sites_write")
        return np.ascontiguousarray(out.cpu().numpy()).view(SITE_DTYPE).reshape(-1)[:total]

    # ---- indel_sites.py: long insertions and deletions in reads (include/gci_hip.h: gci_bam_indel_*, gci_indel_sites_*; k_indels.hip) ----
    def bam_indel(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, d_ref_sel: Buffer, excl_flags: int = 0x704, min_mapq: int = 0,
                  min_len: int = 50, check: bool = True, rec_idx_base: int = 0) -> Tuple[Buffer, Buffer, List[int]]:
        """-> (the deletions, the insertions, [records counted, deletions, insertions]): two views of one buffer of intervals int32
        [n, 4] -- per D operation of at least min_len bases in a counted record of an inflated BAM stream (has_seq) or a heads stream
        (contig, first deleted base, last deleted base, 0), per such I operation (contig, site, site, 0) with the site the base in front
        of the inserted bases --, each in (record, operation) order, for depth_build with flank 0.  Needs the layout of the selected
        contigs."""
        n = int(d_rec_off.shape[0])
        counts = (ctypes.c_uint64 * 3)()
        self._chk(self.lib.gci_bam_indel_size(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                              self._p(d_ref_sel), int(d_ref_sel.shape[0]), int(excl_flags), int(min_mapq), int(min_len), counts,
                                              self._p(self._status)), "gci_bam_indel_size")
        if check:
            self._raise_status(self._status.item(), "gci_bam_indel_size", rec_idx_base)
        n_del, n_ins = int(counts[1]), int(counts[2])
        out = self.T.empty((max(n_del + n_ins, 1), 4), self.T.int32, self.device)
        self._chk(self.lib.gci_bam_indel_write(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                               self._p(out), n_del + n_ins, self._p(self._status)), "gci_bam_indel_write")
        return out[:n_del], out[n_del:n_del + n_ins], [int(c) for c in counts]

    def indel_sites(self, dele: Buffer, ins: Buffer, depth: Optional[Buffer], min_reads: int,
                    windows: Sequence[Tuple[int, int]] = ()) -> np.ndarray:
        """-> INDEL_SITE_DTYPE [n]: the maximal runs of elements of the tracks `dele` / `ins` with del >= min_reads or ins >= min_reads
        inside the sorted, disjoint [begin, end) windows of track elements (none: every contig), in ascending order: contig, start, end
        (exclusive) and the maxima of the two tracks and of `depth` (0 without a depth track) over the run."""
        nw = len(windows)
        arr = self._window_array(windows)
        n = ctypes.c_uint64(0)
        head = (self.ctx, self._p(dele), self._p(ins), self._p(depth), int(min_reads), arr, nw)
        self._chk(self.lib.gci_indel_sites_size(*head, ctypes.byref(n)), "gci_indel_sites_size")
        total = int(n.value)
        if total == 0:
            return np.zeros(0, dtype=INDEL_SITE_DTYPE)
        out = self.T.empty((total, 6), self.T.int32, self.device)
        self._chk(self.lib.gci_indel_sites_write(*head, self._p(out), total), "gci_indel_sites_write")
        return np.ascontiguousarray(out.cpu().numpy()).view(INDEL_SITE_DTYPE).reshape(-1)[:total]

    # ---- mismatch_sites.py: bases where the reads disagree with the assembly (include/gci_hip.h: gci_fasta_codes, gci_bam_mismatch_*,
    # gci_mismatch_sites_*; k_mismatch.hip) ----
    def fasta_codes(self, text: np.ndarray, bodies: np.ndarray, dst: np.ndarray, codes: Optional[Buffer] = None,
                    before_codes=None) -> Tuple[Buffer, np.ndarray]:
        """The assembly as one 4-bit code per base in the track layout -> (uint8 [layout total] on the device, the uint32 sequence-byte
        count of every 4096-byte tile of the file).  text = the FASTA file's bytes, bodies = int64 [n_records, 2] byte ranges of the
        record bodies, dst[r] = the flat element of record r's first base or -1 to leave it out.  codes: the array to write into
        (default: a new one filled with 15); elements no base goes to keep what they held.  before_codes(tile counts): called between
        the counting and the writing -- where a caller checks the records' lengths (formats/fasta.body_lengths) and may raise."""
        n = int(text.shape[0])
        d_text = self.upload_staged(text) if n >= (256 << 20) else self.to_device(text)
        bodies = np.ascontiguousarray(bodies, dtype=np.int64).reshape(-1, 2)
        d_body = self.to_device(bodies)
        d_dst = self.to_device(np.ascontiguousarray(dst, dtype=np.int64))
        tiles = (n + 4095) // 4096
        kept = self.T.zeros(max(tiles, 1), self.T.int32, self.device)
        self._chk(self.lib.gci_fasta_n_scan(self.ctx, self._p(d_text), n, self._p(d_body), int(bodies.shape[0]), self._p(kept), None, 0,
                                            self._p(self._count)), "gci_fasta_n_scan")
        kept0 = self.T.empty(tiles + 1, self.T.int64, self.device)
        self._chk(self.lib.gci_dev_u32_scan_u64(self.device.index or 0, self._p(kept), tiles, self._p(kept0),
                                                ctypes.c_void_p(self.stream.cuda_stream)), "gci_dev_u32_scan_u64")
        h_kept = kept.cpu().numpy().view(np.uint32)[:tiles]
        if before_codes is not None:
            before_codes(h_kept)
        if codes is None:
            codes = self.T.empty(max(int(self.total), 1), self.T.uint8, self.device)
            codes[:] = 15
        self._chk(self.lib.gci_fasta_codes(self.ctx, self._p(d_text), n, self._p(d_body), int(bodies.shape[0]), self._p(d_dst), self._p(kept0),
                                           self._p(codes)), "gci_fasta_codes")
        return codes, h_kept

    def bam_mismatch(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, d_ref_sel: Buffer, d_codes: Buffer, excl_flags: int = 0x704,
                     min_mapq: int = 0, check: bool = True, rec_idx_base: int = 0) -> Tuple[Buffer, List[int]]:
        """-> (the events, [records counted, mismatches, pairs compared]): intervals int32 [n, 4], (contig, p, p, 0) per base p of a
        counted record of an inflated BAM stream (has_seq must hold) where the read's base and the assembly's code in d_codes are both
        one of A, C, G, T and differ, in (record, reference position) order, for depth_build with flank 0."""
        n = int(d_rec_off.shape[0])
        counts = (ctypes.c_uint64 * 3)()
        self._chk(self.lib.gci_bam_mismatch_size(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                                 self._p(d_ref_sel), int(d_ref_sel.shape[0]), int(excl_flags), int(min_mapq), self._p(d_codes), counts,
                                                 self._p(self._status)), "gci_bam_mismatch_size")
        if check:
            self._raise_status(self._status.item(), "gci_bam_mismatch_size", rec_idx_base)
        n_mm = int(counts[1])
        out = self.T.empty((max(n_mm, 1), 4), self.T.int32, self.device)
        self._chk(self.lib.gci_bam_mismatch_write(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                                  self._p(d_codes), self._p(out), n_mm, self._p(self._status)), "gci_bam_mismatch_write")
        return out[:n_mm], [int(c) for c in counts]

    def mismatch_sites(self, mismatch: Buffer, depth: Buffer, min_reads: int, frac_ppm: int,
                       windows: Sequence[Tuple[int, int]] = ()) -> np.ndarray:
        """-> MISMATCH_SITE_DTYPE [n]: the maximal runs of elements with mismatch >= min_reads and mismatch * 1000000 >= frac_ppm * depth
        inside the sorted, disjoint [begin, end) windows of track elements (none: every contig), in ascending order: contig, start, end
        (exclusive), the largest mismatch count of the run and the depth at the first base that reaches it."""
        nw = len(windows)
        arr = self._window_array(windows)
        n = ctypes.c_uint64(0)
        head = (self.ctx, self._p(mismatch), self._p(depth), int(min_reads), int(frac_ppm), arr, nw)
        self._chk(self.lib.gci_mismatch_sites_size(*head, ctypes.byref(n)), "gci_mismatch_sites_size")
        total = int(n.value)
        if total == 0:
            return np.zeros(0, dtype=MISMATCH_SITE_DTYPE)
        out = self.T.empty((total, 5), self.T.int32, self.device)
        self._chk(self.lib.gci_mismatch_sites_write(*head, self._p(out), total), "gci_mismatch_sites_write")
        return np.ascontiguousarray(out.cpu().numpy()).view(MISMATCH_SITE_DTYPE).reshape(-1)[:total]

    # ---- allele_sites.py: which base the reads carry where they disagree (include/gci_hip.h: gci_bam_allele_*, gci_allele_sites_*;
    # k_mismatch.hip) ----
    def bam_allele(self, d_stream: Buffer, d_rec_off: Buffer, has_seq: bool, d_ref_sel: Buffer, d_codes: Buffer, excl_flags: int = 0x704,
                   min_mapq: int = 0, check: bool = True, rec_idx_base: int = 0) -> Tuple[Buffer, Buffer, Buffer, Buffer, List[int]]:
        """-> (the A events, the C, the G, the T events, [records counted, A, C, G, T events, pairs compared]): four views of one buffer
        of intervals int32 [n, 4] -- bam_mismatch's events, each in the list of the READ's base, inside a list in (record, reference
        position) order, for depth_build with flank 0."""
        n = int(d_rec_off.shape[0])
        counts = (ctypes.c_uint64 * 6)()
        self._chk(self.lib.gci_bam_allele_size(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                               self._p(d_ref_sel), int(d_ref_sel.shape[0]), int(excl_flags), int(min_mapq), self._p(d_codes), counts,
                                               self._p(self._status)), "gci_bam_allele_size")
        if check:
            self._raise_status(self._status.item(), "gci_bam_allele_size", rec_idx_base)
        ends = np.cumsum([0] + [int(c) for c in counts[1:5]]).tolist()
        out = self.T.empty((max(ends[4], 1), 4), self.T.int32, self.device)
        self._chk(self.lib.gci_bam_allele_write(self.ctx, self._p(d_stream), int(d_stream.shape[0]), self._p(d_rec_off), n, int(has_seq),
                                                self._p(d_codes), self._p(out), ends[4], self._p(self._status)), "gci_bam_allele_write")
        return (*(out[ends[k]:ends[k + 1]] for k in range(4)), [int(c) for c in counts])

    def allele_sites(self, a: Buffer, c: Buffer, g: Buffer, t: Buffer, depth: Buffer, codes: Buffer, min_reads: int, frac_ppm: int,
                     windows: Sequence[Tuple[int, int]] = ()) -> np.ndarray:
        """-> ALLELE_SITE_DTYPE [n]: the single elements where the largest of the four allele tracks is >= min_reads and * 1000000 >=
        frac_ppm * depth, inside the sorted, disjoint [begin, end) windows of track elements (none: every contig), in ascending order:
        contig, pos, ref (the code in `codes` there), alt (1, 2, 4 or 8: the first of A, C, G, T that reaches the largest), the four
        counts and the depth."""
        nw = len(windows)
        arr = self._window_array(windows)
        n = ctypes.c_uint64(0)
        head = (self.ctx, self._p(a), self._p(c), self._p(g), self._p(t), self._p(depth), self._p(codes), int(min_reads), int(frac_ppm), arr, nw)
        self._chk(self.lib.gci_allele_sites_size(*head, ctypes.byref(n)), "gci_allele_sites_size")
        total = int(n.value)
        if total == 0:
            return np.zeros(0, dtype=ALLELE_SITE_DTYPE)
        out = self.T.empty((total, 9), self.T.int32, self.device)
        self._chk(self.lib.gci_allele_sites_write(*head, self._p(out), total), "gci_allele_sites_write")
        return np.ascontiguousarray(out.cpu().numpy()).view(ALLELE_SITE_DTYPE).reshape(-1)[:total]

    def track_add(self, acc: Buffer, add: Buffer) -> Buffer:
        """acc += add over the layout."""
        self._chk(self.lib.gci_track_add(self.ctx, self._p(acc), self._p(add)), "gci_track_add")
        return acc

    def _raise_status(self, w: int, what: str, base: int = 0) -> None:
        """A status word of the library as a GciError (none for a clean one); `base`: what the word's record index counts from."""
        rec = ctypes.c_uint32(0)
        st = self.lib.gci_decode_status(int(w) & _M64, ctypes.byref(rec))
        if st != 0:
            raise GciError(st, "%s: %s (record %d)" % (what, self.lib.gci_strerror(st).decode(), rec.value + base), rec=int(rec.value) + base)

    def check_status(self, what: str) -> None:
        self._raise_status(self._status.item(), what)

    # ---- R5 ----------------------------------------------------------------------------------
    def set_join_mode(self, mode: str = "auto") -> None:
        """'auto' (by size), 'classic' (open-addressing table in HBM) or 'partition' (radix partition + tables in LDS)."""
        self.join_mode = {"auto": 0, "classic": 1, "partition": 2}[mode]
        self._chk(self.lib.gci_join_mode(self.ctx, self.join_mode), "gci_join_mode")

    def _join_files(self, files: Sequence[JoinInput]):
        arr = (JoinFile * len(files))()
        for i, f in enumerate(files):
            arr[i].d_recs = f.recs.data_ptr()
            arr[i].n_recs = int(f.recs.shape[0])
            arr[i].name_delta = int(f.name_delta)
            arr[i].d_name_base = f.name_base.data_ptr()
            arr[i].d_name_off = f.name_off.data_ptr()
        return arr

    def name_join(self, files: Sequence[JoinInput], ovlp_percent: float, contig_map: Optional[Buffer] = None,
                  out: Optional[Buffer] = None, count: Optional[Buffer] = None, check: bool = True,
                  count_flank: Optional[int] = None, fallback: bool = True,
                  status: Optional[Buffer] = None) -> Tuple[Buffer, Buffer]:
        """-> (intervals int32 [cap, 4], device count).  With check=True the count is read back,
        capacity is grown if needed and the record-level status is raised.

        count_flank = the flank of the depth build that follows: gci_name_join_count then does that build's counting
        pass inside the join (pass counted=True to depth_build_fused / depth_build)."""
        total = sum(int(f.recs.shape[0]) for f in files)
        if out is None:
            out = self.T.empty((max(total, 1), 4), self.T.int32, self.device)
        if count is None:
            count = self.T.zeros(1, self.T.int32, self.device)
        arr = self._join_files(files)
        st_word = self._status if status is None else status          # status: the caller reads the word later (check=False)
        while True:
            if count_flank is None:
                st = self.lib.gci_name_join(self.ctx, arr, len(files), float(ovlp_percent), self._p(contig_map),
                                            self._p(out), int(out.shape[0]), self._p(count), self._p(st_word))
            else:
                st = self.lib.gci_name_join_count(self.ctx, arr, len(files), float(ovlp_percent), self._p(contig_map),
                                                  self._p(out), int(out.shape[0]), self._p(count), self._p(st_word),
                                                  int(count_flank))
            self._chk(st, "gci_name_join")
            if not check:
                return out, count
            try:
                self.check_status("gci_name_join")
            except GciError as e:
                # the partitioned join (large inputs) found more distinct names in one hash bucket than its LDS table
                # holds -- only adversarial names get there: redo on the classic global table
                if e.status != _lib.GCI_E_CAPACITY or not fallback:
                    raise
                self._chk(self.lib.gci_join_mode(self.ctx, 1), "gci_join_mode")
                try:
                    return self.name_join(files, ovlp_percent, contig_map, out, count, True, count_flank, False)
                finally:
                    self._chk(self.lib.gci_join_mode(self.ctx, self.join_mode), "gci_join_mode")
            n = int(count.item())
            if n <= out.shape[0]:
                return out, count
            out = self.T.empty((n, 4), self.T.int32, self.device)

    def name_join_fate(self, files: Sequence[JoinInput], ovlp_percent: float, check: bool = True):
        """-> (per file the join's byte of every record uint8 [n] on the device, per file the records per byte as a list of
        JOIN_FATE_CLASSES ints): what the cross-file join does with every record and why (include/gci_hip.h: gci_name_join_fate).
        check: a zero qlen the join divides by raises GciError with .file (index in `files`) and .rec (the record's rec_idx)."""
        n = len(files)
        fate = [self.T.empty(max(int(f.recs.shape[0]), 1), self.T.uint8, self.device) for f in files]
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in fate])
        counts = (ctypes.c_uint64 * (n * _lib.JOIN_FATE_CLASSES))()
        self._chk(self.lib.gci_name_join_fate(self.ctx, self._join_files(files), n, float(ovlp_percent), ptrs, counts, self._p(self._status)),
                  "gci_name_join_fate")
        if check:
            self.check_status("gci_name_join_fate")
        k = _lib.JOIN_FATE_CLASSES
        return [t[:int(f.recs.shape[0])] for t, f in zip(fate, files)], [[int(c) for c in counts[f * k:(f + 1) * k]] for f in range(n)]

    def fate_refine(self, classes: Buffer, join_fate: Buffer, check: bool = True, rec_idx_base: int = 0) -> Buffer:
        """classes[i] == kept becomes join_fate[i] (gci_fate_refine); a record the two passes disagree about raises GciError."""
        n = int(classes.shape[0])
        if int(join_fate.shape[0]) != n:
            raise GciError(_lib.GCI_E_INVALID, "gci_fate_refine: %d class bytes, %d join bytes" % (n, int(join_fate.shape[0])))
        self._chk(self.lib.gci_fate_refine(self.ctx, self._p(classes), self._p(join_fate), n, self._p(self._status)), "gci_fate_refine")
        if check:
            self._raise_status(self._status.item(), "gci_fate_refine", rec_idx_base)
        return classes

    # ---- R7 / N2: gzip members of the depth text, written on the device ----------------------------------------
    MEMBER_BASES = 64 * 4096

    def depth_deflate(self, track: Buffer, from_build: bool = False) -> List[bytes]:
        """-> per contig of the layout, the bytes of the gzip members whose payload is that contig's depth lines
        (f'{depth}\\n' per base, GCI.py:115-117; no '>' line), as memoryviews of a pinned buffer the engine reuses: valid until
        the next call.  gci_depth_deflate_size / _write.  from_build: the caller states that `track` is exactly what the last
        depth_build_fused(want_runs=True) of THIS engine wrote and that nothing has written it since (no other engine, no torch
        operation): the members are then encoded from the run lists that build kept and the track is not read
        (gci_depth_deflate_from_build; the lists serve one call)."""
        elem, cnt, first = [], [], [0]
        for off, length in zip(self.offsets, self.lengths):
            for g in range(0, int(length), self.MEMBER_BASES):
                elem.append(int(off) + g)
                cnt.append(min(self.MEMBER_BASES, int(length) - g))
            first.append(len(elem))
        nm = len(elem)
        if nm == 0:
            return [b"" for _ in self.lengths]
        d_elem = self.to_device(np.asarray(elem, dtype=np.uint64))
        d_cnt = self.to_device(np.asarray(cnt, dtype=np.uint32))
        dev = self.device
        tile_bytes = self.T.empty(nm * 64, self.T.int32, dev)
        mb, crc, isz = (self.T.empty(nm, self.T.int32, dev) for _ in range(3))
        if from_build:
            self._chk(self.lib.gci_depth_deflate_from_build(self.ctx, self._p(track)), "gci_depth_deflate_from_build")
        self._chk(self.lib.gci_depth_deflate_size(self.ctx, self._p(track), self._p(d_elem), self._p(d_cnt), nm, self._p(tile_bytes),
                                                  self._p(mb), self._p(crc), self._p(isz)), "gci_depth_deflate_size")
        # member offsets on the device (no round trip through the host for them); one sync for the total
        d_off64 = self.T.scan_u32_u64(mb)
        total = int(d_off64[nm].item())
        out = self.T.empty(total, self.T.uint8, dev)
        self._chk(self.lib.gci_depth_deflate_write(self.ctx, self._p(track), self._p(d_elem), self._p(d_cnt), nm, self._p(tile_bytes),
                                                   self._p(crc), self._p(isz), self._p(d_off64), self._p(out), total),
                  "gci_depth_deflate_write")
        # the members leave through a pinned staging buffer of the engine (a pageable destination halves the D2H rate and
        # .tobytes() per contig copied everything once more): the caller gets views of it, valid until the next call
        if self._members_host is None or int(self._members_host.shape[0]) < total:
            self._members_host = self.T.pinned(max(total + (total >> 3), 1 << 20))
        host = self._members_host[:total]
        host.copy_(out, non_blocking=True)
        offs = d_off64.cpu().numpy()
        self.sync()
        blob = host.numpy()
        return [memoryview(blob[int(offs[first[c]]):int(offs[first[c + 1]])]) for c in range(len(self.lengths))]

    def hash_bucket(self, recs: Buffer, n_parts: int, part_cap: int, out: Buffer,
                    next_out: Optional[Buffer] = None) -> None:
        """out: int64 [n_parts * (part_cap + 1)]; word 0 of each bucket = its count.  next_out: the array the caller
        alternates with `out` (its count words are zeroed for the next call; `out`'s must be zero on entry)."""
        self._chk(self.lib.gci_hash_bucket(self.ctx, self._p(recs), int(recs.shape[0]), int(n_parts), int(part_cap),
                                           self._p(out), self._p(next_out)), "gci_hash_bucket")

    def hash_conflicts(self, buckets: Buffer, n_parts: int, part_cap: int, n_conflicts: Buffer) -> None:
        """Adds to n_conflicts (int32 [1])."""
        self._chk(self.lib.gci_hash_conflicts(self.ctx, self._p(buckets), int(n_parts), int(part_cap),
                                              self._p(n_conflicts)), "gci_hash_conflicts")

    # ---- multi-GPU: buckets of the name-hash-sharded join (gci_route_*; the collectives are shard.ShardedJoin's) ----------
    def route_records(self, f: JoinInput, n_parts: int, cap: int, out_recs: Buffer, out_names: Buffer,
                      name_slot: int, status: Buffer) -> None:
        """out_recs uint8 [n_parts * (cap + 1), 32], out_names uint8 [n_parts * cap * name_slot], status int64 [1]."""
        self._chk(self.lib.gci_route_records(self.ctx, self._join_files([f]), int(n_parts), int(cap), self._p(out_recs),
                                             self._p(out_names), int(name_slot), self._p(status)), "gci_route_records")

    def route_seal_records(self, recs: Buffer, n_parts: int, cap: int, status: Buffer) -> None:
        self._chk(self.lib.gci_route_seal_records(self.ctx, self._p(recs), int(n_parts), int(cap), self._p(status)),
                  "gci_route_seal_records")

    def route_intervals(self, ivl: Buffer, count: Buffer, owner: Buffer, n_parts: int, cap: int,
                        out: Buffer, status: Buffer) -> None:
        """owner int32 [n_contigs]: rank of every contig; out int32 [n_parts * (cap + 1), 4]."""
        self._chk(self.lib.gci_route_intervals(self.ctx, self._p(ivl), self._p(count), int(ivl.shape[0]), self._p(owner),
                                               int(owner.shape[0]), int(n_parts), int(cap), self._p(out), self._p(status)),
                  "gci_route_intervals")

    def route_seal_intervals(self, ivl: Buffer, n_parts: int, cap: int, cmap: Buffer, status: Buffer) -> None:
        self._chk(self.lib.gci_route_seal_intervals(self.ctx, self._p(ivl), int(n_parts), int(cap), self._p(cmap),
                                                    int(cmap.shape[0]), self._p(status)), "gci_route_seal_intervals")

    def pack_names(self, f: JoinInput) -> Tuple[Buffer, Buffer]:
        n = int(f.recs.shape[0])
        off = self.T.zeros(n + 1, self.T.int64, self.device)
        arr = self._join_files([f])
        self._chk(self.lib.gci_pack_names(self.ctx, arr, None, 0, self._p(off)), "gci_pack_names(size)")
        total = int(off[n].item())
        blob = self.T.empty(max(total, 1), self.T.uint8, self.device)
        self._chk(self.lib.gci_pack_names(self.ctx, arr, self._p(blob), total, self._p(off)), "gci_pack_names")
        return blob[:total], off

    # ---- N1: BGZF inflate + record walk on the device (k_inflate.hip, k_records.hip) ---------------------------------------------------
    def upload_padded(self, raw: np.ndarray) -> Buffer:
        """The bytes of a BGZF file on the device with 16 readable bytes behind them (gci_bgzf_inflate_device takes its
        input as whole aligned 16-byte blocks)."""
        n_raw = int(raw.shape[0])
        with self.T.stream(self.stream), warnings.catch_warnings():      # (may be called from a helper thread)
            warnings.simplefilter("ignore", UserWarning)                     # a read-only memmap is only read
            d_raw = self.T.empty(n_raw + 16, self.T.uint8, self.device)
            d_raw[n_raw:].zero_()
            d_raw[:n_raw].copy_(self._host_src(raw))
        return d_raw

    def _member_table(self, pos: np.ndarray, isize: np.ndarray) -> Tuple[int, int, Buffer, Buffer]:
        """-> (members, inflated bytes, on the device: where every member begins in the file and in the inflated stream)."""
        n = int(isize.shape[0])
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(isize, out=off[1:])
        return n, int(off[n]), self.to_device(np.ascontiguousarray(pos[:n + 1], dtype=np.uint64)), self.to_device(off)

    def bgzf_inflate(self, raw: Optional[np.ndarray], pos: np.ndarray, isize: np.ndarray, check_crc: bool = True,
                     prefix: Optional[Buffer] = None, d_raw: Optional[Buffer] = None) -> Buffer:
        """raw: the bytes of a BGZF file (or of a run of its members) -- or d_raw, the same already on the device
        (upload_padded); pos (uint64, n + 1) / isize (uint64, n): its member table (hostio.bgzf_blocks), pos relative to
        raw.  -> the inflated bytes on the device, behind the bytes of `prefix` (the partial record a previous run of
        members ended in).  Raises GciError(GCI_E_MALFORMED, rec = member) on a bad member / CRC."""
        n_pre = int(prefix.shape[0]) if prefix is not None else 0
        if d_raw is None:
            d_raw = self.upload_padded(raw)
        n, total, d_pos, d_off = self._member_table(pos, isize)
        # (sizes in steps of 256 MiB: the runs of a file differ by a few MB, and a request a little larger than the block the run before
        #  gave back is a new device allocation -- 44 ms beside a copy in flight -- where the same step finds that block again)
        want = max(n_pre + total, 1)
        out = self.T.empty(((want + (1 << 28) - 1) >> 28) << 28 if want > (1 << 28) else want, self.T.uint8, self.device)
        if n_pre:
            out[:n_pre].copy_(prefix)
        self._chk(self.lib.gci_bgzf_inflate_device(self.ctx, self._p(d_raw), self._p(d_pos), self._p(d_off), n, ctypes.c_void_p(out.data_ptr() + n_pre), total,
                                                   int(check_crc), self._p(self._status)), "gci_bgzf_inflate_device")
        self.check_status("gci_bgzf_inflate_device")
        return out[:n_pre + total]

    def bgzf_inflate_ahead(self, d_raw: Buffer, pos: np.ndarray, isize: np.ndarray, headroom: int, check_crc: bool = True
                           ) -> Tuple[Buffer, Buffer, int]:
        """bgzf_inflate() for a run of members of a file that goes through the device run by run, ENQUEUED and not waited for: the
        inflated bytes go `headroom` bytes into a fresh buffer (in front of them the caller later puts the partial record the run
        before ended in -- which it knows only when that run has been walked, while this run is already being inflated) and the
        status word into a buffer of its own, which the caller checks (check_status_word) once it has made its stream wait for this
        one.  -> (buffer of headroom + total bytes, status word, total)."""
        n, total, d_pos, d_off = self._member_table(pos, isize)
        want = max(int(headroom) + total, 1)
        out = self.T.empty(((want + (1 << 28) - 1) >> 28) << 28 if want > (1 << 28) else want, self.T.uint8, self.device)
        status = self.T.empty(1, self.T.int64, self.device)
        self._chk(self.lib.gci_bgzf_inflate_device(self.ctx, self._p(d_raw), self._p(d_pos), self._p(d_off), n, ctypes.c_void_p(out.data_ptr() + int(headroom)),
                                                   total, int(check_crc), self._p(status)), "gci_bgzf_inflate_device")
        return out[:int(headroom) + total], status, total

    def check_status_word(self, status: Buffer, what: str) -> None:
        """check_status() over a status word of the caller's (read on the calling thread's current stream)."""
        self._raise_status(status.item(), what)

    def inflate_stats(self) -> dict:
        """How the members of the last bgzf_inflate fared with the wave decoder (gci_bgzf_inflate_last_stats; synchronises)."""
        c = (ctypes.c_uint32 * 32)()
        self._chk(self.lib.gci_bgzf_inflate_last_stats(self.ctx, c), "gci_bgzf_inflate_last_stats")
        names = ("decoded", "header", "no meeting point", "false end of block", "undecodable", "length", "lanes") + tuple("cause %d" % k for k in range(7, 31)) + ("not tried",)
        return {k: int(v) for k, v in zip(names, c) if v or k in ("decoded", "not tried")}

    def inflate_round(self) -> int:
        """Members gci_bgzf_inflate_device decodes at a time on this device (0: unknown)."""
        return int(self.lib.gci_bgzf_inflate_round(self.ctx))

    def start_upload(self, raw: np.ndarray, parts: int = 2):
        """Begin uploading the bytes of a BGZF file in `parts` pieces on a copy stream of its own (a helper thread: the
        copies come from pageable memory and block their caller) -> a handle for bgzf_inflate_uploaded, which starts
        inflating the members of a piece as soon as that piece has arrived."""
        n_raw = int(raw.shape[0])
        cuts = sorted({min(n_raw, (n_raw * (k + 1) // parts + 15) & ~15) for k in range(parts)} | {n_raw})
        d_raw = self.T.empty(n_raw + 16, self.T.uint8, self.device)
        copy_stream = self.copy_stream()                         # (creating a stream costs milliseconds: one per engine)
        copy_stream.wait_stream(self.stream)                     # (the allocation may recycle memory still in use on the main stream)
        events = [self.T.Event() for _ in cuts]
        queued = [threading.Event() for _ in cuts]               # (a CUDA event that was never recorded counts as complete)

        def run():
            with self.T.stream(copy_stream), warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)     # a read-only memmap is only read
                d_raw[n_raw:].zero_()
                lo = 0
                for k, hi in enumerate(cuts):
                    if hi > lo:
                        d_raw[lo:hi].copy_(self._host_src(raw[lo:hi]))
                    events[k].record(copy_stream)
                    queued[k].set()
                    lo = hi
            return True

        return _Upload(d_raw, cuts, events, queued, copy_stream, run)

    def bgzf_inflate_uploaded(self, up, pos: np.ndarray, isize: np.ndarray, check_crc: bool = True) -> Buffer:
        """bgzf_inflate over a file whose upload start_upload began: one launch per uploaded piece, over the members that lie
        wholly inside what has arrived (and the 16 bytes the decoder may read behind a member)."""
        n, total, d_pos, d_off = self._member_table(pos, isize)
        out = self.T.empty(max(total, 1), self.T.uint8, self.device)
        ends = np.asarray(pos[1:n + 1], dtype=np.uint64)
        n_raw = int(up.d_raw.shape[0]) - 16
        status = self.T.zeros(len(up.cuts), self.T.int64, self.device)
        m_lo, bases = 0, []
        try:
            for k, (cut, ev) in enumerate(zip(up.cuts, up.events)):
                m_hi = n if cut >= n_raw else int(np.searchsorted(ends, np.uint64(max(0, cut - 16)), side="right"))
                m_hi = max(m_hi, m_lo)
                while not up.queued[k].wait(0.05):
                    if up.future.done():
                        up.future.result()                    # the upload failed: its exception, not a hang
                        break
                self.stream.wait_event(ev)
                bases.append(m_lo)
                if m_hi > m_lo:
                    self._chk(self.lib.gci_bgzf_inflate_device(self.ctx, self._p(up.d_raw), ctypes.c_void_p(d_pos.data_ptr() + 8 * m_lo),
                                                               ctypes.c_void_p(d_off.data_ptr() + 8 * m_lo), m_hi - m_lo, self._p(out), total,
                                                               int(check_crc), ctypes.c_void_p(status.data_ptr() + 8 * k)), "gci_bgzf_inflate_device")
                else:
                    status[k] = -1
                m_lo = m_hi
            up.future.result()
        finally:
            up.close()
        for k, w in enumerate(status.cpu().numpy().view(np.uint64).tolist()):
            self._raise_status(w, "gci_bgzf_inflate_device", bases[k])
        self.stream.wait_stream(up.stream)
        return out[:total]

    def bam_record_offsets(self, d_stream: Buffer, first_record: int, n_ref: int) -> Tuple[Buffer, int, bool]:
        """-> (int64 offsets of every record on the device, bytes consumed, chain_ok).  chain_ok False: a record the strict
        format test rejects sits on the chain -- the caller walks the chain on the host instead."""
        n = int(d_stream.shape[0])
        res = self.T.zeros(3, self.T.int64, self.device)
        cap = max(1024, n // 256)
        while True:
            offs = self.T.empty(cap, self.T.int64, self.device)
            self._chk(self.lib.gci_bam_record_offsets_device(self.ctx, self._p(d_stream), n, int(first_record), int(n_ref), self._p(offs), cap,
                                                             self._p(res)), "gci_bam_record_offsets_device")
            n_rec, used, broken = (int(x) for x in res.cpu().tolist())
            if n_rec <= cap:
                return offs[:n_rec], used, broken == 0
            cap = n_rec

    # ---- R3 / N4: the PAF path of filter() on the device (k_paf.hip) -----------------------------------------------
    def paf_filter(self, paths: Sequence[str], targets: Sequence[str], map_qual: int, mq_cutoff: int, iden_percent: float
                   ) -> List[JoinInput]:
        """gci_paf_filter_device over the PAF files `paths` (command-line order): -> one JoinInput per file, holding a
        compact record per query seen so far (files < i included: the reference never resets its block table) and
        pointing at the names inside the uploaded text.  Raises GciError with .rec = the 1-based line the reference
        would have raised on (GCI_E_MALFORMED: IndexError / ValueError, GCI_E_ZERO_DIV: ZeroDivisionError)."""
        sizes = [int(os.path.getsize(p)) for p in paths]
        ends = np.cumsum(sizes, dtype=np.uint64) if sizes else np.zeros(0, np.uint64)
        total = int(ends[-1]) if sizes else 0
        if total < int(os.environ.get("GCI_PAF_STAGE_MIN", str(256 << 20))):          # (small files: read, put together, one copy)
            bufs = [np.fromfile(p, dtype=np.uint8) for p in paths]
            text = np.concatenate(bufs) if bufs and total else np.zeros(1, np.uint8)
            return self.paf_filter_text(self.to_device(text), ends, targets, map_qual, mq_cutoff, iden_percent)
        # Files of GBs (the reference's published CHM13 run reads a 3.6 GB HiFi and a 48 GB ONT PAF, README.md:321): their bytes go
        # from the mapped files through the ring of pinned slots straight to their places in ONE device buffer -- round 5 read every
        # file into host memory, concatenated the arrays and handed the result to a pageable copy: three passes over 52 GB of host
        # memory and 104 GB of it held, before the first byte moved
        d_text = self.T.empty(total, self.T.uint8, self.device)
        staging, copy = self.staging(), self.copy_stream()
        copy.wait_stream(self.stream)
        at = 0
        for p, n in zip(paths, sizes):
            if n:
                raw = np.memmap(p, dtype=np.uint8, mode="r")
                staging.send(raw, 0, n, d_text[at:at + n], copy)
                del raw
            at += n
        self.stream.wait_stream(copy)
        return self.paf_filter_text(d_text, ends, targets, map_qual, mq_cutoff, iden_percent)

    def paf_filter_text(self, d_text: Buffer, ends: np.ndarray, targets: Sequence[str], map_qual: int, mq_cutoff: int,
                        iden_percent: float) -> List[JoinInput]:
        """paf_filter() over PAF text that is on the device already: the bytes of all files back to back, ends[i] = end offset
        of file i."""
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        bufs = list(range(int(ends.shape[0])))
        tnames = [t.encode() for t in targets]
        tarr = (ctypes.c_char_p * max(len(tnames), 1))(*tnames)
        handle, line = ctypes.c_void_p(None), ctypes.c_uint64(0)
        st = self.lib.gci_paf_filter_device(self.ctx, self._p(d_text), ends.ctypes.data_as(ctypes.c_void_p), len(bufs), tarr,
                                            len(tnames), int(map_qual), int(mq_cutoff), float(iden_percent), ctypes.byref(handle),
                                            ctypes.byref(line))
        if st != 0:
            detail = self.lib.gci_last_error(self.ctx).decode() if st == _lib.GCI_E_HIP else ""
            raise GciError(st, "gci_paf_filter_device: %s (line %d) %s" % (self.lib.gci_strerror(st).decode(), line.value, detail),
                           rec=int(line.value))
        try:
            return self._paf_dev_inputs(handle, len(bufs), d_text)
        finally:
            self.lib.gci_paf_dev_free(handle)

    def paf_global_groups(self) -> int:
        """Workgroups of the tokeniser that walked global memory instead of an LDS copy in the last paf_filter*() / paf_hits_text()."""
        return int(self.lib.gci_paf_global_groups(self.ctx))

    # ---- the PAF filter in two halves (runs that shard a PAF file by byte range: shard.paf_by_byte_range) ----
    PAF_HIT_BYTES = 80

    def _paf_dev_inputs(self, handle, n_files: int, d_names: Buffer) -> List[JoinInput]:
        out = []
        for f in range(n_files):
            n = int(self.lib.gci_paf_dev_count(handle, f))
            recs = self.T.empty((max(n, 1), 32), self.T.uint8, self.device)
            off = self.T.empty(max(n, 1), self.T.int64, self.device)
            self._chk(self.lib.gci_paf_dev_export(handle, f, self._p(recs), self._p(off)), "gci_paf_dev_export")
            out.append(JoinInput(recs[:n], d_names, off[:n], 0))
        self.sync()
        return out

    def paf_hits_text(self, d_text: Buffer, ends: np.ndarray, targets: Sequence[str], map_qual: int, mq_cutoff: int,
                      iden_percent: float) -> List[Buffer]:
        """Stage A (gci_paf_hits_device) over the byte ranges in d_text (ends[i] = end of file i's range): per file the lines
        that pass, as a uint8 tensor [n, 80] of gci_paf_hit in line order (qn_off points into d_text)."""
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        n_files = int(ends.shape[0])
        tnames = [t.encode() for t in targets]
        tarr = (ctypes.c_char_p * max(len(tnames), 1))(*tnames)
        handle, line = ctypes.c_void_p(None), ctypes.c_uint64(0)
        st = self.lib.gci_paf_hits_device(self.ctx, self._p(d_text), ends.ctypes.data_as(ctypes.c_void_p), n_files, tarr, len(tnames),
                                          int(map_qual), int(mq_cutoff), float(iden_percent), ctypes.byref(handle), ctypes.byref(line))
        if st != 0:
            raise GciError(st, "gci_paf_hits_device: %s (line %d of the range)" % (self.lib.gci_strerror(st).decode(), line.value),
                           rec=int(line.value))
        try:
            out = []
            for f in range(n_files):
                n = int(self.lib.gci_paf_hits_count(handle, f))
                h = self.T.empty((max(n, 1), self.PAF_HIT_BYTES), self.T.uint8, self.device)
                self._chk(self.lib.gci_paf_hits_export(handle, f, self._p(h)), "gci_paf_hits_export")
                out.append(h[:n])
            self.sync()
            return out
        finally:
            self.lib.gci_paf_hits_free(handle)

    def route_hits(self, hits: Buffer, d_name_base: Buffer, n_parts: int, cap: int, out_hits: Buffer,
                   out_names: Buffer, name_slot: int, status: Buffer) -> None:
        """gci_route_hits: hits [n, 80] -> out_hits [n_parts * (cap + 1), 80] (slot 0 of a bucket: header, qhash = count), their
        query names into out_names [n_parts * cap * name_slot]."""
        n = int(hits.shape[0])
        self._chk(self.lib.gci_route_hits(self.ctx, self._p(hits) if n else None, n, self._p(d_name_base), int(n_parts), int(cap),
                                          self._p(out_hits), self._p(out_names), int(name_slot), self._p(status)), "gci_route_hits")

    def paf_score_hits(self, d_names: Buffer, d_hits: Buffer, upto: Sequence[int], targets: Sequence[str]) -> List[JoinInput]:
        """Stage B (gci_paf_score_device): d_hits [total, 80] = the hits of the queries this rank owns, file after file
        (upto[f] = first hit of file f, upto[-1] = total), qn_off relative to d_names -> one JoinInput per file."""
        n_files = len(upto) - 1
        h_upto = np.ascontiguousarray(upto, dtype=np.uint32)
        tnames = [t.encode() for t in targets]
        tarr = (ctypes.c_char_p * max(len(tnames), 1))(*tnames)
        handle = ctypes.c_void_p(None)
        st = self.lib.gci_paf_score_device(self.ctx, self._p(d_names), self._p(d_hits) if int(h_upto[-1]) else None,
                                           h_upto.ctypes.data_as(ctypes.c_void_p), n_files, tarr, len(tnames), ctypes.byref(handle))
        if st != 0:
            raise GciError(st, "gci_paf_score_device: %s" % self.lib.gci_strerror(st).decode(), rec=0)
        try:
            return self._paf_dev_inputs(handle, n_files, d_names)
        finally:
            self.lib.gci_paf_dev_free(handle)

    # ---- R6 / R8 / R9 / R15 --------------------------------------------------------------------
    def depth_build(self, ivl: Buffer, count: Optional[Buffer], flank: int, track: Buffer,
                    max_n: Optional[int] = None) -> Buffer:
        n = int(ivl.shape[0]) if max_n is None else int(max_n)
        st = self.lib.gci_depth_build(self.ctx, self._p(ivl) if n else None, self._p(count), n, int(flank),
                                      self._p(track))
        self._chk(st, "gci_depth_build")
        return track

    def depth_build_fused(self, ivl: Buffer, count: Optional[Buffer], flank: int, track: Buffer,
                          want_text: bool = True, want_sums: bool = False,
                          issue: Optional[Tuple[float, float, int]] = None, max_n: Optional[int] = None,
                          counted: bool = False, key_cap: int = 1 << 16, want_runs: bool = False):
        """Depth build that also returns what the reference derives from the fresh depths, computed in
        the same pass (no re-read of the track): decimal text, per-contig sums and -- only valid when
        no gap mask follows -- the raw issue runs for (lo, hi, flank).  want_runs: the library keeps the constant-depth runs of
        every tile as the build wrote them, and a depth_deflate() of this track -- before anything else writes it -- takes them
        from there instead of reading the track (gci_build_opts.want_runs).

        -> dict(text=uint8 tensor | None, text_off=int64 ndarray | None, sums=ndarray | None,
                runs=list of per-contig arrays | None)"""
        n = int(ivl.shape[0]) if max_n is None else int(max_n)
        nc = len(self.lengths)
        o = BuildOpts()
        o.flank = int(flank)
        o.counted = 1 if counted else 0
        o.want_text = 1 if want_text else 0
        o.want_runs = 1 if want_runs else 0
        text_off = self.T.zeros(nc + 1, self.T.int64, self.device) if want_text else None
        # want_sums: True = per-contig sums returned as a host array; a device tensor (int64 [n_contigs]) = written there, nothing copied
        sums_dev = want_sums if self.T.is_buffer(want_sums) else None
        want_sums = bool(sums_dev is not None or want_sums is True)
        sums = sums_dev if sums_dev is not None else (self.T.zeros(max(nc, 1), self.T.int64, self.device) if want_sums else None)
        o.d_contig_text_off = text_off.data_ptr() if want_text else None
        o.d_sums = sums.data_ptr() if want_sums else None
        cap = int(key_cap)                                 # grown (and the first pass repeated) when more run boundaries turn up
        keys = None
        while True:
            if issue is not None:
                keys = self.T.empty(cap, self.T.int64, self.device)
                o.d_n_keys, o.d_keys, o.key_cap = self._count.data_ptr(), keys.data_ptr(), cap
                o.lo, o.hi, o.issue_flank = float(issue[0]), float(issue[1]), int(issue[2])
            self._chk(self.lib.gci_depth_build_begin(self.ctx, self._p(ivl) if n else None, self._p(count), n,
                                                     ctypes.byref(o)), "gci_depth_build_begin")
            if issue is None:
                break
            nk = int(self._count.item())
            if nk <= cap:
                break
            cap = nk
            o.counted = 0                                  # the join's counts are used up: the second begin counts again
        out = dict(text=None, text_off=None, sums=None, runs=None)
        text = None
        if want_text:
            h = text_off.cpu().numpy()
            total = int(h[nc])
            text = self.T.empty(max(total, 1), self.T.uint8, self.device)
            out["text_off"] = h
        self._chk(self.lib.gci_depth_build_finish(self.ctx, self._p(track), self._p(text), int(text.shape[0]) if want_text else 0),
                  "gci_depth_build_finish")
        if want_text:
            out["text"] = text[:int(out["text_off"][nc])]
        if want_sums:
            out["sums"] = sums if sums_dev is not None else sums.cpu().numpy()[:nc]
        if issue is not None:
            out["runs"] = self._keys_to_runs(keys[:nk].cpu().numpy().view(np.uint64), nc)
        return out

    def gap_mask(self, track: Buffer, gaps: Buffer) -> Buffer:
        n = int(gaps.shape[0])
        if n:
            self._chk(self.lib.gci_gap_mask(self.ctx, self._p(track), self._p(gaps), n), "gci_gap_mask")
        return track

    def max2(self, a: Buffer, b: Buffer, out: Optional[Buffer] = None) -> Buffer:
        if out is None:
            out = self.new_track()
        self._chk(self.lib.gci_max2(self.ctx, self._p(a), self._p(b), self._p(out)), "gci_max2")
        return out

    def two_type_tail(self, a: Buffer, b: Buffer, gaps: Optional[np.ndarray], lo: float, hi: float, flank: int,
                      out: Optional[Buffer] = None, keys: Optional[Buffer] = None, n_keys: Optional[Buffer] = None,
                      read: bool = True, sums: Optional[Buffer] = None):
        """gci_two_type_tail: N-run masks of both tracks (in place; gaps = int32 [n, 4] rows (contig, start, end, 0) on the HOST, or
        None), their maximum and the issue runs of all three in one pass.  -> (maximum track, [runs of a, of b, of the maximum]);
        read=False: (maximum track, keys int64 [3, cap] on the device, n_keys int32 [3]) with nothing copied to the host.
        sums: int64 [3, n_contigs] on the device, filled with the per-contig sums of depth of the three tracks."""
        if out is None:
            out = self.new_track()
        g = np.ascontiguousarray(gaps, dtype=np.int32).reshape(-1, 4) if gaps is not None and len(gaps) else None
        cap = int(keys.shape[1]) if keys is not None else 1 << 16
        while True:
            if keys is None:
                keys = self.T.empty((3, cap), self.T.int64, self.device)
            if n_keys is None:
                n_keys = self.T.zeros(3, self.T.int32, self.device)
            self._chk(self.lib.gci_two_type_tail(self.ctx, self._p(a), self._p(b), self._p(out),
                                                 ctypes.c_void_p(g.ctypes.data) if g is not None else None, 0 if g is None else int(g.shape[0]),
                                                 float(lo), float(hi), int(flank), self._p(keys), cap, self._p(n_keys), self._p(sums)),
                      "gci_two_type_tail")
            if not read:
                return out, keys, n_keys
            n = n_keys.cpu().numpy()
            if int(n.max()) <= cap:
                break
            cap, keys = int(n.max()), None                  # (masking again changes nothing; the maximum is recomputed)
        hk = keys.cpu().numpy().view(np.uint64)
        return out, [self._keys_to_runs(hk[x, :int(n[x])], len(self.lengths)) for x in range(3)]

    def depth_sum(self, track: Buffer) -> np.ndarray:
        sums = self.T.zeros(max(len(self.lengths), 1), self.T.int64, self.device)
        self._chk(self.lib.gci_depth_sum(self.ctx, self._p(track), self._p(sums)), "gci_depth_sum")
        return sums.cpu().numpy()[:len(self.lengths)]

    def fasta_n_scan(self, text: np.ndarray, bodies: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """gci_fasta_n_scan over the bytes of a FASTA file: bodies = int64 [n_records, 2] byte ranges of the record
        bodies -> (uint32 kept-byte count per 4096-byte tile, sorted uint64 keys (offset << 1 | is_end))."""
        n = int(text.shape[0])
        d_text = self.upload_staged(text) if n >= (256 << 20) else self.to_device(text)
        d_body = self.to_device(np.ascontiguousarray(bodies, dtype=np.int64).reshape(-1, 2))
        tiles = (n + 4095) // 4096
        kept = self.T.zeros(max(tiles, 1), self.T.int32, self.device)
        cap = 1 << 16
        while True:
            keys = self.T.empty(cap, self.T.int64, self.device)
            self._chk(self.lib.gci_fasta_n_scan(self.ctx, self._p(d_text), n, self._p(d_body), int(bodies.shape[0]), self._p(kept),
                                                self._p(keys), cap, self._p(self._count)), "gci_fasta_n_scan")
            nk = int(self._count.item())
            if nk <= cap:
                break
            cap = nk
        return kept.cpu().numpy().view(np.uint32)[:tiles], np.sort(keys[:nk].cpu().numpy().view(np.uint64))

    def _text_index(self, call, d_text: Buffer, cap: int) -> Tuple[Buffer, np.ndarray, np.ndarray, int]:
        """call(n, counts, keys, cap, n_keys, bad) until every key fitted, then the exclusive scan of the tile counts
        (gci_dev_u32_scan_u64) -> (device uint64 [n_tiles + 1] first line index of every tile, the same on the host, the sorted
        uint64 keys, the smallest offending byte offset or 2**64 - 1)."""
        n = int(d_text.shape[0])
        tiles = (n + 4095) // 4096
        counts = self.T.empty(max(tiles, 1), self.T.int32, self.device)
        bad = self.T.empty(1, self.T.int64, self.device)
        while True:
            keys = self.T.empty(max(cap, 1), self.T.int64, self.device)
            call(n, counts, keys, cap, self._count, bad)
            nk = int(self._count.item())
            if nk <= cap:
                break
            cap = nk
        line0 = self.T.empty(tiles + 1, self.T.int64, self.device)
        self._chk(self.lib.gci_dev_u32_scan_u64(self.device.index or 0, self._p(counts), tiles, self._p(line0),
                                                ctypes.c_void_p(self.stream.cuda_stream)), "gci_dev_u32_scan_u64")
        h_line0 = line0.cpu().numpy().view(np.uint64)
        return line0, h_line0, np.sort(keys[:nk].cpu().numpy().view(np.uint64)), int(bad.cpu().numpy().view(np.uint64)[0])

    def _text_parse(self, fn, what: str, d_text: Buffer, d_line0: Buffer, base: tuple, segs: np.ndarray, track: Buffer) -> Buffer:
        """fn(ctx, text, n, tile_line0, *base, segs, n_segs, track, track_n); segs = int64 [n, 3], sorted, uploaded here."""
        segs = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1, 3)
        d_segs = self.to_device(segs) if segs.shape[0] else None
        self._chk(fn(self.ctx, self._p(d_text), int(d_text.shape[0]), self._p(d_line0), *base, self._p(d_segs), int(segs.shape[0]),
                     self._p(track), int(track.shape[0])), what)
        return track

    def depth_text_index(self, d_text: Buffer) -> Tuple[Buffer, np.ndarray, np.ndarray, int]:
        """gci_depth_text_index + the exclusive scan of its tile counts (gci_dev_u32_scan_u64) over depth text in HBM
        -> (device uint64 [n_tiles + 1] first line index of every tile, the same on the host, sorted uint64 header keys
        (byte offset << 12 | rank in its tile), smallest byte offset of a data line outside the strict grammar or 2**64 - 1)."""
        def call(n, counts, keys, cap, n_keys, bad):
            self._chk(self.lib.gci_depth_text_index(self.ctx, self._p(d_text), n, self._p(counts), self._p(keys), cap, self._p(n_keys),
                                                    self._p(bad)), "gci_depth_text_index")
        return self._text_index(call, d_text, 1 << 12)

    def depth_text_parse(self, d_text: Buffer, d_line0: Buffer, segs: np.ndarray, track: Buffer) -> Buffer:
        """gci_depth_text_parse: segs = int64 [n, 3] (first data line, data lines, track element of the first or -1), sorted."""
        return self._text_parse(self.lib.gci_depth_text_parse, "gci_depth_text_parse", d_text, d_line0, (), segs, track)

    # ---- this project's own .depth.gz to a track without inflating it (k_depth_gz.hip) ------------------------------------
    def depth_gz_scan(self, d_raw: Buffer, cand_pos: np.ndarray) -> np.ndarray:
        """gci_depth_gz_scan over the bytes of a .depth.gz in HBM: one lane per candidate member start -> DGZ_INFO_DTYPE on the host
        (status, end offset, lines, runs, CRC-32 / ISIZE verdicts)."""
        from .formats.depthfile import DGZ_INFO_DTYPE
        cand = np.ascontiguousarray(cand_pos, dtype=np.uint64)
        n = int(cand.shape[0])
        if n == 0:
            return np.zeros(0, dtype=DGZ_INFO_DTYPE)
        d_cand = self.to_device(cand.view(np.int64))
        d_info = self.T.empty(n * DGZ_INFO_DTYPE.itemsize, self.T.uint8, self.device)
        self._chk(self.lib.gci_depth_gz_scan(self.ctx, self._p(d_raw), int(d_raw.shape[0]), self._p(d_cand), n, self._p(d_info)),
                  "gci_depth_gz_scan")
        return d_info.cpu().numpy().view(DGZ_INFO_DTYPE)

    def depth_gz_runs(self, d_raw: Buffer, members: np.ndarray) -> Tuple[Buffer, Buffer]:
        """gci_depth_gz_runs: members = DGZ_MEMBER_DTYPE on the host -> (device runs, 8 bytes each, every member's at its run0;
        the member table on the device, for depth_gz_expand)."""
        from .formats.depthfile import DGZ_MEMBER_DTYPE, DGZ_RUN_DTYPE
        members = np.ascontiguousarray(members, dtype=DGZ_MEMBER_DTYPE)
        d_members = self.to_device(members.view(np.uint8)) if members.shape[0] else None
        n_runs = int(members["runs"].astype(np.uint64).sum())
        d_runs = self.T.empty(max(n_runs, 1) * DGZ_RUN_DTYPE.itemsize, self.T.uint8, self.device)
        self._chk(self.lib.gci_depth_gz_runs(self.ctx, self._p(d_raw), int(d_raw.shape[0]), self._p(d_members), int(members.shape[0]),
                                             self._p(d_runs)), "gci_depth_gz_runs")
        return d_runs, d_members

    def depth_gz_expand(self, d_runs: Buffer, d_members: Buffer, n_members: int, track: Buffer) -> Buffer:
        """gci_depth_gz_expand, right behind depth_gz_runs over the same member table."""
        self._chk(self.lib.gci_depth_gz_expand(self.ctx, self._p(d_runs), self._p(d_members), int(n_members), self._p(track),
                                               int(track.shape[0])), "gci_depth_gz_expand")
        return track

    def depth_gz_track(self, d_raw: Buffer, members: np.ndarray, track: Buffer) -> Buffer:
        """The members' lines into `track` at each member's elem0: runs, then their expansion."""
        d_runs, d_members = self.depth_gz_runs(d_raw, members)
        return self.depth_gz_expand(d_runs, d_members, int(members.shape[0]), track)

    def sdepth_index(self, d_text: Buffer, prev_name: bytes = b"", cap: int = 1 << 12) -> Tuple[Buffer, np.ndarray, np.ndarray, int]:
        """gci_sdepth_index + the exclusive scan of its tile counts over `samtools depth` text in HBM -> (device uint64 [n_tiles + 1]
        first line index of every tile, the same on the host, sorted uint64 keys (byte offset << 12 | rank in its tile) of the
        lines whose name differs from the line in front -- the first line: from prev_name --, smallest byte offset of a line
        outside the strict grammar or 2**64 - 1)."""
        d_prev = self.to_device(np.frombuffer(bytes(prev_name), dtype=np.uint8)) if prev_name else None

        def call(n, counts, keys, cap, n_keys, bad):
            self._chk(self.lib.gci_sdepth_index(self.ctx, self._p(d_text), n, self._p(d_prev), len(prev_name), self._p(counts), self._p(keys),
                                                cap, self._p(n_keys), self._p(bad)), "gci_sdepth_index")
        return self._text_index(call, d_text, cap)

    def sdepth_parse(self, d_text: Buffer, d_line0: Buffer, segs: np.ndarray, track: Buffer, line_base: int = 0) -> Buffer:
        """gci_sdepth_parse: segs = int64 [n, 3] (first line in the file, lines, track element of the first or -1), sorted; line_base =
        the lines of the file in front of d_text."""
        return self._text_parse(self.lib.gci_sdepth_parse, "gci_sdepth_parse", d_text, d_line0, (int(line_base),), segs, track)

    def range_sums(self, track: Buffer, ranges: np.ndarray) -> np.ndarray:
        """Sum of the depths in each [begin, end) of track element indices (int64 [n, 2]) -> int64 [n]."""
        ranges = np.ascontiguousarray(ranges, dtype=np.int64).reshape(-1, 2)
        n = int(ranges.shape[0])
        if n == 0:
            return np.zeros(0, dtype=np.int64)
        d_r = self.to_device(ranges)
        sums = self.T.empty(n, self.T.int64, self.device)
        self._chk(self.lib.gci_range_sums(self.ctx, self._p(track), self._p(d_r), n, self._p(sums)), "gci_range_sums")
        return sums.cpu().numpy()

    # ---- R10 ---------------------------------------------------------------------------------
    @staticmethod
    def _keys_to_runs(keys: np.ndarray, n_windows: int) -> List[np.ndarray]:
        """Sorted boundary keys -> per window int64 [k, 2] of (rel start, rel end)."""
        keys = np.sort(keys.astype(np.uint64))
        win = (keys >> np.uint64(33)).astype(np.int64)
        rel = ((keys >> np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
        is_end = (keys & np.uint64(1)).astype(bool)
        out = []
        bounds = np.searchsorted(win, np.arange(n_windows + 1))
        for w in range(n_windows):
            a, b = bounds[w], bounds[w + 1]
            r, e = rel[a:b], is_end[a:b]
            if ((b - a) & 1) or e[0::2].any() or not e[1::2].all():
                raise GciError(_lib.GCI_E_INVALID, "issue scan produced unpaired run boundaries")
            out.append(np.stack([r[0::2], r[1::2]], axis=1) if b > a else np.zeros((0, 2), dtype=np.int64))
        return out

    def _scan(self, call, n_windows: int, counts: Optional[Buffer] = None):
        """call(keys, cap) until every key fitted, the buffer grown to what the counters ask for.  counts: the call's counters when it
        fills several key arrays of `cap` keys each, back to back (one counter per array) -> the runs per array; None: one array,
        counted in self._count -> its runs."""
        n_arrays = 1 if counts is None else int(counts.shape[0])
        cap = 1 << 16
        while True:
            keys = self.T.empty(n_arrays * cap, self.T.int64, self.device)
            call(keys, cap)
            n = (self._count if counts is None else counts).cpu().numpy().view(np.uint32)
            if int(n.max()) <= cap:
                break
            cap = int(n.max())
        runs = [self._keys_to_runs(keys[x * cap:x * cap + int(n[x])].cpu().numpy().view(np.uint64), n_windows) for x in range(n_arrays)]
        return runs[0] if counts is None else runs

    def issue_scan(self, track: Buffer, lo: float, hi: float, flank: int) -> List[np.ndarray]:
        """Raw maximal runs of lo < depth <= hi inside [flank, L - flank) of every contig, as
        positions relative to the window start (add `flank` for contig coordinates)."""
        def call(keys, cap):
            self._chk(self.lib.gci_issue_scan(self.ctx, self._p(track), float(lo), float(hi), int(flank),
                                              self._p(keys), cap, self._p(self._count)), "gci_issue_scan")
        return self._scan(call, len(self.lengths))

    def issue_scan_windows(self, track: Buffer, windows: Sequence[Tuple[int, int]], lo: float, hi: float
                           ) -> List[np.ndarray]:
        arr = (Window * max(len(windows), 1))()
        for i, (a, b) in enumerate(windows):
            arr[i].begin, arr[i].end = int(a), int(b)

        def call(keys, cap):
            self._chk(self.lib.gci_issue_scan_windows(self.ctx, self._p(track), arr, len(windows), float(lo), float(hi),
                                                      self._p(keys), cap, self._p(self._count)),
                      "gci_issue_scan_windows")
        return self._scan(call, len(windows))

    def depth_classes(self, track: Buffer, windows: Sequence[Tuple[int, int]], low_below: int = 5
                      ) -> Tuple[List[np.ndarray], List[np.ndarray], np.ndarray]:
        """gci_depth_classes over [begin, end) windows of track elements: per window the runs of depth 0 and the runs of
        0 < depth < low_below, each int64 [k, 2] of (start, exclusive end) relative to the window's beginning, and int64 [n, 2] of
        (sum, count) of the depths > 0 -- one read of the windows (depth_plotter_v2.py)."""
        nw = len(windows)
        arr = (Window * max(nw, 1))()
        for i, (a, b) in enumerate(windows):
            arr[i].begin, arr[i].end = int(a), int(b)
        stats = self.T.zeros(max(2 * nw, 1), self.T.int64, self.device)
        counts = self.T.zeros(2, self.T.int32, self.device)

        def call(keys, cap):
            self._chk(self.lib.gci_depth_classes(self.ctx, self._p(track), arr, nw, int(low_below), self._p(keys), cap,
                                                 self._p(counts), self._p(stats)), "gci_depth_classes")
        zero, low = self._scan(call, nw, counts)
        return zero, low, stats.cpu().numpy()[:2 * nw].reshape(nw, 2)

    # ---- depth_to_bedgraph.py: the constant-depth runs of windows, in order, and their bedGraph text (k_bedgraph.hip) ----
    @staticmethod
    def _window_array(windows: Sequence[Tuple[int, int]]):
        arr = (Window * max(len(windows), 1))()
        for i, (a, b) in enumerate(windows):
            arr[i].begin, arr[i].end = int(a), int(b)
        return arr

    def _depth_runs(self, track: Buffer, arr, nw: int) -> Tuple[Buffer, Buffer, np.ndarray]:
        """-> (the runs, the per-window run offsets) on the device and the offsets on the host; the run buffer is sized from the count
        call and allocated after it."""
        d_run0 = self.T.empty(nw + 1, self.T.int64, self.device)
        self._chk(self.lib.gci_depth_runs_count(self.ctx, self._p(track), arr, nw, self._p(d_run0)), "gci_depth_runs_count")
        run0 = d_run0.cpu().numpy().view(np.uint64)
        total = int(run0[nw])
        d_runs = self.T.empty(max(total, 1), self.T.int64, self.device)
        self._chk(self.lib.gci_depth_runs_write(self.ctx, self._p(track), self._p(d_runs), total), "gci_depth_runs_write")
        return d_runs, d_run0, run0

    def depth_runs(self, track: Buffer, windows: Sequence[Tuple[int, int]]) -> Tuple[np.ndarray, np.ndarray]:
        """The maximal runs of equal depth inside each [begin, end) window of track elements (a run never crosses a window's edge),
        window after window and ascending inside a window -> (RUN_DTYPE [total]: start relative to the window's beginning and depth,
        uint64 [n + 1]: every window's first run, then the total)."""
        nw = len(windows)
        d_runs, _, run0 = self._depth_runs(track, self._window_array(windows), nw)
        return d_runs.cpu().numpy().view(RUN_DTYPE)[:int(run0[nw])], run0

    def bedgraph(self, track: Buffer, windows: Sequence[Tuple[int, int]], names: Sequence[bytes], coord0: Sequence[int]
                 ) -> Tuple[Any, np.ndarray]:
        """The bedGraph lines `name\\tstart\\tend\\tdepth\\n` of every run of every window, in the windows' order: names[w] byte for
        byte, start / end = coord0[w] + the run's bounds relative to the window's beginning (coord0[w] >= 0: the contig coordinate of
        the window's first base) -> (the text as a memoryview of the engine's pinned staging buffer, valid until the next call that
        uses it, uint64 [n + 1]: every window's first byte, then the total).  One round: bedgraph_runs, then bedgraph_text."""
        return self.bedgraph_text(self.bedgraph_runs(track, windows), names, coord0)

    def bedgraph_runs(self, track: Buffer, windows: Sequence[Tuple[int, int]]):
        """First half of bedgraph(): the runs of the windows, left on the device -> what bedgraph_text takes."""
        arr = self._window_array(windows)
        return (arr, len(windows)) + self._depth_runs(track, arr, len(windows))

    def bedgraph_text(self, held, names: Sequence[bytes], coord0: Sequence[int]) -> Tuple[Any, np.ndarray]:
        """Second half of bedgraph(): the text of the runs bedgraph_runs left on the device; the text buffer is sized from the size
        call and allocated after it."""
        arr, nw, d_runs, d_run0, _ = held
        coord = np.ascontiguousarray(coord0, dtype=np.int64)
        name_len = np.array([len(x) for x in names], dtype=np.uint32)
        if coord.shape[0] != nw or name_len.shape[0] != nw:
            raise GciError(_lib.GCI_E_INVALID, "bedgraph: one name and one coordinate per window")
        name_off = np.zeros(max(nw, 1), dtype=np.uint64)
        name_off[1:nw] = np.cumsum(name_len[:-1], dtype=np.uint64)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                   # noqa: E731
        d_byte0 = self.T.empty(nw + 1, self.T.int64, self.device)
        self._chk(self.lib.gci_bedgraph_size(self.ctx, self._p(d_runs), self._p(d_run0), arr, nw, vp(coord), vp(name_len),
                                             self._p(d_byte0)), "gci_bedgraph_size")
        byte0 = d_byte0.cpu().numpy().view(np.uint64)
        total = int(byte0[nw])
        if total == 0:
            return memoryview(b""), byte0
        d_names = self.to_device(np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8))
        out = self.T.empty(total, self.T.uint8, self.device)
        self._chk(self.lib.gci_bedgraph_write(self.ctx, self._p(d_runs), self._p(d_run0), arr, nw, vp(coord), self._p(d_names),
                                              vp(name_off), vp(name_len), self._p(out), total), "gci_bedgraph_write")
        if self._members_host is None or int(self._members_host.shape[0]) < total:          # (depth_deflate's pinned staging)
            self._members_host = self.T.pinned(max(total + (total >> 3), 1 << 20))
        host = self._members_host[:total]
        host.copy_(out, non_blocking=True)
        self.sync()
        return memoryview(host.numpy()), byte0

    # ---- depth_dist.py: the depth histogram and the sum / min / max / count of windows, one read (k_hist.hip) ----
    HIST_LDS_BINS = _lib.HIST_LDS_BINS               # bins a workgroup of k_depth_hist keeps in LDS (GCI_HIST_LDS_BINS)

    def depth_hist(self, track: Buffer, windows: Sequence[Tuple[int, int]], n_bins: int) -> Tuple[np.ndarray, np.ndarray]:
        """gci_depth_hist over [begin, end) windows of track elements -> (uint64 [n, n_bins + 2]: per window the elements with depth
        == b in column b, with depth >= n_bins in column n_bins, with depth < 0 in column n_bins + 1; int64 [n, 4]: sum, min, max,
        elements -- 0, INT32_MAX, INT32_MIN, 0 for an empty window).  n_bins == 0: the statistics and over / under alone."""
        nw, n_bins = len(windows), int(n_bins)
        cols = n_bins + 2
        d_hist = self.T.empty(max(nw * cols, 1), self.T.int64, self.device)
        d_stats = self.T.empty(max(4 * nw, 1), self.T.int64, self.device)
        self._chk(self.lib.gci_depth_hist(self.ctx, self._p(track), self._window_array(windows), nw, n_bins, self._p(d_hist),
                                          self._p(d_stats)), "gci_depth_hist")
        hist = d_hist.cpu().numpy().view(np.uint64)[:nw * cols].reshape(nw, cols)
        return hist, d_stats.cpu().numpy()[:4 * nw].reshape(nw, 4)

    # ---- R7 ----------------------------------------------------------------------------------
    def depth_text(self, track: Buffer, out: Optional[Buffer] = None) -> Tuple[Buffer, np.ndarray]:
        """-> (uint8 text of all contigs back to back, int64 [n_contigs + 1] byte offsets)."""
        n = len(self.lengths)
        offs = self.T.zeros(n + 1, self.T.int64, self.device)
        self._chk(self.lib.gci_depth_text_size(self.ctx, self._p(track), self._p(offs)), "gci_depth_text_size")
        h = offs.cpu().numpy()
        total = int(h[n])
        if out is None or out.shape[0] < total:
            out = self.T.empty(max(total, 1), self.T.uint8, self.device)
        self._chk(self.lib.gci_depth_text_write(self.ctx, self._p(track), self._p(out), total), "gci_depth_text_write")
        return out[:total], h
