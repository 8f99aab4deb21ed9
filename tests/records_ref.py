"""The model of the parallel BAM record walk (gci_bam_record_offsets_device, k_records.hip), from the SAM specification section 4.2
and the contract the kernel file states: plain numpy / Python, every byte position tested on its own, the chain followed one record
at a time.

A record at byte p of an inflated stream: int32 block_size, then block_size bytes that begin with the fixed 32 -- int32 refID,
int32 pos, uint8 l_read_name, uint8 mapq, uint16 bin, uint16 n_cigar_op, uint16 flag, int32 l_seq, int32 next_refID, int32 next_pos,
int32 tlen -- followed by the name, 4 bytes per CIGAR operation, (l_seq + 1) // 2 bytes of SEQ and l_seq bytes of QUAL.

candidates(stream, lo, n_ref) -> the positions where a record could start; walk(stream, first, n_ref) -> (offsets, used, ok)."""
from typing import List, Tuple

import numpy as np

HEAD = 36          # block_size + the fixed 32 bytes: what the test of one position reads


def _i32(s: np.ndarray, at: int, m: int) -> np.ndarray:
    """The little-endian int32 at byte `at` of every one of the first m positions, as int64."""
    w = s[at:at + m].astype(np.int64) | (s[at + 1:at + 1 + m].astype(np.int64) << 8) | (s[at + 2:at + 2 + m].astype(np.int64) << 16) \
        | (s[at + 3:at + 3 + m].astype(np.int64) << 24)
    return np.where(w >= 1 << 31, w - (1 << 32), w)


def candidate_mask(stream: np.ndarray, n_ref: int) -> np.ndarray:
    """mask[p] for p + 36 <= n: the eight conditions of a well-formed record hold at p."""
    s = np.ascontiguousarray(stream, dtype=np.uint8)
    m = int(s.shape[0]) - HEAD + 1
    if m <= 0:
        return np.zeros(0, dtype=bool)
    block_size, ref_id, pos = _i32(s, 0, m), _i32(s, 4, m), _i32(s, 8, m)
    l_read_name = s[12:12 + m].astype(np.int64)
    n_cigar = s[16:16 + m].astype(np.int64) | (s[17:17 + m].astype(np.int64) << 8)
    l_seq, next_ref, next_pos = _i32(s, 20, m), _i32(s, 24, m), _i32(s, 28, m)
    ok = (block_size >= 32) & (ref_id >= -1) & (ref_id < n_ref) & (pos >= -1) & (l_read_name >= 1) & (l_seq >= 0)
    ok &= (next_ref >= -1) & (next_ref < n_ref) & (next_pos >= -1)
    need = 32 + l_read_name + 4 * n_cigar + (np.maximum(l_seq, 0) + 1) // 2 + np.maximum(l_seq, 0)
    return ok & (need <= block_size)


def candidates(stream: np.ndarray, lo: int, n_ref: int) -> np.ndarray:
    """The sorted positions p >= lo with p + 36 <= n at which a record could start."""
    p = np.flatnonzero(candidate_mask(stream, n_ref))
    return p[p >= lo].astype(np.int64)


def block_size_at(stream: np.ndarray, p: int) -> int:
    return int.from_bytes(bytes(stream[p:p + 4]), "little", signed=True)


def walk(stream: np.ndarray, first: int, n_ref: int) -> Tuple[List[int], int, bool]:
    """-> (offsets of the complete records from `first` on, bytes consumed, chain ok)."""
    n = int(stream.shape[0])
    if n - first < HEAD:
        return [], first, True                       # no complete record head: everything is tail
    mask = candidate_mask(stream, n_ref)
    if not mask[first]:
        return [], first, False
    offs: List[int] = []
    p = first
    while True:
        q = p + 4 + block_size_at(stream, p)
        if q > n:
            return offs, p, True                     # a partial last record: carried into the next chunk
        offs.append(p)
        if q == n:
            return offs, n, True
        if q + HEAD <= n and mask[q]:
            p = q
            continue
        if q + HEAD > n:
            return offs, q, True                     # a partial record head behind the last complete record
        return offs, p, False                        # the record at q fails the test: the chain is broken behind p
