"""`.depth.gz`, BED3 and region-BED I/O.

Grammar of the depth file (/root/reference/GCI.py:110-117; consumers
utility/GCI_score.py:25-37, utility/convert_samtools_depth.py:11-20):

    ( '>' contig '\\n' ( decimal '\\n' ) ^ contig_length ) *      contigs in header order

The reference emits one gzip member per (contig, thread-chunk) and its compressed bytes
carry mtime and file names, so only the *decompressed* stream is comparable
(SURVEY.md F5).  Any multi-member gzip whose concatenated payload equals that text is a
valid output; members here are compressed in parallel at a fast level.
"""
from __future__ import annotations

import gzip
import hashlib
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterable, Iterator, Tuple

import numpy as np

MEMBER_BYTES = 8 << 20


def _gzip_member(data, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def write_depth_gz(path: str, pieces: Iterable[Tuple[str, memoryview]], level: int = 1, threads: int = 1) -> None:
    """pieces: (contig name, text bytes of that contig's depth lines) in header order."""
    with open(path, "wb") as f, ThreadPoolExecutor(max(1, threads)) as ex:
        for name, text in pieces:
            mv = memoryview(text)
            chunks = [(">%s\n" % name).encode()]
            chunks += [mv[i:i + MEMBER_BYTES] for i in range(0, len(mv), MEMBER_BYTES)]
            for member in ex.map(lambda c: _gzip_member(c, level), chunks):
                f.write(member)


def iter_depth_text(path: str, block: int = 1 << 24) -> Iterator[bytes]:
    with gzip.open(path, "rb") as f:
        while True:
            b = f.read(block)
            if not b:
                return
            yield b


def sha256_of_text(path: str) -> str:
    h = hashlib.sha256()
    for b in iter_depth_text(path):
        h.update(b)
    return h.hexdigest()


def read_depth_gz(path: str) -> Dict[str, np.ndarray]:
    """Parse into {contig: int64 array}.  Vectorised: one pass over the inflated bytes."""
    data = np.frombuffer(b"".join(iter_depth_text(path)), dtype=np.uint8)
    out: Dict[str, np.ndarray] = {}
    if data.size == 0:
        return out
    nl = np.flatnonzero(data == 10)
    starts = np.concatenate(([0], nl[:-1] + 1)) if nl.size else np.zeros(0, dtype=np.int64)
    is_hdr = data[starts] == ord(">")
    hdr_idx = np.flatnonzero(is_hdr)
    # numeric value of every line (garbage for header lines, skipped below)
    digit = data.astype(np.int64) - 48
    lens = nl - starts
    maxlen = int(lens[~is_hdr].max()) if (~is_hdr).any() else 0
    vals = np.zeros(starts.shape[0], dtype=np.int64)
    for k in range(maxlen):
        sel = (lens > k) & ~is_hdr
        vals[sel] = vals[sel] * 10 + digit[starts[sel] + k]
    bounds = list(hdr_idx) + [starts.shape[0]]
    for a, b in zip(bounds[:-1], bounds[1:]):
        name = bytes(data[starts[a] + 1:nl[a]]).decode()
        out[name] = vals[a + 1:b].copy()
    return out


# ---- reading a .depth.gz back (GCI_score.py): host halves of the device parse (k_depth_parse.hip) ----------------------------------

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def header_name(line: bytes) -> str:
    """The contig a header line names, by the reference's own expression (utility/GCI_score.py:26-31)."""
    return line.decode("utf-8").strip().split(">")[-1]


def _line_at(text: np.ndarray, at: int) -> bytes:
    """The line of `text` that begins at byte `at`, with its '\\n'."""
    k = 256
    while True:
        piece = text[at:at + k].tobytes()
        j = piece.find(b"\n")
        if j >= 0:
            return piece[:j + 1]
        if at + k >= text.shape[0]:
            return piece
        k *= 4


def header_name_v2(line: bytes) -> str:
    """The sequence a header line names for utility/depth_plotter_v2.py: everything behind the '>' of the stripped line."""
    return line.decode("utf-8").strip()[1:]


def header_segments(text: np.ndarray, keys: np.ndarray, tile_line0: np.ndarray, plotter_v2: bool = False):
    """The header lines of a text found by gci_depth_text_index -> (names in first-appearance order, their lengths, a callback
    segs(offsets) -> int64 [n_headers, 3] (first data line, data lines, track element of the first or -1)), or None when the text
    does not begin with a header line (the reference then raises: the slow path reproduces that).  A name that appears again
    restarts its contig: its last segment wins and it keeps its first place (parse_depth's dict).
    plotter_v2: the names by depth_plotter_v2.py's expression, and None also for a name that appears again (that utility draws a
    sequence once per header: the lock-step read below takes such a file)."""
    total_lines = int(tile_line0[-1])
    if keys.shape[0] == 0:
        return None
    keys = keys.astype(np.uint64)
    off = (keys >> np.uint64(12)).astype(np.int64)
    line = tile_line0[off >> 12].astype(np.int64) + (keys & np.uint64(0xFFF)).astype(np.int64)
    if int(line[0]) != 0:
        return None
    name_of = header_name_v2 if plotter_v2 else header_name
    names = [name_of(_line_at(text, int(o))) for o in off.tolist()]
    if any(nm == "" for nm in names):
        return None                        # (a header naming '' is kept apart by parse_depth's `target != ''`: the slow path)
    if plotter_v2 and len(set(names)) != len(names):
        return None
    n_data = np.diff(np.concatenate([line, [total_lines]])) - 1
    last = {nm: k for k, nm in enumerate(names)}
    order = list(dict.fromkeys(names))
    lengths = [int(n_data[last[nm]]) for nm in order]

    def segs(offsets) -> np.ndarray:
        base = {nm: int(o) for nm, o in zip(order, offsets)}
        out = np.empty((len(names), 3), dtype=np.int64)
        out[:, 0] = line + 1
        out[:, 1] = n_data
        out[:, 2] = [base[nm] if last[nm] == k else -1 for k, nm in enumerate(names)]
        return out
    return order, lengths, segs


def parse_depth_lines(lines) -> Dict[str, object]:
    """utility/GCI_score.py:23-37 statement for statement over an iterable of byte lines (a gzip file object or the inflated text):
    the slow path for text outside the strict grammar (CRLF, blanks, '+7', ...) and the way a damaged file raises what the
    reference raises.  -> {contig: int64 array}, in the reference's dict order."""
    depths = {}
    target = ""
    for line in lines:
        item = line.decode("utf-8").strip()
        if item.startswith(">"):
            if target != "":
                depths[target] = np.array(depths[target])
            target = item.split(">")[-1]
            depths[target] = []
        else:
            depths[target].append(int(item))
    depths[target] = np.array(depths[target])
    return depths


# ---- utility/depth_plotter_v2.py: its reader steps through the HiFi and the ONT file one line of each at a time ---------------------

def open_depth_lines(path: str):
    """A depth file as text lines, as depth_plotter_v2.py opens it: gzip only when the name ends in `.gz`."""
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path, "rt")


def lockstep_sequences(hifi_lines, ont_lines, wanted, n_targets: int, say=print):
    """The sequences depth_plotter_v2.py's SynchronizedDepthReader yields, for ANY pair of files (either may be None): the slow path of
    depth_plotter_v2 for files the device path does not take -- text outside the strict grammar, names that repeat, two files whose
    headers do not line up.  One line of each file per step; what follows from that is kept:
      * a header line in either file closes the sequence read so far and opens the next one, named by the HiFi header when both
        lines are headers; the other file's data line of that step is dropped;
      * a header that names nothing ('>') opens nothing, and is no data either;
      * a data line that is no integer counts as 0;
      * the file that ends first ends the read (a line already taken from the HiFi file in that step is dropped);
      * a sequence is yielded when wanted(name), once; when n_targets of them were yielded the read stops.
    -> (name, HiFi depths, ONT depths) as lists of int; the reader's transcript goes through say()."""
    def number(word: str) -> int:
        try:
            return int(word)
        except ValueError:
            return 0

    if hifi_lines is not None and ont_lines is not None:
        steps = zip(hifi_lines, ont_lines)
    elif hifi_lines is not None:
        steps = ((line, None) for line in hifi_lines)
    else:
        steps = ((None, line) for line in (ont_lines if ont_lines is not None else ()))
    done = set()
    name, hifi, ont = None, [], []
    try:
        for pair in steps:
            words = [None if line is None else line.strip() for line in pair]
            heads = [None if w is None or not w.startswith(">") else w[1:] for w in words]
            opened = heads[0] or heads[1]
            if not opened:
                for w, h, depths in zip(words, heads, (hifi, ont)):
                    if w is not None and h is None:
                        depths.append(number(w))
                continue
            if name and wanted(name):
                done.add(name)
                say(f"Processing sequence: {name}, remaining target sequences: {n_targets - len(done)}")
                yield name, hifi, ont
                if n_targets and len(done) >= n_targets:
                    say("All target sequences have been processed, stopping reading")
                    break
            name, hifi, ont = opened, [], []
        if name and wanted(name) and name not in done:
            done.add(name)
            say(f"Processing last sequence: {name}")
            yield name, hifi, ont
    finally:
        say(f"File reading ended, processed {len(done)} sequences in total")


def conforming_sequences(names, wanted, n_targets: int, say=print):
    """lockstep_sequences for files whose headers line up (one file, or two with the same names and lengths in the same order, every
    name once and none empty): which of `names` are yielded, and the same transcript, from the header sequence alone."""
    done = 0
    try:
        for k, name in enumerate(names):
            if not wanted(name):
                continue
            done += 1
            if k + 1 == len(names):
                say(f"Processing last sequence: {name}")
                yield name
                return
            say(f"Processing sequence: {name}, remaining target sequences: {n_targets - done}")
            yield name
            if n_targets and done >= n_targets:
                say("All target sequences have been processed, stopping reading")
                return
    finally:
        say(f"File reading ended, processed {done} sequences in total")


# ---- this project's own .depth.gz read without inflating it: host halves of the compressed-domain read (k_depth_gz.hip) --------------

MEMBER_HEAD = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])       # the ten bytes a member of k_deflate.hip begins with
DGZ_OK, DGZ_FOREIGN = 0, 1
# include/gci_hip.h: gci_dgz_info, gci_dgz_member, gci_dgz_run
DGZ_INFO_DTYPE = np.dtype([("end", "<u8"), ("status", "<u4"), ("lines", "<u4"), ("runs", "<u4"), ("crc_ok", "<u4"), ("isize_ok", "<u4"),
                           ("reserved", "<u4")])
DGZ_MEMBER_DTYPE = np.dtype([("pos", "<u8"), ("run0", "<u8"), ("elem0", "<u8"), ("runs", "<u4"), ("lines", "<u4")])
DGZ_RUN_DTYPE = np.dtype([("depth", "<i4"), ("count", "<u4")])
HEADER_MEMBER_MAX = 4096                   # bytes of a '>name\n' member, raw and inflated: anything larger is not one


def member_candidates(buf) -> np.ndarray:
    """Every position of the ten-byte member header in `buf` (bytes / bytearray) -> uint64 array, ascending.  Most are member
    starts; one inside another member's bits is possible and harmless (member_chain never looks at it)."""
    out, at = [], buf.find(MEMBER_HEAD)
    while at >= 0:
        out.append(at)
        at = buf.find(MEMBER_HEAD, at + 1)
    return np.asarray(out, dtype=np.uint64)


def header_member(view, pos: int):
    """The gzip member at view[pos:] when it is exactly one header line '>name\\n' whose name is what the reference's
    `line.decode().strip().split('>')[-1]` yields -> (name, end offset), else None."""
    d = zlib.decompressobj(31)
    piece = view[pos:pos + HEADER_MEMBER_MAX]
    try:
        text = d.decompress(piece, HEADER_MEMBER_MAX)
    except zlib.error:
        return None
    if not d.eof or len(text) < 3 or text[:1] != b">" or text[-1:] != b"\n" or text.count(b"\n") != 1:
        return None
    try:
        name = text[1:-1].decode("utf-8")
    except UnicodeDecodeError:
        return None
    if name == "" or ">" in name or name != name.strip() or header_name(text) != name:
        return None
    return name, pos + len(piece) - len(d.unused_data)


def member_chain(buf, cand: np.ndarray, info: np.ndarray):
    """The file as a chain of members from byte 0.  A position that the device accepted (gci_depth_gz_scan: status OK, CRC-32 and
    ISIZE matching) is a data member of the contig named last and the chain continues at its end offset; any other position must be
    a '>name\\n' member, inflated here.  -> (names, lengths, members: DGZ_MEMBER_DTYPE without elem0) or None: the file is not
    wholly of this kind -- data lines in a host member, NUL padding, a damaged member, a name seen twice, data in front of the first
    header, a contig without lines -- and the text path, which defines every result and every exception, takes all of it."""
    view = memoryview(buf)
    n = len(view)
    at = {int(p): k for k, p in enumerate(cand.tolist())}
    names, lengths, rows = [], [], []
    seen = set()
    pos = 0
    while pos < n:
        k = at.get(pos)
        if k is not None and int(info["status"][k]) == DGZ_OK:
            if not (info["crc_ok"][k] and info["isize_ok"][k]) or not names:
                return None
            end = int(info["end"][k])
            if end <= pos or end > n:
                return None
            rows.append((pos, int(info["runs"][k]), int(info["lines"][k]), len(names) - 1))
            lengths[-1] += int(info["lines"][k])
            pos = end
            continue
        got = header_member(view, pos)
        if got is None or got[0] in seen:
            return None
        seen.add(got[0])
        names.append(got[0])
        lengths.append(0)
        pos = got[1]
    if not names or any(L == 0 for L in lengths):
        return None
    members = np.zeros(len(rows), dtype=DGZ_MEMBER_DTYPE)
    contig = np.zeros(len(rows), dtype=np.int64)
    if rows:
        r = np.asarray(rows, dtype=np.int64)
        members["pos"], members["runs"], members["lines"], contig = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
        members["run0"] = np.cumsum(r[:, 1]) - r[:, 1]
    return names, lengths, (members, contig)


def place_members(members_contig, offsets) -> np.ndarray:
    """member_chain's members with elem0 = the track element of each member's first line, for the layout's contig offsets."""
    members, contig = members_contig
    members = members.copy()
    if members.shape[0]:
        lines = members["lines"].astype(np.int64)
        before = np.cumsum(lines) - lines                                  # lines of the file in front of the member
        first = np.full(len(offsets), -1, dtype=np.int64)                  # ... in front of the contig's first member
        first[contig[::-1]] = before[::-1]
        members["elem0"] = np.asarray(offsets, dtype=np.int64)[contig] + before - first[contig]
    return members


# ---- `samtools depth` text -> .depth.gz (utility/convert_samtools_depth.py): host halves of the device path (k_sdepth.hip) -----------

SDEPTH_LINE_MAX = 255                      # bytes of a line with its '\n': the bound of the device's grammar (k_sdepth.hip)


def convert_samtools_host(in_path: str, out_path: str) -> None:
    """utility/convert_samtools_depth.py:11-20 statement for statement: the slow path for text outside the device's strict grammar
    (CRLF, blank-padded or signed depths, blanks in names, bytes beyond ASCII) and the way a damaged file raises what the
    reference raises.  The output is opened first, as there."""
    f_out = gzip.open(out_path, "wb")
    try:
        with open(in_path, "r") as f:
            pre_chr_id = ""
            for line in f:
                chr_id, _, depth = line.strip().split("\t")
                if chr_id != pre_chr_id:
                    f_out.write((f">{chr_id}\n").encode("utf-8"))
                    pre_chr_id = chr_id
                f_out.write((f"{depth}\n").encode("utf-8"))
    finally:
        f_out.close()


def _last_newline(raw, a: int, b: int) -> int:
    """Offset of the last '\\n' in raw[a:b], or -1; read from the back in small pieces (raw: the file's mapping)."""
    hi = b
    while hi > a:
        lo = max(a, hi - (1 << 16))
        idx = np.flatnonzero(np.asarray(raw[lo:hi]) == 10)
        if idx.size:
            return lo + int(idx[-1])
        hi = lo
    return -1


def _next_newline(raw, a: int, b: int) -> int:
    lo = a
    while lo < b:
        hi = min(b, lo + (1 << 16))
        idx = np.flatnonzero(np.asarray(raw[lo:hi]) == 10)
        if idx.size:
            return lo + int(idx[0])
        lo = hi
    return -1


def sdepth_chunks(raw, chunk_bytes: int):
    """Cut the text into [a, b) pieces of at most chunk_bytes that end behind a '\\n' (or at the end of the text); a line longer than
    a piece gets a piece of its own.  -> [(a, b, name of the last line in front of a)]: with that name a piece needs nothing
    from the piece in front of it (gci_sdepth_index: prev_name)."""
    n = int(raw.shape[0])
    out, a, prev = [], 0, b""
    while a < n:
        b = min(n, a + max(1, int(chunk_bytes)))
        if b < n:
            j = _last_newline(raw, a, b)
            if j < 0:
                j = _next_newline(raw, b, n)
            b = j + 1 if j >= 0 else n
        out.append((a, b, prev))
        # the last line of this piece begins behind the last '\n' in front of its closing byte
        j = _last_newline(raw, a, b - 1)
        prev = sdepth_name(raw, j + 1 if j >= 0 else a)
        a = b
    return out


def sdepth_name(raw, at: int) -> bytes:
    """The name column of the line that begins at `at`, cut at the device's bound (a longer one is outside the grammar anyway)."""
    piece = np.asarray(raw[at:at + SDEPTH_LINE_MAX]).tobytes()
    for k, c in enumerate(piece):
        if c in (9, 10):
            return piece[:k]
    return piece


def sdepth_segments(raw, keys: np.ndarray, tile_line0: np.ndarray, byte_base: int = 0, line_base: int = 0):
    """The keys of gci_sdepth_index over raw[byte_base:] -> [(name, first line index in the file)] in file order: one segment per
    line whose name differs from the line in front, so a name that returns gets a segment of its own (as the reference writes a
    second header for it -- unlike header_segments, where the last one wins)."""
    keys = keys.astype(np.uint64)
    off = (keys >> np.uint64(12)).astype(np.int64)
    line = tile_line0[off >> 12].astype(np.int64) + (keys & np.uint64(0xFFF)).astype(np.int64) + line_base
    return [(sdepth_name(raw, byte_base + int(o)), int(g)) for o, g in zip(off.tolist(), line.tolist())]
