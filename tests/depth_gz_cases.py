"""Inputs shared by tests/test_depth_gz_cpu.py and tests/test_gpu_depth_gz.py: tracks and the members CpuEngine.depth_deflate writes
for them, forged members (tests/deflate_forge.py) that zlib accepts but the grammar of include/gci_hip.h does not, and files of
candidates that are no member starts."""
import functools
import struct
import zlib

import numpy as np

import deflate_forge as forge
from gci_amd.formats import depthfile

HEAD = depthfile.MEMBER_HEAD
LENGTHS = [1, 5, 4095, 4096, 4097, 64 * 4096, 64 * 4096 + 1, 1_000_003]
# every line width 2 .. 11
VALUES = [0, 7, 38, 123, 1234, 12345, 123_456, 1_234_567, 12_345_678, 123_456_789, 1_000_000_000, 2_147_483_647]


def header_member(name: str) -> bytes:
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    return c.compress((">%s\n" % name).encode()) + c.flush()


def build_file(names, blobs) -> bytearray:
    buf = bytearray()
    for name, blob in zip(names, blobs):
        buf += header_member(name) + bytes(blob)
    return buf


@functools.lru_cache(maxsize=None)
def member_set():
    """-> (lengths, track of a CpuEngine layout, offsets, file bytes): contigs of LENGTHS with runs of VALUES that cross tile and
    member boundaries, one tile in which every base differs, a pile-up stretch of runs of one."""
    from gci_amd.cpu import CpuEngine
    e = CpuEngine()
    rng = np.random.default_rng(20)
    e.set_layout(LENGTHS)
    track = e.new_track()
    for c, L in enumerate(LENGTHS):
        a = e.contig(track, c)
        pos = 0
        while pos < L:
            n = int(rng.integers(1, 9000)) if L > 100 else int(rng.integers(1, 3))
            a[pos:pos + n] = VALUES[int(rng.integers(0, len(VALUES)))]
            pos += n
    big = e.contig(track, len(LENGTHS) - 1)
    big[8192:8192 + 4096] = (np.arange(4096) * 7919) % 100_003 + 1          # a tile in which every base differs
    big[64 * 4096 - 5000:64 * 4096 + 5000] = 38                             # one run across a member boundary
    big[3 * 64 * 4096 - 2:3 * 64 * 4096 + 2] = [0, 0, 0, 0]                 # "0\n0\n" as literals on either side of a member boundary
    e.contig(track, 5)[4096 - 1:4096 + 1] = 7                               # ... and across a tile boundary
    blobs = e.depth_deflate(track)
    names = ["ctg%d" % c for c in range(len(LENGTHS))]
    offsets = [int(o) for o in e.offsets]
    e.close()
    return list(LENGTHS), track, offsets, bytes(build_file(names, blobs))


@functools.lru_cache(maxsize=None)
def layout_200():
    """-> (names, lengths, track, offsets, file bytes): 200 contigs of 1 .. 5000 bases, about 400 members with the headers."""
    from gci_amd.cpu import CpuEngine
    e = CpuEngine()
    rng = np.random.default_rng(21)
    lengths = [1, 5000] + [int(x) for x in rng.integers(1, 5001, 198)]
    e.set_layout(lengths)
    track = e.new_track()
    for c, L in enumerate(lengths):
        runs = rng.integers(1, 400, L // 100 + 2)
        vals = rng.choice(VALUES, runs.shape[0])
        e.contig(track, c)[:] = np.repeat(vals, runs)[:L].astype(np.int32)
    names = ["c%03d" % c for c in range(len(lengths))]
    blobs = e.depth_deflate(track)
    offsets = [int(o) for o in e.offsets]
    e.close()
    return names, lengths, track, offsets, bytes(build_file(names, blobs))


# ---- forged members ---------------------------------------------------------------------------------------------------------------

def member(blocks, head: bytes = HEAD, crc_add: int = 0, isize_add: int = 0):
    """-> (member bytes, the text zlib must give)"""
    f = forge.forge(blocks)
    tail = struct.pack("<II", (zlib.crc32(f.payload) + crc_add) & 0xFFFFFFFF, (len(f.payload) + isize_add) & 0xFFFFFFFF)
    return head + f.data + tail, f.payload


def line(v) -> list:
    return list(("%s\n" % v).encode())


def run_tokens(v, n: int, rng=None) -> list:
    """n copies of the line of v as the grammar wants them: the literals, then matches of distance = width (rng: random lengths)"""
    w = len(str(v)) + 1
    out, rest = line(v), (n - 1) * w
    while rest >= 3:
        k = min(rest, 258) if rng is None else int(rng.integers(3, min(rest, 258) + 1))
        if 0 < rest - k < 3:                               # never leave one or two bytes behind
            k = rest if rest <= 258 else 255
        out.append((k, w))
        rest -= k
    return out + (line(v) if rest else [])                 # (two lines of two bytes: the second as literals)


def _dynamic(tokens):
    rng = np.random.default_rng(3)
    lit, dist = forge.used_symbols(tokens)
    return forge.Dynamic(tokens, forge.lengths_for(rng, lit, 286), forge.lengths_for(rng, dist | {0}, 30))


def outside_grammar():
    """name -> (member bytes, text): legal gzip members, every one outside the grammar"""
    F, S = forge.Fixed, forge.Stored
    one = line(12)
    fnam = bytes([0x1F, 0x8B, 8, 8, 0, 0, 0, 0, 0, 0xFF]) + b"x.depth\0"
    cases = {
        "distance w - 1": [F(one + [(6, 2)])],
        "distance != w behind a first line": [F(one + [(6, 3)] + line(7) + [(4, 3)])],
        "match ends mid-line, then a literal": [F(one + [(4, 3), 50, 10])],
        "block ends mid-line": [F(one + [(4, 3)], final=False), S(), F([50, 10])],
        "match with no line in its block": [F(one, final=False), S(), F([(6, 3)])],
        "dynamic block": [_dynamic(one + [(6, 3)])],
        "1-byte stored block": [F(one, final=False), S(b"5"), F([10])],
        "stored block in front": [S(), F(one)],
        "final stored block": [F(one, final=False), S()],
        "11 digits": [F(line(12345678901))],
        "2147483648": [F(line(2147483648))],
        "leading zero": [F(line("07"))],
        "empty line": [F([10])],
        "a letter": [F([65, 10])],
        "66 fixed blocks": [b for _ in range(65) for b in (F(one, final=False), S())] + [F([])],
    }
    out = {k: member(v) for k, v in cases.items()}
    out["FLG with FNAME"] = member([F(one)], head=fnam)
    return out


def inside_grammar():
    """name -> (member bytes, text): forged members the grammar takes, in forms k_deflate.hip never writes"""
    F, S = forge.Fixed, forge.Stored
    rng = np.random.default_rng(4)
    one = line(12)
    cases = {
        "65 fixed blocks": [b for _ in range(64) for b in (F(one, final=False), S())] + [F([])],
        "258 as code 284 + 31": [F(one + [(258, 3, True), (3, 3)])],
        "fixed blocks back to back": [F(one, final=False), F(line(5) + [(4, 2)])],
        "no lines at all": [F([])],
        "a final block with lines": [F(run_tokens(2147483647, 40))],
        "random match lengths": [F(run_tokens(38, 5000, rng) + run_tokens(0, 3) + run_tokens(1_000_000_000, 700, rng), final=False), S(),
                                 F(run_tokens(7, 9000, rng))],
        "262144 lines": [F(run_tokens(3, 262_144))],
    }
    return {k: member(v) for k, v in cases.items()}


def over_the_line_cap():
    return member([forge.Fixed(run_tokens(3, 262_145))])


def off_by_one():
    ok = [forge.Fixed(run_tokens(12, 100))]
    return {"crc": member(ok, crc_add=1), "isize": member(ok, isize_add=1)}


def zlib_member(data: bytes):
    """One gzip member at the front of data by zlib -> (text, bytes consumed) or None when zlib refuses it."""
    d = zlib.decompressobj(31)
    try:
        text = d.decompress(data)
    except zlib.error:
        return None
    if not d.eof:
        return None
    return text, len(data) - len(d.unused_data)


def text_of_runs(runs) -> bytes:
    return b"".join(b"%d\n" % int(r["depth"]) * int(r["count"]) for r in runs)


def stamped(data: bytes, offsets) -> bytes:
    """data with the ten-byte member header written over it at every one of `offsets`: candidates in the middle of other members' bits"""
    b = bytearray(data)
    for o in offsets:
        b[o:o + 10] = HEAD
    return bytes(b[:len(data)])
