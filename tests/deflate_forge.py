"""A DEFLATE writer for tests, written from RFC 1951: it writes what it is told to, legal or not, and says where every bit went.

zlib's encoder is one dialect of the format -- optimal length-limited codes, its own run-length coding of the header, none of the
rarer forms.  The inflaters (k_inflate_wave.hip, k_inflate.hip) must take every legal stream, so the tests need streams no
encoder on this machine writes: the caller gives the tokens of every block and the code lengths to send them with, down to the
run-length symbols of the header, and gets back the bytes, the payload the tokens expand to, and a LEDGER of bit offsets (block
header, body, every symbol, the end-of-block code) that the geometric tests assert on.

    forge([Stored(b"abc"), Fixed([65, (4, 1)]), Dynamic(tokens, lit_lens, dist_lens)]) -> Forged(data, payload, ledger)

A token is a literal byte (int), a match (length, distance), (258, distance, True) for length 258 written as code 284 with extra
bits 31, or -- for malformed streams -- ("lit", symbol) / ("match", length symbol, extra, distance symbol, extra).
Nothing here checks legality: test_deflate_forge_cpu.py holds every forged stream against zlib.
"""
import struct
import zlib

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0) + tuple(k for k in range(1, 14) for _ in (0, 1))
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

_LEN_SYM = [0] * 259
for _s, (_b, _e) in enumerate(zip(LEN_BASE, LEN_EXTRA)):
    for _v in range(_b, min(_b + (1 << _e), 259)):
        _LEN_SYM[_v] = _s                              # (258 ends up with code 285: the last writer wins)


def length_symbol(length: int, alt: bool = False):
    """-> (lit/len symbol, extra value, extra bits); alt: 258 as 284 + 31"""
    if alt:
        assert length == 258
        return 284, 31, 5
    s = _LEN_SYM[length]
    return 257 + s, length - LEN_BASE[s], LEN_EXTRA[s]


def dist_symbol(dist: int):
    s = 29
    while DIST_BASE[s] > dist:
        s -= 1
    return s, dist - DIST_BASE[s], DIST_EXTRA[s]


def canonical(lens):
    """RFC 1951 3.2.2 -> per symbol (code bit-reversed for an LSB-first writer, length); (0, 0) for an unused symbol.
    An over-subscribed set gets codes all the same (cut to their length): such a header is written to be refused."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l == 0:
            out.append((0, 0))
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    @property
    def pos(self) -> int:
        return 8 * len(self.buf) + self.n

    def put(self, value: int, bits: int) -> None:
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def align(self, pad: int = 0) -> None:
        """to the next byte boundary, the bits in between taken from `pad`"""
        k = -self.pos & 7
        self.put(pad, k)

    def bytes_(self, data: bytes) -> None:
        assert self.pos & 7 == 0
        self.align()
        k = self.n >> 3
        self.buf += self.acc.to_bytes(k, "little")
        self.acc, self.n = 0, 0
        self.buf += data

    def done(self, pad: int = 0) -> bytes:
        self.align(pad)
        self.bytes_(b"")
        return bytes(self.buf)


class Stored:
    """pad: the bits between the 3 header bits and the byte boundary (RFC: ignored); len_field / nlen_field: overrides"""
    def __init__(self, data: bytes = b"", pad: int = 0, final=None, len_field=None, nlen_field=None):
        self.data, self.pad, self.final, self.len_field, self.nlen_field = bytes(data), pad, final, len_field, nlen_field


class Fixed:
    def __init__(self, tokens=(), final=None, eob=True):
        self.tokens, self.final, self.eob = list(tokens), final, eob


class Dynamic:
    """lit_lens: up to 286 code lengths (trailing zeros are cut to HLIT unless hlit says otherwise), dist_lens likewise (HDIST >= 1).
    cl_lens: the 19 lengths of the code-length code (default: a complete near-flat code over the symbols the header uses);
    hclen: how many of them are sent (default: up to the last non-zero one in transmission order, at least 4);
    rle: the header's symbols, [(length 0..15,) | (16, repeat 3..6) | (17, repeat 3..10) | (18, repeat 11..138)] (default: rle_greedy);
    hlit_field / hdist_field: raw 5-bit fields (malformed headers)."""
    def __init__(self, tokens, lit_lens, dist_lens, cl_lens=None, hclen=None, rle=None, hlit=None, hdist=None, final=None, eob=True,
                 hlit_field=None, hdist_field=None):
        self.tokens, self.final, self.eob = list(tokens), final, eob
        self.lit_lens, self.dist_lens = list(lit_lens), list(dist_lens)
        self.cl_lens, self.hclen, self.rle, self.hlit, self.hdist = cl_lens, hclen, rle, hlit, hdist
        self.hlit_field, self.hdist_field = hlit_field, hdist_field


class Raw:
    """bits as they are (a block of type 3, a header cut short ...)"""
    def __init__(self, value: int, bits: int):
        self.value, self.bits = value, bits


class Forged:
    def __init__(self, data, payload, ledger):
        self.data, self.payload, self.ledger = data, payload, ledger


def rle_none(lengths):
    return [(l,) for l in lengths]


def rle_greedy(lengths):
    """runs of zeros by 18 / 17, runs of a length by the length and 16s -- the longest repeat first"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k)); run -= k
            if run >= 3:
                out.append((17, run)); run = 0
            out += [(0,)] * run
        else:
            out.append((v,)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k)); run -= k
            out += [(v,)] * run
        i = j
    return out


def rle_random(rng, lengths):
    """a random legal coding: every run cut into random repeats and plain lengths"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v != 0:                                     # (16 repeats the length in front of it: the run's first one is sent plainly)
            out.append((v,)); run -= 1
        while run > 0:
            r = rng.random()
            if v == 0 and run >= 11 and r < 0.5:
                k = int(rng.integers(11, min(run, 138) + 1)); out.append((18, k))
            elif v == 0 and run >= 3 and r < 0.8:
                k = int(rng.integers(3, min(run, 10) + 1)); out.append((17, k))
            elif v != 0 and run >= 3 and r < 0.7:
                k = int(rng.integers(3, min(run, 6) + 1)); out.append((16, k))
            else:
                k = 1; out.append((v,))
            run -= k
        i = j
    return out


def flat_lengths(used, n):
    """a complete code, as flat as it gets, over the symbols in `used` (out of n); one symbol gets a partner: two codes of 1 bit"""
    used = sorted(set(used))
    if len(used) == 1:
        used = sorted(set(used) | {(used[0] + 1) % n})
    k = len(used)
    L = max(1, (k - 1).bit_length())
    short = (1 << L) - k
    lens = [0] * n
    for i, s in enumerate(used):
        lens[s] = L - 1 if i < short else L
    return lens


def expand(tokens, out: bytearray) -> None:
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        if isinstance(t[0], str):
            if t[0] == "lit":
                if t[1] < 256:
                    out.append(t[1])
                continue
            length, dist = LEN_BASE[min(t[1] - 257, 28)] + t[2], DIST_BASE[min(t[3], 29)] + t[4]
        else:
            length, dist = t[0], t[1]
        if dist > len(out):                            # (malformed: a decoder without the check reads what lies in front; say zeros)
            for _ in range(length):
                k = len(out) - dist
                out.append(out[k] if k >= 0 else 0)
        elif dist >= length:
            out += out[len(out) - dist:len(out) - dist + length]
        else:
            pat = bytes(out[len(out) - dist:])
            out += (pat * (length // dist + 1))[:length]


def _put_tokens(w, tokens, lit, dist, pos_out):
    for t in tokens:
        pos_out.append(w.pos)
        if isinstance(t, int):
            c, l = lit[t]
            assert l, "literal %d has no code" % t
            w.put(c, l)
            continue
        if isinstance(t[0], str):
            if t[0] == "lit":
                w.put(*lit[t[1]])
                continue
            ls, lx, lb, ds, dx, db = t[1], t[2], LEN_EXTRA[min(t[1] - 257, 28)], t[3], t[4], DIST_EXTRA[min(t[3], 29)]
        else:
            ls, lx, lb = length_symbol(t[0], len(t) > 2 and t[2])
            ds, dx, db = dist_symbol(t[1])
        assert lit[ls][1] and dist[ds][1], "match symbol without a code"
        w.put(*lit[ls]); w.put(lx, lb); w.put(*dist[ds]); w.put(dx, db)


def forge(blocks, tail_pad: int = 0, tail: bytes = b"") -> Forged:
    """blocks back to back in one bit writer; the last one is the final block unless `final` says otherwise.  tail_pad: the bits
    behind the last block up to the byte boundary; tail: bytes behind that (unused by a decoder)."""
    w, payload, ledger = BitWriter(), bytearray(), []
    for k, b in enumerate(blocks):
        if isinstance(b, Raw):
            ledger.append(dict(kind="raw", header=w.pos, end=w.pos + b.bits))
            w.put(b.value, b.bits)
            continue
        final = b.final if b.final is not None else k == len(blocks) - 1
        led = dict(header=w.pos, final=final)
        if isinstance(b, Stored):
            w.put(int(final), 1); w.put(0, 2); w.align(b.pad)
            n = len(b.data)
            w.put(n if b.len_field is None else b.len_field, 16)
            w.put((n ^ 0xFFFF) if b.nlen_field is None else b.nlen_field, 16)
            led.update(kind="stored", body=w.pos)
            w.bytes_(b.data)
            payload += b.data
            led["end"] = w.pos
            ledger.append(led)
            continue
        if isinstance(b, Fixed):
            w.put(int(final), 1); w.put(1, 2)
            lit, dist = canonical(FIXED_LIT), canonical(FIXED_DIST)
            led["kind"] = "fixed"
        else:
            w.put(int(final), 1); w.put(2, 2)
            ll, dl = list(b.lit_lens), list(b.dist_lens)
            hlit = b.hlit if b.hlit is not None else max(257, max([i + 1 for i, l in enumerate(ll) if l] or [257]))
            hdist = b.hdist if b.hdist is not None else max(1, max([i + 1 for i, l in enumerate(dl) if l] or [1]))
            ll = (ll + [0] * hlit)[:hlit]
            dl = (dl + [0] * hdist)[:hdist]
            rle = b.rle if b.rle is not None else rle_greedy(ll + dl)
            cl = b.cl_lens if b.cl_lens is not None else flat_lengths([r[0] for r in rle], 19)
            hclen = b.hclen if b.hclen is not None else max(4, max(i + 1 for i, s in enumerate(CLEN_ORDER) if cl[s]))
            w.put(hlit - 257 if b.hlit_field is None else b.hlit_field, 5)
            w.put(hdist - 1 if b.hdist_field is None else b.hdist_field, 5)
            w.put(hclen - 4, 4)
            for i in range(hclen):
                w.put(cl[CLEN_ORDER[i]], 3)
            led["lengths"] = w.pos
            cc = canonical(cl)
            for r in rle:
                assert cc[r[0]][1], "code-length symbol %d has no code" % r[0]
                w.put(*cc[r[0]])
                if r[0] == 16: w.put(r[1] - 3, 2)
                elif r[0] == 17: w.put(r[1] - 3, 3)
                elif r[0] == 18: w.put(r[1] - 11, 7)
            lit, dist = canonical(ll + [0] * (288 - len(ll))), canonical(dl + [0] * (32 - len(dl)))
            led.update(kind="dynamic", hlit=hlit, hdist=hdist, hclen=hclen)
        led["body"] = w.pos
        syms = []
        _put_tokens(w, b.tokens, lit, dist, syms)
        led["syms"] = syms
        led["eob"] = w.pos
        if b.eob:
            assert lit[256][1], "no code for 256"
            w.put(*lit[256])
        led["end"] = w.pos
        expand(b.tokens, payload)
        ledger.append(led)
    end = w.pos
    data = w.done(tail_pad) + tail
    f = Forged(data, bytes(payload), ledger)
    f.end_bit, f.blocks = end, list(blocks)
    return f


# ---- helpers ------------------------------------------------------------------------------------------------------------------

def complete_lengths(rng, symbols: int, max_len: int = 15):
    """`symbols` code lengths in 1 .. max_len with Kraft sum exactly 1, in random order: from the complete set {1, 1} leaves are split
    (one of length l -> two of l + 1) until there are enough, then random merge + split pairs move the shape about."""
    assert 2 <= symbols <= (1 << max_len)
    cnt = [0] * (max_len + 2)
    cnt[1] = 2
    n = 2
    while n < symbols:
        ok = [l for l in range(1, max_len) if cnt[l]]
        # (the leaves left must still be able to supply what is missing: a leaf of length l splits into at most 2^(max_len - l))
        l = int(rng.choice(ok)) if rng.random() < 0.7 else min(ok)
        cap = sum(cnt[j] << (max_len - j) for j in range(1, max_len + 1))
        if cap < symbols:
            raise AssertionError("cannot reach %d symbols" % symbols)
        cnt[l] -= 1; cnt[l + 1] += 2; n += 1
    for _ in range(int(rng.integers(0, 2 * symbols + 1))):
        merge = [l for l in range(2, max_len + 1) if cnt[l] >= 2]
        if not merge:
            break
        m = int(rng.choice(merge))
        cnt[m] -= 2; cnt[m - 1] += 1
        split = [l for l in range(1, max_len) if cnt[l]]
        s = int(rng.choice(split))
        cnt[s] -= 1; cnt[s + 1] += 2
    lens = [l for l in range(1, max_len + 1) for _ in range(cnt[l])]
    assert len(lens) == symbols and sum(1 << (max_len - l) for l in lens) == 1 << max_len
    return [int(x) for x in rng.permutation(lens)]


def parse(rng, payload: bytes, p_match: float = 0.6, window_start: int = 0):
    """a random legal LZ77 parse of payload[window_start:], never the greedy one on purpose: at a position with earlier occurrences
    of its next three bytes, one of them (any distance up to 32 768, overlapping ones included) with a random length between 3 and
    what matches (258 at most).  Matches may reach in front of window_start, down to 0."""
    n, i, tokens = len(payload), window_start, []
    where = {}
    for j in range(0, min(window_start, n - 2)):
        where.setdefault(payload[j:j + 3], []).append(j)
    while i < n:
        cand = where.get(payload[i:i + 3]) if i + 3 <= n else None
        took = 1
        if cand and rng.random() < p_match:
            j = cand[int(rng.integers(0, len(cand)))] if rng.random() < 0.5 else cand[-1]
            if i - j <= 32768:
                m = 3
                while m < 258 and i + m < n and payload[j + m] == payload[i + m]:
                    m += 1
                took = m if rng.random() < 0.4 else int(rng.integers(3, m + 1))
                tokens.append((took, i - j))
        if took == 1:
            tokens.append(payload[i])
        for j in range(i, min(i + took, n - 2)):
            where.setdefault(payload[j:j + 3], []).append(j)
        i += took
    return tokens


def used_symbols(tokens):
    """-> (set of lit/len symbols incl. 256, set of distance symbols) the tokens need codes for"""
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        elif isinstance(t[0], str):
            lit.add(t[1])
            if t[0] == "match":
                dist.add(t[3])
        else:
            lit.add(length_symbol(t[0], len(t) > 2 and t[2])[0])
            dist.add(dist_symbol(t[1])[0])
    return lit, dist


def lengths_for(rng, used, n, spare: int = 0, max_len: int = 15):
    """random complete code lengths over `used` and `spare` more symbols of the n"""
    used = set(used)
    rest = [s for s in range(n) if s not in used]
    extra = [int(x) for x in rng.permutation(rest)[:spare]] if spare and rest else []
    syms = sorted(used) + extra
    if len(syms) < 2:
        syms.append(next(s for s in range(n) if s not in syms))
    ls = complete_lengths(rng, len(syms), max_len)
    out = [0] * n
    for s, l in zip(syms, ls):
        out[s] = l
    return out


def bgzf_member(deflate_bytes: bytes, payload: bytes, extra: bytes = b"", extra_front: bytes = b"", isize=None, crc=None) -> bytes:
    """the stream as a BGZF member (SAM spec 4.1): gzip header with the BC subfield, other subfields in front of it (extra_front)
    or behind it (extra) -- so XLEN and the payload's alignment vary --, CRC-32 and ISIZE of `payload` unless given."""
    xlen = len(extra_front) + 6 + len(extra)
    bsize = 12 + xlen + len(deflate_bytes) + 8 - 1
    assert bsize <= 0xFFFF, "does not fit a BGZF member"
    head = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, xlen) + extra_front + struct.pack("<BBHH", 66, 67, 2, bsize) + extra
    crc = zlib.crc32(payload) & 0xFFFFFFFF if crc is None else crc
    return head + deflate_bytes + struct.pack("<II", crc, (len(payload) if isize is None else isize) & 0xFFFFFFFF)


def subfield(n_data: int, tag: bytes = b"ZZ") -> bytes:
    """a gzip extra subfield of 4 + n_data bytes"""
    return tag + struct.pack("<H", n_data) + bytes(range(1, n_data + 1))


def zlib_verdict(deflate_bytes: bytes, isize: int):
    """the reference's rule: accept iff zlib reports no error, reaches the end of the stream and gives isize bytes -> (ok, bytes)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(deflate_bytes)
    except zlib.error:
        return False, b""
    return bool(d.eof) and len(out) == isize, out
