"""The forged DEFLATE streams of test_deflate_forge_cpu.py (held against zlib, no GPU) and test_gpu_inflate_forged.py (the same
streams through both GPU inflaters): one table of classes, built from fixed seeds, so both modules see the same bytes.

LEGAL[name]() -> [Case]: streams zlib inflates to Case.payload.  MALFORMED[name]() -> [Case]: streams zlib refuses (or, for the
two ISIZE cases, inflates to another length than the trailer says); Case.isize / Case.payload are what a decoder WITHOUT the
check in question would produce, so that only the stream gives the member away.

Geometry.  The wave decoder (k_inflate_wave.hip) reads a member's payload as 8-byte units from the aligned address in front of
it -- the payload begins `mis` bytes (0 .. 7) into a unit --, cuts the body of a block into chunks of 64 pieces of PIECE bits,
and a chunk begins with the unit in which its first symbol begins.  Case.geo = (block, what, rel) claims that `what` of that
block (its end-of-block code, or symbol i) begins `rel` bits into the block's FIRST chunk; the CPU module proves every claim
from the forge's ledger (chunk_rel).  build_file() places a member so that `mis` is what the case was built for.
"""
import functools
import itertools
import zlib

import numpy as np

from deflate_forge import (DIST_BASE, DIST_EXTRA, FIXED_LIT, Dynamic, Fixed, Raw, Stored, bgzf_member, canonical, flat_lengths, forge,
                           lengths_for, parse, rle_greedy, rle_none, rle_random, subfield, used_symbols)

# k_inflate_wave.hip: IW_PIECE_LOG2 9, IW_GRAIN_LOG2 6, 64 pieces per chunk, LIT_TAIL / DIST_TAIL, MAXS (test_deflate_forge_cpu reads
# them out of the source and compares)
PIECE, GRAIN, CHUNK, LIT_TAIL, DIST_TAIL, MAXS = 512, 64, 64 * 512, 512, 256, 256
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_DEFLATE = 65536 - 18 - 8                       # what fits a BGZF member with the BC subfield alone


class Case:
    def __init__(self, name, forged, mis=None, geo=None, isize=None, payload=None, note=""):
        self.name, self.f, self.mis, self.geo, self.note = name, forged, mis, geo, note
        self.data, self.ledger = forged.data, forged.ledger
        self.payload = forged.payload if payload is None else payload
        self.isize = len(self.payload) if isize is None else isize


def chunk_rel(case, block: int, bit: int) -> int:
    """bit (of the stream) relative to the first chunk of the body of `block`, as the wave decoder cuts it for case.mis"""
    body = case.ledger[block]["body"]
    return 8 * case.mis + bit - 64 * ((8 * case.mis + body) // 64)


def text(rng, n: int) -> bytes:
    """compressible bytes of a few kinds (record-like text, skewed bytes, runs)"""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        words = [b"chr%d\t" % int(rng.integers(1, 23)), b"ACGT", b"m64011/", b"\t255\t", b"TTAGGG", b"ccs\n"] + [bytes(rng.integers(48, 58, 5, dtype=np.uint8))]
        out = b"".join(words[int(k)] for k in rng.integers(0, len(words), n // 3 + 2))
    elif kind == 1:
        out = bytes(rng.choice(np.arange(256, dtype=np.uint8), size=n, p=np.r_[0.4, 0.3, np.full(254, 0.3 / 254)]))
    elif kind == 2:
        seed = bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))
        out = b"".join(seed[:int(k) + 1] * int(r) for k, r in zip(rng.integers(0, len(seed), n // 8 + 2), rng.integers(1, 30, n // 8 + 2)))
    else:
        out = bytes(rng.integers(0, 4, n, dtype=np.uint8) + 65)
    return (out * (n // max(len(out), 1) + 1))[:n]


def dyn(rng, tokens, max_len=15, spare=None, dist_mode=None, coder=None, **kw):
    """a dynamic block with random complete codes over what the tokens use (and `spare` more symbols); no distance used:
    dist_mode 0 = HDIST 1 with length 0, 1 = one code of length 1, 2 = a complete code nobody uses"""
    lit, dist = used_symbols(tokens)
    lit = {s for s in lit if s < 286}
    ll = lengths_for(rng, lit, 286, int(rng.integers(0, 40)) if spare is None else spare, max_len)
    dist = {s for s in dist if s < 30}
    if not dist:
        m = int(rng.integers(0, 3)) if dist_mode is None else dist_mode
        dl = [0] if m == 0 else [0] * int(rng.integers(0, 30)) + [1] if m == 1 else lengths_for(rng, set(), 30, int(rng.integers(2, 30)), max_len)
    elif len(dist) == 1 and (dist_mode == 1 or (dist_mode is None and rng.random() < 0.5)):
        dl = [0] * 30
        dl[next(iter(dist))] = 1
    else:
        dl = lengths_for(rng, dist, 30, int(rng.integers(0, 10)) if spare is None else min(spare, 29 - len(dist)), max_len)
    if coder is not None and "rle" not in kw:
        hl = max(257, max(i + 1 for i, l in enumerate(ll) if l))
        hd = max(1, max([i + 1 for i, l in enumerate(dl) if l] or [1]))
        kw["rle"] = coder((ll + [0] * 286)[:hl] + (dl + [0] * 30)[:hd])
    return Dynamic(tokens, ll, dl, **kw)


def random_cl(rng, rle):
    """a random complete code-length code (at most 7 bits) over the symbols the header uses"""
    used = sorted({r[0] for r in rle})
    return lengths_for(rng, used, 19, int(rng.integers(0, 19 - len(used) + 1)) if len(used) < 19 else 0, 7)


def counts_lengths(counts, n, symbols):
    """{length: how many} -> n lengths, the longest codes on the first of `symbols`; the set must be complete"""
    assert sum(c << (15 - l) for l, c in counts.items()) == 1 << 15, "not a complete set"
    ls = sorted((l for l, c in counts.items() for _ in range(c)), reverse=True)
    assert len(ls) <= len(symbols)
    out = [0] * n
    for s, l in zip(symbols, ls):
        out[s] = l
    return out


def literals_for_bits(rng, lit_lens, nbits: int):
    """literals whose codes add up to exactly nbits"""
    by_len = {}
    for s in range(256):
        if lit_lens[s]:
            by_len.setdefault(lit_lens[s], []).append(s)
    ls = sorted(by_len)
    toks, rest = [], nbits
    while rest > 40 * ls[-1]:
        l = ls[int(rng.integers(0, len(ls)))]
        toks.append(int(rng.choice(by_len[l]))); rest -= l
    reach = [None] * (rest + 1)
    reach[0] = 0
    for v in range(1, rest + 1):
        for l in ls:
            if v >= l and reach[v - l] is not None:
                reach[v] = l
                break
    assert reach[rest] is not None, "no literals add up to %d bits" % rest
    while rest:
        l = reach[rest]
        toks.append(int(rng.choice(by_len[l]))); rest -= l
    return toks


# ---- legal: code shapes ---------------------------------------------------------------------------------------------------------

def skewed_lit():
    """complete lit/len codes of lengths 1, 2, ..., 14, 15, 15; the 1-bit code on a literal, on 256, on a length code"""
    rng = np.random.default_rng(101)
    out = []
    for k in range(8):
        lits = [int(x) for x in rng.permutation(256)[:15]]
        order = [lits + [256], [256] + lits, lits[:14] + [257, 256], [257] + lits[:14] + [256]][k % 4]
        ll = [0] * 286
        for i, s in enumerate(order):
            ll[s] = min(i + 1, 15)
        syms = [s for s in order if s != 256]
        p = np.array([2.0 ** -ll[s] for s in syms]) + 0.02
        body = [lits[0]] + [int(x) for x in rng.choice(syms, size=int(rng.integers(50, 6000)), p=p / p.sum())]
        body = [(3, 1) if b == 257 else b for b in body]
        out.append(Case("skewed %d" % k, forge([Dynamic(body, ll, [1] if 257 in order else [0])])))
    return out


def _long_lit(rng, shape, n_tok):
    syms = [int(x) for x in rng.permutation(256)[:sum(shape.values()) - 1]] + [256]
    ll = counts_lengths(shape, 286, syms[::-1])               # (256 among the longest)
    longs = [s for s in syms if s < 256 and ll[s] >= 10]
    return [int(x) for x in rng.choice(longs, size=n_tok)], ll


def lit_tail_overflow():
    """used lit/len codes of 10 .. 15 bits whose 15-bit values span 1024 > LIT_TAIL entries: the wave decoder's search_l"""
    rng = np.random.default_rng(102)
    shape = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 10: 16, 11: 16, 12: 16, 13: 16, 14: 16, 15: 32}
    out = []
    for k in range(4):
        toks, ll = _long_lit(rng, shape, int(rng.integers(100, 3000)))
        out.append(Case("lit tail %d" % k, forge([Dynamic(toks, ll, [0]), Fixed(toks[:20])][:1 + k % 2])))
    return out


def _dist_tokens(rng, dsyms, n):
    """literals first, then matches whose distance symbols come from dsyms (distances that reach at most to the start)"""
    toks, size = [int(x) for x in rng.integers(0, 256, 40)], 40
    for _ in range(n):
        ok = [d for d in dsyms if DIST_BASE[d] <= size]
        if not ok or rng.random() < 0.3:
            toks.append(int(rng.integers(0, 256))); size += 1
            continue
        d = int(rng.choice(ok))
        dist = min(size, DIST_BASE[d] + int(rng.integers(0, 1 << DIST_EXTRA[d])))
        length = int(rng.integers(3, 259))
        toks.append((length, dist)); size += length
    return toks


def dist_shapes():
    """30 distance codes, maximally skewed with two of 15 bits; used distance codes of 9 .. 13 bits whose values span 1024 >
    DIST_TAIL entries (search_d); every used distance code longer than both decoders' primary tables (8 and 5 bits)"""
    rng = np.random.default_rng(103)
    out = []
    skew = list(range(1, 15)) + [15, 15]
    while len(skew) < 30:                                       # split the shortest leaf: still complete, still two of 15
        skew.sort()
        l = skew.pop(0)
        skew += [l + 1, l + 1]
    assert sum(1 << (15 - l) for l in skew) == 1 << 15 and skew.count(15) >= 2
    wide = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 9: 12, 10: 6, 11: 2, 12: 3, 13: 2}
    for k in range(6):
        if k < 3:
            dl = [int(x) for x in rng.permutation(skew)]
            dsyms = list(range(30))
        else:
            order = [int(x) for x in rng.permutation(30)]
            dl = counts_lengths(wide, 30, order)
            dsyms = [s for s in range(30) if dl[s] >= 9]
        toks = _dist_tokens(rng, dsyms, int(rng.integers(60, 200)))
        ll = lengths_for(rng, used_symbols(toks)[0], 286, 10)
        out.append(Case("dist %s %d" % ("skew" if k < 3 else "tail", k), forge([Dynamic(toks, ll, dl)])))
    return out


def long_used_codes():
    """every USED lit/len code is longer than the primary tables of both decoders (9 and 8 bits): 64 symbols of 15 bits, the
    nine short codes of the set (a complete set cannot do without them) never appear in the body"""
    rng = np.random.default_rng(104)
    out = []
    for k in range(3):
        toks, ll = _long_lit(rng, {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1, 9: 1, 15: 64}, int(rng.integers(100, 2500)))
        out.append(Case("long used %d" % k, forge([Dynamic(toks, ll, [0])])))
    return out


def few_dist_codes():
    """the distance alphabets zlib's encoder never writes: one code of length 1 (incomplete, and allowed), HDIST 1 with length 0,
    and a lit/len alphabet that is the end-of-block code alone (an empty dynamic block)"""
    rng = np.random.default_rng(105)
    out = []
    for d in (0, 3, 10, 29):
        toks = [int(x) for x in rng.integers(0, 256, DIST_BASE[d] + (1 << DIST_EXTRA[d]) + 5)]
        for _ in range(40):
            toks.append((int(rng.integers(3, 259)), DIST_BASE[d] + int(rng.integers(0, 1 << DIST_EXTRA[d]))))
            toks.append(int(rng.integers(0, 256)))
        if d == 29:
            toks = toks[:DIST_BASE[d] + (1 << DIST_EXTRA[d]) + 5 + 30]
        out.append(Case("one distance code %d" % d, forge([dyn(rng, toks, dist_mode=1)])))
    toks = [int(x) for x in rng.integers(0, 256, 3000)]
    out.append(Case("hdist 1 length 0", forge([dyn(rng, toks, dist_mode=0)])))
    empty = Dynamic([], [0] * 256 + [1], [0])
    out.append(Case("empty dynamic alone", forge([empty])))
    out.append(Case("empty dynamic first", forge([empty, Fixed(toks[:100]), empty, dyn(rng, toks[:500]), empty])))
    return out


def header_extremes():
    """HLIT 257 and 286, HCLEN 19 and 5.  (HCLEN 4 sends the lengths of the symbols 16, 17, 18 and 0 only: no code length but 0 can
    be sent, so 256 has no code -- it is a malformed class; 5 adds length 8: 256 codes of 8 bits are the one legal set.)"""
    rng = np.random.default_rng(106)
    out = []
    toks = [int(x) for x in rng.integers(0, 256, 2000)]
    b = dyn(rng, toks, spare=0, dist_mode=0)
    assert max(i for i, l in enumerate(b.lit_lens) if l) == 256
    out.append(Case("hlit 257", forge([b])))
    t2 = toks[:500] + [(258, 7), (200, 400)]
    b = dyn(rng, t2, spare=0)
    b.hlit = 286
    out.append(Case("hlit 286 by trailing zeros", forge([b])))
    out.append(Case("hlit 286 by a code for 285", forge([dyn(rng, t2 + [(258, 1)], spare=0)])))
    b = dyn(rng, toks, dist_mode=0)
    b.hclen = 19
    out.append(Case("hclen 19 by trailing zeros", forge([b])))
    ll = [8] * 257
    ll[int(rng.integers(0, 256))] = 0
    b = Dynamic([t for t in toks if ll[t]], ll, [0])
    f = forge([b])
    assert f.ledger[0]["hclen"] == 5
    out.append(Case("hclen 5", f))
    return out


# ---- legal: header coding --------------------------------------------------------------------------------------------------------

def header_coding():
    """lengths sent with no repeats; repeats that run across the lit / dist boundary (of zeros and of a length); chains of 16 with 6
    and 18 with 138; random codings with random code-length codes"""
    rng = np.random.default_rng(107)
    out = []
    toks = parse(rng, text(rng, 3000))
    out.append(Case("no repeats", forge([dyn(rng, toks, coder=rle_none)])))
    # zeros across the boundary: no length code above 268 (lengths up to 18), HLIT 286 all the same, no distance symbol below 10
    pay = text(rng, 3000)
    t, i = [], 0
    for x in parse(rng, pay):
        n = 1 if isinstance(x, int) else x[0]
        t += [x] if isinstance(x, int) or (x[0] <= 18 and x[1] >= 33) else list(pay[i:i + n])
        i += n
    t += [(18, 33), (3, 1000)]
    b = dyn(rng, t, spare=0)
    b.hlit = 286
    coding = rle_greedy((b.lit_lens + [0] * 286)[:286] + b.dist_lens)
    k = next(i for i, r in enumerate(coding) if sum(1 if len(q) == 1 else q[1] for q in coding[:i + 1]) > 286)
    assert coding[k][0] == 18 and sum(1 if len(q) == 1 else q[1] for q in coding[:k]) < 286, "no run of zeros across the boundary"
    out.append(Case("zeros across the boundary", forge([b])))
    # a length across the boundary: 32 lit/len symbols of 5 bits that end with 283 .. 285, distance codes that begin with 5-bit ones
    lits = [int(x) for x in rng.permutation(256)[:28]]
    ll = flat_lengths(lits + [256, 283, 284, 285], 286)
    dl = [5] * 28 + [4] * 2
    body = [int(x) for x in rng.choice(lits, 300)] + [(258, 3), (227, 100), (258, 200, True), (200, 50)]
    b = Dynamic(body, ll, dl)
    coding = rle_greedy(ll + dl)
    k = next(i for i, r in enumerate(coding) if r == (5,) and sum(1 if len(q) == 1 else q[1] for q in coding[:i]) == 283)
    assert coding[k + 1] == (16, 6), "the repeat does not run across the boundary"
    out.append(Case("a length across the boundary", forge([b])))
    # chains: 286 lit/len codes of 8 and 9 bits (16 with 6, dozens in a row); literals 200 .. 255 only (18 with 138 in front of them)
    ll = flat_lengths(range(286), 286)
    out.append(Case("chains of 16", forge([Dynamic(toks, ll, flat_lengths(range(30), 30))])))
    hi = [int(x) for x in rng.integers(200, 256, 1500)]
    b = dyn(rng, hi, spare=0, dist_mode=0)
    assert rle_greedy(b.lit_lens)[0] == (18, 138)
    out.append(Case("18 with 138", forge([b])))
    for k in range(12):
        tk = parse(rng, text(rng, int(rng.integers(10, 3000))))
        b = dyn(rng, tk, coder=lambda ls: rle_random(rng, ls))
        b.cl_lens = random_cl(rng, b.rle)
        out.append(Case("random coding %d" % k, forge([b])))
    return out


LONGEST_HEADER = 3 + 14 + 19 * 3 + 316 * 7          # every one of 286 + 30 lengths sent plainly by a 7-bit code: 2 286 bits


def longest_header():
    """the longest legal header: HLIT 286, HDIST 30, HCLEN 19, and every length a 7-bit code of its own -- a repeat code sends three
    lengths at least for 9 bits, so nothing is longer.  (k_inflate_wave.hip stages 8 192 bits for a header.)"""
    rng = np.random.default_rng(108)
    cl = [0] * 19
    for s, l in zip((16, 17, 18, 0, 1), (2, 2, 2, 3, 6)):
        cl[s] = l
    for s in range(2, 16):
        cl[s] = 7
    assert sum(1 << (7 - l) for l in cl if l) == 128
    ll = flat_lengths(range(286), 286)                  # 8 and 9
    dl = flat_lengths(range(30), 30)                    # 4 and 5
    out = []
    for k in range(2):
        toks = parse(rng, text(rng, 4000))
        out.append(Case("longest header %d" % k, forge([Fixed(toks[:k * 7]), Dynamic(toks, ll, dl, cl_lens=cl, rle=rle_none(ll + dl))])))
    return out


def header_offsets():
    """a dynamic header beginning at every bit offset 0 .. 63 of an 8-byte unit (a fixed block of the right length in front of it)"""
    rng = np.random.default_rng(109)
    out = []
    for k in range(64):
        mis = k % 8
        target = (k - 8 * mis) % 64                      # where the header begins in the stream, mod 64
        nb = (target - 2) % 8
        na = next(a for a in range(8) if (10 + 8 * a + 9 * nb) % 64 == target)
        front = [int(x) for x in rng.integers(0, 144, na)] + [int(x) for x in rng.integers(144, 256, nb)]
        toks = parse(rng, text(rng, int(rng.integers(20, 1500))))
        c = Case("header at bit %d" % k, forge([Fixed(front), dyn(rng, toks)]), mis=mis)
        c.header_bit = k
        out.append(c)
    return out


# ---- legal: block structure ----------------------------------------------------------------------------------------------------------

def _blocks_of(rng, pay, kinds, pad=0):
    """pay cut into len(kinds) blocks ('s' stored, 'f' fixed, 'd' dynamic); matches reach back into the blocks in front"""
    cuts = sorted(int(x) for x in rng.integers(0, len(pay) + 1, len(kinds) - 1))
    blocks, lo = [], 0
    for kind, hi in zip(kinds, cuts + [len(pay)]):
        if kind == "s":
            blocks.append(Stored(pay[lo:hi], pad=pad))
        else:
            toks = parse(rng, pay[:hi], window_start=lo)
            blocks.append(Fixed(toks) if kind == "f" else dyn(rng, toks))
        lo = hi
    return blocks


def block_orders():
    """the three block types in every order (all 27 sequences of three), matches reaching across the boundaries"""
    rng = np.random.default_rng(110)
    out = []
    for kinds in itertools.product("sfd", repeat=3):
        pay = text(rng, int(rng.integers(30, 4000)))
        out.append(Case("blocks " + "".join(kinds), forge(_blocks_of(rng, pay, kinds))))
    return out


def empty_and_stored_blocks():
    """empty stored and empty fixed blocks in mid-stream (sync / partial flushes); stored blocks behind a Huffman block with padding
    bits that are not zero; stored blocks of 0, 1 and 65 505 bytes (the largest a BGZF member holds); members of stored blocks only"""
    rng = np.random.default_rng(111)
    out = []
    pay = text(rng, 3000)
    b = _blocks_of(rng, pay, "fdfd")
    out.append(Case("empty blocks between", forge([Stored()] + [x for y in b for x in (y, Stored(), Fixed(), Fixed(), Stored(pad=0x7F))])))
    for k in range(8):
        front = [int(x) for x in rng.integers(0, 144, k)]           # the stored block's header at every bit of a byte
        f = forge([Fixed(front), Stored(pay[:100 + k], pad=0xFF), dyn(rng, parse(rng, pay[:500])), Stored(pay[:k], pad=0x55), Fixed([(50, 3)])])
        out.append(Case("stored behind huffman, padding set %d" % k, f))
    out.append(Case("stored 0 alone", forge([Stored()])))
    out.append(Case("stored 1", forge([Stored(b"x")])))
    big = bytes(rng.integers(0, 256, MAX_DEFLATE - 5, dtype=np.uint8))
    out.append(Case("stored 65505", forge([Stored(big)])))
    out.append(Case("stored only", forge([Stored(pay[:7]), Stored(), Stored(pay[7:2000]), Stored(pay[2000:2001]), Stored(pay[2001:])])))
    return out


def many_blocks():
    """more than 60 blocks of a few symbols, each with tables of its own"""
    rng = np.random.default_rng(112)
    out = []
    for k in range(3):
        pay = text(rng, 1200)
        n = 61 + 20 * k
        kinds = "".join("d" if rng.random() < 0.8 else "fs"[int(rng.integers(0, 2))] for _ in range(n))
        out.append(Case("%d blocks" % n, forge(_blocks_of(rng, pay, kinds))))
    return out


def trailing_bytes():
    """a last block followed by bytes no block uses, in front of the CRC (zlib leaves them in unused_data; so must the GPU)"""
    rng = np.random.default_rng(113)
    out = []
    for k, tail in enumerate((b"\x00", b"\xff" * 3, bytes(rng.integers(0, 256, 200, dtype=np.uint8)))):
        pay = text(rng, 2000)
        f = forge(_blocks_of(rng, pay, "df"[:1 + k % 2]), tail_pad=0x7F, tail=tail)
        out.append(Case("unused bytes %d" % len(tail), f))
    return out


# ---- legal: geometry -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _geo_code(kind):
    """the literal code of the geometric cases -> (lit/len lengths, bits of the header of a member's first block)"""
    if kind == "fixed":
        return tuple(FIXED_LIT), 3
    ll = lengths_for(np.random.default_rng(77), set(range(0, 256, 3)) | {256}, 286, 0, 12)
    return tuple(ll), forge([Dynamic([], ll, [0])]).ledger[0]["body"]


def _geo_block(kind, toks):
    return Fixed(toks) if kind == "fixed" else Dynamic(toks, list(_geo_code(kind)[0]), [0])


def _body_to(rng, kind, rel, mis):
    """a block (first of its member) whose end-of-block code begins `rel` bits into the body's first chunk"""
    ll, body0 = _geo_code(kind)
    return _geo_block(kind, literals_for_bits(rng, ll, rel - (8 * mis + body0) % 64))


def eob_positions():
    """the end-of-block code ending on the last bit / beginning on the first bit of a piece, of a grain and of a chunk, straddling a
    piece and a chunk boundary; bodies of one chunk and one chunk +- 1 bit; a block that ends in lane 0's piece.  Fixed and dynamic
    codes, every payload alignment."""
    rng = np.random.default_rng(114)
    out = []
    n = 0
    for kind in ("fixed", "dynamic"):
        for what, base, how in (("piece", 5 * PIECE, "ends"), ("piece", 9 * PIECE, "begins"), ("grain", 3 * PIECE + 5 * GRAIN, "ends"),
                                ("grain", 62 * PIECE + 7 * GRAIN, "begins"), ("chunk", CHUNK, "ends"), ("chunk", CHUNK, "begins"),
                                ("piece", 17 * PIECE, "straddles"), ("chunk", CHUNK, "straddles"), ("lane 0", 200, "ends the block in")):
            mis = n % 8
            n += 1
            L = _geo_code(kind)[0][256]
            rel = base - L if how == "ends" else base - 3 if how == "straddles" else base
            b = _body_to(rng, kind, rel, mis)
            follow = [] if n % 3 == 0 else [Fixed([int(x) for x in rng.integers(0, 256, 700)])]
            c = Case("%s eob %s %s" % (kind, how, what), forge([b] + follow), mis=mis, geo=(0, "eob", rel))
            c.eob_len, c.how, c.unit = L, how, {"piece": PIECE, "grain": GRAIN, "chunk": CHUNK, "lane 0": PIECE}[what]
            out.append(c)
        for d in (-1, 0, 1):                                    # the body, its end-of-block code included, is CHUNK + d bits
            mis = n % 8
            n += 1
            ll = _geo_code(kind)[0]
            b = _geo_block(kind, literals_for_bits(rng, ll, CHUNK + d - ll[256]))
            c = Case("%s body of a chunk %+d" % (kind, d), forge([b, Fixed([65] * 9)]), mis=mis)
            c.body_bits = CHUNK + d
            out.append(c)
    return out


def max_symbol_last_grain():
    """a 48-bit symbol -- 15-bit length code + 5 extra bits + 15-bit distance code + 13 extra bits -- beginning in the last grain
    of a chunk (64, 48, 17 and 1 bits in front of its end): it ends in the units kept behind the chunk"""
    rng = np.random.default_rng(115)
    out = []
    # lit/len: 62 literals of 7 bits, two of 6, 256 at 2, literals of 3, 4, 5 bits: 1 - 2^-6; the rest 7, 8, ..., 14, 15, 15 with the
    # length codes 283 / 284 (5 extra bits) at 15.  Distance: 1, 2, ..., 14, 15, 15 with the codes 28 / 29 (13 extra bits) at 15.
    ll = [0] * 286
    for s in range(62):
        ll[s] = 7
    ll[62], ll[63], ll[256], ll[100], ll[101], ll[102] = 6, 6, 2, 3, 4, 5
    for s, l in zip((103, 104, 105, 106, 107, 108, 109, 110, 283, 284), (7, 8, 9, 10, 11, 12, 13, 14, 15, 15)):
        ll[s] = l
    assert sum(1 << (15 - l) for l in ll if l) == 1 << 15
    dl = [0] * 30
    for s, l in zip(list(range(14)) + [28, 29], list(range(1, 15)) + [15, 15]):
        dl[s] = l
    for n, back in enumerate((64, 48, 17, 1)):
        mis = (3 * n + 1) % 8
        front = Stored(bytes(rng.integers(0, 256, 33000, dtype=np.uint8)))
        body0 = forge([front, Dynamic([], ll, dl)]).ledger[1]["body"]
        rel = CHUNK - back
        toks = literals_for_bits(rng, ll, rel - (8 * mis + body0) % 64)
        big = ("match", 284, 30, 29, 8191)                      # length 257, distance 32 768: 15 + 5 + 15 + 13 bits
        toks += [big, (258, 32768, True), 5, 6]
        out.append(Case("48-bit symbol %d bits in front of the chunk's end" % back, forge([front, Dynamic(toks, ll, dl)]), mis=mis,
                        geo=(1, len(toks) - 4, rel)))
    return out


def short_symbols():
    """bodies of 1- and 2-bit symbols: more symbols per piece than a lane lists (MAXS), handed back and still right; with matches of
    3 bits (2-bit length code, 1-bit distance code) among them"""
    rng = np.random.default_rng(116)
    out = []
    a, b = 65, 66
    ll = [0] * 257
    ll[a], ll[b], ll[256] = 1, 2, 2
    toks = [int(x) for x in rng.choice([a, b], size=60000, p=[0.7, 0.3])]
    out.append(Case("1- and 2-bit literals", forge([Dynamic(toks, ll, [0])])))
    ll = [0] * 258
    ll[a], ll[257], ll[256] = 1, 2, 2
    toks = [a] + [a if x else (3, 1) for x in rng.integers(0, 2, 21000)]
    out.append(Case("1-bit literals and 3-bit matches", forge([Dynamic(toks, ll, [1])])))
    return out


def _decode_from(bits, start, end, codes):
    """a model of one lane of pass 1: from bit `start` of the 0/1 string `bits` decode literal / end-of-block codes (codes: {code
    string: symbol}; there are no matches) while the position is in front of `end` -> [(position, symbol | None)]; None = no code
    begins there, the lane moves on by one bit (k_inflate_wave.hip step(), kind 3)"""
    out, p, longest = [], start, max(len(c) for c in codes)
    while p < end:
        for l in range(1, longest + 1):
            s = codes.get(bits[p:p + l])
            if s is not None and p + l <= len(bits):
                out.append((p, s)); p += l
                break
        else:
            out.append((p, None)); p += 1
    return out


def _bit_string(data: bytes) -> str:
    return "".join(format(b, "08b")[::-1] for b in data)


def _codes_of(ll):
    return {format(c, "0%db" % l)[::-1]: s for s, (c, l) in enumerate(canonical(ll)) if l}


def false_eobs(want=6):
    """a lane that passes more end-of-block-valued bit patterns on its wrong path than it remembers (four) before it falls into step
    with the true path inside its piece (own_code's `look again`): bodies searched over seeds with a model of a lane (_decode_from).
    The code: fourteen literals and 256 at 4 bits, two literals at 5 bits -- a wrong path keeps its phase over the 4-bit symbols,
    reads one in sixteen of them as 256, and changes phase at a 5-bit one.  Kept: bodies in which EVERY lane is in step within 400
    bits (so that no lane lists more than MAXS symbols and the wave decoder keeps the member).  -> cases with .lane / .false_eobs"""
    out = []
    lits = list(range(97, 113))
    ll = [0] * 257
    for s in lits[:14]:
        ll[s] = 4
    ll[256] = 4
    ll[lits[14]] = ll[lits[15]] = 5
    codes = _codes_of(ll)
    for seed in range(300):
        rng = np.random.default_rng(1000 + seed)
        n = 6 * 128
        toks = [int(x) for x in np.where(rng.random(n) < 0.15, rng.choice(lits[14:], n), rng.choice(lits[:14], n))]
        c = Case("false end-of-block codes, seed %d" % seed, forge([Dynamic(toks, ll, [0]), Fixed([65] * 5)]), mis=seed % 8)
        found = lane_with_false_eobs(c, codes, want)
        if found:
            c.lane, c.false_eobs = found
            out.append(c)
            if len(out) == 4:
                break
    return out


def lane_with_false_eobs(case, codes, want, in_step_within=400):
    """(lane, count): a lane of the first chunk of block 0 that decodes `want` or more end-of-block codes off the true path before it
    stands on a true symbol start -- in a body whose every lane stands on one within `in_step_within` bits; else None"""
    led = case.ledger[0]
    bits = _bit_string(case.data)
    origin = 64 * ((8 * case.mis + led["body"]) // 64) - 8 * case.mis        # the chunk's first bit, in bits of the stream
    true = set(led["syms"]) | {led["eob"]}
    best = None
    for lane in range(1, 64):
        lo = origin + lane * PIECE
        if lo + PIECE > led["eob"]:
            break
        n, met = 0, False
        for p, s in _decode_from(bits, lo, lo + in_step_within, codes):
            if p in true:
                met = True
                break
            n += s == 256
        if not met:
            return None
        if n >= want and (best is None or n > best[1]):
            best = (lane, n)
    return best


def never_in_step():
    """bodies whose lanes never fall into step: 255 literals and 256, all of 8 bits, the body not on the byte grid of the pieces -- a
    lane that starts off the true path stays off it (every code is 8 bits long), lane 0 runs through the whole chunk alone and
    overflows its list.  Proven by the same model: no lane but lane 0 ever stands on a true symbol start."""
    out = []
    for k, mis in enumerate((0, 3, 5)):
        rng = np.random.default_rng(117 + k)
        ll = [8] * 257
        ll[int(rng.integers(0, 256))] = 0
        lits = [s for s in range(256) if ll[s]]
        toks = [int(x) for x in rng.choice(lits, 9000)]
        c = Case("never in step %d" % k, forge([Dynamic(toks, ll, [0])]), mis=mis)
        c.codes = _codes_of(ll)
        out.append(c)
    return out


# ---- legal: copies ---------------------------------------------------------------------------------------------------------------

def copy_depth(tokens):
    """per output byte, how many copies deep it is (a literal: 0)"""
    d = []
    for t in tokens:
        if isinstance(t, int):
            d.append(0)
        else:
            for _ in range(t[0]):
                d.append(d[len(d) - t[1]] + 1)
    return d


def deep_chains():
    """matches on matches, 16 and more deep: a copy of a copy of ...; not overlapping (distance = length), at doubling distances, and
    always into the last few bytes.  Case.tokens: for copy_depth"""
    rng = np.random.default_rng(118)
    first = [int(x) for x in rng.integers(0, 256, 8)]
    a = first + [(8, 8)] * 40
    b, size = list(first), 8
    for k in range(12):
        d = min(8 << k, size)
        b.append((min(d, 258), d)); size += min(d, 258)
    b += [(258, 258)] * 30                                    # each the copy of the one in front of it
    c, size = list(first), 8
    for k in range(300):
        length = int(rng.integers(3, 40))
        c.append((length, int(rng.integers(1, min(size, 30) + 1)))); size += length
    out = [Case("chain distance 8", forge([Fixed(a)])), Case("chain doubling", forge([dyn(rng, b)])), Case("chain of recent copies", forge([dyn(rng, c)]))]
    for case, toks in zip(out, (a, b, c)):
        case.tokens = toks
    return out


def runs():
    """members of 65 536 bytes made of one period (1 .. 9 bytes) of literals and matches at that distance; the same at 65 535"""
    rng = np.random.default_rng(119)
    out = []
    for period in range(1, 10):
        for size in ((65536,) if period > 1 else (65536, 65535)):
            toks = [int(x) for x in rng.integers(0, 256, period)]
            left = size - period
            while left:
                n = min(258, left) if left - min(258, left) == 0 or left - min(258, left) >= 3 else left - 3
                if n < 3:
                    toks += [toks[(size - left + i) % period] for i in range(left)]
                    break
                toks.append((n, period) if n != 258 or rng.random() < 0.7 else (258, period, True))
                left -= n
            b = Fixed(toks) if period % 2 else dyn(rng, toks)
            out.append(Case("period %d, %d bytes" % (period, size), forge([b])))
    return out


def long_matches():
    """length 258 in both codings (code 285, and code 284 with extra bits 31), fixed and dynamic; distance exactly 32 768 at output
    offset 32 768; members of 65 535 and 65 536 bytes of parsed text"""
    rng = np.random.default_rng(120)
    out = []
    first = [int(x) for x in rng.integers(0, 256, 300)]
    toks = first + [(258, 300), (258, 1, True), 7, (258, 258, True), (258, 259), (257, 1), (258, 816, True)]
    out.append(Case("258 both ways, fixed", forge([Fixed(toks)])))
    out.append(Case("258 both ways, dynamic", forge([dyn(rng, toks)])))
    far = [int(x) for x in rng.integers(0, 256, 32768)]
    out.append(Case("distance 32768 at 32768", forge([Fixed(far + [(258, 32768), (3, 32768), 9, (258, 32768, True)])])))
    out.append(Case("distance 32768 at 32768, dynamic", forge([dyn(rng, far + [(258, 32768), 9, (100, 32767)], max_len=12)])))
    for size in (65535, 65536):
        pay = text(np.random.default_rng(size), size)
        toks = parse(rng, pay)
        out.append(Case("parsed text, %d bytes" % size, forge([dyn(rng, toks)])))
        out.append(Case("parsed text in blocks, %d bytes" % size, forge(_blocks_of(rng, pay, "dfdsd"))))
    return out


# ---- legal: randomised -----------------------------------------------------------------------------------------------------------

def _random_member(rng, size):
    pay = text(rng, size)
    n_blocks = int(rng.choice([1, 1, 2, 3, 6]))
    kinds = "".join(rng.choice(list("dddfs")) for _ in range(n_blocks))
    blocks = _blocks_of(rng, pay, kinds, pad=int(rng.integers(0, 128)))
    for b in blocks:
        if isinstance(b, Dynamic) and rng.random() < 0.6:
            hl = max(257, max(i + 1 for i, l in enumerate(b.lit_lens) if l))
            hd = max(1, max([i + 1 for i, l in enumerate(b.dist_lens) if l] or [1]))
            b.rle = rle_random(rng, (b.lit_lens + [0] * 286)[:hl] + (b.dist_lens + [0] * 30)[:hd])
            b.cl_lens = random_cl(rng, b.rle)
    return forge(blocks)


N_RANDOM_SMALL, N_RANDOM_FULL = 700, 12


def _randomised(seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(N_RANDOM_SMALL):
        out.append(Case("random %d/%d" % (seed, k), _random_member(rng, int(rng.choice([0, 1, 2, 5, 40, 300, 1500, 4096])) if k % 3 else int(rng.integers(0, 4097)))))
    for k in range(N_RANDOM_FULL):
        size = int(rng.choice([65536, 65535, 65280, 50000, int(rng.integers(30000, 65537))]))
        while True:
            f = _random_member(rng, size)
            if len(f.data) <= MAX_DEFLATE - 16:
                break
        out.append(Case("random full %d/%d" % (seed, k), f))
    return out


LEGAL = dict(skewed_lit=skewed_lit, lit_tail_overflow=lit_tail_overflow, dist_shapes=dist_shapes, long_used_codes=long_used_codes,
             few_dist_codes=few_dist_codes, header_extremes=header_extremes, header_coding=header_coding, longest_header=longest_header,
             header_offsets=header_offsets, block_orders=block_orders, empty_and_stored_blocks=empty_and_stored_blocks,
             many_blocks=many_blocks, trailing_bytes=trailing_bytes, eob_positions=eob_positions,
             max_symbol_last_grain=max_symbol_last_grain, short_symbols=short_symbols, false_eobs=false_eobs, never_in_step=never_in_step,
             deep_chains=deep_chains, runs=runs, long_matches=long_matches,
             random_seed_1=functools.partial(_randomised, 1), random_seed_2=functools.partial(_randomised, 2),
             random_seed_3=functools.partial(_randomised, 3))


# ---- malformed ---------------------------------------------------------------------------------------------------------------------

def _bad(name, blocks, isize=None, cut=0, **kw):
    f = forge(blocks, **kw)
    if cut:
        f.data = f.data[:-cut]
    return Case(name, f, isize=isize)


def _complete_block(rng, n=400):
    toks = parse(rng, text(rng, n)) + [(5, 1), (9, 7), (30, 20), (4, 300)]
    return toks, dyn(rng, toks, spare=3, dist_mode=2, coder=rle_greedy)


MALFORMED_CLASSES = ("far_distance", "fixed_code_unused_symbols", "over_subscribed", "incomplete", "no_end_of_block_code", "bad_repeats",
                     "too_many_codes", "block_type_3", "stored_lengths", "truncated", "isize")


def malformed():
    rng = np.random.default_rng(200)
    out = {}
    lit = [int(x) for x in rng.integers(0, 256, 300)]
    # a distance reaching before the start of the member; the lengths still add up to ISIZE
    out["far_distance"] = [_bad("first symbol a match", [Fixed([(10, 1)] + lit)]),
                           _bad("one byte too far", [Fixed(lit[:7] + [(20, 8)] + lit)]),
                           _bad("in the second block", [Fixed(lit[:100]), dyn(rng, [(5, 101)] + lit)]),
                           _bad("32768 at 32767", [Stored(bytes(32767)), Fixed([(258, 32768)])])]
    # lit/len symbols 286 / 287 and distance symbols 30 / 31: the fixed code has code words for them
    out["fixed_code_unused_symbols"] = [_bad("lit/len %d" % s, [Fixed(lit[:50] + [("lit", s)] + lit[:50])]) for s in (286, 287)] + \
                                       [_bad("distance %d" % s, [Fixed(lit[:50] + [("match", 257, 0, s, 0)] + lit[:50])]) for s in (30, 31)]
    # over-subscribed and incomplete sets: a complete set with one code more / one code fewer -- a code the body does not use, so
    # that a decoder which does not look at the set decodes the member
    over, under = [], []
    for which in ("lit", "dist", "cl"):
        for more, bucket in ((True, over), (False, under)):
            toks, b = _complete_block(rng)
            if which == "cl":
                b.cl_lens = flat_lengths([r[0] for r in b.rle], 19)
                if more:
                    b.cl_lens[next(s for s in range(19) if b.cl_lens[s] == 0)] = 7
                else:
                    b.cl_lens[next(s for s in range(19) if 0 < b.cl_lens[s] < 7)] += 1
            else:
                lens = b.lit_lens if which == "lit" else b.dist_lens
                used = used_symbols(toks)[0 if which == "lit" else 1]
                if more:
                    lens[next(s for s in range(len(lens)) if lens[s] == 0)] = 15
                else:
                    lens[next(s for s in range(len(lens)) if lens[s] and s not in used)] = 0
                b.rle = None
            bucket.append(_bad("%s set %s" % (which, "over-subscribed" if more else "incomplete"), [b]))
    out["over_subscribed"] = over
    ll = lengths_for(rng, used_symbols(lit + [(9, 1)])[0], 286)
    under.append(_bad("one distance code of 2 bits", [Dynamic(lit[:5] + [(9, 1)] + lit, ll, [2])]))
    under.append(_bad("two distance codes of 2 bits", [Dynamic(lit[:5] + [(9, 1), (9, 2)] + lit, ll, [2, 2])]))
    under.append(_bad("256 alone at 2 bits", [Dynamic([], [0] * 256 + [2], [0])]))
    under.append(_bad("distance codes nobody uses, incomplete", [Dynamic(lit, lengths_for(rng, used_symbols(lit)[0], 286), [3, 3, 3])]))
    out["incomplete"] = under
    # no code for 256 (and HCLEN 4, which can send no length but 0): the stream ends where its literals end
    ll = lengths_for(rng, set(lit) | {257}, 286)
    assert ll[256] == 0
    cl = [0] * 19
    cl[0] = cl[18] = 1
    out["no_end_of_block_code"] = [_bad("no code for 256", [Dynamic(lit, ll, [1], eob=False)]),
                                   _bad("hclen 4", [Dynamic([], [0] * 257, [0], cl_lens=cl, rle=[(18, 138), (18, 119), (0,)], hclen=4, eob=False), Raw(0, 64)], isize=0)]
    # symbol 16 as the first length; a repeat running past HLIT + HDIST
    toks, b = _complete_block(rng)
    first16 = dyn(rng, toks, coder=rle_none)
    first16.rle = [(16, 3)] + first16.rle[3:]
    past = dyn(rng, toks, coder=rle_none)
    past.rle = past.rle[:-1] + [(18, 11)]
    past2 = dyn(rng, toks, coder=rle_none)
    past2.rle = past2.rle[:-1] + [(16, 6)]
    out["bad_repeats"] = [_bad("16 first", [first16]), _bad("18 past the end", [past]), _bad("16 past the end", [past2])]
    # HLIT > 286, HDIST > 30
    hl = []
    for n in (287, 288):
        hl.append(_bad("hlit %d" % n, [Dynamic(lit, flat_lengths(range(n), n), [0], hlit=n)]))
    for n in (31, 32):
        hl.append(_bad("hdist %d" % n, [Dynamic(lit, flat_lengths(range(257), 257), flat_lengths(range(n), n), hdist=n)]))
    out["too_many_codes"] = hl
    out["block_type_3"] = [_bad("first block", [Raw(0b111, 3), Raw(0, 61)], isize=0),
                           _bad("behind a good block", [Fixed(lit, final=False), Raw(0b110, 3), Raw(0, 61)])]
    out["stored_lengths"] = [_bad("len / nlen", [Fixed(lit, final=False), Stored(bytes(lit), nlen_field=len(lit), final=True)]),
                             _bad("nlen off by a bit", [Stored(bytes(lit), nlen_field=(len(lit) ^ 0xFFFF) ^ 0x100)]),
                             _bad("longer than the member", [Fixed(lit, final=False), Stored(bytes(lit), len_field=1000, nlen_field=1000 ^ 0xFFFF, final=True)],
                                  isize=len(lit) + 1000),
                             _bad("longer than the member by one", [Stored(bytes(lit), len_field=301, nlen_field=301 ^ 0xFFFF)], isize=301)]
    toks, b = _complete_block(rng, 2000)
    out["truncated"] = [_bad("no final block", [Fixed(lit, final=False), Stored(b"abc", final=False)]),
                        _bad("no final block, dynamic", [dyn(rng, toks, final=False)]),
                        _bad("ends inside a symbol", [Fixed(lit)], cut=1),
                        _bad("ends inside a header", [Fixed(lit, final=False), b], cut=len(forge([b]).data) - 20, isize=len(lit)),
                        _bad("ends inside a dynamic body", [b], cut=40)]
    ok = forge([dyn(rng, toks)])
    out["isize"] = [Case("one byte short of ISIZE", ok, isize=len(ok.payload) + 1), Case("one byte beyond ISIZE", ok, isize=len(ok.payload) - 1),
                    Case("one byte beyond ISIZE, stored", forge([Stored(bytes(lit))]), isize=len(lit) - 1),
                    Case("one byte short of ISIZE, fixed", forge([Fixed(lit)]), isize=len(lit) + 1)]
    assert set(out) == set(MALFORMED_CLASSES)
    return out


# ---- files -------------------------------------------------------------------------------------------------------------------------

def zmember(rng) -> tuple:
    pay = text(rng, int(rng.integers(0, 3000)))
    c = zlib.compressobj(int(rng.integers(0, 10)), zlib.DEFLATED, -15)
    return bgzf_member(c.compress(pay) + c.flush(), pay), pay


class File:
    """raw: the bytes of a BGZF file; payloads: per member what it inflates to; forged: {member index: Case}"""
    def __init__(self, raw, payloads, forged):
        self.raw, self.payloads, self.forged = raw, payloads, forged


def build_file(cases, seed=0, neighbours=True) -> File:
    """the cases as BGZF members between ordinary zlib members (a write past a member's edge lands in a neighbour's bytes), other
    gzip subfields in front of and behind BC so that XLEN -- and with it the payload's misalignment -- takes every value; a case
    that was built for one misalignment (Case.mis) gets it"""
    rng = np.random.default_rng(5000 + seed)
    parts, pays, forged, pos = [], [], {}, 0

    def add(m, p):
        nonlocal pos
        parts.append(m); pays.append(p); pos += len(m)

    if neighbours:
        add(*zmember(rng))
    for k, c in enumerate(cases):
        if c.mis is not None:
            if (pos + 18) % 8 == c.mis:
                front, behind = b"", b""
            else:
                n = (c.mis - (pos + 22)) % 8
                front, behind = (subfield(n), b"") if k % 2 else (b"", subfield(n))
        else:
            front, behind = [(b"", b""), (b"", subfield(k % 8)), (subfield(k % 5), b""), (subfield(1), subfield(k % 7, b"AB"))][k % 4]
        if len(c.data) + len(front) + len(behind) > MAX_DEFLATE:
            front, behind = b"", b""
            assert c.mis is None
        m = bgzf_member(c.data, c.payload, extra=behind, extra_front=front, isize=c.isize)
        c.mis_in_file = (pos + 12 + 6 + len(front) + len(behind)) % 8
        assert c.mis is None or c.mis_in_file == c.mis
        forged[len(parts)] = c
        add(m, c.payload)
        if neighbours and k % 3 != 1:
            add(*zmember(rng))
    if neighbours:
        add(*zmember(rng))
    return File(b"".join(parts) + BGZF_EOF, pays + [b""], forged)


@functools.lru_cache(maxsize=None)
def legal_cases(name):
    return LEGAL[name]()


@functools.lru_cache(maxsize=None)
def malformed_cases():
    return malformed()
