"""The reference side of the forged-stream tests (deflate_forge.py, forge_cases.py), with no GPU: every legal stream that
test_gpu_inflate_forged.py puts through the GPU inflaters is inflated by zlib here -- no error, end of stream reached, output equal
to the payload the forge says the tokens expand to --, every malformed one is refused by zlib, and every claim about where a symbol
lies in the wave decoder's pieces, grains and chunks is proven from the forge's bit ledger.  A bug in the forge shows up here, never
as a surprise on the GPU.

Measured: the whole module, building every class included, takes 36 s on one core of the development machine (most of it the
random LZ77 parses of the 2 136 randomised members; 36 of them are full-size, the rest at most 4 KB).
"""
import os
import re
import zlib

import numpy as np
import pytest

import forge_cases as fc
from deflate_forge import Fixed, bgzf_member, complete_lengths, forge, parse, subfield, zlib_verdict
from gci_amd import hostio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_geometry_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "gci_amd", "csrc", "k_inflate_wave.hip")).read()
    assert int(re.search(r"#define IW_PIECE_LOG2 (\d+)", src).group(1)) == fc.PIECE.bit_length() - 1
    assert int(re.search(r"#define IW_GRAIN_LOG2 (\d+)", src).group(1)) == fc.GRAIN.bit_length() - 1
    m = re.search(r"LIT_TAIL = (\d+), DIST_TAIL = (\d+)", src)
    assert (int(m.group(1)), int(m.group(2))) == (fc.LIT_TAIL, fc.DIST_TAIL)
    assert "MAXS = PIECE < 512u ? 256u : PIECE / 2u" in src and fc.MAXS == fc.PIECE // 2
    assert "CHUNK_U = 64u * PU" in src and fc.CHUNK == 64 * fc.PIECE


@pytest.mark.parametrize("name", sorted(fc.LEGAL))
def test_zlib_inflates_every_legal_stream_to_its_payload(name):
    cases = fc.legal_cases(name)
    assert cases
    for c in cases:
        ok, out = zlib_verdict(c.data, c.isize)
        assert ok, (name, c.name)
        assert out == c.payload, (name, c.name)
        assert len(c.payload) <= 65536 and len(c.data) <= fc.MAX_DEFLATE, (name, c.name)


def test_zlib_refuses_every_malformed_stream():
    classes = fc.malformed_cases()
    assert len(classes) >= 11
    for name, cases in classes.items():
        for c in cases:
            ok, _ = zlib_verdict(c.data, c.isize)
            assert not ok, (name, c.name)
    # ... and for the right reason where the reason is the header: zlib's message names it
    def message(c):
        try:
            zlib.decompressobj(-15).decompress(c.data)
        except zlib.error as e:
            return str(e)
        return ""
    by = {c.name: message(c) for cs in classes.values() for c in cs}
    assert "invalid literal/lengths set" in by["lit set incomplete"] and "invalid distances set" in by["dist set incomplete"]
    assert "invalid code lengths set" in by["cl set incomplete"] and "invalid code lengths set" in by["cl set over-subscribed"]
    assert "invalid distances set" in by["one distance code of 2 bits"] and "invalid literal/lengths set" in by["256 alone at 2 bits"]
    assert "invalid distances set" in by["distance codes nobody uses, incomplete"]
    assert "missing end-of-block" in by["no code for 256"] and "missing end-of-block" in by["hclen 4"]
    assert "invalid bit length repeat" in by["16 first"] and "invalid bit length repeat" in by["18 past the end"]
    assert "too many length or distance symbols" in by["hlit 287"] and "too many length or distance symbols" in by["hdist 31"]
    assert "invalid distance too far back" in by["one byte too far"] and "invalid block type" in by["first block"]
    assert "invalid stored block lengths" in by["len / nlen"]
    assert "invalid literal/length code" in by["lit/len 286"] and "invalid distance code" in by["distance 30"]


# ---- the claims of the geometric classes, from the ledger -----------------------------------------------------------------------

def test_end_of_block_codes_lie_where_the_cases_say():
    seen = set()
    for c in fc.legal_cases("eob_positions"):
        led = c.ledger[0]
        if hasattr(c, "body_bits"):
            assert led["end"] - led["body"] == c.body_bits
            seen.add(("body", c.body_bits - fc.CHUNK, led["kind"]))
            continue
        block, what, rel = c.geo
        assert what == "eob" and fc.chunk_rel(c, block, led["eob"]) == rel
        L = led["end"] - led["eob"]
        assert L == c.eob_len and L >= 2
        if c.how == "ends":
            assert (rel + L) % c.unit == 0 and rel // c.unit == (rel + L - 1) // c.unit          # its last bit is the unit's last
        elif c.how == "begins":
            assert rel % c.unit == 0
        elif c.how == "straddles":
            assert rel // c.unit + 1 == (rel + L - 1) // c.unit
        else:
            assert rel + L <= fc.PIECE                                                              # lane 0's piece: the lanes behind are void
        seen.add((c.how, c.unit, led["kind"]))
    for kind in ("fixed", "dynamic"):
        for how, unit in (("ends", fc.PIECE), ("ends", fc.GRAIN), ("ends", fc.CHUNK), ("begins", fc.PIECE), ("begins", fc.GRAIN),
                          ("begins", fc.CHUNK), ("straddles", fc.PIECE), ("straddles", fc.CHUNK), ("ends the block in", fc.PIECE)):
            assert (how, unit, kind) in seen
        assert {("body", d, kind) for d in (-1, 0, 1)} <= seen
    assert {c.mis for c in fc.legal_cases("eob_positions")} == set(range(8))


def test_the_48_bit_symbols_begin_in_the_last_grain_of_a_chunk():
    backs = set()
    for c in fc.legal_cases("max_symbol_last_grain"):
        block, i, rel = c.geo
        led = c.ledger[block]
        assert fc.chunk_rel(c, block, led["syms"][i]) == rel
        assert led["syms"][i + 1] - led["syms"][i] == 48
        assert fc.CHUNK - fc.GRAIN <= rel < fc.CHUNK
        backs.add(fc.CHUNK - rel)
    assert backs == {64, 48, 17, 1}


def test_dynamic_headers_begin_at_every_bit_of_a_unit():
    got = set()
    for c in fc.legal_cases("header_offsets"):
        led = c.ledger[1]
        assert led["kind"] == "dynamic" and (8 * c.mis + led["header"]) % 64 == c.header_bit
        got.add(c.header_bit)
    assert got == set(range(64))


def test_the_longest_header_is_the_longest():
    for c in fc.legal_cases("longest_header"):
        led = c.ledger[-1]
        assert led["body"] - led["header"] == fc.LONGEST_HEADER == 2286 and (led["hlit"], led["hdist"], led["hclen"]) == (286, 30, 19)
    led = [c for c in fc.legal_cases("header_extremes") if c.name == "hlit 257"][0].ledger[0]
    assert led["hlit"] == 257 and led["hdist"] == 1
    for c in fc.legal_cases("header_extremes"):
        if c.name.startswith("hlit 286"):
            assert c.ledger[0]["hlit"] == 286
        if c.name.startswith("hclen 19"):
            assert c.ledger[0]["hclen"] == 19


def test_short_symbols_overflow_a_lane_list():
    for c in fc.legal_cases("short_symbols"):
        led = c.ledger[0]
        pos = np.array(led["syms"])
        per_piece = np.bincount((pos - led["body"]) // fc.PIECE)
        assert per_piece[:-1].min() > fc.MAXS * 0.6 and per_piece.max() > fc.MAXS * 0.6          # ... and a lane runs on into the next piece: > MAXS
        two = np.bincount((pos - led["body"]) // (2 * fc.PIECE))
        assert two[:-1].min() > fc.MAXS


def test_the_model_confirms_false_end_of_block_codes_and_lanes_out_of_step():
    cases = fc.legal_cases("false_eobs")
    assert len(cases) == 4
    for c in cases:
        assert c.false_eobs > 4 and 1 <= c.lane < 64
    for c in fc.legal_cases("never_in_step"):
        led = c.ledger[0]
        bits = fc._bit_string(c.data)
        true = set(led["syms"]) | {led["eob"]}
        origin = 64 * ((8 * c.mis + led["body"]) // 64) - 8 * c.mis
        assert (led["body"] - origin) % 8 != 0                        # the pieces begin off the byte grid of the symbols
        false_eobs = 0
        for lane in range(1, 64):
            path = fc._decode_from(bits, origin + lane * fc.PIECE, origin + (lane + 2) * fc.PIECE, c.codes)
            assert not any(p in true for p, _ in path), "lane %d falls into step" % lane
            false_eobs += sum(s == 256 for _, s in path)
        assert led["eob"] - origin > fc.CHUNK and false_eobs > 0


def test_copy_chains_are_deep():
    for c in fc.legal_cases("deep_chains"):
        assert max(fc.copy_depth(c.tokens)) >= 16, c.name
    sizes = {len(c.payload) for c in fc.legal_cases("runs")} | {len(c.payload) for c in fc.legal_cases("long_matches")}
    assert {65535, 65536} <= sizes


def test_tail_overflow_shapes_overflow_the_tail_tables():
    def span(lens, bits):                                         # 15-bit code values of the codes longer than `bits`
        return sum(1 << (15 - l) for l in lens if l > bits)
    for c in fc.legal_cases("lit_tail_overflow"):
        assert span(c.f.blocks[0].lit_lens, 9) > fc.LIT_TAIL
    n = 0
    for c in fc.legal_cases("dist_shapes"):
        if "tail" in c.name:
            assert span(c.f.blocks[0].dist_lens, 8) > fc.DIST_TAIL
            n += 1
        else:
            assert sorted(c.f.blocks[0].dist_lens)[-2:] == [15, 15] and len([l for l in c.f.blocks[0].dist_lens if l]) == 30
    assert n == 3
    for c in fc.legal_cases("long_used_codes"):
        used = {t for t in c.f.blocks[0].tokens if isinstance(t, int)} | {256}
        assert min(c.f.blocks[0].lit_lens[s] for s in used) > 9


# ---- the forge's helpers ---------------------------------------------------------------------------------------------------------

def test_complete_lengths_are_complete():
    rng = np.random.default_rng(3)
    longest = 0
    for n in (2, 3, 19, 30, 257, 286):
        for max_len in (7, 15):
            if n > (1 << max_len) or (max_len == 7 and n > 19):
                continue
            for _ in range(20):
                ls = complete_lengths(rng, n, max_len)
                assert len(ls) == n and min(ls) >= 1 and max(ls) <= max_len and sum(2.0 ** -l for l in ls) == 1.0
                longest = max(longest, max(ls))
    assert longest == 15


def test_parse_is_a_legal_parse_with_far_and_overlapping_matches():
    rng = np.random.default_rng(4)
    pay = (fc.text(np.random.default_rng(65536), 20000) * 4)[:65536]
    toks = parse(rng, pay)
    f = forge([Fixed(toks)])
    assert f.payload == pay
    matches = [t for t in toks if not isinstance(t, int)]
    assert any(t[1] < t[0] for t in matches) and max(t[1] for t in matches) > 16384 and max(t[0] for t in matches) == 258
    # a match as a block's first symbol that reaches into the block in front of it
    first = [b.tokens[0] for c in fc.legal_cases("block_orders") for b, led in zip(c.f.blocks, c.ledger) if led["kind"] != "stored" and b.tokens]
    assert any(not isinstance(t, int) for t in first)


def test_bgzf_member_with_other_subfields_is_found_by_the_host_scan():
    """XLEN varies: subfields in front of and behind BC (the BGZF specification allows them); hostio.bgzf_blocks finds every member,
    and every payload misalignment 0 .. 7 occurs"""
    cases = fc.legal_cases("header_offsets")
    f = fc.build_file(cases)
    buf = np.frombuffer(f.raw, dtype=np.uint8)
    pos, isz = hostio.bgzf_blocks(buf)
    assert len(isz) == len(f.payloads) and [int(x) for x in isz] == [len(p) for p in f.payloads]
    assert hostio.bgzf_inflate(buf, check_crc=True).tobytes() == b"".join(f.payloads)
    assert {c.mis_in_file for c in cases} == set(range(8))
    xlens = {int(buf[int(p) + 10]) | int(buf[int(p) + 11]) << 8 for p in pos[:-1]}
    assert len(xlens) >= 8
    for pays in ([b"", b"x" * 10], ):
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        m = bgzf_member(z.compress(pays[1]) + z.flush(), pays[1], extra=subfield(3), extra_front=subfield(2, b"AA"))
        p, i = hostio.bgzf_blocks(np.frombuffer(m + fc.BGZF_EOF, dtype=np.uint8))
        assert [int(x) for x in i] == [10, 0]


def test_the_host_inflate_gives_the_same_verdicts():
    """the project's host path (host_io.cpp through zlib) on the files the GPU tests use: legal files inflate, a malformed member
    fails the call"""
    from gci_amd._lib import GciError
    f = fc.build_file(fc.legal_cases("few_dist_codes") + fc.legal_cases("trailing_bytes"))
    assert hostio.bgzf_inflate(np.frombuffer(f.raw, dtype=np.uint8), check_crc=True).tobytes() == b"".join(f.payloads)
    for name, cases in fc.malformed_cases().items():
        for c in cases:
            g = fc.build_file([c])
            with pytest.raises(GciError):
                hostio.bgzf_inflate(np.frombuffer(g.raw, dtype=np.uint8), check_crc=False)
