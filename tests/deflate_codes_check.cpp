// deflate_codes_check.cpp -- gci_amd/csrc/gci_deflate_codes.hpp, the code set both GPU inflaters are built on, compiled for the host
// and held against zlib: the functions below are the very ones in libgci_hip.so (the header is all this file includes of the
// project).  tests/test_deflate_codes_host.py builds and runs it:
//   g++ -O2 -std=c++17 -o check tests/deflate_codes_check.cpp -lz && ./check file.bgzf [accept | refuse]
// accept (default): every member of the BGZF file, decoded serially with build_code + build_table + the search over the limits,
//   equals zlib's output byte for byte and has the trailer's CRC-32 and ISIZE; for every fixed or dynamic block on the way
//   * the tables filled entry by entry (table_entry) equal build_table's at the widths the kernels use: 8 and 5 (lane decoder), 9 and
//     8 (wave decoder), 7 (the code-length code);
//   * entry_of_value(c) names the same symbol and length as the search on the bit-reversed c for every 15-bit code value c behind
//     the shortest primary table of the alphabet -- the wave decoder's tail tables rest on that --, and the search that skips the
//     lengths of a primary table finds what the full one finds;
// refuse: every member is refused BY build_code under the policy the kernels pass (CODE_COMPLETE for the code-length code, CODE_ONE
//   for the two alphabets of a dynamic block), and by zlib.
// TEST CODE, not the library's: the gzip / BGZF framing, the bit reader, the parse of a block's header (type, stored lengths, HLIT /
// HDIST / HCLEN, the run-length symbols 16 - 18), the RFC 1951 3.2.5 base tables and the copy loop.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <vector>

#include "../gci_amd/csrc/gci_deflate_codes.hpp"

using namespace deflate_codes;

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } while (0)

enum { M_OK = 0, M_CODE_REFUSED = 1, M_BAD = 2 };

static const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
                                       12289, 16385, 24577};
static const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

static long n_blocks = 0, n_values = 0;

// the stream's bits from bit `pos` on, first bit lowest (the buffer is readable 8 bytes past the payload)
struct Bits {
    const uint8_t* base; size_t nbits, pos;
    uint32_t peek() const { uint64_t v; memcpy(&v, base + (pos >> 3), 8); return (uint32_t)(v >> (pos & 7)); }
    uint32_t take(int n) { const uint32_t v = peek() & ((1u << n) - 1u); pos += (size_t)n; return v; }
};

// one symbol as the lane decoder reads it: the primary table of BITS bits (BITS > 0), else the limits of the lengths BITS + 1 .. MAXL
template <int BITS, int MAXL>
static int decode(Bits& B, const uint16_t* table, const Canon& cn, const uint16_t* sorted)
{
    const uint32_t bits = B.peek();
    if (BITS) {
        const uint32_t e = table[bits & ((1u << BITS) - 1u)];
        if (e) { B.pos += entry_len(e); return (int)entry_sym(e); }
    }
    uint32_t c;
    const int l = code_length<BITS, MAXL>(bits, cn, c);
    if (l > MAXL) return -1;
    B.pos += (size_t)l;
    return (int)sorted[code_index(c, l, cn)];
}

template <int BITS>
static void check_table(const Canon& cn, const uint16_t* sorted)
{
    uint16_t a[1 << BITS], b[1 << BITS];
    build_table<BITS>(cn, sorted, a);
    for (uint32_t k = 0; k < (1u << BITS); k++) b[k] = table_entry(k, BITS, cn, sorted);
    if (memcmp(a, b, sizeof a)) FAIL("the %d-bit table filled entry by entry differs from build_table's", BITS);
}

// every 15-bit code value from limit[SKIP] on: the entry form, the full search and the search that skips SKIP lengths agree
template <int SKIP>
static void check_values(const Canon& cn, const uint16_t* sorted)
{
    for (uint32_t c = cn.limit[SKIP]; c < cn.limit[15]; c++, n_values++) {
        const uint32_t bits = brev32(c) >> 17;                           // (the 15 bits reversed: the stream's order)
        const uint32_t e = entry_of_value(c, cn, sorted);
        int l = 0;
        const int s = code_search(bits, cn, sorted, l);
        if (s < 0 || e == 0u || (uint32_t)s != entry_sym(e) || (uint32_t)l != entry_len(e)) FAIL("entry_of_value(%u) differs from the search", c);
        uint32_t c2;
        if (code_length<SKIP, 15>(bits, cn, c2) != l || c2 != c) FAIL("the search behind a %d-bit table differs from the full one at %u", SKIP, c);
    }
    if (cn.limit[15] < (1u << 15) && entry_of_value(cn.limit[15], cn, sorted) != 0u) FAIL("entry_of_value finds a code where there is none");
}

// -> M_*; out: the member's bytes
static int member(const uint8_t* base, size_t nbits, uint32_t isize, std::vector<uint8_t>& out)
{
    static uint8_t lens[352];                                            // [0, 19): the code-length code; [32, ..): both alphabets
    static uint16_t lit_sorted[288], dist_sorted[32], lit_tab[1 << 8], dist_tab[1 << 5];
    static Canon lit_cn, dist_cn;
    Bits B{base, nbits, 0};
    out.clear();
    out.reserve(isize);
    for (bool last = false; !last;) {
        if (B.pos + 3 > nbits) return M_BAD;
        last = B.take(1) != 0;
        const uint32_t type = B.take(2);
        if (type == 3) return M_BAD;
        if (type == 0) {
            B.pos = (B.pos + 7) & ~(size_t)7;
            if (B.pos + 32 > nbits) return M_BAD;
            const uint32_t len = B.take(16), nlen = B.take(16);
            if ((len ^ 0xFFFFu) != nlen || B.pos + 8 * (size_t)len > nbits || out.size() + len > isize) return M_BAD;
            out.insert(out.end(), base + (B.pos >> 3), base + (B.pos >> 3) + len);
            B.pos += 8 * (size_t)len;
            continue;
        }
        uint8_t* ll = lens + 32;
        int hlit = 288, hdist = 30;
        const int policy = type == 1 ? CODE_ANY : CODE_ONE;
        if (type == 1) {
            for (int i = 0; i < 288; i++) ll[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
            for (int i = 0; i < 30; i++) ll[288 + i] = 5;
        } else {
            hlit = (int)B.take(5) + 257; hdist = (int)B.take(5) + 1;
            const int hclen = (int)B.take(4) + 4;
            if (hlit > 286 || hdist > 30) return M_BAD;
            memset(lens, 0, 19);
            for (int i = 0; i < hclen; i++) lens[c_clen_order[i]] = (uint8_t)B.take(3);
            const bool ok = build_code(lens, 19, dist_cn, dist_sorted, CODE_COMPLETE);
            if (!ok) return M_CODE_REFUSED;
            check_table<7>(dist_cn, dist_sorted);
            int n = 0, prev = 0;
            while (n < hlit + hdist) {
                if (B.pos > nbits) return M_BAD;
                const int sym = decode<0, 7>(B, nullptr, dist_cn, dist_sorted);
                if (sym < 0) return M_BAD;
                int rep = 1, val = sym;
                if (sym == 16) { if (n == 0) return M_BAD; val = prev; rep = 3 + (int)B.take(2); }
                else if (sym == 17) { val = 0; rep = 3 + (int)B.take(3); }
                else if (sym == 18) { val = 0; rep = 11 + (int)B.take(7); }
                if (n + rep > hlit + hdist) return M_BAD;
                for (int i = 0; i < rep; i++) ll[n + i] = (uint8_t)val;
                n += rep; prev = val;
            }
            if (ll[256] == 0) return M_BAD;
        }
        const bool ok_l = build_code(ll, hlit, lit_cn, lit_sorted, policy);
        const bool ok_d = build_code(ll + hlit, hdist, dist_cn, dist_sorted, policy);
        if (!ok_l || !ok_d) return M_CODE_REFUSED;
        n_blocks++;
        build_table<8>(lit_cn, lit_sorted, lit_tab);
        build_table<5>(dist_cn, dist_sorted, dist_tab);
        check_table<8>(lit_cn, lit_sorted); check_table<9>(lit_cn, lit_sorted);
        check_table<5>(dist_cn, dist_sorted); check_table<8>(dist_cn, dist_sorted);
        check_values<8>(lit_cn, lit_sorted);
        check_values<5>(dist_cn, dist_sorted);
        for (;;) {
            if (B.pos > nbits) return M_BAD;
            const int sym = decode<8, 15>(B, lit_tab, lit_cn, lit_sorted);
            if (sym < 0 || sym > 285) return M_BAD;
            if (sym < 256) { if (out.size() >= isize) return M_BAD; out.push_back((uint8_t)sym); continue; }
            if (sym == 256) break;
            const uint32_t len = LEN_BASE[sym - 257] + B.take(LEN_EXTRA[sym - 257]);
            const int ds = decode<5, 15>(B, dist_tab, dist_cn, dist_sorted);
            if (ds < 0 || ds > 29) return M_BAD;
            const uint32_t dist = DIST_BASE[ds] + B.take(DIST_EXTRA[ds]);
            if (dist > out.size() || out.size() + len > isize) return M_BAD;
            for (uint32_t i = 0; i < len; i++) { const uint8_t b = out[out.size() - dist]; out.push_back(b); }
        }
    }
    if (B.pos > nbits || out.size() != isize) return M_BAD;
    return M_OK;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s file.bgzf [accept | refuse]\n", argv[0]); return 2; }
    const bool refuse = argc > 2 && !strcmp(argv[2], "refuse");
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> raw((size_t)n + 64, 0);
    if (fread(raw.data(), 1, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    long members = 0;
    std::vector<uint8_t> got, want;
    for (size_t pos = 0; pos < (size_t)n; members++) {
        const uint8_t* h = raw.data() + pos;
        if (pos + 26 > (size_t)n || h[0] != 0x1F || h[1] != 0x8B || h[2] != 8 || !(h[3] & 4)) FAIL("not a BGZF member at %zu", pos);
        const uint32_t xlen = h[10] | (h[11] << 8);
        uint32_t bsize = 0;
        for (uint32_t x = 0; x + 4 <= xlen;) {                           // the BC subfield among the extra subfields
            const uint8_t* s = h + 12 + x;
            const uint32_t sl = s[2] | (s[3] << 8);
            if (s[0] == 'B' && s[1] == 'C' && sl == 2) bsize = (s[4] | (s[5] << 8)) + 1u;
            x += 4 + sl;
        }
        if (bsize < 12 + xlen + 8 || pos + bsize > (size_t)n) FAIL("member %ld: no BSIZE", members);
        const uint8_t* base = h + 12 + xlen;
        const uint32_t pay = bsize - 12 - xlen - 8;
        uint32_t crc, isize;
        memcpy(&crc, h + bsize - 8, 4);
        memcpy(&isize, h + bsize - 4, 4);
        if (isize > 65536u) FAIL("member %ld: ISIZE %u", members, isize);
        want.assign((size_t)isize + 8, 0);
        z_stream z;
        memset(&z, 0, sizeof z);
        inflateInit2(&z, -15);
        z.next_in = (Bytef*)base; z.avail_in = pay; z.next_out = want.data(); z.avail_out = isize + 8;
        const int zr = inflate(&z, Z_FINISH);
        const bool z_ok = zr == Z_STREAM_END && z.total_out == isize;
        inflateEnd(&z);
        const int st = member(base, 8 * (size_t)pay, isize, got);
        if (refuse) {
            if (z_ok) FAIL("member %ld: zlib accepts it", members);
            if (st != M_CODE_REFUSED) FAIL("member %ld: not refused by build_code (status %d)", members, st);
        } else {
            if (!z_ok) FAIL("member %ld: zlib refuses it", members);
            if (st != M_OK) FAIL("member %ld: not decoded (status %d)", members, st);
            if (memcmp(got.data(), want.data(), isize)) FAIL("member %ld DIFFERS from zlib", members);
            if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), got.data(), isize) != crc) FAIL("member %ld: CRC-32 differs from the trailer's", members);
        }
        pos += bsize;
    }
    printf("%ld members %s, %ld blocks with their tables, %ld code values\n", members, refuse ? "refused by build_code and by zlib" : "equal to zlib byte for byte",
           n_blocks, n_values);
    return 0;
}
