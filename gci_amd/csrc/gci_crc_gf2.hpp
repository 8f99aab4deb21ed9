// gci_crc_gf2.hpp -- CRC-32 of text that is never written, shared by the depth writer (k_deflate.hip) and the compressed-domain
// depth reader (k_depth_gz.hip): CRCs are polynomials mod P over GF(2), crc(A||B) = crc(A) * x^(8|B|) + crc(B), so n copies of a
// line behind a string are a few products with table entries.  One table per context (gci_ctx::deflate_tab), made by whichever
// side needs it first (ensure_crc_tab).
#pragma once
#include <stdio.h>

#include "gci_ctx.hpp"

constexpr uint32_t CRC_POLY = 0xEDB88320u;      // reflected: bit 31 holds x^0, bit 0 holds x^31
constexpr uint32_t GF_ONE = 0x80000000u;        // the polynomial 1

__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b)          // a * b mod P
{
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 0; i < 32; i++) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;                               // + b * x^i
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);                            // b *= x
    }
    return p;
}

// The same product with the multiplier shifted out at its top bit, which the compiler unrolls in full: the CRC check of the inflate
// (k_inflate.hip: up to 17 products per lane and member in k_bgzf_crc, 16 per thread in k_crc_tables).  Measured there, gf_mul's form
// cost 0.1 ms of a 7.6 ms call; the depth writer's size pass is bound by gf_mul as it stands and keeps it.
__device__ __forceinline__ uint32_t gf_mul_shift(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 0; i < 32; i++) {
        r ^= (a & 0x80000000u) ? b : 0u;
        a <<= 1;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return r;
}

// (crc, x^(8 len)) of a byte string; strings concatenate as  (a.c, a.x) . (b.c, b.x) = (a.c * b.x + b.c, a.x * b.x)
struct CrcPair { uint32_t c, x; };
__device__ __forceinline__ CrcPair crc_cat(CrcPair a, CrcPair b) { return {gf_mul(a.c, b.x) ^ b.c, gf_mul(a.x, b.x)}; }

// one line of the text: decimal digits of v (v >= 0) and '\n', as bytes packed little-endian into 96 bits
struct Line { uint32_t lo, mid, hi; uint32_t w; };
__device__ __forceinline__ uint32_t line_byte(const Line& l, uint32_t k)
{
    const uint32_t word = k < 4 ? l.lo : k < 8 ? l.mid : l.hi;
    return (word >> (8u * (k & 3u))) & 0xFFu;
}
__device__ __forceinline__ Line make_line(uint32_t v)
{
    uint32_t nd = 1;
    for (uint32_t t = v; t >= 10u; t /= 10u) nd++;
    Line l{0u, 0u, 0u, nd + 1u};
    uint32_t t = v;
    for (uint32_t k = nd; k-- > 0;) {                                           // digit k (0 = most significant)
        const uint32_t dg = 0x30u + t % 10u;
        t /= 10u;
        const uint32_t sh = 8u * (k & 3u);
        if (k < 4) l.lo |= dg << sh; else if (k < 8) l.mid |= dg << sh; else l.hi |= dg << sh;
    }
    const uint32_t sh = 8u * (nd & 3u);
    if (nd < 4) l.lo |= 0x0Au << sh; else if (nd < 8) l.mid |= 0x0Au << sh; else l.hi |= 0x0Au << sh;
    return l;
}

__device__ __forceinline__ CrcPair crc_line(const Line& l)
{
    uint32_t c = 0xFFFFFFFFu, x = GF_ONE;
    for (uint32_t k = 0; k < l.w; k++) {
        c ^= line_byte(l, k);
        for (int b = 0; b < 8; b++) {
            c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
            x = (x >> 1) ^ ((x & 1u) ? CRC_POLY : 0u);                          // x^(8 w) alongside
        }
    }
    // c is the register of the string started at all-ones; the finalised CRC of a string S is reg(S) ^ ~0, and the
    // concatenation rule above holds for finalised CRCs
    return {c ^ 0xFFFFFFFFu, x};
}

// n >= 1 copies of a line of w bytes behind a string.  With X = x^(8 w) the CRC of n copies behind a string of CRC c is
// c * X^n + line_crc * G_n, G_n = 1 + X + ... + X^(n - 1) -- X^n and G_n depend on w and n only, and G_(a + b) = G_a * X^b + G_b.
// Round 3 put them together from a table of (X^(2^k), G_(2^k)) per line width: two products per set bit of n, three to apply
// them and one more for the string's own x^(8 len) -- ~16 products of 32 shift-and-add steps per run, and the size pass of
// the members (5.3 ms at genome scale, `profiles/r03t_bench_kernel_stats.csv`) was bound by exactly this arithmetic.  Round 5:
// n <= 4096 is two digits to the base 64, the table (made by the host when a context first needs it: 12.5 KB) holds
// (X^(j 64^k), G_(j 64^k)) for j <= 64, so X^n and G_n are ONE product each; the CRC of a line below 1024 is a table entry
// too; and the tile's x^(8 len) is made once, from the bits of its text length, behind the last run: four products per run.
constexpr uint32_t gf_mul_c(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}
constexpr int REP_W = 12;                                                       // line widths 0 .. 11
constexpr int REP_J = 65;                                                       // digits 0 .. 64 (n = 4096 = 64 * 64)
constexpr int LINE_TAB = 1024;                                                  // CRCs of the lines "0\n" .. "1023\n"
constexpr int POW_K = 17;                                                       // x^(8 2^k): a tile's text is < 2^17 bytes
static_assert(TILE <= 64 * 64, "a run is at most two digits to the base 64");
static_assert((uint64_t)TILE * (REP_W - 1) < (1ull << POW_K), "the text of a tile");
// layout of the table (uint32): [REP_W][2][REP_J] pairs (x, g) | LINE_TAB line CRCs | POW_K powers
constexpr size_t TAB_REP = 0, TAB_LINE = (size_t)REP_W * 2 * REP_J * 2, TAB_POW = TAB_LINE + LINE_TAB, TAB_WORDS = TAB_POW + POW_K;

struct CrcTab {
    const uint2* __restrict__ rep;
    const uint32_t* __restrict__ line;
    const uint32_t* __restrict__ pow8;
};

__device__ __forceinline__ uint32_t crc_append_lines(uint32_t front_c, uint32_t line_crc, uint32_t w, uint32_t n, const CrcTab& t)
{
    const uint2 lo = t.rep[(w * 2u + 0u) * REP_J + (n & 63u)], hi = t.rep[(w * 2u + 1u) * REP_J + (n >> 6)];
    const uint32_t xn = gf_mul(hi.x, lo.x);                                     // X^(64 a + b)
    const uint32_t gn = gf_mul(hi.y, lo.x) ^ lo.y;                              // G_(64 a) * X^b + G_b
    return gf_mul(front_c, xn) ^ gf_mul(line_crc, gn);
}

__device__ __forceinline__ uint32_t pow_x8(uint32_t len, const CrcTab& t)       // x^(8 len)
{
    uint32_t x = GF_ONE;
    for (uint32_t k = 0; len; len >>= 1, k++)
        if (len & 1u) x = gf_mul(x, t.pow8[k]);
    return x;
}

// The CRC tables (layout above), made once per process on the host and copied into the context when either side first needs them.
inline const uint32_t* host_crc_tab()
{
    static uint32_t tab[TAB_WORDS];
    static const bool made = [] {
        uint32_t xw = GF_ONE;                                                   // x^(8 w)
        for (int w = 0; w < REP_W; w++) {
            uint32_t base_x = xw, base_g = GF_ONE;                              // (X^m, G_m), m = 64^k
            for (int k = 0; k < 2; k++) {
                uint32_t x = GF_ONE, g = 0u;                                    // (X^(j m), G_(j m)), j = 0
                for (int j = 0; j < REP_J; j++) {
                    uint32_t* e = tab + TAB_REP + 2 * (((size_t)w * 2 + k) * REP_J + j);
                    e[0] = x; e[1] = g;
                    g = gf_mul_c(g, base_x) ^ base_g;                           // G_(a + m) = G_a X^m + G_m
                    x = gf_mul_c(x, base_x);
                }
                // m -> 64 m: entry j = 64 of this digit
                const uint32_t* e64 = tab + TAB_REP + 2 * (((size_t)w * 2 + k) * REP_J + 64);
                base_x = e64[0]; base_g = e64[1];
            }
            xw = gf_mul_c(xw, 0x00800000u);                                     // * x^8
        }
        for (uint32_t v = 0; v < (uint32_t)LINE_TAB; v++) {
            char txt[16];
            const int nc = snprintf(txt, sizeof txt, "%u\n", v);
            uint32_t c = 0xFFFFFFFFu;
            for (int i = 0; i < nc; i++) {
                c ^= (uint8_t)txt[i];
                for (int b = 0; b < 8; b++) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
            }
            tab[TAB_LINE + v] = c ^ 0xFFFFFFFFu;
        }
        uint32_t x = 0x00800000u;                                               // x^8
        for (int k = 0; k < POW_K; k++) { tab[TAB_POW + k] = x; x = gf_mul_c(x, x); }
        return true;
    }();
    (void)made;
    return tab;
}

inline int ensure_crc_tab(gci_ctx* ctx)
{
    if (ctx->deflate_tab_ready) return GCI_OK;
    GCI_TRY(gci_ensure(ctx, ctx->deflate_tab, TAB_WORDS * sizeof(uint32_t)));
    if (hipMemcpyAsync(ctx->deflate_tab.p, host_crc_tab(), TAB_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return GCI_E_HIP;
    ctx->deflate_tab_ready = true;
    return GCI_OK;
}

