// gci_deflate_codes.hpp -- the Huffman code set of DEFLATE (RFC 1951), once: what the lane-per-member decoder (k_inflate.hip) and the
// wave-per-member decoder (k_inflate_wave.hip) both know of a block's codes, and nothing of LDS layouts, waves or bit readers.
// It also compiles with a plain host compiler: tests/deflate_codes_check.cpp holds these very functions against zlib without a GPU.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GCI_DC_FN __device__ __forceinline__
#define GCI_DC_CONST static __constant__            // (internal linkage: two translation units include this header)
#else
#define GCI_DC_FN static inline
#define GCI_DC_CONST static const
#endif

namespace deflate_codes {

// the order in which a dynamic block's header sends the lengths of the code-length code (3.2.7)
GCI_DC_CONST uint8_t c_clen_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Canonical Huffman code of one alphabet (RFC 1951 3.2.2), without a loop over the code lengths: with c = the next 15 bits
// read as a code (first bit highest), the codes of length l are exactly limit[l-1] <= c < limit[l], limit[l] = (first code
// of length l + their number) << (15 - l) -- non-decreasing in l -- so the length is 1 + the number of limits <= c (16: no
// such code), and the symbol is sorted[off[l] + (c >> (15 - l))], off[l] = index of the first symbol of length l in
// `sorted` - its code.  next[l]: one past the last symbol of length l in `sorted`.
// An alphabet may also have a primary table indexed by the next BITS bits of the stream (codes are packed from their most
// significant bit, i.e. bit reversed in the LSB-first bit buffer): entry = symbol | length << 9, 0 = the code is longer (or
// unused).  (Distance symbol 0 with a code of l bits is the entry l << 9: never 0.)
struct alignas(16) Canon { uint16_t limit[16]; int16_t off[16]; uint16_t next[16]; };

GCI_DC_FN uint32_t make_entry(uint32_t sym, uint32_t len) { return sym | (len << 9); }
GCI_DC_FN uint32_t entry_len(uint32_t e) { return e >> 9; }
GCI_DC_FN uint32_t entry_sym(uint32_t e) { return e & 0x1FFu; }

GCI_DC_FN uint32_t brev32(uint32_t v)
{
#if defined(__HIPCC__)
    return __brev(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    return (v >> 16) | (v << 16);
#endif
}
// the next bits of the stream (first bit lowest) as a 15-bit code value (first bit highest)
GCI_DC_FN uint32_t code_value(uint32_t bits) { return brev32(bits) >> 17; }

// eight limits as four words (one 16-byte LDS read on the device)
GCI_DC_FN void load_limits8(const uint16_t* p, uint32_t* w)
{
#if defined(__HIPCC__)
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#else
    memcpy(w, p, 16);
#endif
}

// lens[0 .. n) -> limits, offsets and the symbols sorted by code; false: a set zlib (and with it htslib) refuses -- an
// over-subscribed one always; an incomplete one (code space `left` over) unless `incomplete` allows it: CODE_COMPLETE never (the
// code-length code), CODE_ONE when the set has no code at all or exactly one code of length 1 (the lit/len and distance codes of a
// dynamic block), CODE_ANY always (the fixed distance code: 30 codes of 5 bits)
enum { CODE_COMPLETE = 0, CODE_ONE = 1, CODE_ANY = 2 };
template <typename SortedPtr>
GCI_DC_FN bool build_code(const uint8_t* lens, int n, Canon& cn, SortedPtr sorted, int incomplete)
{
    for (int l = 0; l < 16; l++) cn.next[l] = 0;
    for (int i = 0; i < n; i++) cn.next[lens[i]]++;
    uint32_t code = 0, idx = 0, left = 1u << 15, prev = 0;
    bool ok = true;
    cn.limit[0] = 0; cn.off[0] = 0; cn.next[0] = 0;
    for (int l = 1; l < 16; l++) {
        const uint32_t cnt = cn.next[l];
        code = (code + prev) << 1;
        cn.limit[l] = (uint16_t)((code + cnt) << (15 - l));
        cn.off[l] = (int16_t)((int)idx - (int)code);
        cn.next[l] = (uint16_t)idx;
        idx += cnt; prev = cnt;
        const uint32_t need = cnt << (15 - l);                           // sum count[l] * 2^(15 - l) must not exceed 2^15
        if (need > left) ok = false; else left -= need;
    }
    if (!ok) return false;
    if (left && incomplete != CODE_ANY && !(incomplete == CODE_ONE && (idx == 0u || (idx == 1u && left == 1u << 14)))) return false;
    for (int s = 0; s < n; s++) {
        const int l = lens[s];
        if (l) sorted[cn.next[l]++] = (uint16_t)s;
    }
    return true;
}

// the primary table of the codes of at most BITS bits, from the sorted symbols (the code lengths may be gone by now)
template <int BITS, typename SortedPtr>
GCI_DC_FN void build_table(const Canon& cn, SortedPtr sorted, uint16_t* table)
{
    for (int i = 0; i < (1 << BITS); i++) table[i] = 0;
    uint32_t idx = 0;
    for (int l = 1; l <= BITS; l++) {
        const uint32_t end = cn.next[l];
        const int off = cn.off[l];
        for (; idx < end; idx++) {
            const uint32_t e = make_entry(sorted[idx], (uint32_t)l);
            for (uint32_t k = brev32((uint32_t)((int)idx - off)) >> (32 - l); k < (1u << BITS); k += 1u << l) table[k] = (uint16_t)e;
        }
    }
}

// The search over the limits, for c = the 15-bit code value of the next bits of the stream: the length of its code = the number of limits <= c among
// limit[0 .. 15] (limit[0] = 0 is the "1 +"); more than MAXL: no such code.  SKIP: the lengths a primary table has dealt with --
// their limits are <= c for a code that is not in it, so the first eight are not read when SKIP covers them: a word that was not
// loaded is 0 and counted as it should be.  MAXL < 8: the last eight are not read.  Two limits per word: with c < 2^15 and limit
// <= 2^15, (c + 2^15) - limit has bit 15 set iff c >= limit and never borrows from the half above it -- one subtraction, one AND
// and one population count per pair instead of two compares and their bookkeeping.
template <int SKIP, int MAXL>
GCI_DC_FN int code_length(uint32_t bits, const Canon& cn, uint32_t& c)
{
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (SKIP + 1 < 8) load_limits8(&cn.limit[0], w);
    if (MAXL >= 8) load_limits8(&cn.limit[8], w + 4);
    c = code_value(bits);
    const uint32_t c2 = (c | (c << 16)) + 0x80008000u;
    int l = 0;
#pragma unroll
    for (int k = 0; k < (MAXL >= 8 ? 8 : 4); k++) l += __builtin_popcount((c2 - w[k]) & 0x80008000u);
    return l;
}
// where the symbol of the code of length l that c begins with lies in `sorted`
GCI_DC_FN int code_index(uint32_t c, int l, const Canon& cn) { return (int)cn.off[l] + (int)(c >> (15 - l)); }

// ... and both for the next bits of the stream (first bit lowest), all lengths: the symbol, len = its length; -1: no such code
GCI_DC_FN int code_search(uint32_t bits, const Canon& cn, const uint16_t* sorted, int& len)
{
    uint32_t c;
    const int l = code_length<0, 15>(bits, cn, c);
    if (l > 15) return -1;
    len = l;
    return (int)sorted[code_index(c, l, cn)];
}

// the entry of the 15-bit code value c (first bit highest, zeros behind a shorter code): the canonical search on the value itself
GCI_DC_FN uint16_t entry_of_value(uint32_t c, const Canon& cn, const uint16_t* sorted)
{
    int l = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) l += cn.limit[j] <= c ? 1 : 0;
    if (l > 15) return 0;
    return (uint16_t)make_entry(sorted[code_index(c, l, cn)], (uint32_t)l);
}
// entry k of a primary table of `bits` bits (k = the next bits of the stream, first bit lowest): 0 when the code is longer
GCI_DC_FN uint16_t table_entry(uint32_t k, int bits, const Canon& cn, const uint16_t* sorted)
{
    const uint32_t c = code_value(k);
    if (c >= cn.limit[bits]) return 0;
    return entry_of_value(c, cn, sorted);
}

}  // namespace deflate_codes
