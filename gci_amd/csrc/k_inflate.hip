// k_inflate.hip -- N1 on the GPU: BGZF members inflated by the device (what pysam / htslib do for the reference at
// GCI.py:150-151; the record walk over the inflated stream is k_records.hip).
//
// gci_bgzf_inflate_device.  DEFLATE is a serial bit stream: the parallelism of a BGZF file is ACROSS its members (gzip
// members of at most 64 KiB, RFC 1951 / 1952: 56 k for a chr19 40x HiFi file, millions for a genome).  A first version gave
// every member a whole wave (window and tables in LDS, every lane holding the same decoder state): correct, and bound by
// instruction issue on one lane's worth of work -- ~50 instructions per symbol, one wave per SIMD because of the 32 KiB
// window -- i.e. no faster than 32 host threads (5.9 GB/s).  This version gives every member ONE LANE:
//   * decoder state (bit buffer, positions) in registers; the lane's decode tables in LDS (8-bit primary table for
//     literals / lengths -- the block's code lengths share its space until the codes are built --, the symbols sorted by
//     code and 16 "limits" per alphabet for the longer codes and the distances: 1.3 KB per member, L members per
//     workgroup of one wave);
//   * no window: the output buffer in HBM is the window (a member's matches only reach back into its own output; a wave's
//     memory operations are issued in order, so a lane reads back what it has just written);
//   * the compressed bytes as naturally aligned 16-byte blocks, moved into the bit buffer a dword at a time; literals
//     gathered in a register and stored eight at a time; matches copied in 8-byte pieces (any address).
// Lanes diverge (literal / match, code lengths), but every wave instruction now serves L members, and a CU holds 112 of
// them (L = 8: 14 workgroups).  Stored, fixed and dynamic blocks.  Every member's output length is checked here, its CRC-32
// by k_bgzf_crc: one wave per member over the finished output, every lane the CRC register of its share, the shares
// concatenated with the GF(2) rule crc(A||B) = crc(A) * x^(8|B|) + crc(B) (as htslib verifies every block).
#include "gci_crc_gf2.hpp"
#include "gci_deflate_codes.hpp"
#include <stdlib.h>

namespace {

using namespace deflate_codes;

#define LIT_BITS 8

struct XPow8 { uint32_t v[32]; };
constexpr XPow8 make_xpow8()                       // v[k] = x^(8 * 2^k) mod P, reflected (x^8 = 0x00800000)
{
    XPow8 t{};
    uint32_t p = 0x00800000u;
    for (int k = 0; k < 32; k++) { t.v[k] = p; p = gf_mul_c(p, p); }
    return t;
}
__constant__ XPow8 c_xpow8 = make_xpow8();

// What one member's decoder keeps in LDS: 1.3 KB, which is what bounds the members a CU decodes at a time.  The code
// lengths of a block are only needed until its codes are built and share the primary table's space.
#define INF_WAVES 4
#define INF_DIST_BITS 5                // primary table of the distance codes: 5 bits (-2 % against none; 6 and 7 cost a workgroup per CU)
struct alignas(16) LaneTabs {
    union {
        uint16_t lit_tab[1 << LIT_BITS];
        uint8_t lens[352];          // [0, 19): the code-length code; [32, 32 + 286 + 30): both alphabets
    };
    uint16_t lit_sorted[288];
    uint16_t dist_sorted[32];
    uint16_t dist_tab[1 << INF_DIST_BITS];     // primary table of the distance codes (symbol | length << 9), like lit_tab
    Canon lit_cn, dist_cn;
};
static_assert(sizeof(uint16_t) << LIT_BITS >= 352, "the code lengths must fit under the primary table");

// The compressed bytes arrive as naturally aligned 16-byte loads, one block AHEAD of the one being consumed (the load
// issued when a block is taken up is needed 16 payload bytes later), and move into the bit buffer a dword at a time.
// 16 bytes in the global address space (a generic pointer kept in a struct becomes flat loads, which also count as LDS traffic)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 gu4;
__device__ __forceinline__ uint4 ld_block(const gu4* p) { const u32x4 v = *p; return make_uint4(v.x, v.y, v.z, v.w); }
struct Bits {
    unsigned long long bb;      // bit buffer, next bit = bit 0
    int bn;                     // valid bits
    uint4 res;                  // the block being consumed (lowest dword first)
    int rn;                     // dwords left in res
    uint4 nxt;                  // the block after it
    const gu4* q;               // the block after nxt
    const gu4* qlim;            // the block holding the member's last byte: nothing is loaded beyond it
    uint32_t taken;             // dwords moved out of res so far
};

__device__ __forceinline__ void next_dword(Bits& B)
{
    B.res.x = B.res.y; B.res.y = B.res.z; B.res.z = B.res.w;
    B.rn--; B.taken++;
    if (B.rn == 0) {
        B.res = B.nxt; B.rn = 4;
        B.nxt = ld_block(B.q);
        B.q = B.q < B.qlim ? B.q + 1 : B.q;
    }
}

// at least 32 valid bits (bits past the payload are caught by the position check at the end of the member)
__device__ __forceinline__ void need32(Bits& B)
{
    if (B.bn < 32) {
        B.bb |= (unsigned long long)B.res.x << B.bn;
        B.bn += 32;
        next_dword(B);
    }
}

// eight bytes at any address (the target handles unaligned global accesses)
__device__ __forceinline__ unsigned long long ld8(const uint8_t* p) { unsigned long long v; __builtin_memcpy(&v, p, 8); return v; }
__device__ __forceinline__ void st8(uint8_t* p, unsigned long long v) { __builtin_memcpy(p, &v, 8); }

__device__ __forceinline__ uint32_t take(Bits& B, int n)
{
    const uint32_t v = (uint32_t)(B.bb & ((1ull << n) - 1ull));
    B.bb >>= n; B.bn -= n;
    return v;
}

// one symbol: the primary table (PRIMARY > 0), else the search over the limits of the lengths PRIMARY + 1 .. MAXL
template <int PRIMARY, int MAXL, typename SortedPtr>
__device__ __forceinline__ int decode(Bits& B, const uint16_t* table, const Canon& cn, SortedPtr sorted)
{
    if (PRIMARY) {
        const uint32_t e = table[(uint32_t)B.bb & ((1u << PRIMARY) - 1u)];
        if (e) { const int l = (int)entry_len(e); B.bb >>= l; B.bn -= l; return (int)entry_sym(e); }
    }
    uint32_t c;
    const int l = code_length<PRIMARY, MAXL>((uint32_t)B.bb, cn, c);
    if (l > MAXL) return -1;
    const int at = code_index(c, l, cn);
    B.bb >>= l; B.bn -= l;
    return (int)sorted[at];
}

}  // namespace

// One lane = one member; INF_LANES members per workgroup (one wave; its other lanes leave at once).
template <int INF_LANES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(INF_WAVES, INF_WAVES)))
void k_bgzf_inflate(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ member_pos,
                    const uint64_t* __restrict__ out_off, uint32_t n_members, uint8_t* __restrict__ out,
                    uint64_t out_cap, unsigned long long* __restrict__ status, const uint32_t* __restrict__ done_by_wave)
{
    __shared__ LaneTabs tabs[INF_LANES];
    const int lane = threadIdx.x;
    if (lane >= INF_LANES) return;
    const uint32_t m = blockIdx.x * INF_LANES + lane;
    if (m >= n_members) return;
    if (done_by_wave && done_by_wave[m] == 0u) return;                        // k_inflate_wave.hip decoded this one
    LaneTabs& T = tabs[lane];
    uint16_t* const lit_sorted = T.lit_sorted;
    const uint64_t pos = member_pos[m], pos_next = member_pos[m + 1];
    const uint64_t o0 = out_off[m];
    const uint32_t isize = (uint32_t)(out_off[m + 1] - o0);
    bool bad = pos_next < pos + 26 || o0 + isize > out_cap || isize > 65536u;
    uint32_t pay_len = 0, head = 0;
    Bits B;
    B.bb = 0; B.bn = 0; B.rn = 4; B.taken = 0;
    if (!bad) {
        const uint32_t xlen = (uint32_t)raw[pos + 10] | ((uint32_t)raw[pos + 11] << 8);
        const uint64_t pay0 = pos + 12 + xlen;
        bad = pay0 + 8 > pos_next || raw[pos] != 0x1f || raw[pos + 1] != 0x8b || raw[pos + 2] != 8;
        if (!bad) {
            pay_len = (uint32_t)(pos_next - 8 - pay0);
            const uintptr_t a0 = (uintptr_t)(raw + pay0);
            head = (uint32_t)(a0 & 15u);
            const gu4* base = (const gu4*)(a0 - head);
            B.qlim = (const gu4*)((uintptr_t)(raw + pos_next - 1) & ~(uintptr_t)15);
            B.res = ld_block(base);
            B.q = base < B.qlim ? base + 1 : base;
            B.nxt = ld_block(B.q);
            B.q = B.q < B.qlim ? B.q + 1 : B.q;
            for (uint32_t k = 0; k < (head >> 2); k++) next_dword(B);          // the bytes in front of the payload
            need32(B);
            B.bb >>= (head & 3u) * 8; B.bn -= (int)(head & 3u) * 8;
        }
    }
    uint8_t* __restrict__ dst = out + o0;
    uint8_t* const dst_end = dst + isize;
    // output: literals gather in a register and leave as one 8-byte store (any address).  A partial group is stored as 8
    // bytes as well where that stays inside the member's output: what lies behind `op` is overwritten before it is read.
    unsigned long long ob = 0;
    uint32_t oc = 0, op = 0;
    auto flush = [&]() __attribute__((always_inline)) {
        uint8_t* at = dst + op - oc;
        if (oc && at + 8 <= dst_end) st8(at, ob);
        else for (uint32_t i = 0; i < oc; i++) at[i] = (uint8_t)(ob >> (8 * i));
        ob = 0; oc = 0;
    };
    auto emit = [&](uint32_t byte) __attribute__((always_inline)) {
        ob |= (unsigned long long)byte << (8 * oc);
        oc++; op++;
        if (oc == 8) { st8(dst + op - 8, ob); ob = 0; oc = 0; }
    };
    for (bool last = false; !last && !bad;) {
        // every block header must lie inside the payload (a damaged stream of empty non-final blocks would never end otherwise:
        // everything else in a block is bounded by the member's output length)
        if (32ll * B.taken - 8ll * head - B.bn + 3 > 8ll * pay_len) { bad = true; break; }
        need32(B);
        last = take(B, 1) != 0;
        const uint32_t type = take(B, 2);
        if (type == 0) {                                                     // stored
            take(B, B.bn & 7);                                               // to the byte boundary
            need32(B);
            const uint32_t len = take(B, 16), nlen = take(B, 16);
            if ((len ^ 0xFFFFu) != nlen || op + len > isize) { bad = true; break; }
            for (uint32_t i = 0; i < len; i++) { need32(B); emit(take(B, 8)); }
            continue;
        }
        if (type == 3) { bad = true; break; }
        uint8_t* ll = T.lens + 32;
        if (type == 1) {                                                     // fixed code (RFC 1951 3.2.6)
            for (int i = 0; i < 288; i++) ll[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
            for (int i = 0; i < 30; i++) ll[288 + i] = 5;
            if (!build_code(ll, 288, T.lit_cn, lit_sorted, CODE_ANY) || !build_code(ll + 288, 30, T.dist_cn, T.dist_sorted, CODE_ANY)) { bad = true; break; }
        } else {                                                             // dynamic code (3.2.7)
            need32(B);
            const int hlit = (int)take(B, 5) + 257, hdist = (int)take(B, 5) + 1, hclen = (int)take(B, 4) + 4;
            if (hlit > 286 || hdist > 30) { bad = true; break; }
            for (int i = 0; i < 19; i++) T.lens[i] = 0;
            for (int i = 0; i < hclen; i++) { need32(B); T.lens[c_clen_order[i]] = (uint8_t)take(B, 3); }
            // the code-length code: 19 symbols of at most 7 bits, decoded bit by bit (dist_cn / dist_sorted are free until below)
            if (!build_code(T.lens, 19, T.dist_cn, T.dist_sorted, CODE_COMPLETE)) { bad = true; break; }
            int n = 0, prev = 0;
            while (n < hlit + hdist) {
                need32(B);
                const int sym = decode<0, 7>(B, nullptr, T.dist_cn, T.dist_sorted);
                if (sym < 0) { bad = true; break; }
                int rep = 1, val = sym;
                if (sym == 16) { if (n == 0) { bad = true; break; } val = prev; rep = 3 + (int)take(B, 2); }
                else if (sym == 17) { val = 0; rep = 3 + (int)take(B, 3); }
                else if (sym == 18) { val = 0; rep = 11 + (int)take(B, 7); }
                if (n + rep > hlit + hdist) { bad = true; break; }
                for (int i = 0; i < rep; i++) ll[n + i] = (uint8_t)val;
                n += rep; prev = val;
            }
            if (bad) break;
            if (ll[256] == 0) { bad = true; break; }                          // no end-of-block code
            if (!build_code(ll, hlit, T.lit_cn, lit_sorted, CODE_ONE) || !build_code(ll + hlit, hdist, T.dist_cn, T.dist_sorted, CODE_ONE)) { bad = true; break; }
        }
        build_table<LIT_BITS>(T.lit_cn, lit_sorted, T.lit_tab);
        build_table<INF_DIST_BITS>(T.dist_cn, T.dist_sorted, T.dist_tab);
        // ---- symbols of the block: runs of literals (the lanes of the wave meet again at their next match) -------------------
        for (;;) {
            int sym;
            for (;;) {
                need32(B);
                sym = decode<LIT_BITS, 15>(B, T.lit_tab, T.lit_cn, lit_sorted);
                if (sym < 0 || sym >= 256) break;
                if (op >= isize) { sym = -1; break; }
                emit((uint32_t)sym);
            }
            if (sym < 0 || sym > 285) { bad = true; break; }
            if (sym == 256) break;
            // length and distance codes (RFC 1951 3.2.5) by arithmetic: a table in constant memory is a vector-memory load
            // and a wait per look-up here
            const uint32_t lc = (uint32_t)sym - 257u;
            const uint32_t le = lc < 8u || lc == 28u ? 0u : (lc >> 2) - 1u;
            uint32_t len = (lc < 8u ? 3u + lc : lc == 28u ? 258u : 3u + ((4u + (lc & 3u)) << le)) + take(B, (int)le);
            need32(B);
            const int ds = decode<INF_DIST_BITS, 15>(B, T.dist_tab, T.dist_cn, T.dist_sorted);
            if (ds < 0 || ds > 29) { bad = true; break; }
            const uint32_t de = ds < 4 ? 0u : ((uint32_t)ds >> 1) - 1u;
            const uint32_t dist = (ds < 4 ? (uint32_t)ds + 1u : 1u + ((2u + ((uint32_t)ds & 1u)) << de)) + take(B, (int)de);
            if (dist > op || op + len > isize) { bad = true; break; }
            // the copy reads this member's own output back from memory (a lane's stores and loads stay in order)
            flush();
            const uint8_t* src = dst + op - dist;
            uint8_t* to = dst + op;
            op += len;
            if (dist >= 8) {
                // up to four 8-byte pieces per round trip: as many as lie wholly in front of what the round itself writes
                while (len) {
                    const uint32_t nb = min(min(4u, dist >> 3), (len + 7u) >> 3);
                    unsigned long long v[4];
#pragma unroll
                    for (uint32_t i = 0; i < 4; i++) v[i] = i < nb ? ld8(src + 8 * i) : 0ull;
#pragma unroll
                    for (uint32_t i = 0; i < 4; i++) {
                        if (i >= nb) continue;
                        uint8_t* t = to + 8 * i;
                        if (t + 8 <= dst_end) st8(t, v[i]);
                        else for (uint32_t k = 0; 8 * i + k < len; k++) t[k] = (uint8_t)(v[i] >> (8 * k));
                    }
                    const uint32_t adv = min(len, 8u * nb);
                    src += adv; to += adv; len -= adv;
                }
            } else {
                // a short period: its bytes once, made periodic over eight bytes, stored in steps of whole periods
                unsigned long long pat = 0;
                if (op - len >= 8) pat = ld8(to - 8) >> (8 * (8 - dist));
                else {
#pragma unroll
                    for (int i = 0; i < 7; i++) pat |= (unsigned long long)((uint32_t)i < dist ? src[i] : (uint8_t)0) << (8 * i);
                }
                pat &= ~0ull >> (8 * (8 - dist));
                if (dist < 8) pat |= pat << (8 * dist);
                if (dist < 4) pat |= pat << (16 * dist);
                if (dist < 2) pat |= pat << 32;
                const uint32_t step = dist * (8u / dist);
                while (len) {
                    const uint32_t adv = min(len, step);
                    if (to + 8 <= dst_end) st8(to, pat);
                    else for (uint32_t k = 0; k < adv; k++) to[k] = (uint8_t)(pat >> (8 * k));
                    to += adv; len -= adv;
                }
            }
        }
    }
    flush();
    if (!bad && op != isize) bad = true;
    if (!bad) {                                                                // the stream may not run past the payload
        const long long bits = 32ll * B.taken - 8ll * head - B.bn;
        if (bits > 8ll * pay_len) bad = true;
    }
    if (bad) atomicMin(status, ((unsigned long long)m << 8) | (unsigned long long)(uint8_t)(-GCI_E_MALFORMED));
}

// CRC-32 of every member's output against its trailer: one wave per member, CRC_PER_WAVE members one after the other.
//
// The wave reads the member as rows of 1 KB -- lane l the 16 bytes at 16 l of every row: coalesced, where a contiguous share per lane
// made every load touch 64 cache lines for 16 bytes each (1 TB/s) -- and CRC's linearity puts the pieces together: lane l's register
// runs over ITS pieces as if the 1008 bytes between two of them were zeros, i.e. absorbing a piece and skipping to the next one is
//   reg' = sum over the 16 bytes b_j of W[15 - j][b_j]     (the first four bytes xor-ed with reg, as in slicing-by-16),
//   W[k][b] = T[k][b] * x^(8 * 1008),  T[k][b] = the register after byte b and k zero bytes;
// the lane's last piece is absorbed with T (nothing is skipped behind it), the register then multiplied by x^(8 * bytes behind
// the piece) from the powers x^(8 * 2^k), and the 64 products xor-ed.  The register starts at all ones where the member starts;
// the fewer than 16 bytes behind the last whole piece are one lane's, byte by byte, with no bytes behind them.  The 32 tables are
// made once per context (k_crc_tables) and copied into LDS by every workgroup.
#define CRC_ROW 1024u
#define CRC_PER_WAVE 8

__global__ __launch_bounds__(256) void k_crc_tables(uint32_t* __restrict__ tabs)          // tabs[0..16): T, [16..32): W
{
    __shared__ uint32_t t0[256];
    const int i = threadIdx.x;
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
    t0[i] = c;
    __syncthreads();
    uint32_t skip = 0x80000000u;                                               // x^(8 * (CRC_ROW - 16))
    for (uint32_t e = CRC_ROW - 16u, k = 0; e; e >>= 1, k++) if (e & 1u) skip = gf_mul_shift(skip, c_xpow8.v[k]);
    for (int k = 0; k < 16; k++) {
        tabs[k * 256 + i] = c;
        tabs[(16 + k) * 256 + i] = gf_mul_shift(c, skip);
        c = (c >> 8) ^ t0[c & 0xFFu];
    }
}

__global__ __launch_bounds__(BLOCK) void k_bgzf_crc(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ member_pos,
                                                    const uint64_t* __restrict__ out_off, uint32_t n_members, const uint8_t* __restrict__ out,
                                                    const uint32_t* __restrict__ tabs, unsigned long long* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint32_t T[32][256];
    for (int i = threadIdx.x; i < 32 * 256 / 4; i += BLOCK)
        reinterpret_cast<uint4*>(&T[0][0])[i] = reinterpret_cast<const uint4*>(tabs)[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    for (uint32_t m = wave * CRC_PER_WAVE; m < min(n_members, (wave + 1) * CRC_PER_WAVE); m++) {
        const uint64_t o0 = out_off[m];
        const uint32_t n = (uint32_t)(out_off[m + 1] - o0);
        const uint8_t* p0 = out + o0;
        const uint32_t full = n >> 4;                                         // whole 16-byte pieces; piece j is lane j % 64's
        const uint32_t count = full > lane ? (full - lane + 63u) >> 6 : 0u;
        uint32_t c = (lane == 0 && full) ? 0xFFFFFFFFu : 0u;
        const uint8_t* q = p0 + 16u * lane;
        for (uint32_t i = 0; i < count; i++, q += CRC_ROW) {
            uint4 v;
            __builtin_memcpy(&v, q, 16);                                      // (any address: the member starts where the one before it ended)
            const uint32_t x = v.x ^ c;
            const uint32_t (*S)[256] = i + 1 < count ? &T[16] : &T[0];        // W but for the lane's last piece
            c = S[15][x & 0xFFu] ^ S[14][(x >> 8) & 0xFFu] ^ S[13][(x >> 16) & 0xFFu] ^ S[12][x >> 24]
              ^ S[11][v.y & 0xFFu] ^ S[10][(v.y >> 8) & 0xFFu] ^ S[9][(v.y >> 16) & 0xFFu] ^ S[8][v.y >> 24]
              ^ S[7][v.z & 0xFFu] ^ S[6][(v.z >> 8) & 0xFFu] ^ S[5][(v.z >> 16) & 0xFFu] ^ S[4][v.z >> 24]
              ^ S[3][v.w & 0xFFu] ^ S[2][(v.w >> 8) & 0xFFu] ^ S[1][(v.w >> 16) & 0xFFu] ^ S[0][v.w >> 24];
        }
        // the bytes behind the lane's last piece
        const uint32_t behind = count ? n - 16u * ((count - 1u) * 64u + lane + 1u) : 0u;
        uint32_t xp = 0x80000000u;                                            // x^0, reflected
        for (uint32_t e = behind, k = 0; e; e >>= 1, k++) if (e & 1u) xp = gf_mul_shift(xp, c_xpow8.v[k]);
        c = gf_mul_shift(c, xp);
        if (lane == 0 && (n & 15u)) {                                         // the last n % 16 bytes: nothing behind them
            uint32_t r = full ? 0u : 0xFFFFFFFFu;
            for (uint32_t k = 16u * full; k < n; k++) r = T[0][(r ^ p0[k]) & 0xFFu] ^ (r >> 8);
            c ^= r;
        }
        if (lane == 0 && n == 0) c = 0xFFFFFFFFu;
        for (int d = 1; d < 64; d <<= 1) c ^= (uint32_t)__shfl_xor((int)c, d, 64);
        if (lane == 0) {
            const uint32_t got = c ^ 0xFFFFFFFFu;
            const uint64_t tp = member_pos[m + 1] - 8;
            const uint32_t want = (uint32_t)raw[tp] | ((uint32_t)raw[tp + 1] << 8) | ((uint32_t)raw[tp + 2] << 16) | ((uint32_t)raw[tp + 3] << 24);
            if (got != want) atomicMin(status, ((unsigned long long)m << 8) | (unsigned long long)(uint8_t)(-GCI_E_MALFORMED));
        }
    }
}

int gci_inflate_wave_run(gci_ctx* ctx, const uint8_t* d_raw, const uint64_t* d_member_pos, const uint64_t* d_out_off, uint32_t n_members,
                         uint8_t* d_out, uint64_t out_cap, uint32_t* d_wstatus);          // k_inflate_wave.hip

// d_raw must be readable up to 8 bytes past its last member (the decoder loads whole aligned dwords).
extern "C" int gci_bgzf_inflate_device(gci_ctx* ctx, const uint8_t* d_raw, const uint64_t* d_member_pos, const uint64_t* d_out_off,
                                       uint32_t n_members, uint8_t* d_out, uint64_t out_cap, int check_crc, uint64_t* d_status)
{
    if (!ctx || !d_status || (n_members && (!d_raw || !d_member_pos || !d_out_off || !d_out))) return GCI_E_INVALID;
    HIPCHK(hipMemsetAsync(d_status, 0xFF, 8, ctx->stream));
    if (n_members) {
        // GCI_INFLATE=lane: every member by the lane-per-member kernel (round 2 - 4); default: a wave per member (k_inflate_wave.hip),
        // the members it hands back -- its status word != 0 -- by the lane-per-member kernel behind it
        static const bool wave = [] { const char* e = getenv("GCI_INFLATE"); return !(e && !strcmp(e, "lane")); }();
        const uint32_t* d_done = nullptr;
        ctx->inflate_last_n = 0;
        if (wave) {
            int st = gci_ensure(ctx, ctx->inflate_wstatus, (size_t)(n_members > 2048u && n_members < 262144u ? 262144u : n_members) * sizeof(uint32_t));
            if (st) return st;
            HIPCHK(hipMemsetAsync(ctx->inflate_wstatus.p, 0xFF, (size_t)n_members * sizeof(uint32_t), ctx->stream));
            st = gci_inflate_wave_run(ctx, d_raw, d_member_pos, d_out_off, n_members, d_out, out_cap, (uint32_t*)ctx->inflate_wstatus.p);
            if (st) return st;
            d_done = (const uint32_t*)ctx->inflate_wstatus.p;
            ctx->inflate_last_n = n_members;
        }
        // eight members per wave (gci_bgzf_inflate_round assumes the same)
        hipLaunchKernelGGL(k_bgzf_inflate<8>, dim3((n_members + 7) / 8), dim3(64), 0, ctx->stream, d_raw, d_member_pos, d_out_off, n_members,
                           d_out, out_cap, (unsigned long long*)d_status, d_done);
        LAUNCHCHK("k_bgzf_inflate");
        if (check_crc) {
            if (!ctx->crc_tabs_ready) {                                      // (ready only once the launch went through)
                const int st = gci_ensure(ctx, ctx->crc_tabs, 32 * 256 * sizeof(uint32_t));
                if (st) return st;
                hipLaunchKernelGGL(k_crc_tables, dim3(1), dim3(256), 0, ctx->stream, (uint32_t*)ctx->crc_tabs.p);
                LAUNCHCHK("k_crc_tables");
                ctx->crc_tabs_ready = true;
            }
            const uint32_t per_block = (BLOCK / 64) * CRC_PER_WAVE;
            hipLaunchKernelGGL(k_bgzf_crc, dim3((n_members + per_block - 1) / per_block), dim3(BLOCK), 0, ctx->stream, d_raw, d_member_pos,
                               d_out_off, n_members, (const uint8_t*)d_out, (const uint32_t*)ctx->crc_tabs.p, (unsigned long long*)d_status);
            LAUNCHCHK("k_bgzf_crc");
        }
    }
    return GCI_OK;
}

// How many members the device decodes AT A TIME (CUs x resident workgroups x members per workgroup).  Every member takes about
// as long as every other (~37 ms with the CUs full, whatever the launch size), so a launch is a whole number of such rounds:
// 65 536 members -- a run of 4 GiB -- are 2.3 rounds and take the time of 3.  A caller that cuts a file into runs makes them
// whole multiples of this (pipeline._bam_join_input_gpu).
extern "C" uint32_t gci_bgzf_inflate_round(gci_ctx* ctx)
{
    if (!ctx) return 0;
    int per_cu = 0, cus = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bgzf_inflate<8>, 64, 0) != hipSuccess) return 0;
    return (uint32_t)(cus > 0 && per_cu > 0 ? cus * per_cu * 8 : 0);
}
