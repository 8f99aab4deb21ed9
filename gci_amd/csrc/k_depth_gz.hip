// k_depth_gz.hip -- this library's own .depth.gz back to a track, without inflating it: the counterpart of k_deflate.hip.
//
// k_deflate.hip writes a depth track as runs of one line repeated -- the line's literals, then matches at distance = line width, in
// the fixed Huffman code, a block per 4096 bases closed by an empty stored block, 64 blocks a member -- and takes the CRC-32 of the
// text it never writes by GF(2) algebra over the runs.  The reader does the same in reverse: the tokens of a member ARE its
// (depth, count) runs, the CRC of the text they stand for comes from the same table (gci_crc_gf2.hpp), and the runs expand into the
// int32 track.  150 MB of members cross PCIe for a genome where 9 GB of text crossed the host twice.
//
//   k_dgz_scan    a lane per candidate member start: decodes under the grammar (include/gci_hip.h), counts lines and runs, checks
//                 CRC-32 and ISIZE.  A false candidate in the middle of another member's bits is the normal case: every loop is
//                 bounded by the buffer and by the caps on blocks and lines, and no byte at or beyond raw + n_raw is read.
//   k_dgz_runs    a lane per member of the chain: the same walk, writing the runs at the member's scanned offset and, per 4096 lines,
//                 the run they begin in.
//   k_dgz_expand  a workgroup per 4096 lines: the starts of the tile's runs by a block scan into LDS, every element finds its run by
//                 bisection, consecutive lanes store consecutive 16 bytes.  No lane walks a run alone.
//
// A member is one serial bit stream, so the two decoding passes are latency bound: a wave carries 16 members, not 64 -- a genome has
// ~12 000 members, fewer than the chip has SIMDs times 16, and lanes of a wave that sit in different tokens take turns.
#include "gci_crc_gf2.hpp"

namespace {

constexpr uint32_t MAX_LINES = GCI_DGZ_MAX_LINES, MAX_BLOCKS = GCI_DGZ_MAX_BLOCKS;
constexpr uint32_t MEMBER_TILES = MAX_LINES / TILE;
constexpr int DECODE_LANES = 16;                 // members per wave of the two decoding kernels
static_assert(MEMBER_TILES * TILE == MAX_LINES, "a member is whole tiles");

// ---- bit reader: DEFLATE packs bits LSB first; never reads at or beyond raw + n ---------------------------------------------------
struct BitIn {
    const uint8_t* __restrict__ raw;
    uint64_t n, p;                               // bytes of the buffer, next byte to load
    unsigned long long acc = 0;
    uint32_t nb = 0;                             // bits in acc
    __device__ __forceinline__ bool need(uint32_t k)                            // k <= 32
    {
        if (nb >= k) return true;
        if (p + 4u <= n) { acc |= (unsigned long long)ld_u32(raw + p) << nb; p += 4u; nb += 32u; }
        else while (p < n && nb <= 56u) { acc |= (unsigned long long)raw[p++] << nb; nb += 8u; }
        return nb >= k;
    }
    __device__ __forceinline__ uint32_t take(uint32_t k)                        // k <= 32 bits that need() has seen
    {
        const uint32_t v = (uint32_t)(acc & ((1ull << k) - 1ull));
        acc >>= k; nb -= k;
        return v;
    }
    __device__ __forceinline__ void align() { const uint32_t k = nb & 7u; acc >>= k; nb -= k; }
    __device__ __forceinline__ uint64_t byte_pos() const { return p - (nb >> 3); }   // behind align()
};

// One member under the grammar.  sink.run(depth, lines) takes every run as it closes (false: stop).  -> false: not this writer's.
// Every token is asked for with 20 bits in hand (the longest is 8 + 5 + 5 + 2): the trailer's 64 bits follow the last one.
template <class Sink>
__device__ bool decode_member(const uint8_t* __restrict__ raw, uint64_t n_raw, uint64_t pos, Sink& sink, uint32_t& lines_out,
                              uint64_t& end, uint32_t& crc_file, uint32_t& isize_file)
{
    if (pos >= n_raw || n_raw - pos < 10u) return false;
    const uint8_t* h = raw + pos;
    if (h[0] != 0x1F || h[1] != 0x8B || h[2] != 8 || h[3] != 0 || h[4] != 0 || h[5] != 0 || h[6] != 0 || h[7] != 0 || h[8] != 0 ||
        h[9] != 0xFF) return false;
    BitIn b{raw, n_raw, pos + 10u};
    uint32_t blocks = 0, lines = 0;
    bool prev_fixed = false;
    for (;;) {
        if (!b.need(3u)) return false;
        const uint32_t hd = b.take(3u), bfinal = hd & 1u, btype = hd >> 1;
        if (btype == 0u) {                                                      // stored: empty, behind a fixed block, never final
            if (!prev_fixed || bfinal) return false;
            b.align();
            if (!b.need(32u) || b.take(32u) != 0xFFFF0000u) return false;       // LEN = 0, NLEN = ~0
            prev_fixed = false;
            continue;
        }
        if (btype != 1u || ++blocks > MAX_BLOCKS) return false;
        uint32_t w = 0;                          // width of the run's line (0: no run yet in this block)
        uint32_t run_val = 0, run_lines = 0, rem = 0;    // rem: bytes of a line that matches have begun
        uint32_t digits = 0;                     // of the line that literals are spelling
        uint64_t val = 0;
        bool spelling = false;
        for (;;) {
            if (!b.need(20u)) return false;
            const uint32_t c7 = __brev((uint32_t)b.acc & 0x7Fu) >> 25;
            uint32_t sym;
            if (c7 <= 23u) {                                                    // 7-bit codes: 256 .. 279
                b.take(7u);
                if (c7 == 0u) break;
                sym = 256u + c7;
            } else {
                const uint32_t c8 = __brev((uint32_t)b.acc & 0xFFu) >> 24;
                b.take(8u);
                if (c8 >= 0x30u && c8 <= 0xBFu) {                               // a literal byte 0 .. 143
                    const uint32_t ch = c8 - 0x30u;
                    if (rem) return false;                                      // inside a line begun by a match
                    if (!spelling) {
                        if (w && !sink.run(run_val, run_lines)) return false;
                        w = 0; spelling = true; digits = 0; val = 0;
                    }
                    if (ch >= '0' && ch <= '9') {
                        if (digits == 10u || (digits == 1u && val == 0u)) return false;   // too long, or a leading zero
                        val = val * 10u + (ch - '0');
                        digits++;
                    } else if (ch == '\n') {
                        if (digits == 0u || val > 0x7FFFFFFFull || lines == MAX_LINES) return false;
                        w = digits + 1u; run_val = (uint32_t)val; run_lines = 1; lines++;
                        spelling = false;
                    } else return false;
                    continue;
                }
                if (c8 < 0xC0u || c8 > 0xC5u) return false;                     // literals >= 144, symbols 286 / 287
                sym = 280u + (c8 - 0xC0u);
            }
            // a match: length symbol 257 .. 285, then the distance
            const uint32_t s = sym - 257u;
            uint32_t len;
            if (s < 8u) len = 3u + s;
            else if (s == 28u) len = 258u;
            else { const uint32_t e = (s >> 2) - 1u; len = 3u + ((4u + (s & 3u)) << e) + b.take(e); }
            const uint32_t c5 = __brev((uint32_t)b.acc & 0x1Fu) >> 27;
            b.take(5u);
            uint32_t dist;
            if (c5 < 4u) dist = c5 + 1u;
            else if (c5 < 6u) dist = 5u + 2u * (c5 - 4u) + b.take(1u);
            else if (c5 < 8u) dist = 9u + 4u * (c5 - 6u) + b.take(2u);
            else return false;                                                  // 17 and beyond (codes 30 / 31 among them)
            if (spelling || w == 0u || dist != w) return false;
            rem += len;
            const uint32_t whole = rem / w;
            rem -= whole * w;
            if (whole > MAX_LINES - lines) return false;
            run_lines += whole; lines += whole;
        }
        if (spelling || rem) return false;                                      // the block ends inside a line
        if (w && !sink.run(run_val, run_lines)) return false;
        prev_fixed = true;
        if (bfinal) break;
    }
    b.align();
    const uint64_t q = b.byte_pos();
    if (q > n_raw || n_raw - q < 8u) return false;
    crc_file = (uint32_t)raw[q] | (uint32_t)raw[q + 1] << 8 | (uint32_t)raw[q + 2] << 16 | (uint32_t)raw[q + 3] << 24;
    isize_file = (uint32_t)raw[q + 4] | (uint32_t)raw[q + 5] << 8 | (uint32_t)raw[q + 6] << 16 | (uint32_t)raw[q + 7] << 24;
    end = q + 8u;
    lines_out = lines;
    return true;
}

// CRC-32 and length of the text the runs stand for, as the writer computes them
struct CrcSink {
    CrcTab t;
    uint32_t c = 0, len = 0, runs = 0;
    __device__ __forceinline__ bool run(uint32_t v, uint32_t n)
    {
        runs++;
        const Line l = make_line(v);
        len += n * l.w;                                                         // <= 262 144 * 11
        if (n == 1u) {                                                          // (pile-ups: the line's bytes through the register)
            uint32_t r = c ^ 0xFFFFFFFFu;
            for (uint32_t k = 0; k < l.w; k++) {
                r ^= line_byte(l, k);
                for (int i = 0; i < 8; i++) r = (r >> 1) ^ ((r & 1u) ? CRC_POLY : 0u);
            }
            c = r ^ 0xFFFFFFFFu;
            return true;
        }
        const uint32_t lc = v < (uint32_t)LINE_TAB ? t.line[v] : crc_line(l).c;
        while (n) {                                                             // (a forged block may hold more than a tile's lines)
            const uint32_t k = n < (uint32_t)TILE ? n : (uint32_t)TILE;
            c = crc_append_lines(c, lc, l.w, k, t);
            n -= k;
        }
        return true;
    }
};

// the runs to their place, and per 4096 lines of the member the run they begin in: {run, lines of it in front of the tile}
struct RunSink {
    gci_dgz_run* __restrict__ out;
    uint2* __restrict__ tiles;
    uint32_t cap;
    uint32_t r = 0, line = 0;
    __device__ __forceinline__ bool run(uint32_t v, uint32_t n)
    {
        if (r >= cap) return false;
        for (uint32_t b = (line + (TILE - 1u)) & ~(uint32_t)(TILE - 1u); b < line + n; b += TILE)    // line + n <= MAX_LINES
            tiles[b / TILE] = make_uint2(r, b - line);
        out[r].depth = (int32_t)v;
        out[r].count = n;
        r++;
        line += n;
        return true;
    }
};

__global__ __launch_bounds__(64) void k_dgz_scan(const uint8_t* __restrict__ raw, uint64_t n_raw, const uint64_t* __restrict__ cand,
                                                 uint32_t n_cand, gci_dgz_info* __restrict__ info, const uint32_t* __restrict__ crc_tab)
{
    if (threadIdx.x >= DECODE_LANES) return;
    const uint64_t i = (uint64_t)blockIdx.x * DECODE_LANES + threadIdx.x;
    if (i >= n_cand) return;
    CrcSink sink{CrcTab{reinterpret_cast<const uint2*>(crc_tab + TAB_REP), crc_tab + TAB_LINE, crc_tab + TAB_POW}};
    uint64_t end = 0;
    uint32_t lines = 0, crc_file = 0, isize_file = 0;
    const bool ok = decode_member(raw, n_raw, cand[i], sink, lines, end, crc_file, isize_file);
    gci_dgz_info o;
    o.end = ok ? end : 0ull;
    o.status = ok ? GCI_DGZ_OK : GCI_DGZ_FOREIGN;
    o.lines = ok ? lines : 0u;
    o.runs = ok ? sink.runs : 0u;
    o.crc_ok = ok && sink.c == crc_file;
    o.isize_ok = ok && sink.len == isize_file;
    o.reserved = 0u;
    info[i] = o;
}

__global__ __launch_bounds__(64) void k_dgz_runs(const uint8_t* __restrict__ raw, uint64_t n_raw, const gci_dgz_member* __restrict__ members,
                                                 uint32_t n_members, gci_dgz_run* __restrict__ runs, uint2* __restrict__ tiles)
{
    if (threadIdx.x >= DECODE_LANES) return;
    const uint64_t m = (uint64_t)blockIdx.x * DECODE_LANES + threadIdx.x;
    if (m >= n_members) return;
    const gci_dgz_member mem = members[m];
    RunSink sink{runs + mem.run0, tiles + m * MEMBER_TILES, mem.runs};
    uint64_t end;
    uint32_t lines, crc_file, isize_file;
    (void)decode_member(raw, n_raw, mem.pos, sink, lines, end, crc_file, isize_file);
}

__global__ __launch_bounds__(BLOCK) void k_dgz_expand(const gci_dgz_run* __restrict__ runs, const gci_dgz_member* __restrict__ members,
                                                      const uint2* __restrict__ tiles, int32_t* __restrict__ track, uint64_t track_n)
{
    __shared__ uint32_t starts[TILE];            // first line (of the tile) of every run the tile touches; ~0: no such run
    __shared__ int32_t vals[TILE];
    __shared__ uint32_t wtot[BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t m = blockIdx.x / MEMBER_TILES;
    const uint32_t t = blockIdx.x % MEMBER_TILES;
    const gci_dgz_member mem = members[m];
    const uint32_t first = t * TILE;
    if (first >= mem.lines || mem.lines > MAX_LINES) return;
    const uint32_t n = min((uint32_t)TILE, mem.lines - first);
    const uint2 ts = tiles[m * MEMBER_TILES + t];
    if (ts.x >= mem.runs) return;
    const gci_dgz_run* __restrict__ src = runs + mem.run0 + ts.x;
    const uint32_t avail = mem.runs - ts.x;
    uint32_t base = 0, nr = 0;
    // a run holds a line at least: TILE runs at most reach into the tile
    for (uint32_t chunk = 0; chunk < TILE / BLOCK && base < n && chunk * BLOCK < avail; chunk++) {
        const uint32_t i = chunk * BLOCK + tid;
        uint32_t cnt = 0;
        int32_t v = 0;
        if (i < avail) {
            const gci_dgz_run r = src[i];
            v = r.depth;
            cnt = r.count;
            if (i == 0u) cnt = cnt > ts.y ? cnt - ts.y : 0u;
            cnt = min(cnt, (uint32_t)TILE);                                     // (what reaches beyond the tile does not matter)
        }
        const uint32_t inc = wave_inclusive<uint32_t>(cnt, (int)lane);
        if (lane == 63u) wtot[wave] = inc;
        __syncthreads();
        uint32_t pre = base + inc - cnt, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < BLOCK / 64; k++) { const uint32_t x = wtot[k]; if (k < wave) pre += x; all += x; }
        starts[i] = i < avail ? pre : 0xFFFFFFFFu;
        vals[i] = v;
        base += all;
        nr = min(avail, (chunk + 1u) * BLOCK);
        __syncthreads();
    }
    const uint64_t g0 = mem.elem0 + first;
    const bool wide = (mem.elem0 & 3u) == 0u;
#pragma unroll
    for (uint32_t k = 0; k < TILE / (BLOCK * 4); k++) {
        const uint32_t e = (k * BLOCK + tid) * 4u;
        if (e >= n) continue;
        uint32_t lo = 0, hi = nr;                                               // starts[lo] <= e < starts[hi]  (starts[0] == 0)
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (starts[mid] <= e) lo = mid; else hi = mid;
        }
        int32_t x[4];
        x[0] = vals[lo];
#pragma unroll
        for (uint32_t j = 1; j < 4; j++) {
            while (lo + 1u < nr && starts[lo + 1u] <= e + j) lo++;
            x[j] = vals[lo];
        }
        const uint64_t g = g0 + e;
        if (wide && e + 4u <= n && g + 4u <= track_n) {
            *reinterpret_cast<int4*>(track + g) = make_int4(x[0], x[1], x[2], x[3]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                if (e + j < n && g + j < track_n) track[g + j] = x[j];
        }
    }
}

}  // namespace

extern "C" int gci_depth_gz_scan(gci_ctx* ctx, const uint8_t* d_raw, uint64_t n_raw, const uint64_t* d_cand_pos, uint32_t n_cand,
                                 gci_dgz_info* d_info)
{
    if (!ctx || (n_cand && (!d_raw || !d_cand_pos || !d_info))) return GCI_E_INVALID;
    if (n_cand == 0) return GCI_OK;
    GCI_TRY(ensure_crc_tab(ctx));
    hipLaunchKernelGGL(k_dgz_scan, dim3((n_cand + DECODE_LANES - 1) / DECODE_LANES), dim3(64), 0, ctx->stream, d_raw, n_raw, d_cand_pos,
                       n_cand, d_info, (const uint32_t*)ctx->deflate_tab.p);
    LAUNCHCHK("k_dgz_scan");
    return GCI_OK;
}

extern "C" int gci_depth_gz_runs(gci_ctx* ctx, const uint8_t* d_raw, uint64_t n_raw, const gci_dgz_member* d_members, uint32_t n_members,
                                 gci_dgz_run* d_runs)
{
    if (!ctx || (n_members && (!d_raw || !d_members || !d_runs)) || n_members > (1u << 24)) return GCI_E_INVALID;   // (the grid of the expansion)
    ctx->dgz_members = 0;
    if (n_members == 0) return GCI_OK;
    GCI_TRY(gci_ensure(ctx, ctx->dgz_tiles, (size_t)n_members * MEMBER_TILES * sizeof(uint2)));
    HIPCHK(hipMemsetAsync(ctx->dgz_tiles.p, 0xFF, (size_t)n_members * MEMBER_TILES * sizeof(uint2), ctx->stream));
    hipLaunchKernelGGL(k_dgz_runs, dim3((n_members + DECODE_LANES - 1) / DECODE_LANES), dim3(64), 0, ctx->stream, d_raw, n_raw, d_members,
                       n_members, d_runs, (uint2*)ctx->dgz_tiles.p);
    LAUNCHCHK("k_dgz_runs");
    ctx->dgz_members = n_members;
    ctx->dgz_key = d_members;
    return GCI_OK;
}

extern "C" int gci_depth_gz_expand(gci_ctx* ctx, const gci_dgz_run* d_runs, const gci_dgz_member* d_members, uint32_t n_members,
                                   int32_t* d_track, uint64_t track_n)
{
    if (!ctx || (n_members && (!d_runs || !d_members || !d_track))) return GCI_E_INVALID;
    if (n_members == 0) return GCI_OK;
    if (ctx->dgz_members != n_members || ctx->dgz_key != d_members) return GCI_E_INVALID;    // not behind gci_depth_gz_runs over them
    hipLaunchKernelGGL(k_dgz_expand, dim3(n_members * MEMBER_TILES), dim3(BLOCK), 0, ctx->stream, d_runs, d_members,
                       (const uint2*)ctx->dgz_tiles.p, d_track, track_n);
    LAUNCHCHK("k_dgz_expand");
    return GCI_OK;
}
