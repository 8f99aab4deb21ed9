// k_depth_parse.hip -- the text of a `.depth.gz` back to an int32 depth track: the parse of utility/GCI_score.py:11-39
// (parse_depth), one Python int() per base there.
//
// The text is ('>' name '\n' (decimal '\n')^L)*.  It is cut into tiles of 4096 bytes, and a line belongs to the tile that
// holds its FIRST byte: that tile parses it and reads past its own end where it must (a data line has at most 11 bytes, so 16
// bytes of halo are enough; a header line is only recorded, never read through).  Two passes and no chain between
// workgroups (the project's rule): pass 1 counts the lines of every tile, records the header lines and checks the
// strict grammar of the data lines; the host scans the counts (gci_dev_u32_scan_u64), resolves the headers into segments
// (repeated names: the last segment wins) and lays out the track; pass 2 ranks every line globally and writes its value.
//
// Both passes stage the tile in LDS with one 16-byte load per lane (256 lanes x 16 B = the tile; two lanes fetch the 16 bytes
// in front of it and the 16 behind it).  A lane owns 16 bytes: its line starts are a 16-bit mask, their rank in the tile a
// block prefix count (wave scan by DPP + the 4 wave totals).  Pass 2 puts (value, destination) of every line into LDS by rank and
// then stores the values with consecutive lanes on consecutive lines: the track is written coalesced.
#include "gci_ctx.hpp"

namespace {

constexpr int PBLOCK = 256;
constexpr uint32_t PTILE = 4096;                   // bytes per tile (as k_fasta_n_scan)
constexpr uint32_t HALO = 16;                      // bytes staged in front of and behind the tile
constexpr uint32_t MAX_LINES = PTILE / 2 + 1;      // valid text: every line but a last one without '\n' has >= 2 bytes

struct TileText {
    uint4 v[(HALO + PTILE + HALO) / 16];           // [0]: the 16 bytes in front of the tile, [1 .. 256]: the tile, [257]: behind
};

__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ text, uint64_t n, int64_t at)
{
    if (at >= 0 && (uint64_t)at + 16 <= n) return *reinterpret_cast<const uint4*>(text + at);
    union { uint4 v; uint8_t b[16]; } u;
    for (int k = 0; k < 16; k++) u.b[k] = (at + k >= 0 && (uint64_t)(at + k) < n) ? text[at + k] : (uint8_t)0;
    return u.v;
}

// stage the tile of this workgroup; returns the tile's first byte offset
__device__ __forceinline__ uint64_t stage_tile(const uint8_t* __restrict__ text, uint64_t n, TileText& s)
{
    const int t = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * PTILE;
    s.v[1 + t] = load16(text, n, (int64_t)(tile0 + 16u * t));
    if (t == 0) s.v[0] = load16(text, n, (int64_t)tile0 - 16);
    if (t == 1) s.v[1 + PBLOCK] = load16(text, n, (int64_t)(tile0 + PTILE));
    __syncthreads();
    return tile0;
}

__device__ __forceinline__ const uint8_t* bytes(const TileText& s) { return reinterpret_cast<const uint8_t*>(s.v); }

// the line starts among this lane's 16 bytes (bit k: byte 16 t + k of the tile)
__device__ __forceinline__ uint32_t line_starts(const TileText& s, uint64_t tile0, uint64_t n)
{
    const uint8_t* b = bytes(s) + HALO + 16u * threadIdx.x;
    const uint64_t at = tile0 + 16u * threadIdx.x;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const bool in = at + k < n;
        const bool start = (at + k == 0) || b[k - 1] == '\n';
        m |= (in && start) ? (1u << k) : 0u;
    }
    return m;
}

// exclusive prefix of `cnt` over the workgroup and the workgroup's total
__device__ __forceinline__ uint32_t block_exclusive(uint32_t cnt, uint32_t& total)
{
    __shared__ uint32_t part[PBLOCK / 64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const uint32_t inc = (uint32_t)wave_inclusive<int32_t>((int32_t)cnt, lane);
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < PBLOCK / 64; w++) { before += w < wave ? part[w] : 0u; all += part[w]; }
    total = all;
    return before + inc - cnt;
}

// strict grammar of a data line at LDS position p (global offset i): [0-9]{1,10} then '\n' or the end of the text, value
// <= INT32_MAX.  -> value, or -1 outside the grammar.
__device__ __forceinline__ int64_t strict_value(const uint8_t* __restrict__ b, uint32_t p, uint64_t i, uint64_t n)
{
    uint64_t v = 0;
    uint32_t d = 0;
    for (; d < 11u; d++) {
        if (i + d >= n) break;
        const uint32_t c = (uint32_t)b[p + d] - '0';
        if (c > 9u) break;
        v = v * 10u + c;
    }
    const bool closed = (i + d == n) || b[p + d] == '\n';
    return (d >= 1u && d <= 10u && closed && v <= 0x7FFFFFFFull) ? (int64_t)v : -1;
}

__global__ __launch_bounds__(PBLOCK) void k_depth_text_index(const uint8_t* __restrict__ text, uint64_t n,
                                                             uint32_t* __restrict__ tile_lines, unsigned long long* __restrict__ keys,
                                                             uint32_t cap, uint32_t* __restrict__ n_hdr,
                                                             unsigned long long* __restrict__ bad)
{
    __shared__ TileText s;
    const uint64_t tile0 = stage_tile(text, n, s);
    const uint32_t mask = line_starts(s, tile0, n);
    uint32_t total;
    uint32_t rank = block_exclusive((uint32_t)__builtin_popcount(mask), total);
    if (threadIdx.x == 0) tile_lines[blockIdx.x] = total;
    const uint8_t* b = bytes(s);
    for (uint32_t m = mask; m; m &= m - 1u, rank++) {
        const uint32_t k = (uint32_t)__builtin_ctz(m);
        const uint32_t p = HALO + 16u * threadIdx.x + k;
        const uint64_t i = tile0 + 16u * threadIdx.x + k;
        if (b[p] == '>') {
            const uint32_t slot = atomicAdd(n_hdr, 1u);
            if (slot < cap) keys[slot] = ((unsigned long long)i << 12) | rank;
        } else if (strict_value(b, p, i, n) < 0) {
            atomicMin(bad, (unsigned long long)i);
        }
    }
}

__global__ __launch_bounds__(PBLOCK) void k_depth_text_parse(const uint8_t* __restrict__ text, uint64_t n,
                                                             const uint64_t* __restrict__ tile_line0, const int64_t* __restrict__ segs,
                                                             uint32_t n_segs, int32_t* __restrict__ track, uint64_t track_n)
{
    __shared__ TileText s;
    __shared__ int32_t s_val[MAX_LINES];
    __shared__ int64_t s_dst[MAX_LINES];
    __shared__ int32_t s_seg0;
    const uint64_t tile0 = stage_tile(text, n, s);
    const uint64_t line0 = tile_line0[blockIdx.x];
    if (threadIdx.x == 0) {                          // the last segment whose first data line is at or before the tile's first line
        uint32_t lo = 0, hi = n_segs;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)segs[3 * mid] <= line0) lo = mid + 1; else hi = mid; }
        s_seg0 = (int32_t)lo - 1;
    }
    const uint32_t mask = line_starts(s, tile0, n);
    uint32_t total;
    uint32_t rank = block_exclusive((uint32_t)__builtin_popcount(mask), total);   // (its barrier also publishes s_seg0)
    const uint8_t* b = bytes(s);
    int32_t seg = s_seg0;
    for (uint32_t m = mask; m; m &= m - 1u, rank++) {
        const uint32_t k = (uint32_t)__builtin_ctz(m);
        const uint32_t p = HALO + 16u * threadIdx.x + k;
        const uint64_t i = tile0 + 16u * threadIdx.x + k;
        const uint64_t g = line0 + rank;
        while (seg + 1 < (int32_t)n_segs && (uint64_t)segs[3 * (seg + 1)] <= g) seg++;
        int64_t dst = -1;
        int32_t val = 0;
        if (b[p] != '>' && seg >= 0) {
            const int64_t first = segs[3 * seg], cnt = segs[3 * seg + 1], base = segs[3 * seg + 2];
            if (base >= 0 && (int64_t)g >= first && (int64_t)g < first + cnt) {
                uint32_t v = 0;
                for (uint32_t d = 0; d < 10u && i + d < n; d++) {
                    const uint32_t c = (uint32_t)b[p + d] - '0';
                    if (c > 9u) break;
                    v = v * 10u + c;
                }
                const int64_t e = base + ((int64_t)g - first);
                if ((uint64_t)e < track_n) { dst = e; val = (int32_t)v; }
            }
        }
        if (rank < MAX_LINES) { s_val[rank] = val; s_dst[rank] = dst; }
        else if (dst >= 0) track[dst] = val;         // (only text outside the grammar has this many lines in a tile)
    }
    __syncthreads();
    const uint32_t staged = total < MAX_LINES ? total : MAX_LINES;
    for (uint32_t r = threadIdx.x; r < staged; r += PBLOCK) {
        const int64_t dst = s_dst[r];
        if (dst >= 0) track[dst] = s_val[r];
    }
}

}  // namespace

extern "C" int gci_depth_text_index(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t* d_tile_lines, uint64_t* d_hdr_keys,
                                    uint32_t cap, uint32_t* d_n_hdr, uint64_t* d_bad)
{
    if (!ctx || !d_n_hdr || !d_bad || (n_bytes && (!d_text || !d_tile_lines)) || (cap && !d_hdr_keys)) return GCI_E_INVALID;
    HIPCHK(hipMemsetAsync(d_n_hdr, 0, 4, ctx->stream));
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
    if (!n_bytes) return GCI_OK;
    const uint64_t tiles = (n_bytes + PTILE - 1) / PTILE;
    if (tiles > 0x7FFFFFFFull || (n_bytes >> 51)) return GCI_E_INVALID;
    hipLaunchKernelGGL(k_depth_text_index, dim3((uint32_t)tiles), dim3(PBLOCK), 0, ctx->stream, d_text, n_bytes, d_tile_lines,
                       (unsigned long long*)d_hdr_keys, cap, d_n_hdr, (unsigned long long*)d_bad);
    LAUNCHCHK("k_depth_text_index");
    return GCI_OK;
}

extern "C" int gci_depth_text_parse(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_tile_line0, const int64_t* d_segs,
                                    uint32_t n_segs, int32_t* d_track, uint64_t track_n)
{
    if (!ctx || (n_bytes && (!d_text || !d_tile_line0)) || (n_segs && !d_segs) || (track_n && !d_track)) return GCI_E_INVALID;
    if (!n_bytes || !n_segs || !track_n) return GCI_OK;
    const uint64_t tiles = (n_bytes + PTILE - 1) / PTILE;
    if (tiles > 0x7FFFFFFFull) return GCI_E_INVALID;
    hipLaunchKernelGGL(k_depth_text_parse, dim3((uint32_t)tiles), dim3(PBLOCK), 0, ctx->stream, d_text, n_bytes, d_tile_line0, d_segs,
                       n_segs, d_track, track_n);
    LAUNCHCHK("k_depth_text_parse");
    return GCI_OK;
}
