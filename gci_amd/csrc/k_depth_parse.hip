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
#include "gci_text_tiles.hpp"

namespace {

constexpr uint32_t HALO = 16;                      // bytes staged in front of and behind the tile
constexpr uint32_t MAX_LINES = TEXT_TILE / 2 + 1;  // valid text: every line but a last one without '\n' has >= 2 bytes

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

__global__ __launch_bounds__(TEXT_BLOCK) void k_depth_text_index(const uint8_t* __restrict__ text, uint64_t n,
                                                                 uint32_t* __restrict__ tile_lines, unsigned long long* __restrict__ keys,
                                                                 uint32_t cap, uint32_t* __restrict__ n_hdr,
                                                                 unsigned long long* __restrict__ bad)
{
    __shared__ TileText<HALO, HALO> s;
    __shared__ uint32_t wtot[TEXT_BLOCK / 64];
    const uint64_t tile0 = stage_tile(text, n, s);
    const uint8_t* b = s.bytes();
    const uint32_t mask = line_starts(b + HALO, tile0, n);
    uint32_t total;
    uint32_t rank = block_exclusive<uint32_t, TEXT_BLOCK / 64>((uint32_t)__builtin_popcount(mask), wtot, total);
    if (threadIdx.x == 0) tile_lines[blockIdx.x] = total;
    for (uint32_t m = mask; m; m &= m - 1u, rank++) {
        const uint32_t k = (uint32_t)__builtin_ctz(m);
        const uint32_t p = HALO + 16u * threadIdx.x + k;
        const uint64_t i = tile0 + 16u * threadIdx.x + k;
        if (b[p] == '>') push_key(keys, cap, n_hdr, i, rank);
        else if (strict_value(b, p, i, n) < 0) atomicMin(bad, (unsigned long long)i);
    }
}

__global__ __launch_bounds__(TEXT_BLOCK) void k_depth_text_parse(const uint8_t* __restrict__ text, uint64_t n,
                                                                 const uint64_t* __restrict__ tile_line0, const int64_t* __restrict__ segs,
                                                                 uint32_t n_segs, int32_t* __restrict__ track, uint64_t track_n)
{
    __shared__ TileText<HALO, HALO> s;
    __shared__ int32_t s_val[MAX_LINES];
    __shared__ int64_t s_dst[MAX_LINES];
    __shared__ uint32_t wtot[TEXT_BLOCK / 64];
    __shared__ int32_t s_seg0;
    const uint64_t tile0 = stage_tile(text, n, s);
    const uint64_t line0 = tile_line0[blockIdx.x];
    if (threadIdx.x == 0) s_seg0 = seg_search(segs, n_segs, line0);     // (segments begin with their first data line)
    const uint8_t* b = s.bytes();
    const uint32_t mask = line_starts(b + HALO, tile0, n);
    uint32_t total;
    uint32_t rank = block_exclusive<uint32_t, TEXT_BLOCK / 64>((uint32_t)__builtin_popcount(mask), wtot, total);   // (its barrier also publishes s_seg0)
    int32_t seg = s_seg0;
    for (uint32_t m = mask; m; m &= m - 1u, rank++) {
        const uint32_t k = (uint32_t)__builtin_ctz(m);
        const uint32_t p = HALO + 16u * threadIdx.x + k;
        const uint64_t i = tile0 + 16u * threadIdx.x + k;
        const uint64_t g = line0 + rank;
        seg_advance(segs, n_segs, seg, g);
        const int64_t dst = b[p] != '>' ? seg_dest(segs, seg, g, track_n) : -1;
        uint32_t v = 0;
        if (dst >= 0) {                              // forwards from the line start
            for (uint32_t d = 0; d < 10u && i + d < n; d++) {
                const uint32_t c = (uint32_t)b[p + d] - '0';
                if (c > 9u) break;
                v = v * 10u + c;
            }
        }
        rank_put<MAX_LINES>(s_val, s_dst, rank, (int32_t)v, dst, track);
    }
    rank_flush<MAX_LINES>(s_val, s_dst, total, track);
}

}  // namespace

extern "C" int gci_depth_text_index(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t* d_tile_lines, uint64_t* d_hdr_keys,
                                    uint32_t cap, uint32_t* d_n_hdr, uint64_t* d_bad)
{
    if (!ctx || !d_n_hdr || !d_bad || (n_bytes && (!d_text || !d_tile_lines)) || (cap && !d_hdr_keys)) return GCI_E_INVALID;
    HIPCHK(hipMemsetAsync(d_n_hdr, 0, 4, ctx->stream));
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
    if (!n_bytes) return GCI_OK;
    const int64_t tiles = text_tiles(n_bytes, true);
    if (tiles < 0) return GCI_E_INVALID;
    hipLaunchKernelGGL(k_depth_text_index, dim3((uint32_t)tiles), dim3(TEXT_BLOCK), 0, ctx->stream, d_text, n_bytes, d_tile_lines,
                       (unsigned long long*)d_hdr_keys, cap, d_n_hdr, (unsigned long long*)d_bad);
    LAUNCHCHK("k_depth_text_index");
    return GCI_OK;
}

extern "C" int gci_depth_text_parse(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_tile_line0, const int64_t* d_segs,
                                    uint32_t n_segs, int32_t* d_track, uint64_t track_n)
{
    if (!ctx || (n_bytes && (!d_text || !d_tile_line0)) || (n_segs && !d_segs) || (track_n && !d_track)) return GCI_E_INVALID;
    if (!n_bytes || !n_segs || !track_n) return GCI_OK;
    const int64_t tiles = text_tiles(n_bytes, false);
    if (tiles < 0) return GCI_E_INVALID;
    hipLaunchKernelGGL(k_depth_text_parse, dim3((uint32_t)tiles), dim3(TEXT_BLOCK), 0, ctx->stream, d_text, n_bytes, d_tile_line0, d_segs,
                       n_segs, d_track, track_n);
    LAUNCHCHK("k_depth_text_parse");
    return GCI_OK;
}
