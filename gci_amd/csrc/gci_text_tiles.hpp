// gci_text_tiles.hpp -- the scaffold of the kernels that read line-oriented text into a depth track (k_depth_parse.hip,
// k_sdepth.hip).  The text is cut into tiles of TEXT_TILE bytes, one workgroup of TEXT_BLOCK threads per tile, and a line belongs
// to the tile that holds its FIRST byte.  A lane owns 16 bytes of the tile.  Here: staging the tile with its halos in LDS, the
// lane's line starts, the key an index pass records for a line, the segment a line falls into and its element of the track, and
// the store of (value, element) by rank that lets consecutive lanes write consecutive elements.  The grammars, and which end of
// a line a value is read from, stay with the kernels.
#pragma once
#include "gci_ctx.hpp"

constexpr int TEXT_BLOCK = 256;
constexpr uint32_t TEXT_TILE = 4096;               // bytes per tile (as k_fasta_n_scan)
static_assert(TEXT_TILE == 16u * TEXT_BLOCK, "a lane owns 16 bytes of the tile");

// 16 bytes of the text at offset `at`; bytes outside [0, n) read as zero
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ text, uint64_t n, int64_t at)
{
    if (at >= 0 && (uint64_t)at + 16 <= n) return *reinterpret_cast<const uint4*>(text + at);
    union { uint4 v; uint8_t b[16]; } u;
    for (int k = 0; k < 16; k++) u.b[k] = (at + k >= 0 && (uint64_t)(at + k) < n) ? text[at + k] : (uint8_t)0;
    return u.v;
}

// A tile in LDS with FRONT bytes of the text in front of it and BACK bytes behind it (multiples of 16): byte FRONT + k of
// bytes() is byte k of the tile.
template <uint32_t FRONT, uint32_t BACK>
struct TileText {
    static_assert(FRONT % 16u == 0 && BACK % 16u == 0 && FRONT + BACK <= 16u * TEXT_BLOCK, "halos are whole 16-byte pieces, a lane each");
    uint4 v[(FRONT + TEXT_TILE + BACK) / 16];
    __device__ __forceinline__ const uint8_t* bytes() const { return reinterpret_cast<const uint8_t*>(v); }
};

// Stage the tile of this workgroup: every lane its 16 bytes, the first FRONT / 16 lanes the halo in front, the next BACK / 16
// the halo behind.  Ends with a barrier.  Returns the tile's first byte offset.
template <uint32_t FRONT, uint32_t BACK>
__device__ __forceinline__ uint64_t stage_tile(const uint8_t* __restrict__ text, uint64_t n, TileText<FRONT, BACK>& s)
{
    constexpr int NF = FRONT / 16, NB = BACK / 16;
    const int t = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * TEXT_TILE;
    s.v[NF + t] = load16(text, n, (int64_t)(tile0 + 16u * t));
    if (t < NF) s.v[t] = load16(text, n, (int64_t)tile0 - (int64_t)FRONT + 16 * t);
    else if (t < NF + NB) s.v[(FRONT + TEXT_TILE) / 16 + (t - NF)] = load16(text, n, (int64_t)(tile0 + TEXT_TILE) + 16 * (t - NF));
    __syncthreads();
    return tile0;
}

// the line starts among this lane's 16 bytes (bit k: byte 16 t + k of the tile); b = the tile's first byte in LDS, FRONT >= 1
__device__ __forceinline__ uint32_t line_starts(const uint8_t* b, uint64_t tile0, uint64_t n)
{
    b += 16u * threadIdx.x;
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

// an index pass records the line at byte offset i, the rank-th of its tile: offset << 12 | rank (rank < 4096; the host sorts
// the keys, so their order of arrival does not matter)
__device__ __forceinline__ void push_key(unsigned long long* __restrict__ keys, uint32_t cap, uint32_t* __restrict__ n_keys, uint64_t i,
                                         uint32_t rank)
{
    const uint32_t slot = atomicAdd(n_keys, 1u);
    if (slot < cap) keys[slot] = ((unsigned long long)i << 12) | rank;
}

// Segments are (first line, lines, first element of the track or -1) triples, sorted by first line.
// The last segment whose first line is at or before `line`, or -1.
__device__ __forceinline__ int32_t seg_search(const int64_t* __restrict__ segs, uint32_t n_segs, uint64_t line)
{
    uint32_t lo = 0, hi = n_segs;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)segs[3 * mid] <= line) lo = mid + 1; else hi = mid; }
    return (int32_t)lo - 1;
}

// ... moved on to line g >= the line `seg` was found for
__device__ __forceinline__ void seg_advance(const int64_t* __restrict__ segs, uint32_t n_segs, int32_t& seg, uint64_t g)
{
    while (seg + 1 < (int32_t)n_segs && (uint64_t)segs[3 * (seg + 1)] <= g) seg++;
}

// the element of the track line g goes to, or -1: in front of every segment, behind the lines of its segment, a segment the
// host dropped, or outside the track
__device__ __forceinline__ int64_t seg_dest(const int64_t* __restrict__ segs, int32_t seg, uint64_t g, uint64_t track_n)
{
    if (seg < 0) return -1;
    const int64_t first = segs[3 * seg], cnt = segs[3 * seg + 1], base = segs[3 * seg + 2];
    if (!(base >= 0 && (int64_t)g >= first && (int64_t)g < first + cnt)) return -1;
    const int64_t e = base + ((int64_t)g - first);
    return (uint64_t)e < track_n ? e : -1;
}

// (value, element) of the tile's lines by rank in LDS, then consecutive lanes store consecutive lines: the track is written
// coalesced.  The caller owns val[CAP] and dst[CAP] (LDS); CAP = the lines a tile of text inside the grammar can hold, and what
// a tile has beyond that goes straight to memory.
template <uint32_t CAP>
__device__ __forceinline__ void rank_put(int32_t* s_val, int64_t* s_dst, uint32_t r, int32_t val, int64_t dst, int32_t* __restrict__ track)
{
    if (r < CAP) { s_val[r] = val; s_dst[r] = dst; }
    else if (dst >= 0) track[dst] = val;             // (only text outside the grammar has this many lines in a tile)
}

// after every rank_put of the workgroup (the barrier is inside); total = the lines of the tile
template <uint32_t CAP>
__device__ __forceinline__ void rank_flush(const int32_t* s_val, const int64_t* s_dst, uint32_t total, int32_t* __restrict__ track)
{
    __syncthreads();
    const uint32_t staged = total < CAP ? total : CAP;
    for (uint32_t r = threadIdx.x; r < staged; r += TEXT_BLOCK) {
        const int64_t dst = s_dst[r];
        if (dst >= 0) track[dst] = s_val[r];
    }
}

// host side: the tiles of a text, or -1 when a grid does not hold them (keyed: or an offset does not fit a key)
static inline int64_t text_tiles(uint64_t n_bytes, bool keyed)
{
    const uint64_t tiles = (n_bytes + TEXT_TILE - 1) / TEXT_TILE;
    return (tiles > 0x7FFFFFFFull || (keyed && (n_bytes >> 51))) ? -1 : (int64_t)tiles;
}
