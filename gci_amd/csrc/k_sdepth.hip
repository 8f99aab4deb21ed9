// k_sdepth.hip -- the text of `samtools depth -a` (name '\t' position '\t' depth '\n', one line per base) to an int32 depth
// track: the line loop of utility/convert_samtools_depth.py:12-19, one Python strip().split('\t') per base there.  The sibling
// of k_depth_parse.hip and built the same way.
//
// The text is cut into tiles of 4096 bytes, and a line belongs to the tile that holds its FIRST byte.  Two passes and no chain
// between workgroups (the project's rule): pass 1 counts the lines of every tile, checks every line against the strict
// grammar and records a key for every line whose name differs from the name of the line in front of it; the host scans the
// counts (gci_dev_u32_scan_u64), turns the keys into segments and lays out the track; pass 2 writes the depth of every line.
//
// THE BOUND: a line, its '\n' included, has at most SD_LINE_MAX = 255 bytes; a longer one is outside the grammar.  Pass 1 stages
// 256 bytes in front of the tile and 256 behind it, so the line in front of the tile's first line (whose name that line is
// compared with) together with the '\n' in front of THAT, and a line that begins on the tile's last byte, are whole in LDS.  A
// name may then have 250 bytes; names of real assemblies have 4 to 40.
//
// THE GRAMMAR, decided here: name = 1 or more bytes 0x21 .. 0x7E; '\t'; position = [0-9]{1,10}; '\t'; depth = 0 or
// [1-9][0-9]{0,9} with a value <= INT32_MAX; then '\n' or the end of the text.  Everything samtools writes is inside it.  Bytes
// >= 0x7F are kept out of names because the reference decodes the file as UTF-8 and strip() removes Unicode blanks (U+0085,
// U+00A0, ...): what those do is the host's business (formats.depthfile.convert_samtools_lines).
//
// Both passes stage the tile with one 16-byte load per lane (256 lanes x 16 B = the tile; further lanes fetch the halo).  A lane
// owns 16 bytes; pass 1 owns their line STARTS (a 16-bit mask, ranked by a block prefix count, the start positions published
// in LDS by rank so that a line finds the one in front of it).  Pass 2 owns their line ENDS: the depth column is the digits in
// front of a '\n', so a line's value is read backwards from its end -- two or three bytes instead of the whole line -- and its
// index is the tile's first line + the '\n's in front of it in the tile - 1 (a line that began in an earlier tile: first line -
// 1).  16 bytes of halo in front are enough for that.  Values go to LDS by rank and are stored with consecutive lanes on
// consecutive lines: the track is written coalesced.
#include "gci_text_tiles.hpp"

namespace {

constexpr uint32_t SD_LINE_MAX = 255;              // bytes of a line with its '\n': the bound of the grammar
constexpr uint32_t IHALO = 256;                    // pass 1: bytes staged in front of and behind the tile
constexpr uint32_t PHALO = 16;                     // pass 2: bytes staged in front of the tile
constexpr uint32_t MAX_ENDS = TEXT_TILE / 6 + 4;   // valid text: every line but a last one without '\n' has >= 6 bytes

__device__ __forceinline__ bool name_end(uint32_t c) { return c == '\t' || c == '\n'; }

// the strict grammar of the line at LDS position p (global offset i)
__device__ __forceinline__ bool strict_line(const uint8_t* __restrict__ b, uint32_t p, uint64_t i, uint64_t n)
{
    const uint32_t lim = (uint32_t)(n - i < SD_LINE_MAX ? n - i : SD_LINE_MAX);      // bytes of the text this line may use
    uint32_t k = 0;
    while (k < lim && (uint32_t)b[p + k] - 0x21u <= 0x7Eu - 0x21u) k++;
    if (k == 0 || k >= lim || b[p + k] != '\t') return false;
    k++;
    uint32_t d = 0;
    while (k < lim && d < 11u && (uint32_t)b[p + k] - '0' <= 9u) { k++; d++; }
    if (d == 0 || d > 10u || k >= lim || b[p + k] != '\t') return false;
    k++;
    if (k >= lim) return false;
    const bool zero = b[p + k] == '0';
    uint64_t v = 0;
    d = 0;
    while (k < lim && d < 11u && (uint32_t)b[p + k] - '0' <= 9u) { v = v * 10u + ((uint32_t)b[p + k] - '0'); k++; d++; }
    if (d == 0 || d > 10u || (zero && d > 1u) || v > 0x7FFFFFFFull) return false;
    return i + k == n || (k < lim && b[p + k] == '\n');
}

// the names of the lines at LDS positions q < p are equal (p at global offset i).  A name ends in front of the first '\t' or
// '\n'; a name that has no end within the bound, or within the text, equals nothing.
__device__ __forceinline__ bool same_name(const uint8_t* __restrict__ b, uint32_t q, uint32_t p, uint64_t i, uint64_t n)
{
    const uint32_t lim = (uint32_t)(n - i < SD_LINE_MAX ? n - i : SD_LINE_MAX);
    for (uint32_t k = 0; k < lim; k++) {
        const uint32_t a = b[q + k], c = b[p + k];
        if (name_end(a) || name_end(c)) return name_end(a) && name_end(c);
        if (a != c) return false;
    }
    return false;
}

// the same against the caller's prev_name (the first line of the text)
__device__ __forceinline__ bool same_as_prev(const uint8_t* __restrict__ b, uint32_t p, uint64_t n, const uint8_t* __restrict__ prev,
                                             uint32_t prev_len)
{
    const uint32_t lim = (uint32_t)(n < SD_LINE_MAX ? n : SD_LINE_MAX);
    for (uint32_t k = 0; k < lim; k++) {
        const uint32_t c = b[p + k];
        if (k >= prev_len || name_end(c)) return k >= prev_len && name_end(c);
        if (prev[k] != c) return false;
    }
    return false;
}

__global__ __launch_bounds__(TEXT_BLOCK) void k_sdepth_index(const uint8_t* __restrict__ text, uint64_t n, const uint8_t* __restrict__ prev,
                                                             uint32_t prev_len, uint32_t* __restrict__ tile_lines,
                                                             unsigned long long* __restrict__ keys, uint32_t cap, uint32_t* __restrict__ n_keys,
                                                             unsigned long long* __restrict__ bad)
{
    __shared__ TileText<IHALO, IHALO> s;
    __shared__ uint16_t s_start[TEXT_TILE];          // LDS position of the tile's line starts, by rank
    __shared__ uint32_t wtot[TEXT_BLOCK / 64];
    const int t = threadIdx.x;
    const uint64_t tile0 = stage_tile(text, n, s);
    const uint8_t* b = s.bytes();
    const uint32_t p0 = IHALO + 16u * t;
    const uint64_t at = tile0 + 16u * t;
    const uint32_t mask = line_starts(b + IHALO, tile0, n);
    uint32_t total;
    const uint32_t rank0 = block_exclusive<uint32_t, TEXT_BLOCK / 64>((uint32_t)__builtin_popcount(mask), wtot, total);
    if (t == 0) tile_lines[blockIdx.x] = total;
    uint32_t rank = rank0;
    for (uint32_t m = mask; m; m &= m - 1u, rank++) s_start[rank] = (uint16_t)(p0 + (uint32_t)__builtin_ctz(m));
    __syncthreads();
    rank = rank0;
    for (uint32_t m = mask; m; m &= m - 1u, rank++) {
        const uint32_t k = (uint32_t)__builtin_ctz(m);
        const uint32_t p = p0 + k;
        const uint64_t i = at + k;
        if (!strict_line(b, p, i, n)) atomicMin(bad, (unsigned long long)i);
        bool same;
        if (i == 0) {
            same = same_as_prev(b, p, n, prev, prev_len);
        } else {
            // the start of the line in front: by rank inside the tile, by a walk back through the halo for the tile's first
            // line.  Farther away than the bound: that line is outside the grammar, and nothing equals it.
            uint32_t q = 0xFFFFFFFFu;
            if (rank > 0) {
                q = s_start[rank - 1];
            } else {
                const uint32_t back = (uint32_t)(i < SD_LINE_MAX + 1u ? i : SD_LINE_MAX + 1u);
                for (uint32_t d = 2; d <= back; d++)
                    if (b[p - d] == '\n') { q = p - d + 1; break; }
                if (q == 0xFFFFFFFFu && i <= SD_LINE_MAX) q = p - (uint32_t)i;      // (the first line of the text)
            }
            same = q != 0xFFFFFFFFu && p - q <= SD_LINE_MAX && same_name(b, q, p, i, n);
        }
        if (!same) push_key(keys, cap, n_keys, i, rank);
    }
}

__global__ __launch_bounds__(TEXT_BLOCK) void k_sdepth_parse(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ tile_line0,
                                                             uint64_t line_base, const int64_t* __restrict__ segs, uint32_t n_segs,
                                                             int32_t* __restrict__ track, uint64_t track_n)
{
    __shared__ TileText<PHALO, 0> s;
    __shared__ int32_t s_val[MAX_ENDS];
    __shared__ int64_t s_dst[MAX_ENDS];
    __shared__ uint32_t wtot[TEXT_BLOCK / 64];
    __shared__ int32_t s_seg0;
    const int t = threadIdx.x;
    const uint64_t tile0 = stage_tile(text, n, s);
    const uint8_t* b = s.bytes();
    // the line that holds the tile's first byte: the first line of the tile if it begins there, else the one in front of it
    const bool begins = tile0 == 0 || b[PHALO - 1] == '\n';
    const uint64_t g0 = line_base + tile_line0[blockIdx.x] - (begins ? 0u : 1u);
    if (t == 0) s_seg0 = seg_search(segs, n_segs, g0);
    const uint32_t p0 = PHALO + 16u * t;
    const uint64_t at = tile0 + 16u * t;
    // line ends among this lane's bytes: a '\n' (the digits end in front of it), and the text's last byte when it is no '\n'
    // (the digits end on it).  nl: the '\n's alone -- they are what separates the lines in front of an end from it.
    uint32_t ends = 0, nl = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const bool in = at + k < n;
        const bool isnl = in && b[p0 + k] == '\n';
        nl |= isnl ? (1u << k) : 0u;
        ends |= (isnl || (in && at + k + 1 == n)) ? (1u << k) : 0u;
    }
    // (a line end with r '\n's of the tile in front of it closes line g0 + r)
    uint32_t total_nl;
    const uint32_t before = block_exclusive<uint32_t, TEXT_BLOCK / 64>((uint32_t)__builtin_popcount(nl), wtot, total_nl);   // (its barrier also publishes s_seg0)
    int32_t seg = s_seg0;
    const uint32_t total_ends = total_nl + ((tile0 + TEXT_TILE >= n && n && text[n - 1] != '\n') ? 1u : 0u);
    for (uint32_t m = ends; m; m &= m - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctz(m);
        const uint32_t r = before + (uint32_t)__builtin_popcount(nl & ((1u << k) - 1u));
        const uint64_t g = g0 + r;
        uint32_t e = p0 + k;                         // one behind the last digit
        if (!((nl >> k) & 1u)) e++;
        seg_advance(segs, n_segs, seg, g);
        const int64_t dst = seg_dest(segs, seg, g, track_n);
        uint32_t v = 0, mul = 1;
        if (dst >= 0) {                              // backwards from the line end
            for (uint32_t d = 1; d <= 10u && d <= e; d++) {
                const uint32_t c = (uint32_t)b[e - d] - '0';
                if (c > 9u) break;
                v += c * mul;
                mul *= 10u;
            }
        }
        rank_put<MAX_ENDS>(s_val, s_dst, r, (int32_t)v, dst, track);
    }
    rank_flush<MAX_ENDS>(s_val, s_dst, total_ends, track);
}

}  // namespace

extern "C" int gci_sdepth_index(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint8_t* d_prev_name, uint32_t prev_len,
                                uint32_t* d_tile_lines, uint64_t* d_keys, uint32_t cap, uint32_t* d_n_keys, uint64_t* d_bad)
{
    if (!ctx || !d_n_keys || !d_bad || (n_bytes && (!d_text || !d_tile_lines)) || (cap && !d_keys) || (prev_len && !d_prev_name) ||
        prev_len > SD_LINE_MAX || ((uintptr_t)d_text & 15u))
        return GCI_E_INVALID;
    HIPCHK(hipMemsetAsync(d_n_keys, 0, 4, ctx->stream));
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
    if (!n_bytes) return GCI_OK;
    const int64_t tiles = text_tiles(n_bytes, true);
    if (tiles < 0) return GCI_E_INVALID;
    hipLaunchKernelGGL(k_sdepth_index, dim3((uint32_t)tiles), dim3(TEXT_BLOCK), 0, ctx->stream, d_text, n_bytes, d_prev_name, prev_len,
                       d_tile_lines, (unsigned long long*)d_keys, cap, d_n_keys, (unsigned long long*)d_bad);
    LAUNCHCHK("k_sdepth_index");
    return GCI_OK;
}

extern "C" int gci_sdepth_parse(gci_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_tile_line0, uint64_t line_base,
                                const int64_t* d_segs, uint32_t n_segs, int32_t* d_track, uint64_t track_n)
{
    if (!ctx || (n_bytes && (!d_text || !d_tile_line0)) || (n_segs && !d_segs) || (track_n && !d_track) || ((uintptr_t)d_text & 15u))
        return GCI_E_INVALID;
    if (!n_bytes || !n_segs || !track_n) return GCI_OK;
    const int64_t tiles = text_tiles(n_bytes, false);
    if (tiles < 0) return GCI_E_INVALID;
    hipLaunchKernelGGL(k_sdepth_parse, dim3((uint32_t)tiles), dim3(TEXT_BLOCK), 0, ctx->stream, d_text, n_bytes, d_tile_line0, line_base,
                       d_segs, n_segs, d_track, track_n);
    LAUNCHCHK("k_sdepth_parse");
    return GCI_OK;
}
