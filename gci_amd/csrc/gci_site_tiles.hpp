// gci_site_tiles.hpp -- the site lister of k_clips.hip, k_indels.hip and k_mismatch.hip: K8's windows cut into 4096-element tiles, one
// workgroup each; which of a tile's elements lie inside the window and inside their contig; which of them are HOT (a predicate); the
// hot elements (clips, alleles) or the starts of the runs of hot elements (indels, mismatch) counted per tile, scanned, and written by rank; a
// wave per run that walks to its end and reduces what the site reports; and the host frame of a *_sites_size / _write pair.
//
//   k_sites_count<Hot, RUNS>        one workgroup per window tile, the coalesced mapping: lane t of round j takes the four elements at
//                                   (j * BLOCK + t) * 4, 16 bytes a track; one count per tile.  A RUN START is a hot element whose
//                                   predecessor is not hot, or outside the window, or outside the contig
//   k_sites_write<Hot, RUNS, Emit>  one workgroup per window tile, gone at once when the tile's count is 0 (nearly every tile of a
//                                   genome): a thread takes 16 consecutive elements, so ascending order is thread order; a workgroup
//                                   scan ranks them; Emit stores element q as site number `slot`, and names
//                                   its lister: LISTER (the memo's id), RUNS
//   k_site_runs_finish<Hot, Red>    one wave per site: forward from the start, 64 elements a round, to the first element that is not hot
//                                   or the end of the window or contig; Red says what of the run's elements the site keeps
//
// A predicate is a small struct passed by value: four(p), bit k set when element p + k is hot, from its own int4 loads (p a multiple
// of 4); load(q), what it reads of a single element, and is(v), whether that is hot -- one(q) is both.  Its members carry no
// __restrict__: nothing is stored through them or beside them before the last load.
#pragma once
#include "gci_ctx.hpp"

struct SiteTile {
    int64_t p0;                          // the tile's first element (a multiple of TILE)
    int64_t lo, hi;                      // the elements of the tile that are inside the window AND inside their contig
    int64_t run_lo, run_hi;              // ... of the whole track: where a run of this tile may begin and must end
    int64_t contig_off;
    int32_t contig;
};

// the windows of the context and the layout, as the kernels take them
struct SiteGrid {
    const gci_window* win;
    const int64_t* win_tile_first;
    const int64_t* off;
    const int64_t* len;
    const int64_t* tile_first;
    int32_t n_win, n_contigs;
};

// A tile lies in one contig, whose first element is a tile's first: contig_off <= p0.  So lo = max(p0, W.begin, contig_off) is
// max(p0, W.begin), what a lister that knows no runs (clips) needs, and run_lo costs it nothing.
__device__ __forceinline__ SiteTile site_tile_of(const SiteGrid& G, int64_t wt)
{
    SiteTile x;
    const int32_t w = contig_of_tile(G.win_tile_first, G.n_win, wt);
    const gci_window W = G.win[w];
    x.p0 = (W.begin / TILE + (wt - G.win_tile_first[w])) * TILE;
    x.contig = contig_of_tile(G.tile_first, G.n_contigs, x.p0 / TILE);
    x.contig_off = G.off[x.contig];
    x.run_lo = max(W.begin, x.contig_off);
    x.run_hi = min(W.end, x.contig_off + G.len[x.contig]);
    x.lo = max(x.p0, x.run_lo);
    x.hi = min(x.p0 + TILE, x.run_hi);
    return x;
}

// bit k: element p + k is one of the tile's (inside the window and the contig, not padding)
__device__ __forceinline__ uint32_t site_inside4(const SiteTile& x, int64_t p)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) m |= (p + k >= x.lo && p + k < x.hi) ? (1u << k) : 0u;
    return m;
}

// whether the element in front of q is hot AND of the same window and contig -- for the first element of a wave's stretch, which no
// neighbour lane holds; q - 1 may lie in the tile in front
template <class Hot>
__device__ __forceinline__ bool site_prev_hot(const Hot& hot, const SiteTile& x, int64_t q)
{
    if (q - 1 < x.run_lo || q - 1 >= x.run_hi) return false;
    return hot.one(q - 1);
}

// ---- the two predicates -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t site_ge4(const int4 a, const int4 b, int32_t min_reads)
{
    return ((a.x >= min_reads || b.x >= min_reads) ? 1u : 0u) | ((a.y >= min_reads || b.y >= min_reads) ? 2u : 0u) |
           ((a.z >= min_reads || b.z >= min_reads) ? 4u : 0u) | ((a.w >= min_reads || b.w >= min_reads) ? 8u : 0u);
}

struct HotEither {                       // either of two tracks reaches min_reads (clips: left, right; indels: del, ins)
    const int32_t* a;
    const int32_t* b;
    int32_t min_reads;
    __device__ __forceinline__ uint32_t four(int64_t p) const
    {
        return site_ge4(*reinterpret_cast<const int4*>(a + p), *reinterpret_cast<const int4*>(b + p), min_reads);
    }
    typedef int2 Val;                    // (a, b)
    __device__ __forceinline__ Val load(int64_t q) const { return make_int2(a[q], b[q]); }
    __device__ __forceinline__ bool is(Val v) const { return v.x >= min_reads || v.y >= min_reads; }
    __device__ __forceinline__ bool one(int64_t q) const { return is(load(q)); }
};

struct HotMismatch {                     // mismatch >= min_reads and mismatch / depth >= frac_ppm / 10^6, in 64 bits
    const int32_t* mm;
    const int32_t* depth;
    int32_t min_reads;
    int64_t frac_ppm;
    __device__ __forceinline__ bool hot(int32_t m, int32_t d) const { return m >= min_reads && (int64_t)m * 1000000ll >= frac_ppm * (int64_t)d; }
    __device__ __forceinline__ uint32_t four(int64_t p) const
    {
        const int4 m = *reinterpret_cast<const int4*>(mm + p), d = *reinterpret_cast<const int4*>(depth + p);
        return (hot(m.x, d.x) ? 1u : 0u) | (hot(m.y, d.y) ? 2u : 0u) | (hot(m.z, d.z) ? 4u : 0u) | (hot(m.w, d.w) ? 8u : 0u);
    }
    typedef int2 Val;                    // (mismatch, depth)
    __device__ __forceinline__ Val load(int64_t q) const { return make_int2(mm[q], depth[q]); }
    __device__ __forceinline__ bool is(Val v) const { return hot(v.x, v.y); }
    __device__ __forceinline__ bool one(int64_t q) const { return is(load(q)); }
};

// ---- count --------------------------------------------------------------------------------------------------------------------------
template <class Hot, bool RUNS>
__global__ __launch_bounds__(BLOCK) void k_sites_count(Hot hot, SiteGrid G, uint32_t* __restrict__ tile_cnt)
{
    __shared__ uint32_t part[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const SiteTile x = site_tile_of(G, blockIdx.x);
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t p = x.p0 + (int64_t)(j * BLOCK + t) * 4;
        uint32_t h = hot.four(p) & site_inside4(x, p);
        if (RUNS) {
            // the element in front of the lane's four: the lane below holds it, but for the wave's first lane
            uint32_t prev = (uint32_t)__shfl_up((int)(h >> 3), 1, 64);
            if (lane == 0) prev = site_prev_hot(hot, x, p) ? 1u : 0u;
            h &= ~((h << 1) | prev) & 0xFu;
        }
        n += (uint32_t)__builtin_popcount(h);
    }
    n = wave_sum<uint32_t>(n);
    if (lane == 0) part[wave] = n;
    __syncthreads();
    if (t == 0) {
        uint32_t all = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; w++) all += part[w];
        tile_cnt[blockIdx.x] = all;
    }
}

// ---- write --------------------------------------------------------------------------------------------------------------------------
template <class Hot, bool RUNS, class Emit>
__global__ __launch_bounds__(BLOCK) void k_sites_write(Hot hot, SiteGrid G, Emit emit, const uint32_t* __restrict__ tile_cnt,
                                                       const unsigned long long* __restrict__ tile_off, unsigned long long total)
{
    __shared__ uint32_t wtot[BLOCK / 64];
    if (tile_cnt[blockIdx.x] == 0) return;             // (the whole workgroup)
    const int t = threadIdx.x, lane = t & 63;
    const SiteTile x = site_tile_of(G, blockIdx.x);
    const int64_t p = x.p0 + (int64_t)t * 16;          // a thread's 16 consecutive elements: ascending order is thread order
    uint32_t h = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) h |= (hot.four(p + 4 * j) & site_inside4(x, p + 4 * j)) << (4 * j);
    if (RUNS) {
        uint32_t prev = (uint32_t)__shfl_up((int)(h >> 15), 1, 64);
        if (lane == 0) prev = site_prev_hot(hot, x, p) ? 1u : 0u;
        h &= ~((h << 1) | prev) & 0xFFFFu;
    }
    uint32_t all;
    const uint32_t pre = block_exclusive<uint32_t, BLOCK / 64>((uint32_t)__builtin_popcount(h), wtot, all);
    unsigned long long slot = tile_off[blockIdx.x] + pre;
    while (h) {                                        // (few: a genome has thousands of sites)
        const int k = __builtin_ctz(h);
        h &= h - 1u;
        if (slot < total) emit(slot, x, p + k);
        slot++;
    }
}

// ---- run finish ---------------------------------------------------------------------------------------------------------------------
// Site: contig, start, and in `end` where the run ends at the latest (k_sites_write's Emit left run_hi there).  Red: Acc init(), take(acc,
// v, e, q0) for element e of the run, of which the predicate has read v, wave(acc) over the 64 lanes, store(site, acc, q0) by lane 0.
template <class Hot, class Red, class Site>
__global__ __launch_bounds__(BLOCK) void k_site_runs_finish(Hot hot, Red red, const int64_t* __restrict__ off, Site* __restrict__ out,
                                                            unsigned long long total)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long i = (unsigned long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= total) return;                            // (the whole wave)
    Site s = out[i];
    const int64_t base = off[s.contig], lim = base + s.end, q0 = base + s.start;
    int64_t q = q0;                                    // (hot, and below lim)
    typename Red::Acc acc = red.init();
    for (;;) {
        const int64_t e = q + lane;
        const bool in = e < lim;
        const typename Hot::Val v = in ? hot.load(e) : typename Hot::Val();
        const unsigned long long cold = ~__ballot(in && hot.is(v));
        const int first = cold ? __builtin_ctzll(cold) : 64;                    // the run's elements of this round: the lanes below `first`
        if (lane < first) red.take(acc, v, e, q0);
        q += first;
        if (first < 64) break;
    }
    red.wave(acc);
    if (lane == 0) {
        s.end = (int32_t)(q - base);
        red.store(s, acc, q0);
        out[i] = s;
    }
}

// ---- the host frame -------------------------------------------------------------------------------------------------------------------
struct SiteTileScratch { uint32_t* cnt; unsigned long long* off; unsigned long long* blk; };     // carved out of ctx->site_tiles

static inline size_t site_tile_bytes(int64_t tiles) { return 8 * ((size_t)tiles + 1) + 8 * (scan_blocks((uint64_t)tiles) + 2) + 4 * (size_t)tiles; }

static inline SiteTileScratch site_tile_scratch(gci_ctx* ctx, int64_t tiles)
{
    SiteTileScratch s;
    uint8_t* p = (uint8_t*)ctx->site_tiles.p;
    s.off = (unsigned long long*)p; p += 8 * ((size_t)tiles + 1);
    s.blk = (unsigned long long*)p; p += 8 * (scan_blocks((uint64_t)tiles) + 2);
    s.cnt = (uint32_t*)p;
    return s;
}

static inline SiteGrid site_grid(const gci_ctx* ctx)
{
    SiteGrid G;
    G.win = (const gci_window*)ctx->win.p; G.win_tile_first = (const int64_t*)ctx->win_tile_first.p; G.n_win = (int32_t)ctx->win_n;
    G.off = (const int64_t*)ctx->d_off.p; G.len = (const int64_t*)ctx->d_len.p; G.tile_first = (const int64_t*)ctx->d_tile_first.p;
    G.n_contigs = ctx->n_contigs;
    return G;
}

static inline bool site_memo_same(const SiteMemo& a, const SiteMemo& b)
{
    for (int k = 0; k < 6; k++) if (a.track[k] != b.track[k]) return false;
    return a.lister == b.lister && a.min_reads == b.min_reads && a.frac == b.frac && a.n_windows == b.n_windows;
}

// What a *_sites_size export does once its own arguments are checked: the windows (none: every contig) become the context's -- which
// ends what any lister's size call measured before, ctx->site_tiles and ctx->site_memo being the one scratch and the one memo of all
// three --, a count per window tile, their scan, the total.  `ask` holds the arguments; the lister, epoch and total are set here.
// Emit, the type the write call stores with, names the lister: its LISTER goes into the memo, its RUNS chooses the count.
template <class Emit, class Hot>
static inline int site_size(gci_ctx* ctx, const Hot& hot, SiteMemo ask, const gci_window* h_windows, uint64_t* h_n_sites, const char* name)
{
    constexpr bool RUNS = Emit::RUNS;
    ask.lister = Emit::LISTER;
    if (ask.n_windows >= (1u << 31)) return GCI_E_INVALID;
    std::vector<gci_window> ws;
    if (!gci_site_windows(ctx, h_windows, ask.n_windows, ws)) return GCI_E_INVALID;
    ctx->site_memo.epoch = 0;
    *h_n_sites = 0;
    GCI_TRY(gci_set_windows(ctx, ws.data(), (uint32_t)ws.size()));
    ctx->win_flank = INT32_MIN;
    const int64_t tiles = ctx->win_tiles;
    if (tiles > 0x7FFFFFFFll) return GCI_E_INVALID;
    unsigned long long total = 0;
    if (tiles) {
        GCI_TRY(gci_ensure(ctx, ctx->site_tiles, site_tile_bytes(tiles)));
        const SiteTileScratch T = site_tile_scratch(ctx, tiles);
        hipLaunchKernelGGL((k_sites_count<Hot, RUNS>), dim3((uint32_t)tiles), dim3(BLOCK), 0, ctx->stream, hot, site_grid(ctx), T.cnt);
        LAUNCHCHK(name);
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, T.cnt, T.off, T.blk, tiles, true)));
        HIPCHK(hipMemcpyAsync(&total, T.off + tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ask.epoch = ctx->win_epoch; ask.total = total;
    ctx->site_memo = ask;
    *h_n_sites = total;
    return GCI_OK;
}

// ... and a *_sites_write export: GCI_E_INVALID when `ask` is not what the last size call of ANY lister measured on this context, or
// its windows are no longer the context's; then the sites by rank.  After GCI_OK ctx->site_memo.total sites lie in d_out (a total
// above 0 has tiles): what a run finish walks.
template <class Hot, class Emit>
static inline int site_write(gci_ctx* ctx, const Hot& hot, SiteMemo ask, const Emit& emit, const void* d_out, uint64_t cap, const char* name)
{
    constexpr bool RUNS = Emit::RUNS;
    ask.lister = Emit::LISTER;
    const SiteMemo& m = ctx->site_memo;
    if (!m.epoch || m.epoch != ctx->win_epoch || !site_memo_same(m, ask)) return GCI_E_INVALID;
    const unsigned long long total = m.total;
    if (total && !d_out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    const int64_t tiles = ctx->win_tiles;
    if (!tiles || !total) return GCI_OK;
    const SiteTileScratch T = site_tile_scratch(ctx, tiles);
    hipLaunchKernelGGL((k_sites_write<Hot, RUNS, Emit>), dim3((uint32_t)tiles), dim3(BLOCK), 0, ctx->stream, hot, site_grid(ctx), emit, T.cnt, T.off,
                       total);
    LAUNCHCHK(name);
    return GCI_OK;
}
