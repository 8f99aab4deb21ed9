// k_bedgraph.hip -- depth_to_bedgraph.py: the maximal constant-depth runs of a set of windows over a depth track, IN ORDER, and
// their text as bedGraph lines  name '\t' start '\t' end '\t' depth '\n'.
//
// Runs.  K8's windows and tiling (gci_set_windows, one 4096-element tile per workgroup, int4 loads, one predecessor read per wave):
// element p of window [B, E) starts a run iff p == B or depth[p] != depth[p - 1].  K8 appends its rare boundaries with one atomic
// each, unordered; a 40x track has ~20 run starts per tile (10^7 in a genome), so here the count pass writes one number per tile
// (ballots and popcounts, no atomic), a device scan turns the numbers into every tile's first run index, and the write pass
// recomputes the flags, ranks them inside the workgroup and stores {start relative to the window, depth} at the run's global
// index: window after window, ascending inside a window, nothing to sort.
//
// Text.  A workgroup takes GCI_BG_RUNS_PER_BLOCK consecutive runs, a lane one run.  A run's window is found by an upper-bound
// search in the per-window run offsets (empty windows have equal offsets and are stepped over), its end is the next run's start or,
// behind the window's last run, the window's length.  The size pass sums the line lengths per workgroup, a 64-bit device scan makes
// byte offsets of them, and the write pass renders its lines into LDS and copies them out with K10's text_copy_out (16-byte stores
// where the destination is aligned, single bytes at head and tail).  Lines too long for the stage (names of hundreds of bytes) are
// rendered straight into memory.
#include "gci_ctx.hpp"

static_assert(GCI_BG_RUNS_PER_BLOCK == BLOCK, "a lane renders one run");
#define BG_STAGE 16384                   // LDS bytes of staging: 16 for the alignment shift + the lines of a block
#define BG_NAME_MAX 65535u

// ============================================================================================
// runs
// ============================================================================================

// the run-start flags (bit k: element p + k) of the four elements at p, which this lane loads into v
__device__ __forceinline__ uint32_t bg_flags4(const int32_t* __restrict__ depth, const gci_window W, int64_t p, int lane, int4& v)
{
    v = *reinterpret_cast<const int4*>(depth + p);
    int32_t prev = __shfl_up(v.w, 1, 64);
    if (lane == 0 && p > W.begin && p < W.end) prev = depth[p - 1];      // (p <= W.begin: element p is no later than the window's first, which starts a run by position)
    const int32_t d[4] = {v.x, v.y, v.z, v.w};
    uint32_t f = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t q = p + k;
        const bool in = q >= W.begin && q < W.end;
        const bool start = q == W.begin || d[k] != (k ? d[k - 1] : prev);
        f |= (in && start) ? (1u << k) : 0u;
    }
    return f;
}

__global__ __launch_bounds__(BLOCK) void k_bg_count(const int32_t* __restrict__ depth, const gci_window* __restrict__ win,
                                                    const int64_t* __restrict__ win_tile_first, int32_t n_win,
                                                    uint32_t* __restrict__ tile_cnt)
{
    __shared__ uint32_t part[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int32_t w = contig_of_tile(win_tile_first, n_win, blockIdx.x);
    const gci_window W = win[w];
    const int64_t p0 = (W.begin / TILE + ((int64_t)blockIdx.x - win_tile_first[w])) * TILE;
    uint32_t c = 0;                                                       // (the same in every lane of the wave)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int4 v;
        const uint32_t f = bg_flags4(depth, W, p0 + (int64_t)(j * BLOCK + t) * 4, lane, v);
#pragma unroll
        for (int k = 0; k < 4; k++) c += (uint32_t)__popcll(__ballot((f >> k) & 1u));
    }
    if (lane == 0) part[wave] = c;
    __syncthreads();
    if (t == 0) tile_cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(BLOCK) void k_bg_runs(const int32_t* __restrict__ depth, const gci_window* __restrict__ win,
                                                   const int64_t* __restrict__ win_tile_first, int32_t n_win,
                                                   const unsigned long long* __restrict__ tile_off, gci_depth_run* __restrict__ runs)
{
    __shared__ uint32_t wtot[4][BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int32_t w = contig_of_tile(win_tile_first, n_win, blockIdx.x);
    const gci_window W = win[w];
    const int64_t p0 = (W.begin / TILE + ((int64_t)blockIdx.x - win_tile_first[w])) * TILE;
    int4 v[4];
    uint32_t f[4], mine[4], inc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        f[j] = bg_flags4(depth, W, p0 + (int64_t)(j * BLOCK + t) * 4, lane, v[j]);
        mine[j] = (uint32_t)__popc(f[j]);
        inc[j] = (uint32_t)wave_inclusive_i32((int32_t)mine[j]);
    }
    if (lane == 63) {
#pragma unroll
        for (int j = 0; j < 4; j++) wtot[j][wave] = inc[j];
    }
    __syncthreads();
    // the tile's runs go to [tile_off[b], tile_off[b + 1]): the count pass's number, whatever the track holds by now
    unsigned long long at = tile_off[blockIdx.x];
    const unsigned long long end = tile_off[blockIdx.x + 1];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t pre = 0, all = 0;
#pragma unroll
        for (int x = 0; x < BLOCK / 64; x++) { const uint32_t s = wtot[j][x]; if (x < wave) pre += s; all += s; }
        unsigned long long o = at + pre + inc[j] - mine[j];
        const int64_t p = p0 + (int64_t)(j * BLOCK + t) * 4;
        const int32_t d[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((f[j] >> k) & 1u) {
                if (o < end) { gci_depth_run r; r.start = (uint32_t)(p + k - W.begin); r.depth = d[k]; runs[o] = r; }
                o++;
            }
        }
        at += all;
    }
}

// win_run0[w] = first run of window w = first run of its first tile; win_run0[n_win] = the total
__global__ void k_bg_win_run0(const unsigned long long* __restrict__ tile_off, const int64_t* __restrict__ win_tile_first, uint32_t n_win,
                              uint64_t* __restrict__ win_run0)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w <= n_win) win_run0[w] = tile_off[win_tile_first[w]];
}

// the windows as gci_set_windows clamps them
static inline gci_window bg_clamp(const gci_ctx* ctx, gci_window w)
{
    if (w.begin < 0) w.begin = 0;
    if (w.end > ctx->total) w.end = ctx->total;
    if (w.end < w.begin) w.end = w.begin;
    return w;
}

static int bg_read_u64(gci_ctx* ctx, const uint64_t* d_src, uint64_t* h_dst)
{
    HIPCHK(hipMemcpyAsync(h_dst, d_src, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GCI_OK;
}

extern "C" int gci_depth_runs_count(gci_ctx* ctx, const int32_t* d_depth, const gci_window* h_windows, uint32_t n_windows,
                                    uint64_t* d_win_run0)
{
    if (!ctx || !d_depth || !d_win_run0 || (n_windows && !h_windows)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    for (uint32_t i = 0; i < n_windows; i++) {
        const gci_window w = bg_clamp(ctx, h_windows[i]);
        if (w.end - w.begin > 0xFFFFFFFFll) return GCI_E_INVALID;        // (a run's start is a uint32)
    }
    ctx->bg_runs_epoch = 0;
    GCI_TRY(gci_set_windows(ctx, h_windows, n_windows));
    ctx->win_flank = INT32_MIN;
    const int64_t nt = ctx->win_tiles;
    if (nt > 0x7FFFFFFFll) return GCI_E_INVALID;
    uint64_t total = 0;
    if (nt == 0) {
        HIPCHK(hipMemsetAsync(d_win_run0, 0, (size_t)(n_windows + 1) * 8, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    } else {
        GCI_TRY(gci_ensure(ctx, ctx->bg_tile_cnt, (size_t)nt * 4));
        GCI_TRY(gci_ensure(ctx, ctx->bg_tile_off, (size_t)(nt + 1) * 8));
        GCI_TRY(gci_ensure(ctx, ctx->bg_blk, (size_t)(nt / TILE + 2) * 8));
        hipLaunchKernelGGL(k_bg_count, dim3((uint32_t)nt), dim3(BLOCK), 0, ctx->stream, d_depth, (const gci_window*)ctx->win.p,
                           (const int64_t*)ctx->win_tile_first.p, (int32_t)n_windows, (uint32_t*)ctx->bg_tile_cnt.p);
        LAUNCHCHK("k_bg_count");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, (const uint32_t*)ctx->bg_tile_cnt.p,
                                                                     (unsigned long long*)ctx->bg_tile_off.p,
                                                                     (unsigned long long*)ctx->bg_blk.p, nt, true)));
        hipLaunchKernelGGL(k_bg_win_run0, dim3((n_windows + 1 + 63) / 64), dim3(64), 0, ctx->stream,
                           (const unsigned long long*)ctx->bg_tile_off.p, (const int64_t*)ctx->win_tile_first.p, n_windows, d_win_run0);
        LAUNCHCHK("k_bg_win_run0");
        GCI_TRY(bg_read_u64(ctx, d_win_run0 + n_windows, &total));
    }
    ctx->bg_runs_epoch = ctx->win_epoch;
    ctx->bg_runs_total = total;
    ctx->bg_runs_track = d_depth;
    return GCI_OK;
}

extern "C" int gci_depth_runs_write(gci_ctx* ctx, const int32_t* d_depth, gci_depth_run* d_runs, uint64_t cap)
{
    if (!ctx || !d_depth || (cap && !d_runs)) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if (!ctx->bg_runs_epoch || ctx->bg_runs_epoch != ctx->win_epoch || ctx->bg_runs_track != d_depth) return GCI_E_INVALID;
    if (cap < ctx->bg_runs_total) return GCI_E_CAPACITY;
    if (ctx->bg_runs_total == 0) return GCI_OK;
    hipLaunchKernelGGL(k_bg_runs, dim3((uint32_t)ctx->win_tiles), dim3(BLOCK), 0, ctx->stream, d_depth, (const gci_window*)ctx->win.p,
                       (const int64_t*)ctx->win_tile_first.p, (int32_t)ctx->win_n, (const unsigned long long*)ctx->bg_tile_off.p, d_runs);
    LAUNCHCHK("k_bg_runs");
    return GCI_OK;
}

// ============================================================================================
// text
// ============================================================================================

struct BgWin {                           // a window as the text passes see it
    uint64_t len;                        // its elements
    int64_t coord0;                      // the contig coordinate of its first element
    uint64_t name_off;
    uint32_t name_len, pad;
};

struct BgLine { uint64_t start, end; uint64_t name_off; uint32_t name_len, len; int32_t depth; };

__device__ __forceinline__ uint32_t bg_depth_width(int32_t d)
{
    return d < 0 ? 1u + ndigits((uint32_t)(-(int64_t)d)) : ndigits((uint32_t)d);
}

// run r as a line: its window is the last one whose first run is at or before r (behind every empty window with the same offset)
__device__ __forceinline__ BgLine bg_line(const gci_depth_run* __restrict__ runs, const uint64_t* __restrict__ win_run0, uint32_t n_win,
                                          const BgWin* __restrict__ wtab, uint64_t r)
{
    uint32_t lo = 0, hi = n_win;         // invariant: win_run0[lo] <= r < win_run0[hi]
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (win_run0[mid] <= r) lo = mid; else hi = mid; }
    const BgWin W = wtab[lo];
    const gci_depth_run me = runs[r];
    const uint64_t rel_end = r + 1 < win_run0[lo + 1] ? (uint64_t)runs[r + 1].start : W.len;
    BgLine L;
    L.start = (uint64_t)W.coord0 + me.start;
    L.end = (uint64_t)W.coord0 + rel_end;
    L.name_off = W.name_off; L.name_len = W.name_len; L.depth = me.depth;
    L.len = W.name_len + 4u + ndigits64(L.start) + ndigits64(L.end) + bg_depth_width(me.depth);
    return L;
}

__device__ __forceinline__ void bg_render(uint8_t* p, const BgLine& L, const uint8_t* __restrict__ names)
{
    const uint8_t* nm = names + L.name_off;
    for (uint32_t i = 0; i < L.name_len; i++) p[i] = nm[i];
    p += L.name_len;
    *p++ = '\t';
    uint32_t w = ndigits64(L.start);
    put_dec64(p, L.start, w); p += w;
    *p++ = '\t';
    w = ndigits64(L.end);
    put_dec64(p, L.end, w); p += w;
    *p++ = '\t';
    uint64_t mag = (uint64_t)L.depth;
    if (L.depth < 0) { *p++ = '-'; mag = (uint64_t)(-(int64_t)L.depth); }
    w = ndigits((uint32_t)mag);
    put_dec64(p, mag, w); p += w;
    *p = '\n';
}

__global__ __launch_bounds__(BLOCK) void k_bg_size(const gci_depth_run* __restrict__ runs, const uint64_t* __restrict__ win_run0,
                                                   uint32_t n_win, const BgWin* __restrict__ wtab, uint64_t n_runs,
                                                   uint32_t* __restrict__ blk_bytes)
{
    __shared__ uint32_t part[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t r = (uint64_t)blockIdx.x * GCI_BG_RUNS_PER_BLOCK + t;
    uint32_t len = r < n_runs ? bg_line(runs, win_run0, n_win, wtab, r).len : 0u;
    len = wave_sum<uint32_t>(len);
    if (lane == 0) part[wave] = len;
    __syncthreads();
    if (t == 0) blk_bytes[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// win_byte0[w], one wave per entry: the offset of the block that holds window w's first run + the lines in front of it in that block
__global__ __launch_bounds__(BLOCK) void k_bg_win_byte0(const gci_depth_run* __restrict__ runs, const uint64_t* __restrict__ win_run0,
                                                        uint32_t n_win, const BgWin* __restrict__ wtab, uint64_t n_runs,
                                                        const unsigned long long* __restrict__ blk_off, uint64_t n_blocks,
                                                        uint64_t* __restrict__ win_byte0)
{
    const int lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (w > n_win) return;
    const uint64_t r = win_run0[w];
    if (r >= n_runs) { if (lane == 0) win_byte0[w] = blk_off[n_blocks]; return; }
    const uint64_t b = r / GCI_BG_RUNS_PER_BLOCK;
    uint32_t s = 0;
    for (uint64_t i = b * GCI_BG_RUNS_PER_BLOCK + lane; i < r; i += 64) s += bg_line(runs, win_run0, n_win, wtab, i).len;
    s = wave_sum<uint32_t>(s);
    if (lane == 0) win_byte0[w] = blk_off[b] + s;
}

__global__ __launch_bounds__(BLOCK) void k_bg_text(const gci_depth_run* __restrict__ runs, const uint64_t* __restrict__ win_run0,
                                                   uint32_t n_win, const BgWin* __restrict__ wtab, const uint8_t* __restrict__ names,
                                                   uint64_t n_runs, const unsigned long long* __restrict__ blk_off,
                                                   uint8_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[BG_STAGE];
    __shared__ uint32_t wtot[BLOCK / 64];
    const int t = threadIdx.x;
    const uint64_t r = (uint64_t)blockIdx.x * GCI_BG_RUNS_PER_BLOCK + t;
    BgLine L;
    L.len = 0;
    if (r < n_runs) L = bg_line(runs, win_run0, n_win, wtab, r);
    uint32_t total;
    const uint32_t pre = block_exclusive<uint32_t, BLOCK / 64>(L.len, wtot, total);
    const unsigned long long dst = blk_off[blockIdx.x];
    if ((unsigned long long)total != blk_off[blockIdx.x + 1] - dst) return;      // not the runs the size pass measured: write nothing
    if (total + 16u <= BG_STAGE) {
        const uint32_t shift = (uint32_t)((uintptr_t)(out + dst) & 15u);
        if (L.len) bg_render(stage + shift + pre, L, names);
        __syncthreads();
        text_copy_out(out + dst, stage, shift, total, t);
    } else if (L.len) {
        bg_render(out + dst + pre, L, names);
    }
}

// the window table of the text passes on the device (h_name_off == nullptr: the size pass, which needs the lengths alone)
static int bg_upload_wtab(gci_ctx* ctx, const gci_window* h_windows, uint32_t n_windows, const int64_t* h_coord0,
                          const uint64_t* h_name_off, const uint32_t* h_name_len)
{
    std::vector<BgWin> tab(n_windows);
    for (uint32_t i = 0; i < n_windows; i++) {
        const gci_window w = bg_clamp(ctx, h_windows[i]);
        if (w.end - w.begin > 0xFFFFFFFFll || h_coord0[i] < 0 || h_name_len[i] > BG_NAME_MAX) return GCI_E_INVALID;
        tab[i].len = (uint64_t)(w.end - w.begin);
        tab[i].coord0 = h_coord0[i];
        tab[i].name_off = h_name_off ? h_name_off[i] : 0;
        tab[i].name_len = h_name_len[i];
        tab[i].pad = 0;
    }
    GCI_TRY(gci_ensure(ctx, ctx->bg_wtab, (size_t)(n_windows + 1) * sizeof(BgWin)));
    if (n_windows) GCI_TRY(gci_upload_small(ctx, ctx->bg_wtab.p, tab.data(), (size_t)n_windows * sizeof(BgWin)));
    return GCI_OK;
}

extern "C" int gci_bedgraph_size(gci_ctx* ctx, const gci_depth_run* d_runs, const uint64_t* d_win_run0, const gci_window* h_windows,
                                 uint32_t n_windows, const int64_t* h_coord0, const uint32_t* h_name_len, uint64_t* d_win_byte0)
{
    if (!ctx || !d_win_run0 || !d_win_byte0 || (n_windows && (!h_windows || !h_coord0 || !h_name_len))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    ctx->bg_text_run0 = nullptr;
    uint64_t n_runs = 0;
    GCI_TRY(bg_read_u64(ctx, d_win_run0 + n_windows, &n_runs));
    if (n_runs && (!d_runs || !n_windows)) return GCI_E_INVALID;
    const uint64_t nb = (n_runs + GCI_BG_RUNS_PER_BLOCK - 1) / GCI_BG_RUNS_PER_BLOCK;
    if (nb > 0x7FFFFFFFull) return GCI_E_INVALID;
    GCI_TRY(bg_upload_wtab(ctx, h_windows, n_windows, h_coord0, nullptr, h_name_len));
    uint64_t total = 0;
    if (nb == 0) {
        HIPCHK(hipMemsetAsync(d_win_byte0, 0, (size_t)(n_windows + 1) * 8, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    } else {
        GCI_TRY(gci_ensure(ctx, ctx->bg_blk_bytes, (size_t)nb * 4));
        GCI_TRY(gci_ensure(ctx, ctx->bg_blk_off, (size_t)(nb + 1) * 8));
        GCI_TRY(gci_ensure(ctx, ctx->bg_blk2, (size_t)(nb / TILE + 2) * 8));
        hipLaunchKernelGGL(k_bg_size, dim3((uint32_t)nb), dim3(BLOCK), 0, ctx->stream, d_runs, d_win_run0, n_windows,
                           (const BgWin*)ctx->bg_wtab.p, n_runs, (uint32_t*)ctx->bg_blk_bytes.p);
        LAUNCHCHK("k_bg_size");
        GCI_TRY((device_exclusive_scan<uint32_t, unsigned long long>(ctx, (const uint32_t*)ctx->bg_blk_bytes.p,
                                                                     (unsigned long long*)ctx->bg_blk_off.p,
                                                                     (unsigned long long*)ctx->bg_blk2.p, (int64_t)nb, true)));
        hipLaunchKernelGGL(k_bg_win_byte0, dim3((n_windows + 1 + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, ctx->stream, d_runs,
                           d_win_run0, n_windows, (const BgWin*)ctx->bg_wtab.p, n_runs, (const unsigned long long*)ctx->bg_blk_off.p, nb,
                           d_win_byte0);
        LAUNCHCHK("k_bg_win_byte0");
        GCI_TRY(bg_read_u64(ctx, d_win_byte0 + n_windows, &total));
    }
    ctx->bg_text_runs = d_runs;
    ctx->bg_text_run0 = d_win_run0;
    ctx->bg_text_windows = n_windows;
    ctx->bg_text_n_runs = n_runs;
    ctx->bg_text_total = total;
    return GCI_OK;
}

extern "C" int gci_bedgraph_write(gci_ctx* ctx, const gci_depth_run* d_runs, const uint64_t* d_win_run0, const gci_window* h_windows,
                                  uint32_t n_windows, const int64_t* h_coord0, const uint8_t* d_names, const uint64_t* h_name_off,
                                  const uint32_t* h_name_len, uint8_t* d_out, uint64_t cap)
{
    if (!ctx || !d_win_run0 || (cap && !d_out) || (n_windows && (!h_windows || !h_coord0 || !h_name_off || !h_name_len))) return GCI_E_INVALID;
    if (!ctx->n_contigs) return GCI_E_NO_LAYOUT;
    if (!ctx->bg_text_run0 || ctx->bg_text_run0 != d_win_run0 || ctx->bg_text_runs != d_runs || ctx->bg_text_windows != n_windows)
        return GCI_E_INVALID;
    if (cap < ctx->bg_text_total) return GCI_E_CAPACITY;
    if (ctx->bg_text_n_runs == 0) return GCI_OK;
    for (uint32_t i = 0; i < n_windows; i++) if (h_name_len[i] && !d_names) return GCI_E_INVALID;
    GCI_TRY(bg_upload_wtab(ctx, h_windows, n_windows, h_coord0, h_name_off, h_name_len));
    const uint64_t nb = (ctx->bg_text_n_runs + GCI_BG_RUNS_PER_BLOCK - 1) / GCI_BG_RUNS_PER_BLOCK;
    hipLaunchKernelGGL(k_bg_text, dim3((uint32_t)nb), dim3(BLOCK), 0, ctx->stream, d_runs, d_win_run0, n_windows,
                       (const BgWin*)ctx->bg_wtab.p, d_names, ctx->bg_text_n_runs, (const unsigned long long*)ctx->bg_blk_off.p, d_out);
    LAUNCHCHK("k_bg_text");
    return GCI_OK;
}
