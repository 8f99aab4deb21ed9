// gci_ctx.hpp -- internals shared by the translation units of libgci_hip.so: the context, the
// error / launch macros, the per-kernel HIP-event scopes and small device helpers.
//
// Everything on this path is integer, streaming or scatter work: no MFMA anywhere.  The bound is
// HBM bandwidth (depth build, issue scan, text), atomic rate (join) or instruction issue (record
// decode).  Wave = 64 lanes, 256-thread workgroups, 16-byte vector accesses, 4096-element
// (16 KiB) tiles that never straddle contigs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/gci_hip.h"
#include "gci_common.h"
#include "gci_wave.hpp"

#define TILE GCI_TILE
#define TEXT_LUT 1000                    // depths below this come out of a 4-byte-per-entry table
#define BLOCK 256
static_assert(TILE == BLOCK * 16, "a tile is 16 elements per thread");

constexpr int GCI_RUN_MAX = 64;                  // run lists of a tile (k_tile_build / k_depth_runs -> k_depth_deflate): entries per tile
constexpr uint32_t GCI_RUNS_WALK = 0xFFFFFFFFu;  // ... "not listed: walk the track"

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

// block totals a device_exclusive_scan over n entries needs (its callers add 2), and the grid of a kernel that gives every one of n
// items a wave
static inline size_t scan_blocks(uint64_t n) { return (size_t)((n + TILE - 1) / TILE); }
static inline dim3 wave_grid(unsigned long long n) { return dim3((uint32_t)((n + BLOCK / 64 - 1) / (BLOCK / 64))); }

// gci_site_tiles.hpp: what the last *_sites_size call of any lister measured, for the *_sites_write call that follows it
struct SiteMemo {
    int lister = 0;                         // the Emit type's LISTER: 1 clips, 2 indels, 3 mismatch, 4 alleles
    uint64_t epoch = 0, total = 0;          // ctx->win_epoch of its windows (0: no size call yet), its sites
    const void* track[6] = {};              // the arrays the call was given (alleles: A, C, G, T, depth, codes); the rest stay null
    int32_t min_reads = 0, frac = 0;
    uint32_t n_windows = 0;
};

struct gci_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // layout
    int32_t n_contigs = 0;
    std::vector<int64_t> len, off;          // host copies
    std::vector<int64_t> tile_first;        // n_contigs + 1
    int64_t total = 0, n_tiles = 0;
    DevBuf d_len, d_off, d_tile_first;      // int64 each
    // depth-build scratch (per tile unless noted)
    DevBuf tile_cd;                         // uint64 per tile: low word = events in the tile, high word = coarse
                                            // difference (int32); both return to zero by the end of a build
    DevBuf tile_carry;                      // int32: exclusive scan of the coarse difference = depth entering a tile
    DevBuf evt_off;                         // uint32: bucket offsets (n_tiles + 1)
    DevBuf d_tile_valid;                    // int32 per tile: elements of the tile inside its contig (TILE but for the last)
    DevBuf dense_flag;                      // uint8 per tile: pass 2 left it to the dense kernel
    DevBuf dense_list;                      // uint32: [0] = number of flagged tiles, [1 ..] their indices (k_dense_list)
    int32_t sparse_max = 62;                // tiles with more events take the dense path (GCI_FORCE_DENSE=1: all of them)
    bool join_dirty = false;                // the join tables are not in their clean state (a join was cut short)
    int join_mode = 0;                      // gci_join_mode: 0 by size, 1 classic table, 2 radix-partitioned
    uint32_t k1_parity = 0;                 // which of the two K1 counter sets the next gci_bam_filter uses
    int cd_state = 0;                       // tile_cd: 0 clean, 1 counted by gci_name_join_count, 2 in use / left over
    int counted_flank = 0;                  // the flank gci_name_join_count counted with
    bool count_deferred = false;            // cd_state == 1 without counts: the build buckets the events itself (gci_evp_wanted)
    DevBuf evp_items, evp_hist, evp_blk;    // large inputs: the events partitioned by tile range (k_evp_*)
    DevBuf events;                          // uint16 per event: local position << 1 | is_minus
    DevBuf blk_a, blk_b;                    // block totals of the two scans
    DevBuf tile_sum;                        // int64: sum of depth per tile
    DevBuf tile_u32, tile_u64, blk_u64;     // text bytes per tile, byte offsets (n_tiles + 1), block totals
    uint32_t build_max_n = 0;               // capacity the pending begin() was issued with
    int build_flank = 0;
    bool build_pending = false, build_text = false;
    bool build_runs_wanted = false;         // gci_build_opts.want_runs of the pending build
    DevBuf build_nruns, build_runs;         // ... per tile of the layout its constant-depth runs, as k_tile_build saw them
    const void* build_runs_track = nullptr; // ... and the track they describe (nullptr: none; cleared by whatever writes a track)
    bool build_runs_armed = false;          // ... gci_depth_deflate_from_build() has said that track is untouched: the next size / write pair may use them
    // join scratch
    DevBuf join_table, join_last, join_hq;
    DevBuf join_fate;                       // gci_name_join_fate: the counts of every (file, class), then a verdict byte per slot
    DevBuf join_bucket;                     // partitioned join: per bucket its survivor count, first slot and output offset
    DevBuf part_a, part_b, part_hist, part_blk;   // partitioned join: entry ping-pong, histograms + segment table, scan totals
    DevBuf route_tab;                       // gci_route_*: per (part, chunk) counts and their scan
    DevBuf deflate_nruns, deflate_runs;     // gci_depth_deflate_*: per tile its constant-depth runs (k_depth_runs)
    DevBuf deflate_tab;                     // ... the CRC tables of the size pass and of gci_depth_gz_scan (gci_crc_gf2.hpp: host_crc_tab)
    bool deflate_tab_ready = false;
    DevBuf dgz_tiles;                       // gci_depth_gz_runs -> _expand: per 4096 lines of a member the run they begin in
    uint32_t dgz_members = 0;               // ... of the members the last runs call decoded,
    const void* dgz_key = nullptr;          // ... in this member table
    bool deflate_from_build = false;        // ... the last size call took the lists of the build (build_runs) instead
    uint32_t deflate_members = 0;           // ... of the members the last size call measured,
    const void* deflate_key_depth = nullptr;    // ... over this track
    const void* deflate_key_elem = nullptr;     // ... and this member table (the write call reuses the lists only for the same three)
    DevBuf conflict_table;                  // gci_hash_conflicts' own open-addressing tables (two, used alternately)
    uint64_t conflict_slots = 0;            // slots per table
    uint32_t conflict_parity = 0;           // which one the next call inserts into (the other one is clean by then)
    DevBuf text_lut;                        // uint32[TEXT_LUT]: decimal characters of 0..999
    DevBuf long_items;                      // K1: queue of long-CIGAR records + its counter
    DevBuf pg_scan, pg_first;               // record pages: scans of the records' costs and blob bytes, start and first record of a page
    uint32_t pg_n_rec = 0, pg_page_bytes = 0, pg_n_pages = 0;
    uint32_t pg_cus = 0;                    // compute units of the device (k_pg_write's grid; asked for once)
    uint32_t pg_per_cu = 0, pg_per_cu_page_bytes = 0;   // ... and workgroups of k_pg_write a CU holds, for pages of that size
    uint32_t pg_lean_per_cu = 0, pg_lean_page_bytes = 0;   // ... and of k_pg_lean
    uint32_t pg_grid_cap = 0;               // GCI_PAGES_GRID=<n>: at most n workgroups for the page writers (testing; 0: what the device holds)
    DevBuf pg_list;                         // the pages k_pg_lean left to k_pg_write: two counters (u32 each, 16 bytes in all), then the list
    uint32_t pg_parity = 0;                 // which of the two counters the next gci_bam_pages_write uses
    uint64_t pg_blob_off = 0;
    uint64_t pg_blob_bytes = 0;               // total size of the blob the size call measured (without its 16 guard bytes)
    std::vector<DevBuf> paf_pool;           // K2's scratch, in the order a call asks for it (k_paf.hip: PafScratch)
    uint64_t paf_global_groups = 0;         // tokeniser workgroups of the last PAF call that walked global memory
    DevBuf crc_tabs;                        // k_bgzf_crc: the 32 look-up tables (k_crc_tables), made on first use
    bool crc_tabs_ready = false;            // ... set once k_crc_tables has been launched without an error
    uint32_t inflate_last_n = 0;            // members of the last gci_bgzf_inflate_device call (0: the wave decoder was not used)
    DevBuf inflate_sym, inflate_nsym, inflate_wstatus, inflate_lists, inflate_prof, inflate_next;
    DevBuf inflate_sym2, inflate_lists2;    // ... of the batches that run on the second stream
    int inflate_streams = 1;                // gci_bgzf_inflate_streams(): 2 = every other batch of members on inflate_stream2
    hipStream_t inflate_stream2 = nullptr;  // k_inflate_wave.hip: every other batch of members on a stream of its own (made on first use)
    hipEvent_t inflate_ev_in = nullptr, inflate_ev_out = nullptr;   // k_inflate_wave.hip: a batch's symbol streams, per member its symbols and how it fared
    DevBuf tail_sums;                       // gci_two_type_tail: per-tile sums of the three tracks
    DevBuf class_sums;                      // gci_depth_classes: per-tile (sum, count) of the depths > 0
    DevBuf tail_gaps;                       // gci_two_type_tail: the N runs as absolute sorted [begin, end) element ranges
    std::vector<int64_t> tail_gaps_host;    // ... what was uploaded last
    // issue-scan windows
    DevBuf win, win_tile_first;
    int win_flank = INT32_MIN;              // flank the cached per-contig windows were built for
    uint32_t win_n = 0;
    int64_t win_tiles = 0;
    uint64_t win_epoch = 0;                 // counts gci_set_windows(): what a pass keeps about "the windows of the call before it"
    // k_bedgraph.hip: runs per window tile and their scan, of the last gci_depth_runs_count; the window table, bytes per block of runs
    // and their scan, of the last gci_bedgraph_size
    DevBuf bg_tile_cnt, bg_tile_off, bg_blk, bg_wtab, bg_blk_bytes, bg_blk_off, bg_blk2;
    uint64_t bg_runs_epoch = 0, bg_runs_total = 0;      // (epoch 0: no count call yet)
    const void* bg_runs_track = nullptr;
    const void* bg_text_runs = nullptr;                 // the size call's d_runs (nullptr: no size call yet), d_win_run0, n_windows
    const void* bg_text_run0 = nullptr;
    uint32_t bg_text_windows = 0;
    uint64_t bg_text_n_runs = 0, bg_text_total = 0;
    DevBuf hist_chunk_first;                // k_hist.hip: the first chunk (workgroup) of every window of the last gci_depth_hist
    // k_cover.hip: what gci_bam_cover_size keeps for gci_bam_cover_write -- per record (its parse, chunk count, first chunk) and
    // per chunk (reference length, intervals and their scans), the status word of the size pass, and what that call measured
    DevBuf cover_rec, cover_chunk;
    bool cover_valid = false;
    uint32_t cover_n_rec = 0;
    uint64_t cover_n_chunks = 0, cover_n_ivl = 0;
    int cover_count_del = 0;
    const void* cover_stream = nullptr;
    const void* cover_off = nullptr;
    DevBuf fate_rec, fate_chunk;            // k_fate.hip: per record (parse, NM, chunk counts and their scan) and per chunk (base sums)
    // k_reads.hip: what gci_bam_reads_size keeps for gci_bam_reads_write -- per record (parse, totals, row length) and per workgroup
    // of records (row bytes and their scan), per chunk (base sums), the contig name table, and what that call measured
    DevBuf reads_rec, reads_chunk, reads_names;
    bool reads_valid = false;
    uint32_t reads_n_rec = 0, reads_file_no = 0;
    uint64_t reads_n_bytes = 0, reads_rows = 0, reads_total = 0;
    const void* reads_stream = nullptr;
    const void* reads_off = nullptr;
    std::vector<uint32_t> reads_name_len;   // ... and the contig name lengths its rows were measured with
    DevBuf sweep_rec, sweep_chunk;          // k_sweep.hip: per record (parse, NM, window, chunk counts and their scan) + the table, and per chunk (base sums)
    uint32_t sweep_grid_cap = 0;            // GCI_SWEEP_GRID=<n>: at most n workgroups for k_sweep_bin (testing; 0: what the device holds)
    // k_clips.hip: what gci_bam_clip_size keeps for gci_bam_clip_write -- per record (parse, end clips, events, ranks, right site) and
    // per chunk (base sums)
    DevBuf clip_rec, clip_chunk;
    bool clip_valid = false;
    uint32_t clip_n_rec = 0;
    uint64_t clip_n_left = 0, clip_n_right = 0;
    const void* clip_stream = nullptr;
    const void* clip_off = nullptr;
    // k_indels.hip: what gci_bam_indel_size keeps for gci_bam_indel_write -- per record (parse, chunk counts, counted) and per chunk
    // (base sums, reference length, deletions, insertions and their scans)
    DevBuf indel_rec, indel_chunk;
    bool indel_valid = false;
    uint32_t indel_n_rec = 0;
    int indel_min_len = 0;
    uint64_t indel_n_bytes = 0, indel_n_chunks = 0, indel_n_del = 0, indel_n_ins = 0;
    const void* indel_stream = nullptr;
    const void* indel_off = nullptr;
    // k_mismatch.hip: the records' ranks of gci_fasta_codes; what gci_bam_mismatch_size keeps for gci_bam_mismatch_write -- per record
    // (parse, SEQ, chunk counts, counted) and per chunk (base sums, the two lengths, mismatches, pairs and their scans)
    DevBuf mm_fasta, mm_rec, mm_chunk;
    bool mm_valid = false;
    uint32_t mm_n_rec = 0;
    uint64_t mm_n_bytes = 0, mm_n_chunks = 0, mm_n_mm = 0;
    const void* mm_stream = nullptr;
    const void* mm_off = nullptr;
    const void* mm_codes = nullptr;
    // ... and what gci_bam_allele_size keeps for gci_bam_allele_write: the same scratch with four counts a chunk, and a memo of its own
    DevBuf al_rec, al_chunk;
    bool al_valid = false;
    uint32_t al_n_rec = 0;
    uint64_t al_n_bytes = 0, al_n_chunks = 0, al_total = 0;
    const void* al_stream = nullptr;
    const void* al_off = nullptr;
    const void* al_codes = nullptr;
    // gci_site_tiles.hpp: what gci_{clip,indel,mismatch,allele}_sites_size keeps for the _write call -- per window tile its sites or run starts
    // and their scan, and the one memo.  Every size call runs gci_set_windows, so what another lister left here is dead by then
    DevBuf site_tiles;
    SiteMemo site_memo;
    void* h_pinned = nullptr;               // staging for small uploads
    size_t h_pinned_cap = 0;
    // optional per-kernel HIP-event timing (gci_profile_*)
    int prof_mask = 0;
    struct ProfEv { int id; hipEvent_t a, b; };
    std::vector<ProfEv> prof_live, prof_free;
    double prof_ms[GCI_PROF_COUNT] = {0};
    uint64_t prof_n[GCI_PROF_COUNT] = {0};
};

// Scoped HIP-event pair around one launch (or a few), recorded on the ctx stream when that
// kernel id is enabled.  Events are pooled; elapsed times are folded in by gci_profile_read().
struct ProfScope {
    gci_ctx* c; gci_ctx::ProfEv ev; bool on;
    ProfScope(gci_ctx* ctx, int kid) : c(ctx), on(false) {
        if (!(ctx->prof_mask & (1 << kid))) return;
        if (!ctx->prof_free.empty()) { ev = ctx->prof_free.back(); ctx->prof_free.pop_back(); }
        else if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) return;
        ev.id = kid;
        on = hipEventRecord(ev.a, ctx->stream) == hipSuccess;
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(ev.b, c->stream);
        c->prof_live.push_back(ev);
    }
};

int gci_fail(gci_ctx* c, hipError_t e, const char* what);
int gci_ensure(gci_ctx* ctx, DevBuf& b, size_t bytes);
int gci_upload_small(gci_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);

// every device allocation of the library comes from the arena of k_hbm.hip (slabs of GBs, cut up here: no driver call per buffer)
hipError_t gci_dmalloc(int device, void** out, size_t bytes);
hipError_t gci_dfree(void* p);

#define HIPCHK(call)                                      \
    do {                                                  \
        hipError_t _e = (call);                           \
        if (_e != hipSuccess) return gci_fail(ctx, _e, #call); \
    } while (0)
#define LAUNCHCHK(name)                                   \
    do {                                                  \
        hipError_t _e = hipGetLastError();                \
        if (_e != hipSuccess) return gci_fail(ctx, _e, name); \
    } while (0)
#define GCI_TRY(expr)                                     \
    do {                                                  \
        int _r = (expr);                                  \
        if (_r) return _r;                                \
    } while (0)

// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------

// contig of a tile: largest c with tile_first[c] <= tile   (tile_first has n + 1 entries)
__device__ __forceinline__ int32_t contig_of_tile(const int64_t* __restrict__ tile_first, int32_t n, int64_t tile)
{
    int32_t lo = 0, hi = n;          // invariant: tile_first[lo] <= tile < tile_first[hi]
    while (hi - lo > 1) {
        int32_t mid = (lo + hi) >> 1;
        if (tile_first[mid] <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ int32_t ld_i32(const uint8_t* p) { int32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint16_t ld_u16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

// Large inputs bucket their events by radix partition instead of one device-scope atomic per event (k_depth.hip, k_evp_*);
// gci_name_join_count then leaves the counting to the build.  GCI_EVENTS=atomic|radix overrides the size rule.
#define EVP_MAX_TILES (int64_t(1) << 23)
static inline bool gci_evp_wanted(const gci_ctx* ctx, uint64_t n_items)
{
    if (ctx->n_tiles == 0 || ctx->n_tiles > EVP_MAX_TILES) return false;
    const char* e = getenv("GCI_EVENTS");
    if (e && !strcmp(e, "atomic")) return false;
    if (e && !strcmp(e, "radix")) return true;
    return n_items >= (1u << 20);
}

// ---- interval -> tile events (shared by k_evt_count / k_evt_scatter and the counting join) -------------------------
struct IvlSpan { int64_t tile_a, tile_b; uint32_t pos_a, pos_b; bool valid, has_b; int64_t tile_bc; };

__device__ __forceinline__ IvlSpan span_of(const gci_ivl v, int flank, const int64_t* __restrict__ len,
                                           const int64_t* __restrict__ tile_first, int32_t n_contigs)
{
    IvlSpan s;
    s.valid = false; s.has_b = false; s.tile_a = s.tile_b = s.tile_bc = 0; s.pos_a = s.pos_b = 0;
    if (v.contig < 0 || v.contig >= n_contigs) return s;
    const int64_t L = len[v.contig];
    const int64_t a = gci_slice_bound((int64_t)v.start + flank, L);
    const int64_t b = gci_slice_bound((int64_t)v.end - flank + 1, L);
    if (a >= b) return s;
    const int64_t t0 = tile_first[v.contig];
    s.valid = true;
    s.tile_a = t0 + a / TILE; s.pos_a = (uint32_t)(a % TILE);
    s.has_b = b < (L + TILE - 1) / TILE * TILE;          // b == L lands in tail padding when there is any
    s.tile_b = t0 + b / TILE; s.pos_b = (uint32_t)(b % TILE);
    s.tile_bc = t0 + (b < L ? b : L - 1) / TILE;         // coarse -1: last tile of the contig when b == L
    return s;
}

// One 64-bit atomic per interval end: the low word of tile_cd counts the events of a tile, the high word carries
// the coarse difference (+1 in the tile of the start, -1 in the tile of the stop).
__device__ __forceinline__ void count_span(const IvlSpan& s, unsigned long long* __restrict__ tile_cd)
{
    const unsigned long long minus1 = 0xFFFFFFFFull << 32;         // -1 in the high word (the low word never carries)
    atomicAdd(tile_cd + s.tile_a, 1ull | (1ull << 32));
    if (s.has_b && s.tile_b == s.tile_bc) atomicAdd(tile_cd + s.tile_b, 1ull | minus1);
    else {
        if (s.has_b) atomicAdd(tile_cd + s.tile_b, 1ull);
        atomicAdd(tile_cd + s.tile_bc, minus1);
    }
}

__device__ __forceinline__ uint32_t ndigits(uint32_t v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
           (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}

// depths are small almost everywhere: five compares, the long tail behind a rarely taken branch
__device__ __forceinline__ uint32_t ndigits_fast(uint32_t v)
{
    uint32_t n = 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u);
    if (__builtin_expect(v >= 100000u, 0)) n = ndigits(v);
    return n;
}

// the same for 64-bit values (coordinates, base totals), and the decimal digits of v, w = ndigits64(v) of them, at p (LDS or global)
__device__ __forceinline__ uint32_t ndigits64(uint64_t v)
{
    if (v <= 0xFFFFFFFFull) return ndigits((uint32_t)v);
    uint32_t n = 10;
    for (v /= 10000000000ull; v; v /= 10) n++;
    return n;
}

__device__ __forceinline__ void put_dec64(uint8_t* p, uint64_t v, uint32_t w)
{
    if (v <= 0xFFFFFFFFull) { uint32_t x = (uint32_t)v; for (uint32_t d = w; d-- > 0;) { p[d] = (uint8_t)('0' + x % 10u); x /= 10u; } }
    else for (uint32_t d = w; d-- > 0;) { p[d] = (uint8_t)('0' + v % 10u); v /= 10u; }
}

// `lo < d <= hi` for an integer d as integer bounds: d in [ilo, ihi]  (empty range: ilo > ihi)
struct IntRange { int32_t lo, hi; };
static inline IntRange gci_int_range(double lo, double hi)
{
    IntRange r;
    if (!(lo == lo) || !(hi == hi)) { r.lo = 1; r.hi = 0; return r; }           // NaN: every comparison is false
    double fl = __builtin_floor(lo) + 1.0, fh = __builtin_floor(hi);
    if (fl < -2147483648.0) fl = -2147483648.0;
    if (fh > 2147483647.0) fh = 2147483647.0;
    if (fl > fh) { r.lo = 1; r.hi = 0; return r; }
    r.lo = (int32_t)fl; r.hi = (int32_t)fh;
    return r;
}

// issue-scan boundary key: (window << 33) | (rel << 1) | is_end
__device__ __forceinline__ unsigned long long issue_key(uint32_t window, int64_t rel, bool is_end)
{
    return ((unsigned long long)window << 33) | ((unsigned long long)rel << 1) | (is_end ? 1ull : 0ull);
}

// ---------------------------------------------------------------------------------------------
// exclusive scan over per-tile tables (n up to millions): local scan per 4096 entries + add
// ---------------------------------------------------------------------------------------------

template <typename TIn, typename TOut>
__device__ __forceinline__ void scan_local_body(const TIn* __restrict__ in, TOut* __restrict__ out,
                                                TOut* __restrict__ blk_tot, int64_t n, uint32_t blk, int64_t stride = 1)
{
    __shared__ TOut wtot[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t base = (int64_t)blk * TILE + (int64_t)t * 16;
    TOut v[16];
    TOut run = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) { v[i] = base + i < n ? (TOut)in[(base + i) * stride] : (TOut)0; run += v[i]; }
    const TOut inc = wave_inclusive<TOut>(run, lane);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    TOut pre = inc - run;
    TOut all = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) { if (w < wave) pre += wtot[w]; all += wtot[w]; }
#pragma unroll
    for (int i = 0; i < 16; i++) { if (base + i < n) out[base + i] = pre; pre += v[i]; }
    if (t == 0) blk_tot[blk] = all;
}

// out[i] += sum of blk_tot[0 .. block(i) - 1]; the extra block n_blocks writes the grand total to out[n]
template <typename TOut>
__device__ __forceinline__ void scan_add_body(TOut* __restrict__ out, const TOut* __restrict__ blk_tot, int64_t n,
                                              int32_t n_blocks, uint32_t me)
{
    __shared__ TOut part[BLOCK / 64];
    __shared__ TOut s_pre;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    TOut s = 0;
    for (int32_t b = t; b < (int32_t)me; b += BLOCK) s += blk_tot[b];
    s = wave_sum<TOut>(s);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (t == 0) { TOut a = 0; for (int w = 0; w < BLOCK / 64; w++) a += part[w]; s_pre = a; }
    __syncthreads();
    const TOut pre = s_pre;
    if ((int32_t)me == n_blocks) { if (t == 0) out[n] = pre; return; }
    if (pre == 0) return;
    const int64_t base = (int64_t)me * TILE + (int64_t)t * 16;
#pragma unroll
    for (int i = 0; i < 16; i++) if (base + i < n) out[base + i] += pre;
}

template <typename TIn, typename TOut>
__global__ __launch_bounds__(BLOCK) void k_scan_local(const TIn* __restrict__ in, TOut* __restrict__ out,
                                                      TOut* __restrict__ blk_tot, int64_t n)
{
    scan_local_body<TIn, TOut>(in, out, blk_tot, n, blockIdx.x);
}

template <typename TOut>
__global__ __launch_bounds__(BLOCK) void k_scan_add(TOut* __restrict__ out, const TOut* __restrict__ blk_tot, int64_t n,
                                                    int32_t n_blocks)
{
    scan_add_body<TOut>(out, blk_tot, n, n_blocks, blockIdx.x);
}

// out must have n + 1 entries when write_total is set
template <typename TIn, typename TOut>
static inline int device_exclusive_scan(gci_ctx* ctx, const TIn* in, TOut* out, TOut* blk_tot, int64_t n, bool write_total)
{
    const int32_t nb = (int32_t)((n + TILE - 1) / TILE);
    if (nb == 0) {
        if (write_total) HIPCHK(hipMemsetAsync(out, 0, sizeof(TOut), ctx->stream));
        return GCI_OK;
    }
    hipLaunchKernelGGL((k_scan_local<TIn, TOut>), dim3(nb), dim3(BLOCK), 0, ctx->stream, in, out, blk_tot, n);
    LAUNCHCHK("k_scan_local");
    if (nb > 1 || write_total) {
        hipLaunchKernelGGL((k_scan_add<TOut>), dim3(nb + (write_total ? 1 : 0)), dim3(BLOCK), 0, ctx->stream, out,
                           blk_tot, n, nb);
        LAUNCHCHK("k_scan_add");
    }
    return GCI_OK;
}

// ---------------------------------------------------------------------------------------------
// decimal text of depth values through LDS staging (K10)
// ---------------------------------------------------------------------------------------------

#define TEXT_STAGE 16384                 // LDS bytes of staging: 16 for the alignment shift + text

// lut[x] = the characters of "x\n" packed little endian (x < 1000: at most 3 digits + newline).
// Built once per context in global memory (gci_text_lut_host); every workgroup copies it to LDS.
static inline void gci_text_lut_host(uint32_t* lut)
{
    for (uint32_t x = 0; x < TEXT_LUT; x++) {
        const uint32_t d2 = x / 100u, d1 = (x / 10u) % 10u, d0 = x % 10u;
        if (x >= 100u) lut[x] = ('0' + d2) | (('0' + d1) << 8) | (('0' + d0) << 16) | ((uint32_t)'\n' << 24);
        else if (x >= 10u) lut[x] = ('0' + d1) | (('0' + d0) << 8) | ((uint32_t)'\n' << 16);
        else lut[x] = ('0' + d0) | ((uint32_t)'\n' << 8);
    }
}

__device__ __forceinline__ void text_lut_load(uint32_t* lut, const uint32_t* __restrict__ g_lut, int t)
{
    for (uint32_t x = t; x < TEXT_LUT; x += BLOCK) lut[x] = g_lut[x];
}

__device__ __forceinline__ void lds_put_u32(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }   // any alignment

// write the decimal lines of 4 consecutive elements into the staging buffer at byte offset o.
// Common case -- all four below 1000 with the same width W (digits + newline): the 4 * W bytes are assembled
// from the table words in registers and leave as W unaligned dword stores (gfx950 LDS takes any alignment).
__device__ __forceinline__ void text_put4(const uint32_t (&v)[4], const uint32_t (&nd)[4], uint32_t o, uint8_t* stage,
                                          const uint32_t* lut)
{
    const uint32_t W = nd[0];
    const bool uniform = W >= 2u && nd[1] == W && nd[2] == W && nd[3] == W &&
                         v[0] < TEXT_LUT && v[1] < TEXT_LUT && v[2] < TEXT_LUT && v[3] < TEXT_LUT;
    if (uniform) {
        const uint32_t w0 = lut[v[0]], w1 = lut[v[1]], w2 = lut[v[2]], w3 = lut[v[3]];
        if (W == 3u) {
            lds_put_u32(stage + o, w0 | (w1 << 24));
            lds_put_u32(stage + o + 4, (w1 >> 8) | (w2 << 16));
            lds_put_u32(stage + o + 8, (w2 >> 16) | (w3 << 8));
        } else if (W == 2u) {
            lds_put_u32(stage + o, w0 | (w1 << 16));
            lds_put_u32(stage + o + 4, w2 | (w3 << 16));
        } else {
            lds_put_u32(stage + o, w0); lds_put_u32(stage + o + 4, w1);
            lds_put_u32(stage + o + 8, w2); lds_put_u32(stage + o + 12, w3);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!nd[k]) continue;
        if (v[k] < TEXT_LUT) {
            const uint32_t w = lut[v[k]];
            stage[o] = (uint8_t)w;
            stage[o + 1] = (uint8_t)(w >> 8);
            if (nd[k] > 2) stage[o + 2] = (uint8_t)(w >> 16);
            if (nd[k] > 3) stage[o + 3] = (uint8_t)(w >> 24);
        } else {
            uint32_t x = v[k];
            const uint32_t e = o + nd[k] - 1;
            stage[e] = '\n';
            for (uint32_t d = 1; d < nd[k]; d++) { stage[e - d] = (uint8_t)('0' + x % 10u); x /= 10u; }
        }
        o += nd[k];
    }
}

// staging -> global.  The staging buffer mirrors the 16-byte alignment of the destination (the text starts
// at stage[shift], shift = dst & 15), so whole chunks move as ds_read_b128 + global_store_dwordx4; the first
// and last partial chunk are written byte-wise and only where this tile owns the bytes.
__device__ __forceinline__ void text_copy_out(uint8_t* __restrict__ g, const uint8_t* stage, uint32_t shift,
                                              uint32_t total, int t)
{
    uint8_t* ga = g - shift;
    const uint32_t end = shift + total;
    const uint32_t nchunks = (end + 15u) >> 4;
    for (uint32_t c = t; c < nchunks; c += BLOCK) {
        const uint32_t lo = c << 4, hi = lo + 16u;
        if (lo >= shift && hi <= end) {
            *reinterpret_cast<int4*>(ga + lo) = *reinterpret_cast<const int4*>(stage + lo);
        } else {
            const uint32_t a = lo > shift ? lo : shift, b = hi < end ? hi : end;
            for (uint32_t i = a; i < b; i++) ga[i] = stage[i];
        }
    }
}

// Decimal text of one tile held in registers (thread t, group j: elements (j * 256 + t) * 4 .. + 3) to
// out[dst ...].  One staging round
// when the tile's text fits the LDS buffer (it does unless depths reach 5+ digits), else one per group.
// Needs: stage[TEXT_STAGE] (16-byte aligned), wtot[4][BLOCK / 64], lut[TEXT_LUT] built and synced.
template <bool FULL>
__device__ __forceinline__ void text_tile(const int4 (&v)[4], int64_t valid, uint8_t* stage,
                                          uint32_t (*wtot)[BLOCK / 64], const uint32_t* lut, uint8_t* __restrict__ out,
                                          uint64_t dst, uint64_t cap, int t, int lane, int wave)
{
    uint32_t u[4][4], nd[4][4], mine[4], inc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        u[j][0] = (uint32_t)v[j].x; u[j][1] = (uint32_t)v[j].y; u[j][2] = (uint32_t)v[j].z; u[j][3] = (uint32_t)v[j].w;
        const int64_t i = (int64_t)(j * BLOCK + t) * 4;
        mine[j] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            nd[j][k] = (FULL || i + k < valid) ? ndigits_fast(u[j][k]) + 1u : 0u;
            mine[j] += nd[j][k];
        }
        inc[j] = (uint32_t)wave_inclusive_i32((int32_t)mine[j]);
    }
    if (lane == 63) {
#pragma unroll
        for (int j = 0; j < 4; j++) wtot[j][wave] = inc[j];
    }
    __syncthreads();
    uint32_t off[4], gtot[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t pre = 0, all = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; w++) { const uint32_t x = wtot[j][w]; if (w < wave) pre += x; all += x; }
        off[j] = pre + inc[j] - mine[j];
        gtot[j] = all;
    }
    const uint32_t tile_bytes = gtot[0] + gtot[1] + gtot[2] + gtot[3];
    if (dst + tile_bytes > cap) return;                       // caller's buffer too small: write nothing
    if (tile_bytes + 16u <= TEXT_STAGE) {
        const uint32_t shift = (uint32_t)((uintptr_t)(out + dst) & 15u);
        uint32_t base = shift;
#pragma unroll
        for (int j = 0; j < 4; j++) { text_put4(u[j], nd[j], base + off[j], stage, lut); base += gtot[j]; }
        __syncthreads();
        text_copy_out(out + dst, stage, shift, tile_bytes, t);
    } else {
        for (int j = 0; j < 4; j++) {
            const uint32_t shift = (uint32_t)((uintptr_t)(out + dst) & 15u);
            text_put4(u[j], nd[j], shift + off[j], stage, lut);
            __syncthreads();
            text_copy_out(out + dst, stage, shift, gtot[j], t);
            dst += gtot[j];
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------
// small kernels launched from more than one translation unit (k_track.hip has them)
// ---------------------------------------------------------------------------------------------

#define REDUCE_SPLIT 32                  // workgroups per contig of k_reduce_tiles, and of the same reduction fused into k_depth.hip's scan
// sums[c] += the sum of tile_sum over the tiles of contig c, for every contig of the layout (sums must be zeroed first)
int gci_launch_reduce_tiles(gci_ctx* ctx, const long long* tile_sum, unsigned long long* sums);
// contig_off[c] = tile_off[tile_first[c]] for c < n_contigs, contig_off[n_contigs] = tile_off[n_tiles]
int gci_launch_contig_text_off(gci_ctx* ctx, const uint64_t* tile_off, uint64_t* contig_off);
// the windows of an issue scan, clamped to the track, with their tiles: ctx->win, win_tile_first (n_win + 1 entries), win_n, win_tiles
int gci_set_windows(gci_ctx* ctx, const gci_window* h_win, uint32_t n_win);

// the windows of a sites call (gci_site_tiles.hpp: site_size) on the host: clamped as gci_set_windows clamps them, none: every contig of the
// layout; false when they are not sorted and disjoint
static inline bool gci_site_windows(const gci_ctx* ctx, const gci_window* h_windows, uint32_t n_windows, std::vector<gci_window>& ws)
{
    ws.clear();
    if (n_windows == 0) {
        for (int32_t c = 0; c < ctx->n_contigs; c++) ws.push_back(gci_window{ctx->off[(size_t)c], ctx->off[(size_t)c] + ctx->len[(size_t)c]});
        return true;
    }
    int64_t at = 0;
    for (uint32_t i = 0; i < n_windows; i++) {
        gci_window w = h_windows[i];
        if (w.begin < 0) w.begin = 0;
        if (w.end > ctx->total) w.end = ctx->total;
        if (w.end < w.begin) w.end = w.begin;
        if (w.begin < at) return false;
        at = w.end;
        ws.push_back(w);
    }
    return true;
}
