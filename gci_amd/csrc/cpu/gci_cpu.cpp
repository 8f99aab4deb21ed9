// gci_cpu.cpp -- libgci_cpu.so: the function seams of include/gci_hip.h on HOST memory and host threads
// ("same header compiled twice"; 8(d)(ii): the CPU baseline behind the same C-ABI).
//
// Same signatures, same structs, same status words as libgci_hip.so for the seam set
//   gci_bam_filter   gci_name_join   gci_depth_build   gci_gap_mask   gci_max2   gci_issue_scan(_windows)
//   gci_depth_text_size / _write   gci_depth_sum   gci_range_sums   gci_depth_classes
// and the context / layout / memory calls around them.  "d_" pointers are host pointers here (gci_malloc is an aligned
// malloc, gci_memcpy_* a memcpy, gci_sync a no-op): a host written against the header runs on either library.  What a GPU
// makes worthwhile -- record pages, the partitioned join, the tile build with its fused by-products, the BGZF / DEFLATE
// kernels, the PAF filter, the multi-GPU routing -- is not restated here.
//
// The code is this repository's own statement of the reference's rules (citations into /root/reference/GCI.py), written for
// threads and caches; it shares nothing with oracle/ (the tests hold the two against each other).
#include "../../../include/gci_hip.h"
#include "../gci_common.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

struct gci_ctx {
    int threads = 1;
    bool heads = false;                     // gci_bam_filter reads a HEADS stream (records without SEQ / QUAL, gci_bam_heads)
    std::string err;
    int32_t n_contigs = 0;
    std::vector<int64_t> len, off;
    int64_t total = 0;
    // depth_to_bedgraph.py: the last gci_depth_runs_count (its clamped windows in pieces, the runs in front of every piece) and
    // the last gci_bedgraph_size (whose text it measured)
    struct BgPiece { int64_t begin, lo, hi; uint64_t run0; };
    std::vector<BgPiece> bg_pieces;
    const void* bg_track = nullptr;
    uint64_t bg_runs_total = 0;
    const void* bg_text_run0 = nullptr;
    const void* bg_text_runs = nullptr;
    uint32_t bg_text_windows = 0;
    // bam_depth.py: what the last gci_bam_cover_size keeps for gci_bam_cover_write (per record its parse and its first interval)
    struct CoverRec { uint64_t ops_off; uint32_t n_ops; int32_t contig; int32_t pos; };
    std::vector<CoverRec> cover_rec;
    std::vector<uint64_t> cover_ivl0;
    uint64_t cover_status = ~0ull;
    bool cover_valid = false, cover_count_del = false;
    const void* cover_stream = nullptr;
    const void* cover_off = nullptr;
    // filter_reads.py: what the last gci_bam_reads_size keeps for gci_bam_reads_write (per selected record what its row holds besides
    // the contig's name, and where the row begins)
    struct ReadsRow { uint64_t M, I, D, S, end, name_at, byte0; int64_t nm; int32_t contig, pos; uint16_t flag; uint8_t mapq, name_len, cls; };
    std::vector<ReadsRow> reads_rows;
    std::vector<uint32_t> reads_name_len;
    uint64_t reads_total = 0, reads_n_bytes = 0;
    uint32_t reads_n_rec = 0, reads_file_no = 0;
    bool reads_valid = false;
    const void* reads_stream = nullptr;
    const void* reads_off = nullptr;
    // clip_sites.py: the events the last gci_bam_clip_size found (left, then right, each in record order) and the sites the last
    // gci_clip_sites_size found, with what each call measured
    std::vector<gci_ivl> clip_left, clip_right;
    uint64_t clip_status = ~0ull;
    bool clip_valid = false;
    uint32_t clip_n_rec = 0;
    const void* clip_stream = nullptr;
    const void* clip_off = nullptr;
    std::vector<gci_clip_site> sites;
    struct SiteAsk {                        // what a *_sites_size call measured: its _write call must ask the same
        bool valid = false;
        const void* track[6] = {};          // (gci_allele_sites_*: six arrays; the others leave the rest null)
        int32_t min_reads = 0, frac = 0;
        uint32_t n_windows = 0;
    };
    SiteAsk sites_ask;
    // indel_sites.py: the events the last gci_bam_indel_size found (deletions, then insertions, each in record and operation order)
    // and the sites the last gci_indel_sites_size found, with what each call measured
    std::vector<gci_ivl> indel_del, indel_ins;
    uint64_t indel_status = ~0ull;
    bool indel_valid = false;
    uint32_t indel_n_rec = 0;
    uint64_t indel_n_bytes = 0;
    const void* indel_stream = nullptr;
    const void* indel_off = nullptr;
    std::vector<gci_indel_site> isites;
    SiteAsk isites_ask;
    // mismatch_sites.py: the events the last gci_bam_mismatch_size found, in record and position order, and the sites the last
    // gci_mismatch_sites_size found, with what each call measured
    std::vector<gci_ivl> mm_events;
    uint64_t mm_status = ~0ull;
    bool mm_valid = false;
    uint32_t mm_n_rec = 0;
    uint64_t mm_n_bytes = 0;
    const void* mm_stream = nullptr;
    const void* mm_off = nullptr;
    const void* mm_codes = nullptr;
    std::vector<gci_mismatch_site> msites;
    SiteAsk msites_ask;
    // allele_sites.py: the events the last gci_bam_allele_size found, a list per read base (A, C, G, T), each in record and position
    // order, and the sites the last gci_allele_sites_size found, with what each call measured
    std::vector<gci_ivl> al_events[4];
    uint64_t al_status = ~0ull;
    bool al_valid = false;
    uint32_t al_n_rec = 0;
    uint64_t al_n_bytes = 0;
    const void* al_stream = nullptr;
    const void* al_off = nullptr;
    const void* al_codes = nullptr;
    std::vector<gci_allele_site> asites;
    SiteAsk asites_ask;
};

namespace {

// fn(t, n_threads) on every thread
template <typename F>
void on_threads(int threads, F fn)
{
    if (threads <= 1) { fn(0, 1); return; }
    std::vector<std::thread> pool;
    pool.reserve((size_t)threads - 1);
    for (int t = 1; t < threads; t++) pool.emplace_back([&fn, t, threads] { fn(t, threads); });
    fn(0, threads);
    for (auto& th : pool) th.join();
}

// [0, n) in blocks of `grain`, handed out by a counter: fn(lo, hi)
template <typename F>
void parallel_blocks(int threads, uint64_t n, uint64_t grain, F fn)
{
    if (n == 0) return;
    std::atomic<uint64_t> next{0};
    on_threads(threads, [&](int, int) {
        for (;;) {
            const uint64_t lo = next.fetch_add(grain);
            if (lo >= n) break;
            fn(lo, std::min(n, lo + grain));
        }
    });
}

inline void report(std::atomic<uint64_t>& status, uint32_t rec, int code)
{
    const uint64_t v = ((uint64_t)rec << 8) | (uint64_t)(uint8_t)(-code);
    uint64_t cur = status.load();
    while (v < cur && !status.compare_exchange_weak(cur, v)) {}
}

inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }

// size of an aux value of type t at p; -1: malformed / past the end of the record
int64_t aux_value_size(const uint8_t* p, const uint8_t* end, uint8_t t)
{
    switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'Z': case 'H': {
        const uint8_t* q = p;
        while (q < end && *q) q++;
        return q < end ? (q - p) + 1 : -1;
    }
    case 'B': {
        if (p + 5 > end) return -1;
        const uint8_t sub = p[0];
        const int64_t n = rd32(p + 1);
        const int64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : -1;
        return es < 0 ? -1 : 5 + n * es;
    }
    default: return -1;
    }
}

bool nm_value(const uint8_t* t, int64_t& NM)
{
    switch (t[0]) {
    case 'c': NM = (int8_t)t[1]; return true;
    case 'C': NM = t[1]; return true;
    case 's': NM = (int16_t)rd16(t + 1); return true;
    case 'S': NM = rd16(t + 1); return true;
    case 'i': NM = (int32_t)rd32(t + 1); return true;
    case 'I': NM = rd32(t + 1); return true;
    default: return false;
    }
}

uint64_t name_hash(const uint8_t* name, uint32_t len)
{
    uint64_t acc = 0;
    for (uint32_t k = 0; k * 8 < len; k++) {
        uint64_t w = 0;
        const uint32_t n = std::min(8u, len - 8 * k);
        memcpy(&w, name + 8 * k, n);
        acc += gci_hash_word(w, k);
    }
    return gci_hash_finish(acc, len);
}

// read_sam on one record (GCI.py:146-169); the record's compact form into r, GCI_OK also when it is filtered
int filter_record(const uint8_t* bam, uint64_t n_bytes, uint64_t off, const int32_t* ref_sel, int32_t n_ref, int map_qual, int mq_cutoff,
                  double clip_percent, double iden_percent, bool has_seq, gci_rec& r)
{
    if (off + 36 > n_bytes) return GCI_E_MALFORMED;
    const uint8_t* p = bam + off;
    const int32_t block_size = (int32_t)rd32(p), ref_id = (int32_t)rd32(p + 4), pos = (int32_t)rd32(p + 8);
    const uint32_t l_read_name = p[12];
    const int mapq = p[13];
    const uint32_t n_cigar = rd16(p + 16), flag = rd16(p + 18);
    const int32_t l_seq = (int32_t)rd32(p + 20);
    const uint64_t rec_end = off + 4 + (uint64_t)(uint32_t)block_size;
    const uint64_t aux_off = off + 36 + l_read_name + 4ull * n_cigar + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
    r.mapq = (uint8_t)mapq;
    if (block_size < 32 || rec_end > n_bytes || l_seq < 0 || aux_off > rec_end) return GCI_E_MALFORMED;
    // mapped, primary, MAPQ (GCI.py:152-156); fetch(contig = target) only yields records of selected contigs (:151, :260)
    if (ref_id < 0 || ref_id >= n_ref || (flag & (0x4u | 0x100u | 0x800u)) || mapq < map_qual) return GCI_OK;
    const int32_t contig = ref_sel[ref_id];
    if (contig < 0) return GCI_OK;
    const uint8_t* name = p + 36;
    const uint8_t* end = bam + rec_end;
    uint32_t name_len = 0;
    while (name_len < l_read_name && name[name_len]) name_len++;
    r.name_hash = name_hash(name, name_len);
    r.name_len = (uint16_t)name_len;
    // the first NM and the first CG tag (bam_aux_get)
    const uint8_t* nm_p = nullptr;
    const uint8_t* cg_p = nullptr;
    for (const uint8_t* q = bam + aux_off; q + 3 <= end;) {
        const int64_t sz = aux_value_size(q + 3, end, q[2]);
        if (sz < 0 || q + 3 + sz > end) break;
        if (q[0] == 'N' && q[1] == 'M' && !nm_p) nm_p = q + 2;
        if (q[0] == 'C' && q[1] == 'G' && !cg_p) cg_p = q + 2;
        q += 3 + sz;
    }
    int64_t NM = 0;
    const bool nm_bad = nm_p ? !nm_value(nm_p, NM) : false;
    // htslib puts a CIGAR of more than 65535 operations back from CG:B,I when op0 is <l_seq>S
    const uint8_t* ops = name + l_read_name;
    uint32_t n_ops = n_cigar;
    if (n_cigar > 0 && pos >= 0) {
        const uint32_t op0 = rd32(ops);
        if ((op0 & 0xF) == 4 && (op0 >> 4) == (uint32_t)l_seq && cg_p && cg_p[0] == 'B' && (cg_p[1] == 'I' || cg_p[1] == 'i')) {
            const uint32_t cg_len = rd32(cg_p + 2);
            if (cg_len >= n_cigar && cg_len < (1u << 29)) { ops = cg_p + 6; n_ops = cg_len; }
        }
    }
    // base totals per operation (get_cigar_stats()[0], GCI.py:157-162): M, = and X together
    int64_t M = 0, I = 0, D = 0, N = 0, S = 0;
    for (uint32_t k = 0; k < n_ops; k++) {
        const uint32_t v = rd32(ops + 4ull * k);
        const int64_t len = v >> 4;
        switch (v & 0xF) {
        case 0: case 7: case 8: M += len; break;
        case 1: I += len; break;
        case 2: D += len; break;
        case 3: N += len; break;
        case 4: S += len; break;
        default: break;
        }
    }
    if (!nm_p) return GCI_E_NO_NM;                                          // get_tag('NM'): KeyError
    if (nm_bad) return GCI_E_BAD_NM_TYPE;
    const int64_t den1 = M + I + S, den2 = M + I + D, rlen = M + D + N;
    if (den1 == 0) return GCI_E_ZERO_DIV;
    if (!((double)S / (double)den1 <= clip_percent)) return GCI_OK;         // GCI.py:165; `and` short-circuits
    if (den2 == 0) return GCI_E_ZERO_DIV;
    if (!((double)(den2 - NM) / (double)den2 >= iden_percent)) return GCI_OK;
    if (n_cigar == 0) return GCI_E_NO_END;
    r.contig = contig;
    r.start = pos;
    r.end = (int32_t)((int64_t)pos + (rlen > 0 ? rlen : 1));               // bam_endpos
    r.qlen = l_seq;
    r.flags = GCI_REC_PASS | (mapq >= mq_cutoff ? GCI_REC_HQ : 0);         // GCI.py:166-168
    return GCI_OK;
}

// bam_depth.py and the three site tools, one record: bounds, the skip decision and where its operations lie (include/gci_hip.h:
// gci_bam_cover_size) -- the record's own, or the first CG:B,I / B,i array behind <l_seq>S (none usable: the record's own stay).
// GCI_E_MALFORMED, or GCI_OK with r.contig < 0 for a skipped record.  sq: where SEQ lies (behind the in-record words, also in the CG
// case) and l_seq.
struct SeqAt { uint64_t seq_off; uint32_t l_seq; };

int cover_parse(const uint8_t* bam, uint64_t n_bytes, uint64_t off, bool has_seq, const int32_t* ref_sel, int32_t n_ref, uint32_t excl_flags,
                int min_mapq, gci_ctx::CoverRec& r, SeqAt* sq = nullptr)
{
    r.ops_off = 0; r.n_ops = 0; r.contig = -1; r.pos = 0;
    if (sq) { sq->seq_off = 0; sq->l_seq = 0; }
    if (off > n_bytes || n_bytes - off < 36) return GCI_E_MALFORMED;
    const uint8_t* p = bam + off;
    const int32_t block_size = (int32_t)rd32(p), ref_id = (int32_t)rd32(p + 4), pos = (int32_t)rd32(p + 8);
    const uint32_t l_read_name = p[12];
    const int mapq = p[13];
    const uint32_t n_cigar = rd16(p + 16), flag = rd16(p + 18);
    const int32_t l_seq = (int32_t)rd32(p + 20);
    const uint64_t rec_end = off + 4 + (uint64_t)(uint32_t)block_size;
    const uint64_t cig_off = off + 36 + l_read_name;
    const uint64_t aux_off = cig_off + 4ull * n_cigar + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
    if (block_size < 32 || rec_end > n_bytes || l_seq < 0 || aux_off > rec_end) return GCI_E_MALFORMED;
    if ((flag & excl_flags) || mapq < min_mapq || ref_id < 0 || ref_id >= n_ref || pos < 0 || ref_sel[ref_id] < 0) return GCI_OK;
    r.contig = ref_sel[ref_id]; r.pos = pos; r.ops_off = cig_off; r.n_ops = n_cigar;
    if (sq) { sq->seq_off = cig_off + 4ull * n_cigar; sq->l_seq = (uint32_t)l_seq; }
    if (n_cigar > 0) {                                                      // the CG:B,I placeholder, as filter_record restores it
        const uint32_t op0 = rd32(bam + cig_off);
        if ((op0 & 0xFu) == 4u && (op0 >> 4) == (uint32_t)l_seq) {
            const uint8_t* end = bam + rec_end;
            for (const uint8_t* q = bam + aux_off; q + 3 <= end;) {
                const int64_t sz = aux_value_size(q + 3, end, q[2]);
                if (sz < 0 || q + 3 + sz > end) break;
                if (q[0] == 'C' && q[1] == 'G') {                           // the first CG tag (bam_aux_get)
                    if (q[2] == 'B' && (q[3] == 'I' || q[3] == 'i')) {
                        const uint32_t cg_len = rd32(q + 4);
                        if (cg_len >= n_cigar && cg_len < (1u << 29)) { r.ops_off = (uint64_t)(q + 8 - bam); r.n_ops = cg_len; }
                    }
                    break;
                }
                q += 3 + sz;
            }
        }
    }
    return GCI_OK;
}

// the windows of a *_sites_size call: clamped to the track, none: every contig of the layout; false when not sorted and disjoint
bool site_windows(const gci_ctx* ctx, const gci_window* h_windows, uint32_t n_windows, std::vector<gci_window>& ws)
{
    if (n_windows == 0) {
        for (int32_t c = 0; c < ctx->n_contigs; c++) ws.push_back(gci_window{ctx->off[(size_t)c], ctx->off[(size_t)c] + ctx->len[(size_t)c]});
        return true;
    }
    int64_t at = 0;
    for (uint32_t i = 0; i < n_windows; i++) {
        gci_window w = h_windows[i];
        w.begin = std::max<int64_t>(w.begin, 0);
        w.end = std::max(std::min(w.end, ctx->total), w.begin);
        if (w.begin < at) return false;
        at = w.end;
        ws.push_back(w);
    }
    return true;
}

gci_ctx::SiteAsk site_ask(const void* a, const void* b, const void* c, int32_t min_reads, int32_t frac, uint32_t n_windows)
{
    gci_ctx::SiteAsk m;
    m.valid = true; m.track[0] = a; m.track[1] = b; m.track[2] = c; m.min_reads = min_reads; m.frac = frac; m.n_windows = n_windows;
    return m;
}

// a *_sites_write call: the sites its size call kept, when it asks what that call measured
template <typename Site>
int sites_write(const gci_ctx::SiteAsk& kept, const gci_ctx::SiteAsk& ask, const std::vector<Site>& sites, Site* out, uint64_t cap)
{
    if (!kept.valid || !std::equal(kept.track, kept.track + 6, ask.track) || kept.min_reads != ask.min_reads || kept.frac != ask.frac ||
        kept.n_windows != ask.n_windows)
        return GCI_E_INVALID;
    if (!sites.empty() && !out) return GCI_E_INVALID;
    if (cap < sites.size()) return GCI_E_CAPACITY;
    std::copy(sites.begin(), sites.end(), out);
    return GCI_OK;
}

// filter_depth.py, one record: its class (include/gci_hip.h: gci_bam_fate) and what the status word says of it (GCI_OK for a record of the
// classes none .. kept).  The tests and their order are filter_record's.
int fate_record(const uint8_t* bam, uint64_t n_bytes, uint64_t off, bool has_seq, const int32_t* ref_sel, int32_t n_ref, int map_qual,
                double clip_percent, double iden_percent, uint8_t& cls)
{
    cls = GCI_FATE_ERROR;
    if (off > n_bytes || n_bytes - off < 36) return GCI_E_MALFORMED;
    const uint8_t* p = bam + off;
    const int32_t block_size = (int32_t)rd32(p), ref_id = (int32_t)rd32(p + 4), pos = (int32_t)rd32(p + 8);
    const uint32_t l_read_name = p[12];
    const int mapq = p[13];
    const uint32_t n_cigar = rd16(p + 16), flag = rd16(p + 18);
    const int32_t l_seq = (int32_t)rd32(p + 20);
    const uint64_t rec_end = off + 4 + (uint64_t)(uint32_t)block_size;
    const uint64_t cig_off = off + 36 + l_read_name;
    const uint64_t aux_off = cig_off + 4ull * n_cigar + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
    if (block_size < 32 || rec_end > n_bytes || l_seq < 0 || aux_off > rec_end) return GCI_E_MALFORMED;
    if ((flag & 0x4u) || ref_id < 0 || ref_id >= n_ref || pos < 0 || ref_sel[ref_id] < 0) { cls = GCI_FATE_NONE; return GCI_OK; }
    if (flag & 0x100u) { cls = GCI_FATE_SECONDARY; return GCI_OK; }          // GCI.py:156, test by test
    if (flag & 0x800u) { cls = GCI_FATE_SUPPLEMENTARY; return GCI_OK; }
    if (mapq < map_qual) { cls = GCI_FATE_MAPQ; return GCI_OK; }
    const uint8_t* end = bam + rec_end;
    const uint8_t* nm_p = nullptr;                                          // the first NM and the first CG tag (bam_aux_get)
    const uint8_t* cg_p = nullptr;
    for (const uint8_t* q = bam + aux_off; q + 3 <= end;) {
        const int64_t sz = aux_value_size(q + 3, end, q[2]);
        if (sz < 0 || q + 3 + sz > end) break;
        if (q[0] == 'N' && q[1] == 'M' && !nm_p) nm_p = q + 2;
        if (q[0] == 'C' && q[1] == 'G' && !cg_p) cg_p = q + 2;
        q += 3 + sz;
    }
    int64_t NM = 0;
    const bool nm_bad = nm_p ? !nm_value(nm_p, NM) : false;
    const uint8_t* ops = bam + cig_off;
    uint32_t n_ops = n_cigar;
    if (n_cigar > 0) {
        const uint32_t op0 = rd32(ops);
        if ((op0 & 0xF) == 4 && (op0 >> 4) == (uint32_t)l_seq && cg_p && cg_p[0] == 'B' && (cg_p[1] == 'I' || cg_p[1] == 'i')) {
            const uint32_t cg_len = rd32(cg_p + 2);
            if (cg_len >= n_cigar && cg_len < (1u << 29)) { ops = cg_p + 6; n_ops = cg_len; }
        }
    }
    int64_t M = 0, I = 0, D = 0, S = 0;
    for (uint32_t k = 0; k < n_ops; k++) {
        const uint32_t v = rd32(ops + 4ull * k);
        const int64_t len = v >> 4;
        switch (v & 0xF) {
        case 0: case 7: case 8: M += len; break;
        case 1: I += len; break;
        case 2: D += len; break;
        case 4: S += len; break;
        default: break;
        }
    }
    if (!nm_p) return GCI_E_NO_NM;
    if (nm_bad) return GCI_E_BAD_NM_TYPE;
    const int64_t den1 = M + I + S, den2 = M + I + D;
    if (den1 == 0) return GCI_E_ZERO_DIV;
    if (!((double)S / (double)den1 <= clip_percent)) { cls = GCI_FATE_CLIP; return GCI_OK; }
    if (den2 == 0) return GCI_E_ZERO_DIV;
    cls = (double)(den2 - NM) / (double)den2 >= iden_percent ? GCI_FATE_KEPT : GCI_FATE_IDENTITY;
    return GCI_OK;
}

// filter_reads.py, one record whose class is asked for (include/gci_hip.h: gci_bam_reads_size): `row` says whether it makes a row, w what
// the row holds; the return value is what the status word says of the record (GCI_OK: nothing)
constexpr int64_t READS_NM_NONE = INT64_MAX;

int reads_record(const uint8_t* bam, uint64_t n_bytes, uint64_t off, bool has_seq, const int32_t* ref_sel, int32_t n_ref, int32_t n_sel,
                 const gci_window* win, const uint32_t* contig_win0, gci_ctx::ReadsRow& w, bool& row)
{
    row = false;
    gci_ctx::CoverRec r;
    if (cover_parse(bam, n_bytes, off, has_seq, ref_sel, n_ref, 0, 0, r) != GCI_OK) return GCI_E_MALFORMED;
    if (r.contig < 0 || r.contig >= n_sel) return GCI_E_INVALID;            // the class bytes of another input: such a record is `none`
    const uint8_t* p = bam + off;
    int64_t win_b = INT64_MIN;
    if (contig_win0) {                                                      // the contig's first window that ends behind pos
        const gci_window* a = win + contig_win0[r.contig];
        const gci_window* b = win + contig_win0[r.contig + 1];
        const gci_window* it = std::upper_bound(a, b, (int64_t)r.pos, [](int64_t pos, const gci_window& x) { return pos < x.end; });
        if (it == b) return GCI_OK;
        win_b = it->begin;
    }
    const uint32_t l_read_name = p[12], n_cigar = rd16(p + 16);
    const int32_t l_seq = (int32_t)rd32(p + 20);
    const uint8_t* end = bam + off + 4 + (uint64_t)rd32(p);
    w.nm = READS_NM_NONE;
    bool have_nm = false;
    for (const uint8_t* q = bam + off + 36 + l_read_name + 4ull * n_cigar + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
         q + 3 <= end && !have_nm;) {
        const int64_t sz = aux_value_size(q + 3, end, q[2]);
        if (sz < 0 || q + 3 + sz > end) break;
        if (q[0] == 'N' && q[1] == 'M') { have_nm = true; if (!nm_value(q + 2, w.nm)) w.nm = READS_NM_NONE; }
        q += 3 + sz;
    }
    int code = GCI_OK;
    uint64_t N = 0;
    w.M = w.I = w.D = w.S = 0;
    for (uint32_t k = 0; k < r.n_ops; k++) {
        const uint32_t v = rd32(bam + r.ops_off + 4ull * k);
        const uint64_t len = v >> 4;
        switch (v & 0xFu) {
        case 0: case 7: case 8: w.M += len; break;
        case 1: w.I += len; break;
        case 2: w.D += len; break;
        case 3: N += len; break;
        case 4: w.S += len; break;
        case 5: case 6: break;
        default: code = GCI_E_MALFORMED; break;                             // (9 - 15 add to no total; the row is listed)
        }
    }
    const uint64_t R = w.M + w.D + N;
    w.end = (uint64_t)r.pos + R;
    if ((int64_t)((uint64_t)r.pos + (R ? R : 1)) <= win_b) return GCI_OK;
    w.contig = r.contig; w.pos = r.pos;
    w.flag = (uint16_t)rd16(p + 18); w.mapq = p[13];
    w.name_at = off + 36;
    uint32_t nl = 0;
    while (nl < l_read_name && p[36 + nl]) nl++;
    w.name_len = (uint8_t)nl;
    row = true;
    return code;
}

// filter_sweep.py, one record (include/gci_hip.h: gci_bam_sweep): `counted` says whether it is a primary record that overlaps a window;
// then rows[3] are its rows in the mapq, clip and identity tables, pass[3] the three tests at the thresholds, each on its own, and M
// the bases it covers.  The return value is what the status word says of the record (GCI_OK: nothing).
uint32_t sweep_digits(uint64_t n, uint64_t d, int digits, bool& rest)      // floor(n * 10^digits / d) by long division, 0 <= n <= d
{
    uint64_t q = n / d, r = n % d;                                          // (r < d < 2^59: r * 10 fits)
    for (int k = 0; k < digits; k++) { r *= 10; q = q * 10 + r / d; r %= d; }
    rest = r != 0;
    return (uint32_t)q;
}

int sweep_record(const uint8_t* bam, uint64_t n_bytes, uint64_t off, bool has_seq, const int32_t* ref_sel, int32_t n_ref, int32_t n_sel,
                 const gci_window* win, const uint32_t* contig_win0, int map_qual, double clip_percent, double iden_percent, int digits,
                 bool& counted, uint32_t rows[3], bool pass[3], uint64_t& M)
{
    counted = false;
    gci_ctx::CoverRec r;
    if (cover_parse(bam, n_bytes, off, has_seq, ref_sel, n_ref, 0x904, 0, r) != GCI_OK) return GCI_E_MALFORMED;
    if (r.contig < 0) return GCI_OK;                                        // none, secondary or supplementary
    int64_t win_b = INT64_MIN;
    if (contig_win0) {                                                      // the contig's first window that ends behind pos
        if (r.contig >= n_sel) return GCI_OK;
        const gci_window* a = win + contig_win0[r.contig];
        const gci_window* b = win + contig_win0[r.contig + 1];
        const gci_window* it = std::upper_bound(a, b, (int64_t)r.pos, [](int64_t pos, const gci_window& x) { return pos < x.end; });
        if (it == b) return GCI_OK;
        win_b = it->begin;
    }
    const uint8_t* p = bam + off;
    const uint32_t l_read_name = p[12], n_cigar = rd16(p + 16);
    const int32_t l_seq = (int32_t)rd32(p + 20);
    const uint8_t* end = bam + off + 4 + (uint64_t)rd32(p);
    int64_t nm = 0;
    bool have_nm = false, nm_ok = false;
    for (const uint8_t* q = bam + off + 36 + l_read_name + 4ull * n_cigar + (has_seq ? (((uint64_t)(uint32_t)l_seq + 1) >> 1) + (uint64_t)(uint32_t)l_seq : 0ull);
         q + 3 <= end && !have_nm;) {
        const int64_t sz = aux_value_size(q + 3, end, q[2]);
        if (sz < 0 || q + 3 + sz > end) break;
        if (q[0] == 'N' && q[1] == 'M') { have_nm = true; nm_ok = nm_value(q + 2, nm); }
        q += 3 + sz;
    }
    int code = GCI_OK;
    uint64_t I = 0, D = 0, N = 0, S = 0;
    M = 0;
    for (uint32_t k = 0; k < r.n_ops; k++) {
        const uint32_t v = rd32(bam + r.ops_off + 4ull * k);
        const uint64_t len = v >> 4;
        switch (v & 0xFu) {
        case 0: case 7: case 8: M += len; break;
        case 1: I += len; break;
        case 2: D += len; break;
        case 3: N += len; break;
        case 4: S += len; break;
        case 5: case 6: break;
        default: code = GCI_E_MALFORMED; break;                             // (9 - 15 add to no total; the record is counted)
        }
    }
    const uint64_t R = M + D + N;
    if ((int64_t)((uint64_t)r.pos + (R ? R : 1)) <= win_b) return GCI_OK;
    counted = true;
    const uint32_t mapq = p[13];
    const uint64_t den1 = M + I + S, den2 = M + I + D;
    bool rest = false;
    rows[0] = GCI_SWEEP_MAPQ(mapq);
    pass[0] = (int)mapq >= map_qual;
    pass[1] = pass[2] = false;
    if (den1 == 0) rows[1] = GCI_SWEEP_CLIP_UNDEF(digits);
    else {
        const uint32_t q = sweep_digits(S, den1, digits, rest);
        rows[1] = GCI_SWEEP_CLIP(digits, q + (rest ? 1u : 0u));
        pass[1] = (double)S / (double)den1 <= clip_percent;
    }
    if (!nm_ok || den2 == 0) rows[2] = GCI_SWEEP_IDEN_UNDEF(digits);
    else {
        const int64_t num = (int64_t)den2 - nm;
        if (num < 0) rows[2] = GCI_SWEEP_IDEN_BELOW(digits);
        else if ((uint64_t)num > den2) rows[2] = GCI_SWEEP_IDEN_ABOVE(digits);
        else rows[2] = GCI_SWEEP_IDEN(digits, sweep_digits((uint64_t)num, den2, digits, rest));
        pass[2] = (double)num / (double)den2 >= iden_percent;
    }
    return code;
}

void reads_dec6(std::string& s, int64_t n, uint64_t d)
{
    if (n < 0) s += '-';
    const uint64_t a = n < 0 ? 0ull - (uint64_t)n : (uint64_t)n;
    s += std::to_string(a / d);
    s += '.';
    uint64_t r = a % d;                                                     // (r < d < 2^59: r * 10 fits)
    for (int k = 0; k < 6; k++) { r *= 10; s += (char)('0' + r / d); r %= d; }
}

// the row of w without the contig's name
void reads_text(std::string& s, const gci_ctx::ReadsRow& w, uint32_t file_no, const uint8_t* bam, const uint8_t* contig, uint32_t contig_len)
{
    static const char* const names[13] = {"none", "secondary", "supplementary", "mapq", "clip", "identity", "kept", "error",
                                          "shadowed", "unpaired", "contig", "overlap", "joined"};
    s += std::to_string(file_no); s += '\t';
    s.append((const char*)(bam + w.name_at), w.name_len); s += '\t';
    if (contig) s.append((const char*)contig, contig_len);
    s += '\t';
    s += std::to_string(w.pos); s += '\t';
    s += std::to_string(w.end); s += '\t';
    s += (w.flag & 0x10) ? '-' : '+'; s += '\t';
    s += std::to_string(w.flag); s += '\t';
    s += std::to_string(w.mapq); s += '\t';
    s += std::to_string(w.M); s += '\t';
    s += std::to_string(w.I); s += '\t';
    s += std::to_string(w.D); s += '\t';
    s += std::to_string(w.S); s += '\t';
    if (w.nm == READS_NM_NONE) s += '.'; else s += std::to_string(w.nm);
    s += '\t';
    const uint64_t den1 = w.M + w.I + w.S, den2 = w.M + w.I + w.D;
    if (den1 == 0) s += '.'; else reads_dec6(s, (int64_t)w.S, den1);
    s += '\t';
    if (den2 == 0 || w.nm == READS_NM_NONE) s += '.'; else reads_dec6(s, (int64_t)den2 - w.nm, den2);
    s += '\t';
    s += names[w.cls < 13 ? w.cls : 7];
    s += '\n';
}

// the maximal runs of covering operations of one record: emit(start, end) with `end` the last covered base, both clamped to `lim`;
// false when an operation code 9 - 15 turns up
template <typename F>
bool cover_walk(const uint8_t* bam, const gci_ctx::CoverRec& r, bool count_del, uint64_t lim, F emit)
{
    bool ok = true, open = false;
    uint64_t at = (uint64_t)(uint32_t)r.pos, start = 0;
    auto close = [&] { if (open) { emit((int32_t)std::min(start, lim), (int32_t)std::min(at - 1, lim)); open = false; } };
    for (uint32_t k = 0; k < r.n_ops; k++) {
        const uint32_t v = rd32(bam + r.ops_off + 4ull * k), op = v & 0xFu, len = v >> 4;
        if (op >= 9u) { ok = false; continue; }
        if (!((0x18Du >> op) & 1u) || len == 0) continue;                   // consumes no reference: a run goes on across it
        if (((0x181u >> op) & 1u) || (count_del && op == 2u)) { if (!open) { open = true; start = at; } }
        else close();
        at += len;
    }
    close();
    return ok;
}

int need_layout(gci_ctx* ctx) { return !ctx ? GCI_E_INVALID : ctx->n_contigs <= 0 ? GCI_E_NO_LAYOUT : GCI_OK; }

int issue_scan(gci_ctx* ctx, const int32_t* depth, const gci_window* win, uint32_t n_win, double lo, double hi, uint64_t* keys, uint32_t cap,
               uint32_t* n_keys)
{
    if (!depth || !n_keys || (cap && !keys)) return GCI_E_INVALID;
    std::atomic<uint32_t> n{0};
    // a window in pieces of 4 M elements: a piece reports the boundaries inside it, its neighbours' edges are matched up by looking
    // one element back
    struct Piece { uint32_t w; int64_t lo, hi; };
    std::vector<Piece> pieces;
    for (uint32_t w = 0; w < n_win; w++)
        for (int64_t a = win[w].begin; a < win[w].end; a += (int64_t)1 << 22) pieces.push_back({w, a, std::min(win[w].end, a + ((int64_t)1 << 22))});
    parallel_blocks(ctx->threads, pieces.size(), 1, [&](uint64_t a, uint64_t) {
        const Piece pc = pieces[a];
        const gci_window W = win[pc.w];
        auto emit = [&](bool is_end, int64_t at) {
            const uint32_t k = n.fetch_add(1);
            if (k < cap) keys[k] = ((uint64_t)pc.w << 33) | ((uint64_t)(at - W.begin) << 1) | (is_end ? 1u : 0u);
        };
        auto in_range = [&](int64_t i) { const double d = (double)depth[i]; return lo < d && d <= hi; };
        bool in = pc.lo > W.begin ? in_range(pc.lo - 1) : false;
        for (int64_t i = pc.lo; i < pc.hi; i++) {
            const bool now = in_range(i);
            if (now != in) { emit(in, i); in = now; }
        }
        if (in && pc.hi == W.end) emit(true, W.end);
    });
    *n_keys = n.load();
    return GCI_OK;
}

uint32_t decimal_width(int32_t v)
{
    uint32_t w = v < 0 ? 1u : 0u;
    uint64_t a = v < 0 ? (uint64_t)(-(int64_t)v) : (uint64_t)v;
    do { w++; a /= 10; } while (a);
    return w;
}

// depth_to_bedgraph.py: a window clamped to the track as the issue scan clamps it; the decimal width of a coordinate and its digits;
// the bytes of every window's lines  name '\t' start '\t' end '\t' depth '\n'
gci_window bg_clamp(const gci_ctx* ctx, gci_window w)
{
    w.begin = std::max<int64_t>(w.begin, 0);
    w.end = std::min<int64_t>(w.end, ctx->total);
    if (w.end < w.begin) w.end = w.begin;
    return w;
}

uint32_t bg_width(uint64_t v)
{
    uint32_t w = 0;
    do { w++; v /= 10; } while (v);
    return w;
}

uint8_t* bg_put(uint8_t* p, uint64_t v)
{
    const uint32_t w = bg_width(v);
    for (uint32_t d = w; d-- > 0;) { p[d] = (uint8_t)('0' + v % 10); v /= 10; }
    return p + w;
}

int bg_window_bytes(gci_ctx* ctx, const gci_depth_run* runs, const uint64_t* win_run0, const gci_window* h_windows, uint32_t n_windows,
                    const int64_t* h_coord0, const uint32_t* h_name_len, std::vector<uint64_t>& bytes)
{
    bytes.assign(n_windows, 0);
    for (uint32_t w = 0; w < n_windows; w++) {
        const gci_window c = bg_clamp(ctx, h_windows[w]);
        if (c.end - c.begin > 0xFFFFFFFFll || h_coord0[w] < 0 || h_name_len[w] > 65535u) return GCI_E_INVALID;
    }
    parallel_blocks(ctx->threads, n_windows, 1, [&](uint64_t w, uint64_t) {
        const gci_window c = bg_clamp(ctx, h_windows[w]);
        uint64_t s = 0;
        for (uint64_t k = win_run0[w]; k < win_run0[w + 1]; k++) {
            const uint64_t rel_end = k + 1 < win_run0[w + 1] ? (uint64_t)runs[k + 1].start : (uint64_t)(c.end - c.begin);
            s += h_name_len[w] + 4u + bg_width((uint64_t)h_coord0[w] + runs[k].start) + bg_width((uint64_t)h_coord0[w] + rel_end) +
                 decimal_width(runs[k].depth);
        }
        bytes[w] = s;
    });
    return GCI_OK;
}

// mismatch_sites.py, allele_sites.py: the records of gci_bam_mismatch_size, a base at a time (include/gci_hip.h) -- event(contig, p, nib)
// for every compared pair whose codes differ, nib the read's; the status word, the records counted and the pairs compared
template <typename F>
void mismatch_records(const gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, const int32_t* ref_sel,
                      int32_t n_ref, uint32_t excl_flags, int min_mapq, const uint8_t* codes, uint64_t& st, uint64_t& counted, uint64_t& compared,
                      F event)
{
    st = ~0ull; counted = 0; compared = 0;
    for (uint32_t i = 0; i < n_rec; i++) {
        const uint64_t word = ((uint64_t)i << 8) | (uint64_t)(uint8_t)(-GCI_E_MALFORMED);
        gci_ctx::CoverRec r;
        SeqAt sq;
        if (cover_parse(bam, n_bytes, rec_off[i], true, ref_sel, n_ref, excl_flags, min_mapq, r, &sq) != GCI_OK) { st = std::min(st, word); continue; }
        if (r.contig < 0) continue;                                         // skipped
        counted++;
        const uint8_t* ops = bam + r.ops_off;
        const uint8_t* seq = bam + sq.seq_off;
        const uint64_t n = r.n_ops;
        const uint32_t l_seq = sq.l_seq;
        // first pass: codes 9 - 15 and the query length
        bool bad = false;
        uint64_t qlen = 0;
        for (uint64_t k = 0; k < n; k++) {
            const uint32_t w = rd32(ops + 4 * k), op = w & 0xFu;
            if (op >= 9u) bad = true;
            if (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) qlen += w >> 4;          // M I S = X
        }
        if (l_seq > 0 && qlen != (uint64_t)l_seq) bad = true;
        if (bad) st = std::min(st, word);
        if (l_seq == 0 || qlen != (uint64_t)l_seq) continue;                    // nothing of it is compared
        const int32_t contig = r.contig, pos = r.pos;
        const uint64_t L = contig < ctx->n_contigs ? std::min<uint64_t>((uint64_t)ctx->len[(size_t)contig], 0x7FFFFFFEull) : 0;
        const uint8_t* ref = L ? codes + ctx->off[(size_t)contig] : codes;
        uint64_t at = (uint64_t)pos, q = 0;
        for (uint64_t k = 0; k < n && at < L; k++) {
            const uint32_t w = rd32(ops + 4 * k), op = w & 0xFu;
            const uint64_t len = w >> 4;
            if (op == 0u || op == 7u || op == 8u) {
                for (uint64_t j = 0; j < len && at + j < L; j++) {
                    const uint32_t sb = seq[(q + j) >> 1], nib = ((q + j) & 1u) ? (sb & 15u) : (sb >> 4), rc = ref[at + j];
                    const bool rb = rc == 1 || rc == 2 || rc == 4 || rc == 8, qb = nib == 1 || nib == 2 || nib == 4 || nib == 8;
                    if (!rb || !qb) continue;
                    compared++;
                    if (rc != nib) event(contig, (int32_t)(at + j), nib);
                }
            }
            if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) at += len;              // M D N = X
            if (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) q += len;               // M I S = X
        }
    }
}

}  // namespace

extern "C" {

int gci_abi_version(void) { return GCI_ABI_VERSION; }

int gci_ctx_create(int, void*, int, gci_ctx** out)
{
    if (!out) return GCI_E_INVALID;
    gci_ctx* c = new (std::nothrow) gci_ctx;
    if (!c) return GCI_E_NOMEM;
    const char* e = getenv("GCI_CPU_THREADS");
    const int hw = (int)std::thread::hardware_concurrency();
    c->threads = e && atoi(e) > 0 ? atoi(e) : (hw > 0 ? hw : 1);
    *out = c;
    return GCI_OK;
}
int gci_ctx_destroy(gci_ctx* ctx) { delete ctx; return GCI_OK; }
int gci_sync(gci_ctx* ctx) { return ctx ? GCI_OK : GCI_E_INVALID; }
/* libgci_cpu.so only.  "threads": host threads of the calls on this context (value 0 asks, > 0 sets); "heads": != 0 makes
 * gci_bam_filter read a heads stream (the records without SEQ / QUAL: gci_bam_heads).  Returns the value in force, -1: no such option. */
int gci_cpu_option(gci_ctx* ctx, const char* name, int value)
{
    if (!ctx || !name) return -1;
    if (!strcmp(name, "threads")) { if (value > 0) ctx->threads = value; return ctx->threads; }
    if (!strcmp(name, "heads")) { ctx->heads = value != 0; return ctx->heads ? 1 : 0; }
    return -1;
}
const char* gci_strerror(int status)
{
    switch (status) {
    case GCI_OK: return "ok";
    case GCI_E_INVALID: return "invalid argument";
    case GCI_E_HIP: return "HIP runtime error";
    case GCI_E_NO_NM: return "record has no NM tag";
    case GCI_E_ZERO_DIV: return "division by zero";
    case GCI_E_BAD_NM_TYPE: return "NM tag is not an integer";
    case GCI_E_NO_END: return "record has no reference end";
    case GCI_E_MALFORMED: return "malformed record";
    case GCI_E_CAPACITY: return "output buffer too small";
    case GCI_E_NOMEM: return "out of memory";
    case GCI_E_NO_LAYOUT: return "gci_layout_set has not been called";
    default: return "unknown status";
    }
}
const char* gci_last_error(gci_ctx* ctx) { return ctx ? ctx->err.c_str() : ""; }
int gci_malloc(gci_ctx* ctx, size_t bytes, void** out)
{
    if (!ctx || !out) return GCI_E_INVALID;
    void* p = nullptr;
    if (posix_memalign(&p, 64, bytes ? bytes : 64) != 0) return GCI_E_NOMEM;
    *out = p;
    return GCI_OK;
}
int gci_free(gci_ctx* ctx, void* p) { if (!ctx) return GCI_E_INVALID; free(p); return GCI_OK; }
int gci_memcpy_h2d(gci_ctx* ctx, void* dst, const void* src, size_t bytes) { if (!ctx) return GCI_E_INVALID; memcpy(dst, src, bytes); return GCI_OK; }
int gci_memcpy_d2h(gci_ctx* ctx, void* dst, const void* src, size_t bytes) { if (!ctx) return GCI_E_INVALID; memcpy(dst, src, bytes); return GCI_OK; }
int gci_memset(gci_ctx* ctx, void* dst, int byte, size_t bytes) { if (!ctx) return GCI_E_INVALID; memset(dst, byte, bytes); return GCI_OK; }

/* ---- layout: as libgci_hip.so lays a track out (contigs at multiples of GCI_TILE elements), so that tracks are interchangeable ---- */
int gci_layout_set(gci_ctx* ctx, int32_t n_contigs, const int64_t* h_lengths)
{
    if (!ctx || n_contigs <= 0 || !h_lengths) return GCI_E_INVALID;
    ctx->len.assign(h_lengths, h_lengths + n_contigs);
    ctx->off.assign((size_t)n_contigs, 0);
    int64_t at = 0;
    for (int32_t c = 0; c < n_contigs; c++) {
        if (h_lengths[c] < 0) return GCI_E_INVALID;
        ctx->off[(size_t)c] = at;
        at += (h_lengths[c] + GCI_TILE - 1) / GCI_TILE * GCI_TILE;
    }
    ctx->total = at > 0 ? at : GCI_TILE;
    ctx->n_contigs = n_contigs;
    ctx->bg_track = nullptr; ctx->bg_text_run0 = nullptr;
    ctx->clip_valid = false; ctx->sites_ask.valid = false;
    ctx->indel_valid = false; ctx->isites_ask.valid = false;
    ctx->mm_valid = false; ctx->msites_ask.valid = false;
    return GCI_OK;
}
int64_t gci_layout_total(gci_ctx* ctx) { return ctx ? ctx->total : 0; }
int gci_layout_offsets(gci_ctx* ctx, int64_t* h_offsets)
{
    const int st = need_layout(ctx);
    if (st) return st;
    if (!h_offsets) return GCI_E_INVALID;
    memcpy(h_offsets, ctx->off.data(), (size_t)ctx->n_contigs * sizeof(int64_t));
    return GCI_OK;
}

/* ---- R1 ---------------------------------------------------------------------------------------------------------------- */
uint64_t gci_name_hash(const uint8_t* h_name, uint32_t len) { return name_hash(h_name, len); }

int gci_decode_status(uint64_t word, uint32_t* rec_idx)
{
    if (word == ~0ull) { if (rec_idx) *rec_idx = 0; return GCI_OK; }
    if (rec_idx) *rec_idx = (uint32_t)(word >> 8);
    return -(int)(word & 0xFFu);
}

int gci_bam_filter(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, const int32_t* ref_sel,
                   int32_t n_ref, int map_qual, int mq_cutoff, double clip_percent, double iden_percent, uint32_t rec_idx_base, gci_rec* out,
                   uint64_t* status)
{
    if (!ctx || !status || (n_rec && (!bam || !rec_off || !ref_sel || !out))) return GCI_E_INVALID;
    std::atomic<uint64_t> st{~0ull};
    parallel_blocks(ctx->threads, n_rec, 4096, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            gci_rec r;
            r.name_hash = 0; r.contig = -1; r.start = 0; r.end = 0; r.qlen = 0; r.rec_idx = (uint32_t)i + rec_idx_base; r.mapq = 0; r.flags = 0;
            r.name_len = 0;
            const int code = filter_record(bam, n_bytes, rec_off[i], ref_sel, n_ref, map_qual, mq_cutoff, clip_percent, iden_percent, !ctx->heads, r);
            if (code != GCI_OK) report(st, (uint32_t)i, code);
            out[i] = r;
        }
    });
    *status = st.load();
    return GCI_OK;
}

/* ---- R5: the cross-file join (GCI.py:272-301), name by name ------------------------------------------------------------------ */
int gci_name_join(gci_ctx* ctx, const gci_join_file* files, int n_files, double ovlp_percent, const int32_t* contig_map, gci_ivl* out,
                  uint32_t cap, uint32_t* n_out, uint64_t* status)
{
    if (!ctx || !files || n_files < 1 || n_files > GCI_MAX_JOIN_FILES || !n_out || !status || (cap && !out)) return GCI_E_INVALID;
    struct Ref { uint64_t hash; const uint8_t* name; uint32_t pos; uint16_t len; uint8_t file; uint8_t hq; const gci_rec* rec; };
    // the passing records of every file (read_sam keeps nothing else, GCI.py:166), cut into parts by their hash: a name lives in one part
    const int parts = std::max(1, std::min(256, ctx->threads * 4));
    std::vector<std::vector<Ref>> by_part((size_t)parts);
    {
        std::vector<std::vector<std::vector<Ref>>> local((size_t)ctx->threads, std::vector<std::vector<Ref>>((size_t)parts));
        for (int f = 0; f < n_files; f++) {
            const gci_join_file& F = files[f];
            if (F.n_recs && (!F.d_recs || !F.d_name_base || !F.d_name_off)) return GCI_E_INVALID;
            std::atomic<uint64_t> next{0};
            on_threads(ctx->threads, [&](int t, int) {
                auto& mine = local[(size_t)t];
                for (;;) {
                    const uint64_t lo = next.fetch_add(8192);
                    if (lo >= F.n_recs) break;
                    const uint64_t hi = std::min<uint64_t>(F.n_recs, lo + 8192);
                    for (uint64_t i = lo; i < hi; i++) {
                        const gci_rec& r = F.d_recs[i];
                        if (!(r.flags & GCI_REC_PASS)) continue;
                        mine[(size_t)((r.name_hash >> 33) % (uint64_t)parts)].push_back(
                            Ref{r.name_hash, F.d_name_base + F.d_name_off[i] + F.name_delta, (uint32_t)i, r.name_len, (uint8_t)f,
                                (uint8_t)((r.flags & GCI_REC_HQ) ? 1 : 0), &r});
                    }
                }
            });
        }
        on_threads(ctx->threads, [&](int t, int nt) {
            for (int p = t; p < parts; p += nt) {
                size_t n = 0;
                for (auto& l : local) n += l[(size_t)p].size();
                by_part[(size_t)p].reserve(n);
                for (auto& l : local) by_part[(size_t)p].insert(by_part[(size_t)p].end(), l[(size_t)p].begin(), l[(size_t)p].end());
            }
        });
    }
    std::atomic<uint32_t> n{0};
    std::atomic<uint64_t> st{~0ull};
    parallel_blocks(ctx->threads, (uint64_t)parts, 1, [&](uint64_t p, uint64_t) {
        auto& v = by_part[(size_t)p];
        // same name together (hash, then the bytes), files in order, positions in order
        std::sort(v.begin(), v.end(), [](const Ref& a, const Ref& b) {
            if (a.hash != b.hash) return a.hash < b.hash;
            if (a.len != b.len) return a.len < b.len;
            const int c = memcmp(a.name, b.name, a.len);
            if (c) return c < 0;
            if (a.file != b.file) return a.file < b.file;
            return a.pos < b.pos;
        });
        for (size_t a = 0; a < v.size();) {
            size_t b = a + 1;
            while (b < v.size() && v[b].hash == v[a].hash && v[b].len == v[a].len && memcmp(v[b].name, v[a].name, v[a].len) == 0) b++;
            // per file the LAST record of the name (dict semantics, GCI.py:166, 269); high quality if ANY passing record of it was (:167-168)
            const gci_rec* last[GCI_MAX_JOIN_FILES] = {nullptr};
            bool hq = false;
            int present = 0;
            for (size_t k = a; k < b; k++) { if (!last[v[k].file]) present++; last[v[k].file] = v[k].rec; hq = hq || v[k].hq; }
            bool have = false;
            int32_t contig = 0, s = 0, e = 0;
            if (n_files == 1) { have = true; contig = last[0]->contig; s = last[0]->start; e = last[0]->end; }
            else {
                const bool in_final = hq || present == n_files;                         // GCI.py:277-279
                if (last[0] && in_final) { have = true; contig = last[0]->contig; s = last[0]->start; e = last[0]->end; }
                for (int f = 1; f < n_files; f++) {
                    const gci_rec* r = last[f];
                    if (!r) continue;
                    if (have) {
                        if (r->contig == contig) {
                            const int64_t ovlp = (int64_t)std::min(r->end, e) - (int64_t)std::max(r->start, s);
                            if (r->qlen == 0) { report(st, r->rec_idx, GCI_E_ZERO_DIV); have = false; }     // ZeroDivisionError, GCI.py:292
                            else if ((double)ovlp / (double)r->qlen < ovlp_percent) have = false;
                            else { s = std::max(r->start, s); e = std::min(r->end, e); }
                        } else have = false;                                             // GCI.py:296-297
                    } else if (hq) { have = true; contig = r->contig; s = r->start; e = r->end; }   // GCI.py:298-299
                }
            }
            if (have) {
                const int32_t c = contig_map ? contig_map[contig] : contig;
                if (c >= 0) {
                    const uint32_t k = n.fetch_add(1);
                    if (k < cap) out[k] = gci_ivl{c, s, e, 0};
                }
            }
            a = b;
        }
    });
    *n_out = n.load();
    *status = st.load();
    return GCI_OK;
}

/* ---- filter_depth.py --join: what the join does with every record (k_join.hip's gci_name_join_fate, k_fate.hip's gci_fate_refine) as
 * plain loops: one map from a name to its winners, the statement of include/gci_hip.h name by name, then the records once more ------- */
int gci_name_join_fate(gci_ctx* ctx, const gci_join_file* files, int n_files, double ovlp_percent, uint8_t* const* fate, uint64_t* counts,
                       uint64_t* status)
{
    if (!ctx || !files || n_files < 1 || n_files > GCI_MAX_JOIN_FILES || !fate || !counts || !status) return GCI_E_INVALID;
    for (int f = 0; f < n_files; f++)
        if (files[f].n_recs && (!files[f].d_recs || !files[f].d_name_base || !files[f].d_name_off || !fate[f])) return GCI_E_INVALID;
    struct Name { uint64_t last[GCI_MAX_JOIN_FILES]; bool hq; uint8_t verdict; };
    std::unordered_map<std::string, Name> names;
    auto key_of = [&](const gci_join_file& F, uint32_t i) {                              // the name's bytes, and its hash as the device compares it
        const gci_rec& r = F.d_recs[i];
        std::string k((const char*)(F.d_name_base + F.d_name_off[i] + F.name_delta), r.name_len);
        k.append((const char*)&r.name_hash, 8);
        return k;
    };
    auto order_of = [](const gci_rec& r, uint32_t i) { return (((uint64_t)(uint32_t)r.contig << 32) | i) + 1; };   // contig by contig, file order inside
    for (int f = 0; f < n_files; f++) {
        for (uint32_t i = 0; i < files[f].n_recs; i++) {
            const gci_rec& r = files[f].d_recs[i];
            if (!(r.flags & GCI_REC_PASS)) continue;
            auto it = names.find(key_of(files[f], i));
            if (it == names.end()) it = names.emplace(key_of(files[f], i), Name{{0}, false, 0}).first;
            it->second.last[f] = std::max(it->second.last[f], order_of(r, i));
            if (r.flags & GCI_REC_HQ) it->second.hq = true;
        }
    }
    uint64_t st = ~0ull;
    for (auto& kv : names) {
        Name& n = kv.second;
        if (n_files == 1) { n.verdict = GCI_FATE_JOINED; continue; }
        bool comm = true;
        for (int f = 0; f < n_files; f++) comm = comm && n.last[f] != 0;
        bool have = n.last[0] != 0 && (n.hq || comm);
        uint8_t why = GCI_FATE_UNPAIRED;
        int32_t contig = 0, s = 0, e = 0;
        if (have) { const gci_rec& r = files[0].d_recs[(uint32_t)(n.last[0] - 1)]; contig = r.contig; s = r.start; e = r.end; }
        for (int f = 1; f < n_files; f++) {
            if (!n.last[f]) continue;
            const gci_rec& r = files[f].d_recs[(uint32_t)(n.last[f] - 1)];
            if (have) {
                if (r.contig != contig) { have = false; why = GCI_FATE_CONTIG; continue; }
                const int32_t ms = std::max(r.start, s), me = std::min(r.end, e);
                if (r.qlen == 0) {                                                       // ZeroDivisionError, GCI.py:292: the fold ends here
                    st = std::min(st, ((uint64_t)r.rec_idx << 8) | (uint64_t)(uint8_t)(-GCI_E_ZERO_DIV));
                    have = false; why = GCI_FATE_OVERLAP;
                    break;
                }
                if ((double)((int64_t)me - (int64_t)ms) / (double)r.qlen < ovlp_percent) { have = false; why = GCI_FATE_OVERLAP; }
                else { s = ms; e = me; }
            } else if (n.hq) { have = true; contig = r.contig; s = r.start; e = r.end; }
        }
        n.verdict = have ? (uint8_t)GCI_FATE_JOINED : why;
    }
    for (int f = 0; f < n_files; f++) {
        uint64_t* row = counts + (size_t)f * GCI_JOIN_FATE_CLASSES;
        for (int c = 0; c < GCI_JOIN_FATE_CLASSES; c++) row[c] = 0;
        for (uint32_t i = 0; i < files[f].n_recs; i++) {
            const gci_rec& r = files[f].d_recs[i];
            uint8_t c = 0;
            if (r.flags & GCI_REC_PASS) {
                const Name& n = names.find(key_of(files[f], i))->second;
                c = n.last[f] == order_of(r, i) ? n.verdict : (uint8_t)GCI_FATE_SHADOWED;
            }
            fate[f][i] = c;
            row[c]++;
        }
    }
    *status = st;
    return GCI_OK;
}

int gci_fate_refine(gci_ctx* ctx, uint8_t* cls, const uint8_t* join_fate, uint32_t n_rec, uint64_t* status)
{
    if (!ctx || !status || (n_rec && (!cls || !join_fate))) return GCI_E_INVALID;
    uint64_t st = ~0ull;
    for (uint32_t i = 0; i < n_rec; i++) {
        const bool joined = join_fate[i] >= GCI_FATE_SHADOWED && join_fate[i] <= GCI_FATE_JOINED;
        if (cls[i] == GCI_FATE_KEPT && joined) cls[i] = join_fate[i];
        else if (cls[i] == GCI_FATE_KEPT || join_fate[i] != 0) st = std::min(st, ((uint64_t)i << 8) | (uint64_t)(uint8_t)(-GCI_E_INVALID));
    }
    *status = st;
    return GCI_OK;
}

/* ---- R6: depths[c][s + flank : e - flank + 1] += 1 (GCI.py:302-306), NumPy slice semantics ----------------------------------- */
int gci_depth_build(gci_ctx* ctx, const gci_ivl* ivl, const uint32_t* d_n, uint32_t max_n, int flank, int32_t* depth)
{
    const int st = need_layout(ctx);
    if (st) return st;
    if (!depth || (max_n && !ivl)) return GCI_E_INVALID;
    const uint32_t n = d_n ? std::min(*d_n, max_n) : max_n;
    // the track as a difference array (atomic +1 / -1 at the slice's ends), then a running sum per contig, blocks side by side
    parallel_blocks(ctx->threads, (uint64_t)ctx->total, (uint64_t)1 << 22, [&](uint64_t lo, uint64_t hi) { memset(depth + lo, 0, (hi - lo) * sizeof(int32_t)); });
    parallel_blocks(ctx->threads, n, 1 << 16, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const gci_ivl v = ivl[i];
            if (v.contig < 0 || v.contig >= ctx->n_contigs) continue;
            const int64_t L = ctx->len[(size_t)v.contig], base = ctx->off[(size_t)v.contig];
            const int64_t a = gci_slice_bound((int64_t)v.start + flank, L), b = gci_slice_bound((int64_t)v.end - flank + 1, L);
            if (a >= b) continue;
            __atomic_fetch_add(&depth[base + a], 1, __ATOMIC_RELAXED);
            if (b < L) __atomic_fetch_add(&depth[base + b], -1, __ATOMIC_RELAXED);
        }
    });
    struct Blk { int64_t lo, hi; int32_t c; int64_t sum; };
    std::vector<Blk> blocks;
    const int64_t B = (int64_t)1 << 22;
    for (int32_t c = 0; c < ctx->n_contigs; c++)
        for (int64_t a = 0; a < ctx->len[(size_t)c]; a += B) blocks.push_back({ctx->off[(size_t)c] + a, ctx->off[(size_t)c] + std::min(ctx->len[(size_t)c], a + B), c, 0});
    parallel_blocks(ctx->threads, blocks.size(), 1, [&](uint64_t k, uint64_t) {
        int64_t s = 0;
        for (int64_t i = blocks[k].lo; i < blocks[k].hi; i++) s += depth[i];
        blocks[k].sum = s;
    });
    std::vector<int64_t> carry(blocks.size(), 0);
    for (size_t k = 1; k < blocks.size(); k++) carry[k] = blocks[k].c == blocks[k - 1].c ? carry[k - 1] + blocks[k - 1].sum : 0;
    parallel_blocks(ctx->threads, blocks.size(), 1, [&](uint64_t k, uint64_t) {
        int64_t run = carry[k];
        for (int64_t i = blocks[k].lo; i < blocks[k].hi; i++) { run += depth[i]; depth[i] = (int32_t)run; }
    });
    return GCI_OK;
}

/* ---- R8: depths[c][a:b] = 0 (GCI.py:324-328) --------------------------------------------------------------------------------- */
int gci_gap_mask(gci_ctx* ctx, int32_t* depth, const gci_ivl* gaps, uint32_t n_gaps)
{
    const int st = need_layout(ctx);
    if (st) return st;
    if (!depth || (n_gaps && !gaps)) return GCI_E_INVALID;
    parallel_blocks(ctx->threads, n_gaps, 1, [&](uint64_t i, uint64_t) {
        const gci_ivl g = gaps[i];
        if (g.contig < 0 || g.contig >= ctx->n_contigs) return;
        const int64_t L = ctx->len[(size_t)g.contig];
        const int64_t a = gci_slice_bound(g.start, L), b = gci_slice_bound(g.end, L);
        if (a < b) memset(depth + ctx->off[(size_t)g.contig] + a, 0, (size_t)(b - a) * sizeof(int32_t));
    });
    return GCI_OK;
}

/* ---- R9: max(h[i], n[i]) per base (GCI.py:350) ---------------------------------------------------------------------------------- */
int gci_max2(gci_ctx* ctx, const int32_t* a, const int32_t* b, int32_t* out)
{
    const int st = need_layout(ctx);
    if (st) return st;
    if (!a || !b || !out) return GCI_E_INVALID;
    parallel_blocks(ctx->threads, (uint64_t)ctx->total, (uint64_t)1 << 22, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) out[i] = std::max(a[i], b[i]);
    });
    return GCI_OK;
}

/* ---- bam_depth.py: the reference bases the records cover (k_cover.hip's twins; one interval per maximal run of a RECORD here) --------- */
int gci_bam_cover_size_sel(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq,
                           const int32_t* ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int count_del, const uint8_t* cls,
                           uint32_t class_mask, uint64_t* h_n_ivl, uint64_t* status)
{
    if (!ctx || !h_n_ivl || !status || n_ref < 0 || (n_rec && (!bam || !rec_off || !ref_sel))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    ctx->cover_valid = false;
    *h_n_ivl = 0;
    ctx->cover_rec.assign(n_rec, gci_ctx::CoverRec{0, 0, -1, 0});
    ctx->cover_ivl0.assign((size_t)n_rec + 1, 0);
    std::atomic<uint64_t> st{~0ull};
    parallel_blocks(ctx->threads, n_rec, 4096, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            gci_ctx::CoverRec& r = ctx->cover_rec[i];
            if (cover_parse(bam, n_bytes, rec_off[i], has_seq != 0, ref_sel, n_ref, excl_flags, min_mapq, r) != GCI_OK) { report(st, (uint32_t)i, GCI_E_MALFORMED); continue; }
            if (r.contig >= 0 && cls && !(cls[i] < 32u && ((class_mask >> cls[i]) & 1u))) r = gci_ctx::CoverRec{0, 0, -1, 0};   // not a class of the mask
            if (r.contig < 0) continue;
            uint64_t n = 0;
            if (!cover_walk(bam, r, count_del != 0, 0, [&](int32_t, int32_t) { n++; })) report(st, (uint32_t)i, GCI_E_MALFORMED);
            ctx->cover_ivl0[i + 1] = n;
        }
    });
    for (uint32_t i = 0; i < n_rec; i++) ctx->cover_ivl0[i + 1] += ctx->cover_ivl0[i];
    ctx->cover_status = st.load();
    ctx->cover_valid = true; ctx->cover_count_del = count_del != 0; ctx->cover_stream = bam; ctx->cover_off = rec_off;
    *status = ctx->cover_status;
    *h_n_ivl = ctx->cover_ivl0[n_rec];
    return GCI_OK;
}

int gci_bam_cover_size(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq,
                       const int32_t* ref_sel, int32_t n_ref, uint32_t excl_flags, int min_mapq, int count_del, uint64_t* h_n_ivl, uint64_t* status)
{
    return gci_bam_cover_size_sel(ctx, bam, n_bytes, rec_off, n_rec, has_seq, ref_sel, n_ref, excl_flags, min_mapq, count_del, nullptr, 0, h_n_ivl,
                                  status);
}

/* ---- filter_depth.py: the class of every record (k_fate.hip's twin: a record at a time) ------------------------------------------------ */
int gci_bam_fate(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const int32_t* ref_sel,
                 int32_t n_ref, int map_qual, double clip_percent, double iden_percent, uint8_t* cls, uint64_t* h_counts, uint64_t* status)
{
    if (!ctx || !h_counts || !status || n_ref < 0 || (n_rec && (!bam || !rec_off || !ref_sel || !cls))) return GCI_E_INVALID;
    std::atomic<uint64_t> st{~0ull};
    std::atomic<uint64_t> counts[GCI_FATE_CLASSES];
    for (auto& c : counts) c.store(0);
    parallel_blocks(ctx->threads, n_rec, 4096, [&](uint64_t lo, uint64_t hi) {
        uint64_t mine[GCI_FATE_CLASSES] = {0};
        for (uint64_t i = lo; i < hi; i++) {
            const int code = fate_record(bam, n_bytes, rec_off[i], has_seq != 0, ref_sel, n_ref, map_qual, clip_percent, iden_percent, cls[i]);
            if (code != GCI_OK) report(st, (uint32_t)i, code);
            mine[cls[i]]++;
        }
        for (int c = 0; c < GCI_FATE_CLASSES; c++) counts[c].fetch_add(mine[c]);
    });
    for (int c = 0; c < GCI_FATE_CLASSES; c++) h_counts[c] = counts[c].load();
    *status = st.load();
    return GCI_OK;
}

int gci_bam_cover_write(gci_ctx* ctx, const uint8_t* bam, uint64_t, const uint64_t* rec_off, uint32_t n_rec, int, gci_ivl* out, uint64_t cap,
                        uint64_t* status)
{
    if (!ctx || !status || (n_rec && (!bam || !rec_off))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if (!ctx->cover_valid || ctx->cover_rec.size() != n_rec || bam != ctx->cover_stream || rec_off != ctx->cover_off) return GCI_E_INVALID;
    const uint64_t total = ctx->cover_ivl0[n_rec];
    if (total && !out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    parallel_blocks(ctx->threads, n_rec, 4096, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const gci_ctx::CoverRec& r = ctx->cover_rec[i];
            if (r.contig < 0 || r.contig >= ctx->n_contigs) continue;
            const int64_t L = ctx->len[(size_t)r.contig];
            uint64_t k = ctx->cover_ivl0[i];
            cover_walk(bam, r, ctx->cover_count_del, (uint64_t)std::min<int64_t>(L, 0x7FFFFFFEll), [&](int32_t a, int32_t b) { out[k++] = gci_ivl{r.contig, a, b, 0}; });
        }
    });
    *status = ctx->cover_status;
    return GCI_OK;
}

/* ---- clip_sites.py: where alignments break off (k_clips.hip's twins, from the text of include/gci_hip.h: a record, an element at a time) ---- */
int gci_bam_clip_size(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const int32_t* ref_sel,
                      int32_t n_ref, uint32_t excl_flags, int min_mapq, int min_clip, uint64_t* h_counts, uint64_t* status)
{
    if (!ctx || !h_counts || !status || n_ref < 0 || min_clip < 1 || (n_rec && (!bam || !rec_off || !ref_sel))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    ctx->clip_valid = false;
    ctx->clip_left.clear(); ctx->clip_right.clear();
    uint64_t st = ~0ull, counted = 0;
    auto is_clip = [](uint32_t w) { return (w & 0xFu) == 4u || (w & 0xFu) == 5u; };       // S, H
    for (uint32_t i = 0; i < n_rec; i++) {
        const uint64_t word = ((uint64_t)i << 8) | (uint64_t)(uint8_t)(-GCI_E_MALFORMED);
        gci_ctx::CoverRec r;
        SeqAt sq;
        if (cover_parse(bam, n_bytes, rec_off[i], has_seq != 0, ref_sel, n_ref, excl_flags, min_mapq, r, &sq) != GCI_OK) { st = std::min(st, word); continue; }
        if (r.contig < 0) continue;                                         // skipped
        // this tool's rule on top: <l_seq>S in front of the record's own operations -- the placeholder without a usable CG array -- is
        // no clip: no operations, R counts as 0
        const uint8_t* ops = bam + r.ops_off;
        uint64_t n = r.n_ops;
        if (n > 0 && r.ops_off + 4 * n == sq.seq_off && (rd32(ops) & 0xFu) == 4u && (rd32(ops) >> 4) == sq.l_seq) n = 0;
        uint64_t R = 0;
        bool bad = false;
        for (uint64_t k = 0; k < n; k++) {
            const uint32_t w = rd32(ops + 4 * k), op = w & 0xFu;
            if (op >= 9u) bad = true;
            else if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) R += w >> 4;       // M D N = X
        }
        if (R == 0) continue;                                               // skipped as well
        counted++;
        if (bad) st = std::min(st, word);
        uint64_t lead = 0, trail = 0;
        if (is_clip(rd32(ops))) {
            lead = rd32(ops) >> 4;
            if (n > 1 && is_clip(rd32(ops + 4))) lead += rd32(ops + 4) >> 4;
        }
        if (is_clip(rd32(ops + 4 * (n - 1)))) {
            trail = rd32(ops + 4 * (n - 1)) >> 4;
            if (n > 1 && is_clip(rd32(ops + 4 * (n - 2)))) trail += rd32(ops + 4 * (n - 2)) >> 4;
        }
        const int32_t contig = r.contig, pos = r.pos;
        const uint64_t L = contig < ctx->n_contigs ? (uint64_t)ctx->len[(size_t)contig] : 0;
        const uint64_t right = (uint64_t)pos + R - 1;
        if (lead >= (uint64_t)min_clip && (uint64_t)pos < L) ctx->clip_left.push_back(gci_ivl{contig, pos, pos, 0});
        if (trail >= (uint64_t)min_clip && right < L) ctx->clip_right.push_back(gci_ivl{contig, (int32_t)right, (int32_t)right, 0});
    }
    ctx->clip_status = st;
    ctx->clip_valid = true; ctx->clip_n_rec = n_rec; ctx->clip_stream = bam; ctx->clip_off = rec_off;
    h_counts[0] = counted; h_counts[1] = ctx->clip_left.size(); h_counts[2] = ctx->clip_right.size();
    *status = st;
    return GCI_OK;
}

int gci_bam_clip_write(gci_ctx* ctx, const uint8_t* bam, uint64_t, const uint64_t* rec_off, uint32_t n_rec, int, gci_ivl* out, uint64_t cap,
                       uint64_t* status)
{
    if (!ctx || !status || (n_rec && (!bam || !rec_off))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if (!ctx->clip_valid || ctx->clip_n_rec != n_rec || bam != ctx->clip_stream || rec_off != ctx->clip_off) return GCI_E_INVALID;
    const uint64_t total = ctx->clip_left.size() + ctx->clip_right.size();
    if (total && !out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    std::copy(ctx->clip_left.begin(), ctx->clip_left.end(), out);
    std::copy(ctx->clip_right.begin(), ctx->clip_right.end(), out + ctx->clip_left.size());
    *status = ctx->clip_status;
    return GCI_OK;
}

int gci_clip_sites_size(gci_ctx* ctx, const int32_t* left, const int32_t* right, const int32_t* depth, int32_t min_reads,
                        const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !left || !right || !h_n_sites || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if ((((uintptr_t)left) | ((uintptr_t)right) | ((uintptr_t)depth)) & 15u) return GCI_E_INVALID;
    ctx->sites_ask.valid = false;
    *h_n_sites = 0;
    std::vector<gci_window> ws;
    if (!site_windows(ctx, h_windows, n_windows, ws)) return GCI_E_INVALID;   // not sorted and disjoint
    ctx->sites.clear();
    for (const gci_window& w : ws) {
        for (int64_t p = w.begin; p < w.end; p++) {
            if (left[p] < min_reads && right[p] < min_reads) continue;
            const int32_t c = (int32_t)(std::upper_bound(ctx->off.begin(), ctx->off.end(), p) - ctx->off.begin()) - 1;
            const int64_t pos = p - ctx->off[(size_t)c];
            if (pos >= ctx->len[(size_t)c]) continue;                       // padding
            ctx->sites.push_back(gci_clip_site{c, (int32_t)pos, left[p], right[p], depth ? depth[p] : 0, 0});
        }
    }
    ctx->sites_ask = site_ask(left, right, depth, min_reads, 0, n_windows);
    *h_n_sites = ctx->sites.size();
    return GCI_OK;
}

int gci_clip_sites_write(gci_ctx* ctx, const int32_t* left, const int32_t* right, const int32_t* depth, int32_t min_reads,
                         const gci_window* h_windows, uint32_t n_windows, gci_clip_site* out, uint64_t cap)
{
    if (!ctx || !left || !right || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    return sites_write(ctx->sites_ask, site_ask(left, right, depth, min_reads, 0, n_windows), ctx->sites, out, cap);
}

/* ---- indel_sites.py: long insertions and deletions in reads (k_indels.hip's twins, from the text of include/gci_hip.h: a record, an operation,
 * an element at a time) ---- */
int gci_bam_indel_size(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const int32_t* ref_sel,
                       int32_t n_ref, uint32_t excl_flags, int min_mapq, int min_len, uint64_t* h_counts, uint64_t* status)
{
    if (!ctx || !h_counts || !status || n_ref < 0 || min_len < 1 || (n_rec && (!bam || !rec_off || !ref_sel))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    ctx->indel_valid = false;
    ctx->indel_del.clear(); ctx->indel_ins.clear();
    uint64_t st = ~0ull, counted = 0;
    for (uint32_t i = 0; i < n_rec; i++) {
        const uint64_t word = ((uint64_t)i << 8) | (uint64_t)(uint8_t)(-GCI_E_MALFORMED);
        gci_ctx::CoverRec r;
        SeqAt sq;
        if (cover_parse(bam, n_bytes, rec_off[i], has_seq != 0, ref_sel, n_ref, excl_flags, min_mapq, r, &sq) != GCI_OK) { st = std::min(st, word); continue; }
        if (r.contig < 0) continue;                                         // skipped
        counted++;
        const uint8_t* ops = bam + r.ops_off;
        const uint64_t n = r.n_ops;
        const int32_t contig = r.contig, pos = r.pos;
        const uint64_t L = contig < ctx->n_contigs ? std::min<uint64_t>((uint64_t)ctx->len[(size_t)contig], 0x7FFFFFFEull) : 0;
        uint64_t at = (uint64_t)pos;
        bool bad = false;
        for (uint64_t k = 0; k < n; k++) {
            const uint32_t w = rd32(ops + 4 * k), op = w & 0xFu;
            const uint64_t len = w >> 4;
            if (op >= 9u) { bad = true; continue; }
            if (op == 2u && len >= (uint64_t)min_len && at < L)
                ctx->indel_del.push_back(gci_ivl{contig, (int32_t)at, (int32_t)(std::min(at + len, L) - 1), 0});
            if (op == 1u && len >= (uint64_t)min_len) {
                const uint64_t site = at > 0 ? at - 1 : 0;
                if (site < L) ctx->indel_ins.push_back(gci_ivl{contig, (int32_t)site, (int32_t)site, 0});
            }
            if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) at += len;              // M D N = X
        }
        if (bad) st = std::min(st, word);
    }
    ctx->indel_status = st;
    ctx->indel_valid = true; ctx->indel_n_rec = n_rec; ctx->indel_n_bytes = n_bytes; ctx->indel_stream = bam; ctx->indel_off = rec_off;
    h_counts[0] = counted; h_counts[1] = ctx->indel_del.size(); h_counts[2] = ctx->indel_ins.size();
    *status = st;
    return GCI_OK;
}

int gci_bam_indel_write(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int, gci_ivl* out, uint64_t cap,
                        uint64_t* status)
{
    if (!ctx || !status || (n_rec && (!bam || !rec_off))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if (!ctx->indel_valid || ctx->indel_n_rec != n_rec || ctx->indel_n_bytes != n_bytes || bam != ctx->indel_stream || rec_off != ctx->indel_off)
        return GCI_E_INVALID;
    const uint64_t total = ctx->indel_del.size() + ctx->indel_ins.size();
    if (total && !out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    std::copy(ctx->indel_del.begin(), ctx->indel_del.end(), out);
    std::copy(ctx->indel_ins.begin(), ctx->indel_ins.end(), out + ctx->indel_del.size());
    *status = ctx->indel_status;
    return GCI_OK;
}

int gci_indel_sites_size(gci_ctx* ctx, const int32_t* del, const int32_t* ins, const int32_t* depth, int32_t min_reads, const gci_window* h_windows,
                         uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !del || !ins || !h_n_sites || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if ((((uintptr_t)del) | ((uintptr_t)ins) | ((uintptr_t)depth)) & 15u) return GCI_E_INVALID;
    ctx->isites_ask.valid = false;
    *h_n_sites = 0;
    std::vector<gci_window> ws;
    if (!site_windows(ctx, h_windows, n_windows, ws)) return GCI_E_INVALID;   // not sorted and disjoint
    ctx->isites.clear();
    for (const gci_window& w : ws) {
        bool open = false;                                                  // a run never crosses from one window into the next
        for (int64_t p = w.begin; p < w.end; p++) {
            const int32_t c = (int32_t)(std::upper_bound(ctx->off.begin(), ctx->off.end(), p) - ctx->off.begin()) - 1;
            const int64_t pos = p - ctx->off[(size_t)c];
            const bool hot = pos < ctx->len[(size_t)c] && (del[p] >= min_reads || ins[p] >= min_reads);
            if (open && (!hot || pos == 0)) open = false;                   // ... nor from one contig into the next
            if (!hot) continue;
            if (!open) {
                ctx->isites.push_back(gci_indel_site{c, (int32_t)pos, (int32_t)pos, del[p], ins[p], depth ? depth[p] : 0});
                open = true;
            }
            gci_indel_site& s = ctx->isites.back();
            s.end = (int32_t)pos + 1;
            s.del = std::max(s.del, del[p]); s.ins = std::max(s.ins, ins[p]);
            if (depth) s.depth = std::max(s.depth, depth[p]);
        }
    }
    ctx->isites_ask = site_ask(del, ins, depth, min_reads, 0, n_windows);
    *h_n_sites = ctx->isites.size();
    return GCI_OK;
}

int gci_indel_sites_write(gci_ctx* ctx, const int32_t* del, const int32_t* ins, const int32_t* depth, int32_t min_reads, const gci_window* h_windows,
                          uint32_t n_windows, gci_indel_site* out, uint64_t cap)
{
    if (!ctx || !del || !ins || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    return sites_write(ctx->isites_ask, site_ask(del, ins, depth, min_reads, 0, n_windows), ctx->isites, out, cap);
}

/* ---- mismatch_sites.py: bases where the reads carry another base than the assembly (k_mismatch.hip's twins, from the text of
 * include/gci_hip.h: a byte, a record, a base, an element at a time) ---- */
int gci_fasta_codes(gci_ctx* ctx, const uint8_t* text, uint64_t n_bytes, const int64_t* body, uint32_t n_records, const int64_t* dst,
                    const uint64_t* tile_kept0, uint8_t* codes)
{
    if (!ctx || !codes || (n_bytes && (!text || !tile_kept0)) || (n_records && (!body || !dst))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if (((uintptr_t)text) & 15u) return GCI_E_INVALID;
    static const char iupac[] = "=ACMGRSVTWYHKDBN";
    for (uint32_t r = 0; r < n_records; r++) {
        if (dst[r] < 0) continue;
        const uint64_t a = (uint64_t)std::max<int64_t>(body[2 * r], 0), b = std::min<uint64_t>((uint64_t)std::max<int64_t>(body[2 * r + 1], 0), n_bytes);
        uint64_t e = (uint64_t)dst[r];
        for (uint64_t i = a; i < b; i++) {
            uint8_t c = text[i];
            if (c == '\n' || c == '\r' || c == ' ') continue;
            if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 'a' + 'A');
            if (c == 'U') c = 'T';
            uint8_t code = 15;
            for (int k = 1; k < 16; k++) if (c == (uint8_t)iupac[k]) code = (uint8_t)k;
            if (e < (uint64_t)ctx->total) codes[e] = code;
            e++;
        }
    }
    return GCI_OK;
}

int gci_bam_mismatch_size(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const int32_t* ref_sel,
                          int32_t n_ref, uint32_t excl_flags, int min_mapq, const uint8_t* codes, uint64_t* h_counts, uint64_t* status)
{
    if (!ctx || !h_counts || !status || !codes || n_ref < 0 || has_seq != 1 || (n_rec && (!bam || !rec_off || !ref_sel))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    ctx->mm_valid = false;
    ctx->mm_events.clear();
    uint64_t st, counted, compared;
    mismatch_records(ctx, bam, n_bytes, rec_off, n_rec, ref_sel, n_ref, excl_flags, min_mapq, codes, st, counted, compared,
                     [&](int32_t contig, int32_t p, uint32_t) { ctx->mm_events.push_back(gci_ivl{contig, p, p, 0}); });
    ctx->mm_status = st;
    ctx->mm_valid = true; ctx->mm_n_rec = n_rec; ctx->mm_n_bytes = n_bytes; ctx->mm_stream = bam; ctx->mm_off = rec_off; ctx->mm_codes = codes;
    h_counts[0] = counted; h_counts[1] = ctx->mm_events.size(); h_counts[2] = compared;
    *status = st;
    return GCI_OK;
}

int gci_bam_mismatch_write(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const uint8_t* codes,
                           gci_ivl* out, uint64_t cap, uint64_t* status)
{
    if (!ctx || !status || !codes || has_seq != 1 || (n_rec && (!bam || !rec_off))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if (!ctx->mm_valid || ctx->mm_n_rec != n_rec || ctx->mm_n_bytes != n_bytes || bam != ctx->mm_stream || rec_off != ctx->mm_off || codes != ctx->mm_codes)
        return GCI_E_INVALID;
    const uint64_t total = ctx->mm_events.size();
    if (total && !out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    std::copy(ctx->mm_events.begin(), ctx->mm_events.end(), out);
    *status = ctx->mm_status;
    return GCI_OK;
}

int gci_mismatch_sites_size(gci_ctx* ctx, const int32_t* mm, const int32_t* depth, int32_t min_reads, int32_t frac_ppm, const gci_window* h_windows,
                            uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !mm || !depth || !h_n_sites || min_reads < 1 || frac_ppm < 0 || frac_ppm > 1000000 || (n_windows && !h_windows)) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if ((((uintptr_t)mm) | ((uintptr_t)depth)) & 15u) return GCI_E_INVALID;
    ctx->msites_ask.valid = false;
    *h_n_sites = 0;
    std::vector<gci_window> ws;
    if (!site_windows(ctx, h_windows, n_windows, ws)) return GCI_E_INVALID;   // not sorted and disjoint
    ctx->msites.clear();
    for (const gci_window& w : ws) {
        bool open = false;                                                  // a run never crosses from one window into the next
        for (int64_t p = w.begin; p < w.end; p++) {
            const int32_t c = (int32_t)(std::upper_bound(ctx->off.begin(), ctx->off.end(), p) - ctx->off.begin()) - 1;
            const int64_t pos = p - ctx->off[(size_t)c];
            const bool hot = pos < ctx->len[(size_t)c] && mm[p] >= min_reads && (int64_t)mm[p] * 1000000ll >= (int64_t)frac_ppm * (int64_t)depth[p];
            if (open && (!hot || pos == 0)) open = false;                   // ... nor from one contig into the next
            if (!hot) continue;
            if (!open) {
                ctx->msites.push_back(gci_mismatch_site{c, (int32_t)pos, (int32_t)pos, mm[p], depth[p]});
                open = true;
            }
            gci_mismatch_site& s = ctx->msites.back();
            s.end = (int32_t)pos + 1;
            if (mm[p] > s.mismatch) { s.mismatch = mm[p]; s.depth = depth[p]; }   // the first base that reaches the maximum
        }
    }
    ctx->msites_ask = site_ask(mm, depth, nullptr, min_reads, frac_ppm, n_windows);
    *h_n_sites = ctx->msites.size();
    return GCI_OK;
}

int gci_mismatch_sites_write(gci_ctx* ctx, const int32_t* mm, const int32_t* depth, int32_t min_reads, int32_t frac_ppm, const gci_window* h_windows,
                             uint32_t n_windows, gci_mismatch_site* out, uint64_t cap)
{
    if (!ctx || !mm || !depth || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    return sites_write(ctx->msites_ask, site_ask(mm, depth, nullptr, min_reads, frac_ppm, n_windows), ctx->msites, out, cap);
}

/* ---- allele_sites.py: which base the reads carry where they disagree (the twins of k_mismatch.hip's allele calls, from the text of
 * include/gci_hip.h: a record, a base, an element at a time) ---- */
int gci_bam_allele_size(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const int32_t* ref_sel,
                        int32_t n_ref, uint32_t excl_flags, int min_mapq, const uint8_t* codes, uint64_t* h_counts, uint64_t* status)
{
    if (!ctx || !h_counts || !status || !codes || n_ref < 0 || has_seq != 1 || (n_rec && (!bam || !rec_off || !ref_sel))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    ctx->al_valid = false;
    for (auto& list : ctx->al_events) list.clear();
    uint64_t st, counted, compared;
    mismatch_records(ctx, bam, n_bytes, rec_off, n_rec, ref_sel, n_ref, excl_flags, min_mapq, codes, st, counted, compared,
                     [&](int32_t contig, int32_t p, uint32_t nib) {          // nib is 1, 2, 4 or 8: A, C, G, T
                         ctx->al_events[nib == 1 ? 0 : nib == 2 ? 1 : nib == 4 ? 2 : 3].push_back(gci_ivl{contig, p, p, 0});
                     });
    ctx->al_status = st;
    ctx->al_valid = true; ctx->al_n_rec = n_rec; ctx->al_n_bytes = n_bytes; ctx->al_stream = bam; ctx->al_off = rec_off; ctx->al_codes = codes;
    h_counts[0] = counted; h_counts[5] = compared;
    for (int k = 0; k < 4; k++) h_counts[1 + k] = ctx->al_events[k].size();
    *status = st;
    return GCI_OK;
}

int gci_bam_allele_write(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const uint8_t* codes,
                         gci_ivl* out, uint64_t cap, uint64_t* status)
{
    if (!ctx || !status || !codes || has_seq != 1 || (n_rec && (!bam || !rec_off))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if (!ctx->al_valid || ctx->al_n_rec != n_rec || ctx->al_n_bytes != n_bytes || bam != ctx->al_stream || rec_off != ctx->al_off || codes != ctx->al_codes)
        return GCI_E_INVALID;
    uint64_t total = 0;
    for (const auto& list : ctx->al_events) total += list.size();
    if (total && !out) return GCI_E_INVALID;
    if (cap < total) return GCI_E_CAPACITY;
    for (const auto& list : ctx->al_events) out = std::copy(list.begin(), list.end(), out);      // A, then C, then G, then T
    *status = ctx->al_status;
    return GCI_OK;
}

static gci_ctx::SiteAsk allele_ask(const int32_t* a, const int32_t* c, const int32_t* g, const int32_t* t, const int32_t* depth, const uint8_t* codes,
                                   int32_t min_reads, int32_t frac_ppm, uint32_t n_windows)
{
    gci_ctx::SiteAsk m = site_ask(a, c, g, min_reads, frac_ppm, n_windows);
    m.track[3] = t; m.track[4] = depth; m.track[5] = codes;
    return m;
}

int gci_allele_sites_size(gci_ctx* ctx, const int32_t* a, const int32_t* c, const int32_t* g, const int32_t* t, const int32_t* depth, const uint8_t* codes,
                          int32_t min_reads, int32_t frac_ppm, const gci_window* h_windows, uint32_t n_windows, uint64_t* h_n_sites)
{
    if (!ctx || !a || !c || !g || !t || !depth || !codes || !h_n_sites || min_reads < 1 || frac_ppm < 0 || frac_ppm > 1000000 || (n_windows && !h_windows))
        return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if ((((uintptr_t)a) | ((uintptr_t)c) | ((uintptr_t)g) | ((uintptr_t)t) | ((uintptr_t)depth)) & 15u) return GCI_E_INVALID;
    ctx->asites_ask.valid = false;
    *h_n_sites = 0;
    std::vector<gci_window> ws;
    if (!site_windows(ctx, h_windows, n_windows, ws)) return GCI_E_INVALID;   // not sorted and disjoint
    ctx->asites.clear();
    for (const gci_window& w : ws) {
        for (int64_t p = w.begin; p < w.end; p++) {
            const int32_t n[4] = {a[p], c[p], g[p], t[p]};
            int k = 0;                                                      // the first that reaches the largest: a tie goes to the earlier letter
            for (int j = 1; j < 4; j++) if (n[j] > n[k]) k = j;
            if (n[k] < min_reads || (int64_t)n[k] * 1000000ll < (int64_t)frac_ppm * (int64_t)depth[p]) continue;
            const int32_t contig = (int32_t)(std::upper_bound(ctx->off.begin(), ctx->off.end(), p) - ctx->off.begin()) - 1;
            const int64_t pos = p - ctx->off[(size_t)contig];
            if (pos >= ctx->len[(size_t)contig]) continue;                  // padding
            ctx->asites.push_back(gci_allele_site{contig, (int32_t)pos, (int32_t)codes[p], 1 << k, {n[0], n[1], n[2], n[3]}, depth[p]});
        }
    }
    ctx->asites_ask = allele_ask(a, c, g, t, depth, codes, min_reads, frac_ppm, n_windows);
    *h_n_sites = ctx->asites.size();
    return GCI_OK;
}

int gci_allele_sites_write(gci_ctx* ctx, const int32_t* a, const int32_t* c, const int32_t* g, const int32_t* t, const int32_t* depth, const uint8_t* codes,
                           int32_t min_reads, int32_t frac_ppm, const gci_window* h_windows, uint32_t n_windows, gci_allele_site* out, uint64_t cap)
{
    if (!ctx || !a || !c || !g || !t || !depth || !codes || min_reads < 1 || (n_windows && !h_windows)) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    return sites_write(ctx->asites_ask, allele_ask(a, c, g, t, depth, codes, min_reads, frac_ppm, n_windows), ctx->asites, out, cap);
}

/* ---- filter_reads.py: the records of chosen classes over a set of regions as rows of text (k_reads.hip's twins: a record at a time) ---- */
int gci_bam_reads_size(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const int32_t* ref_sel,
                       int32_t n_ref, const uint8_t* cls, uint32_t class_mask, const gci_window* win, const uint32_t* contig_win0,
                       const uint32_t* h_contig_name_len, uint32_t file_no, uint64_t* h_n_rows, uint64_t* h_n_bytes, uint64_t* status)
{
    if (!ctx || !h_n_rows || !h_n_bytes || !status || n_ref < 0 || (n_rec && (!bam || !rec_off || !ref_sel || !cls))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if ((class_mask & ~0x1F7Eu) || !h_contig_name_len || (contig_win0 && !win)) return GCI_E_INVALID;
    for (int32_t c = 0; c < ctx->n_contigs; c++) if (h_contig_name_len[c] > 65535u) return GCI_E_INVALID;
    ctx->reads_valid = false;
    *h_n_rows = 0; *h_n_bytes = 0;
    std::vector<gci_ctx::ReadsRow> all(n_rec);
    std::vector<uint8_t> made(n_rec, 0);
    std::atomic<uint64_t> st{~0ull};
    parallel_blocks(ctx->threads, n_rec, 4096, [&](uint64_t lo, uint64_t hi) {
        std::string text;
        for (uint64_t i = lo; i < hi; i++) {
            if (!(cls[i] < 32u && ((class_mask >> cls[i]) & 1u))) continue;  // (not read beyond its class byte)
            bool row = false;
            const int code = reads_record(bam, n_bytes, rec_off[i], has_seq != 0, ref_sel, n_ref, ctx->n_contigs, win, contig_win0, all[i], row);
            if (code != GCI_OK) report(st, (uint32_t)i, code);
            if (!row) continue;
            all[i].cls = cls[i];
            text.clear();
            reads_text(text, all[i], file_no, bam, nullptr, 0);
            all[i].byte0 = text.size() + h_contig_name_len[all[i].contig];   // (the row's length, until the scan below)
            made[i] = 1;
        }
    });
    ctx->reads_rows.clear();
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_rec; i++) {
        if (!made[i]) continue;
        const uint64_t len = all[i].byte0;
        all[i].byte0 = total;
        total += len;
        ctx->reads_rows.push_back(all[i]);
    }
    ctx->reads_name_len.assign(h_contig_name_len, h_contig_name_len + ctx->n_contigs);
    ctx->reads_total = total; ctx->reads_n_bytes = n_bytes; ctx->reads_n_rec = n_rec; ctx->reads_file_no = file_no;
    ctx->reads_stream = bam; ctx->reads_off = rec_off;
    ctx->reads_valid = true;
    *status = st.load();
    *h_n_rows = ctx->reads_rows.size();
    *h_n_bytes = total;
    return GCI_OK;
}

int gci_bam_reads_write(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, const uint8_t* contig_names,
                        const uint64_t* h_contig_name_off, const uint32_t* h_contig_name_len, uint8_t* out, uint64_t cap)
{
    if (!ctx || !h_contig_name_off || !h_contig_name_len || (n_rec && (!bam || !rec_off))) return GCI_E_INVALID;
    const int lst = need_layout(ctx);
    if (lst) return lst;
    if (!ctx->reads_valid || n_rec != ctx->reads_n_rec || n_bytes != ctx->reads_n_bytes || bam != ctx->reads_stream || rec_off != ctx->reads_off ||
        (size_t)ctx->n_contigs != ctx->reads_name_len.size())
        return GCI_E_INVALID;
    for (int32_t c = 0; c < ctx->n_contigs; c++) {
        if (h_contig_name_len[c] != ctx->reads_name_len[(size_t)c] || (h_contig_name_len[c] && !contig_names)) return GCI_E_INVALID;
    }
    if (ctx->reads_total && !out) return GCI_E_INVALID;
    if (cap < ctx->reads_total) return GCI_E_CAPACITY;
    parallel_blocks(ctx->threads, ctx->reads_rows.size(), 1024, [&](uint64_t lo, uint64_t hi) {
        std::string text;
        for (uint64_t k = lo; k < hi; k++) {
            const gci_ctx::ReadsRow& w = ctx->reads_rows[k];
            text.clear();
            reads_text(text, w, ctx->reads_file_no, bam, contig_names + h_contig_name_off[w.contig], h_contig_name_len[w.contig]);
            memcpy(out + w.byte0, text.data(), text.size());
        }
    });
    return GCI_OK;
}

/* ---- filter_sweep.py: the three tables of the record filter's thresholds (k_sweep.hip's twin: a plain loop over the records) ------------ */
int gci_bam_sweep(gci_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_off, uint32_t n_rec, int has_seq, const int32_t* ref_sel,
                  int32_t n_ref, const gci_window* win, const uint32_t* contig_win0, int map_qual, double clip_percent, double iden_percent, int digits,
                  uint64_t* h_table, uint64_t* status)
{
    if (!ctx || !h_table || !status || n_ref < 0 || (n_rec && (!bam || !rec_off || !ref_sel))) return GCI_E_INVALID;
    if (digits < 1 || digits > 3 || (contig_win0 && !win)) return GCI_E_INVALID;
    if (contig_win0) {
        const int lst = need_layout(ctx);
        if (lst) return lst;
    }
    const size_t cells = (size_t)GCI_SWEEP_COLS * GCI_SWEEP_ROWS(digits);
    std::fill(h_table, h_table + cells, (uint64_t)0);
    uint64_t st = ~0ull;
    for (uint32_t i = 0; i < n_rec; i++) {
        bool counted = false, pass[3];
        uint32_t rows[3];
        uint64_t M = 0;
        const int code = sweep_record(bam, n_bytes, rec_off[i], has_seq != 0, ref_sel, n_ref, ctx->n_contigs, win, contig_win0, map_qual, clip_percent,
                                      iden_percent, digits, counted, rows, pass, M);
        if (code != GCI_OK) st = std::min(st, ((uint64_t)i << 8) | (uint64_t)(uint8_t)(-code));
        if (!counted) continue;
        for (int k = 0; k < 3; k++) {
            uint64_t* row = h_table + (size_t)rows[k] * GCI_SWEEP_COLS;
            row[0] += 1; row[1] += M;
            if (pass[(k + 1) % 3] && pass[(k + 2) % 3]) { row[2] += 1; row[3] += M; }
        }
    }
    *status = st;
    return GCI_OK;
}

int gci_track_add(gci_ctx* ctx, int32_t* acc, const int32_t* add)
{
    const int st = need_layout(ctx);
    if (st) return st;
    if (!acc || !add || ((((uintptr_t)acc) | ((uintptr_t)add)) & 15u)) return GCI_E_INVALID;     // (16-byte aligned, as libgci_hip.so asks)
    parallel_blocks(ctx->threads, (uint64_t)ctx->total, (uint64_t)1 << 22, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) acc[i] += add[i];
    });
    return GCI_OK;
}

/* ---- R10: the run boundaries of collapse_depth_range (GCI.py:369-390), keys as libgci_hip.so emits them ----------------------------- */
int gci_issue_scan_windows(gci_ctx* ctx, const int32_t* depth, const gci_window* h_windows, uint32_t n_windows, double lo, double hi,
                           uint64_t* keys, uint32_t cap, uint32_t* n_keys)
{
    if (!ctx || (n_windows && !h_windows)) return GCI_E_INVALID;
    return issue_scan(ctx, depth, h_windows, n_windows, lo, hi, keys, cap, n_keys);
}

int gci_issue_scan(gci_ctx* ctx, const int32_t* depth, double lo, double hi, int flank, uint64_t* keys, uint32_t cap, uint32_t* n_keys)
{
    const int st = need_layout(ctx);
    if (st) return st;
    std::vector<gci_window> win((size_t)ctx->n_contigs);
    for (int32_t c = 0; c < ctx->n_contigs; c++) {
        const int64_t L = ctx->len[(size_t)c], base = ctx->off[(size_t)c];
        win[(size_t)c] = L > 2 * (int64_t)flank ? gci_window{base + flank, base + L - flank} : gci_window{base, base};
    }
    return issue_scan(ctx, depth, win.data(), (uint32_t)win.size(), lo, hi, keys, cap, n_keys);
}

/* ---- depth_plotter_v2.py: zero runs, low runs and the non-zero statistics of every window (k_depth_classes' twin) ------------------- */
int gci_depth_classes(gci_ctx* ctx, const int32_t* depth, const gci_window* h_windows, uint32_t n_windows, int32_t low_below, uint64_t* keys,
                      uint32_t cap, uint32_t* n_keys, int64_t* stats)
{
    if (!ctx || !depth || !n_keys || (cap && !keys) || (n_windows && (!h_windows || !stats))) return GCI_E_INVALID;
    const int st = need_layout(ctx);
    if (st) return st;
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    std::atomic<uint32_t> n[2];
    n[0] = 0; n[1] = 0;
    std::vector<std::atomic<int64_t>> acc((size_t)n_windows * 2);
    for (auto& a : acc) a = 0;
    // the windows clamped to the track, as the device's set_windows does; then in pieces of 4 M elements, as issue_scan
    struct Piece { uint32_t w; int64_t begin, end, lo, hi; };
    std::vector<Piece> pieces;
    for (uint32_t w = 0; w < n_windows; w++) {
        int64_t b = std::max<int64_t>(h_windows[w].begin, 0), e = std::min<int64_t>(h_windows[w].end, ctx->total);
        if (e < b) e = b;
        for (int64_t a = b; a < e; a += (int64_t)1 << 22) pieces.push_back({w, b, e, a, std::min(e, a + ((int64_t)1 << 22))});
    }
    auto cls = [&](int64_t i) { const int32_t d = depth[i]; return d == 0 ? 0 : (d > 0 && d < low_below) ? 1 : 2; };
    parallel_blocks(ctx->threads, pieces.size(), 1, [&](uint64_t a, uint64_t) {
        const Piece pc = pieces[a];
        auto emit = [&](int x, bool is_end, int64_t at) {
            const uint32_t k = n[x].fetch_add(1);
            if (k < cap) keys[(size_t)x * cap + k] = ((uint64_t)pc.w << 33) | ((uint64_t)(at - pc.begin) << 1) | (is_end ? 1u : 0u);
        };
        int in = pc.lo > pc.begin ? cls(pc.lo - 1) : 2;
        int64_t sum = 0, cnt = 0;
        for (int64_t i = pc.lo; i < pc.hi; i++) {
            const int now = cls(i);
            if (now != in) {
                if (in < 2) emit(in, true, i);
                if (now < 2) emit(now, false, i);
                in = now;
            }
            if (depth[i] > 0) { sum += depth[i]; cnt++; }
        }
        if (in < 2 && pc.hi == pc.end) emit(in, true, pc.end);
        acc[(size_t)pc.w * 2] += sum;
        acc[(size_t)pc.w * 2 + 1] += cnt;
    });
    n_keys[0] = n[0].load(); n_keys[1] = n[1].load();
    for (size_t i = 0; i < acc.size(); i++) stats[i] = acc[i].load();
    return GCI_OK;
}

/* ---- R7: f'{depth}\n' per base (GCI.py:115-117), contig after contig, without the '>' lines --------------------------------------- */
int gci_depth_text_size(gci_ctx* ctx, const int32_t* depth, uint64_t* contig_off)
{
    const int st = need_layout(ctx);
    if (st) return st;
    if (!depth || !contig_off) return GCI_E_INVALID;
    std::vector<std::atomic<uint64_t>> bytes((size_t)ctx->n_contigs);
    for (auto& b : bytes) b = 0;
    struct Blk { int64_t lo, hi; int32_t c; };
    std::vector<Blk> blocks;
    for (int32_t c = 0; c < ctx->n_contigs; c++)
        for (int64_t a = 0; a < ctx->len[(size_t)c]; a += (int64_t)1 << 22)
            blocks.push_back({ctx->off[(size_t)c] + a, ctx->off[(size_t)c] + std::min(ctx->len[(size_t)c], a + ((int64_t)1 << 22)), c});
    parallel_blocks(ctx->threads, blocks.size(), 1, [&](uint64_t k, uint64_t) {
        uint64_t s = 0;
        for (int64_t i = blocks[k].lo; i < blocks[k].hi; i++) s += decimal_width(depth[i]) + 1u;
        bytes[(size_t)blocks[k].c] += s;
    });
    uint64_t at = 0;
    for (int32_t c = 0; c < ctx->n_contigs; c++) { contig_off[c] = at; at += bytes[(size_t)c].load(); }
    contig_off[ctx->n_contigs] = at;
    return GCI_OK;
}

int gci_depth_text_write(gci_ctx* ctx, const int32_t* depth, uint8_t* out, uint64_t cap)
{
    const int st = need_layout(ctx);
    if (st) return st;
    if (!depth || !out) return GCI_E_INVALID;
    // sizes per block first, so that every block knows where its lines go
    struct Blk { int64_t lo, hi; uint64_t bytes, at; };
    std::vector<Blk> blocks;
    for (int32_t c = 0; c < ctx->n_contigs; c++)
        for (int64_t a = 0; a < ctx->len[(size_t)c]; a += (int64_t)1 << 20)
            blocks.push_back({ctx->off[(size_t)c] + a, ctx->off[(size_t)c] + std::min(ctx->len[(size_t)c], a + ((int64_t)1 << 20)), 0, 0});
    parallel_blocks(ctx->threads, blocks.size(), 1, [&](uint64_t k, uint64_t) {
        uint64_t s = 0;
        for (int64_t i = blocks[k].lo; i < blocks[k].hi; i++) s += decimal_width(depth[i]) + 1u;
        blocks[k].bytes = s;
    });
    uint64_t at = 0;
    for (auto& b : blocks) { b.at = at; at += b.bytes; }
    if (at > cap) return GCI_E_CAPACITY;
    parallel_blocks(ctx->threads, blocks.size(), 1, [&](uint64_t k, uint64_t) {
        uint8_t* w = out + blocks[k].at;
        for (int64_t i = blocks[k].lo; i < blocks[k].hi; i++) {
            const int32_t v = depth[i];
            uint64_t a = v < 0 ? (uint64_t)(-(int64_t)v) : (uint64_t)v;
            const uint32_t wd = decimal_width(v);
            if (v < 0) w[0] = '-';
            for (uint32_t d = wd; d-- > (v < 0 ? 1u : 0u);) { w[d] = (uint8_t)('0' + a % 10); a /= 10; }
            w[wd] = '\n';
            w += wd + 1;
        }
    });
    return GCI_OK;
}

/* ---- R15: the numerator of np.mean (GCI.py:862-868) ------------------------------------------------------------------------------ */
int gci_depth_sum(gci_ctx* ctx, const int32_t* depth, int64_t* sums)
{
    const int st = need_layout(ctx);
    if (st) return st;
    if (!depth || !sums) return GCI_E_INVALID;
    std::vector<std::atomic<int64_t>> acc((size_t)ctx->n_contigs);
    for (auto& a : acc) a = 0;
    struct Blk { int64_t lo, hi; int32_t c; };
    std::vector<Blk> blocks;
    for (int32_t c = 0; c < ctx->n_contigs; c++)
        for (int64_t a = 0; a < ctx->len[(size_t)c]; a += (int64_t)1 << 22)
            blocks.push_back({ctx->off[(size_t)c] + a, ctx->off[(size_t)c] + std::min(ctx->len[(size_t)c], a + ((int64_t)1 << 22)), c});
    parallel_blocks(ctx->threads, blocks.size(), 1, [&](uint64_t k, uint64_t) {
        int64_t s = 0;
        for (int64_t i = blocks[k].lo; i < blocks[k].hi; i++) s += depth[i];
        acc[(size_t)blocks[k].c] += s;
    });
    for (int32_t c = 0; c < ctx->n_contigs; c++) sums[c] = acc[(size_t)c].load();
    return GCI_OK;
}

/* ---- N3: window sums (sliding_window_average_depth, GCI.py:660-705) ---------------------------------------------------------------- */
int gci_range_sums(gci_ctx* ctx, const int32_t* depth, const int64_t* ranges, uint64_t n_ranges, int64_t* sums)
{
    if (!ctx || !depth || (n_ranges && (!ranges || !sums))) return GCI_E_INVALID;
    parallel_blocks(ctx->threads, n_ranges, 64, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t r = lo; r < hi; r++) {
            int64_t s = 0;
            for (int64_t i = ranges[2 * r]; i < ranges[2 * r + 1]; i++) s += depth[i];
            sums[r] = s;
        }
    });
    return GCI_OK;
}

/* ---- depth_dist.py: the depth histogram and the sum / min / max / count of every window (k_depth_hist's twin) ------------------------ */
int gci_depth_hist(gci_ctx* ctx, const int32_t* depth, const gci_window* h_windows, uint32_t n_windows, uint32_t n_bins, uint64_t* hist,
                   int64_t* stats)
{
    if (!ctx || !depth || (n_windows && (!h_windows || !stats || (n_bins && !hist)))) return GCI_E_INVALID;
    if (n_bins > GCI_HIST_MAX_BINS) return GCI_E_INVALID;
    const int st = need_layout(ctx);
    if (st) return st;
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    const size_t cols = (size_t)n_bins + 2;
    if (hist) memset(hist, 0, (size_t)n_windows * cols * 8);
    // the windows clamped to the track, in pieces of 4 M elements; a piece counts into a histogram of its own and adds it once
    struct Piece { uint32_t w; int64_t lo, hi; };
    std::vector<Piece> pieces;
    for (uint32_t w = 0; w < n_windows; w++) {
        const gci_window c = bg_clamp(ctx, h_windows[w]);
        stats[4 * (size_t)w] = 0; stats[4 * (size_t)w + 1] = INT32_MAX; stats[4 * (size_t)w + 2] = INT32_MIN; stats[4 * (size_t)w + 3] = c.end - c.begin;
        for (int64_t a = c.begin; a < c.end; a += (int64_t)1 << 22) pieces.push_back({w, a, std::min(c.end, a + ((int64_t)1 << 22))});
    }
    parallel_blocks(ctx->threads, pieces.size(), 1, [&](uint64_t k, uint64_t) {
        const Piece pc = pieces[k];
        std::vector<uint64_t> h(hist ? cols : 0);
        int64_t sum = 0, lo = INT32_MAX, hi = INT32_MIN;
        for (int64_t i = pc.lo; i < pc.hi; i++) {
            const int32_t d = depth[i];
            sum += d; lo = std::min<int64_t>(lo, d); hi = std::max<int64_t>(hi, d);
            if (hist) h[d < 0 ? (size_t)n_bins + 1 : (uint32_t)d >= n_bins ? (size_t)n_bins : (size_t)d]++;
        }
        int64_t* s = stats + 4 * (size_t)pc.w;
        __atomic_fetch_add(s, sum, __ATOMIC_RELAXED);
        for (int64_t seen = __atomic_load_n(s + 1, __ATOMIC_RELAXED); lo < seen && !__atomic_compare_exchange_n(s + 1, &seen, lo, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);) {}
        for (int64_t seen = __atomic_load_n(s + 2, __ATOMIC_RELAXED); hi > seen && !__atomic_compare_exchange_n(s + 2, &seen, hi, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);) {}
        for (size_t b = 0; b < h.size(); b++) if (h[b]) __atomic_fetch_add(hist + (size_t)pc.w * cols + b, h[b], __ATOMIC_RELAXED);
    });
    return GCI_OK;
}

/* ---- depth_to_bedgraph.py: the constant-depth runs of every window, in order, and their bedGraph lines (k_bedgraph.hip's twins) ---- */
int gci_depth_runs_count(gci_ctx* ctx, const int32_t* depth, const gci_window* h_windows, uint32_t n_windows, uint64_t* win_run0)
{
    if (!ctx || !depth || !win_run0 || (n_windows && !h_windows)) return GCI_E_INVALID;
    const int st = need_layout(ctx);
    if (st) return st;
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    ctx->bg_track = nullptr;
    std::vector<gci_ctx::BgPiece> pieces;
    std::vector<uint64_t> first_piece((size_t)n_windows + 1);
    for (uint32_t w = 0; w < n_windows; w++) {
        const gci_window c = bg_clamp(ctx, h_windows[w]);
        if (c.end - c.begin > 0xFFFFFFFFll) return GCI_E_INVALID;
        first_piece[w] = pieces.size();
        for (int64_t a = c.begin; a < c.end; a += (int64_t)1 << 22) pieces.push_back({c.begin, a, std::min(c.end, a + ((int64_t)1 << 22)), 0});
    }
    first_piece[n_windows] = pieces.size();
    parallel_blocks(ctx->threads, pieces.size(), 1, [&](uint64_t k, uint64_t) {
        gci_ctx::BgPiece& pc = pieces[k];
        uint64_t n = 0;
        for (int64_t i = pc.lo; i < pc.hi; i++) n += (i == pc.begin || depth[i] != depth[i - 1]) ? 1u : 0u;
        pc.run0 = n;
    });
    uint64_t at = 0;
    for (auto& pc : pieces) { const uint64_t n = pc.run0; pc.run0 = at; at += n; }
    for (uint32_t w = 0; w <= n_windows; w++) win_run0[w] = first_piece[w] < pieces.size() ? pieces[first_piece[w]].run0 : at;
    ctx->bg_pieces.swap(pieces);
    ctx->bg_runs_total = at;
    ctx->bg_track = depth;
    return GCI_OK;
}

int gci_depth_runs_write(gci_ctx* ctx, const int32_t* depth, gci_depth_run* runs, uint64_t cap)
{
    if (!ctx || !depth || (cap && !runs)) return GCI_E_INVALID;
    const int st = need_layout(ctx);
    if (st) return st;
    if (!ctx->bg_track || ctx->bg_track != depth) return GCI_E_INVALID;
    if (cap < ctx->bg_runs_total) return GCI_E_CAPACITY;
    parallel_blocks(ctx->threads, ctx->bg_pieces.size(), 1, [&](uint64_t k, uint64_t) {
        const gci_ctx::BgPiece pc = ctx->bg_pieces[k];
        uint64_t o = pc.run0;
        for (int64_t i = pc.lo; i < pc.hi; i++)
            if (i == pc.begin || depth[i] != depth[i - 1]) { runs[o].start = (uint32_t)(i - pc.begin); runs[o].depth = depth[i]; o++; }
    });
    return GCI_OK;
}

int gci_bedgraph_size(gci_ctx* ctx, const gci_depth_run* runs, const uint64_t* win_run0, const gci_window* h_windows, uint32_t n_windows,
                      const int64_t* h_coord0, const uint32_t* h_name_len, uint64_t* win_byte0)
{
    if (!ctx || !win_run0 || !win_byte0 || (n_windows && (!h_windows || !h_coord0 || !h_name_len))) return GCI_E_INVALID;
    const int st = need_layout(ctx);
    if (st) return st;
    if (n_windows >= (1u << 31)) return GCI_E_INVALID;
    ctx->bg_text_run0 = nullptr;
    if (win_run0[n_windows] && (!runs || !n_windows)) return GCI_E_INVALID;
    std::vector<uint64_t> bytes;
    const int r = bg_window_bytes(ctx, runs, win_run0, h_windows, n_windows, h_coord0, h_name_len, bytes);
    if (r) return r;
    uint64_t at = 0;
    for (uint32_t w = 0; w < n_windows; w++) { win_byte0[w] = at; at += bytes[w]; }
    win_byte0[n_windows] = at;
    ctx->bg_text_run0 = win_run0;
    ctx->bg_text_runs = runs;
    ctx->bg_text_windows = n_windows;
    return GCI_OK;
}

int gci_bedgraph_write(gci_ctx* ctx, const gci_depth_run* runs, const uint64_t* win_run0, const gci_window* h_windows, uint32_t n_windows,
                       const int64_t* h_coord0, const uint8_t* names, const uint64_t* h_name_off, const uint32_t* h_name_len, uint8_t* out,
                       uint64_t cap)
{
    if (!ctx || !win_run0 || (cap && !out) || (n_windows && (!h_windows || !h_coord0 || !h_name_off || !h_name_len))) return GCI_E_INVALID;
    const int st = need_layout(ctx);
    if (st) return st;
    if (!ctx->bg_text_run0 || ctx->bg_text_run0 != win_run0 || ctx->bg_text_runs != runs || ctx->bg_text_windows != n_windows) return GCI_E_INVALID;
    std::vector<uint64_t> bytes;
    const int r = bg_window_bytes(ctx, runs, win_run0, h_windows, n_windows, h_coord0, h_name_len, bytes);
    if (r) return r;
    std::vector<uint64_t> at((size_t)n_windows + 1, 0);
    for (uint32_t w = 0; w < n_windows; w++) at[w + 1] = at[w] + bytes[w];
    if (cap < at[n_windows]) return GCI_E_CAPACITY;
    for (uint32_t w = 0; w < n_windows; w++) if (bytes[w] && h_name_len[w] && !names) return GCI_E_INVALID;
    parallel_blocks(ctx->threads, n_windows, 1, [&](uint64_t w, uint64_t) {
        const gci_window c = bg_clamp(ctx, h_windows[w]);
        uint8_t* p = out + at[w];
        for (uint64_t k = win_run0[w]; k < win_run0[w + 1]; k++) {
            const uint64_t rel_end = k + 1 < win_run0[w + 1] ? (uint64_t)runs[k + 1].start : (uint64_t)(c.end - c.begin);
            memcpy(p, names + h_name_off[w], h_name_len[w]);
            p += h_name_len[w];
            *p++ = '\t';
            p = bg_put(p, (uint64_t)h_coord0[w] + runs[k].start);
            *p++ = '\t';
            p = bg_put(p, (uint64_t)h_coord0[w] + rel_end);
            *p++ = '\t';
            const int32_t d = runs[k].depth;
            if (d < 0) *p++ = '-';
            p = bg_put(p, d < 0 ? (uint64_t)(-(int64_t)d) : (uint64_t)d);
            *p++ = '\n';
        }
    });
    return GCI_OK;
}

}  // extern "C"

/* ---- N2: the depth text as gzip members (write_depth incl. its gzip, GCI.py:99-143) ------------------------------------------------------
 * The format libgci_hip.so writes (k_deflate.hip), token for token: a tile of 4096 bases is one fixed-Huffman block -- per run of n
 * equal depths the line's literals and matches of distance = line width over the other (n - 1) lines, never leaving one or two
 * bytes behind a match -- closed by an empty stored block (byte alignment); 64 tiles are one member:
 *     1f 8b 08 00 00000000 00 ff | tile 0 | ... | tile 63 | 03 00 | CRC-32 | ISIZE
 * Here the text of a tile is written out (12 KB) and its CRC taken byte by byte: no GF(2) algebra to agree with. */
namespace {
struct BitW {
    uint8_t* out = nullptr;          // nullptr: count only
    uint64_t acc = 0, total = 0;
    uint32_t nb = 0;
    void put(uint32_t bits, uint32_t n)
    {
        acc |= (uint64_t)bits << nb;
        nb += n;
        total += n;
        while (nb >= 8u) { if (out) *out++ = (uint8_t)acc; acc >>= 8; nb -= 8u; }
    }
    void align() { if (nb) put(0u, 8u - nb); }
};
inline uint32_t rev(uint32_t v, int bits) { uint32_t r = 0; for (int i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i); return r; }
inline void put_literal(BitW& o, uint32_t byte) { o.put(rev(0x30u + byte, 8), 8u); }                     // bytes < 144
inline void put_match(BitW& o, uint32_t len, uint32_t dist)                                              // 3 <= len <= 258, 2 <= dist <= 12
{
    if (len == 258u) o.put(rev(0xC5u, 8), 8u);
    else {
        const uint32_t t = len - 3u;
        uint32_t e = 0;
        if (t >= 8u) { uint32_t lg = 0; while ((t >> (lg + 1u)) != 0u) lg++; e = lg - 2u; }
        const uint32_t sym = 257u + 4u * e + (e ? (t >> e) : t);
        if (sym <= 279u) o.put(rev(sym - 256u, 7), 7u); else o.put(rev(0xC0u + (sym - 280u), 8), 8u);
        if (e) o.put(t & ((1u << e) - 1u), e);
    }
    uint32_t code, eb, ev;
    if (dist <= 4u) { code = dist - 1u; eb = 0; ev = 0; }
    else if (dist <= 8u) { code = 4u + ((dist - 5u) >> 1); eb = 1; ev = (dist - 5u) & 1u; }
    else { code = 6u + ((dist - 9u) >> 2); eb = 2; ev = (dist - 9u) & 3u; }
    o.put(rev(code, 5), 5u);
    if (eb) o.put(ev, eb);
}
const uint32_t* crc_table()
{
    static uint32_t T[256];
    static const bool made = [] {
        for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u); T[i] = c; }
        return true;
    }();
    (void)made;
    return T;
}
// one tile: its block into o, its text's bytes into the running CRC register / length
void deflate_tile(const int32_t* d, uint32_t n, BitW& o, uint32_t& crc_reg, uint32_t& text_len)
{
    if (n == 0) return;
    const uint32_t* T = crc_table();
    o.put(2u, 3u);                                                          // BFINAL = 0, BTYPE = 01
    for (uint32_t i = 0; i < n;) {
        uint32_t j = i + 1;
        while (j < n && d[j] == d[i]) j++;
        const uint32_t reps = j - i;
        char line[16];
        const int w = snprintf(line, sizeof line, "%u\n", (uint32_t)d[i]);
        for (uint32_t r = 0; r < reps; r++)
            for (int k = 0; k < w; k++) crc_reg = T[(crc_reg ^ (uint8_t)line[k]) & 0xFFu] ^ (crc_reg >> 8);
        text_len += reps * (uint32_t)w;
        for (int k = 0; k < w; k++) put_literal(o, (uint8_t)line[k]);
        uint32_t rest = (reps - 1u) * (uint32_t)w;
        while (rest >= 3u) {
            uint32_t len = rest < 258u ? rest : 258u;
            if (rest - len != 0u && rest - len < 3u) len = rest - 3u;       // never leave 1 or 2 bytes behind
            put_match(o, len, (uint32_t)w);
            rest -= len;
        }
        for (uint32_t k = 0; k < rest; k++) put_literal(o, (uint8_t)line[k]);   // (two lines of two bytes: the second as literals)
        i = j;
    }
    o.put(0u, 7u);                                                          // end of block
    o.put(0u, 3u);                                                          // empty stored block
    o.align();
    o.put(0x0000u, 16u);
    o.put(0xFFFFu, 16u);
}
constexpr uint32_t DEF_TILE = 4096, DEF_MEMBER_TILES = 64;
}  // namespace

extern "C" {

int gci_depth_deflate_from_build(gci_ctx* ctx, const int32_t* depth)
{
    (void)ctx; (void)depth;
    return GCI_E_INVALID;                              // this library's build keeps no run lists: the pair always walks the track
}

int gci_depth_deflate_size(gci_ctx* ctx, const int32_t* depth, const uint64_t* member_elem, const uint32_t* member_n, uint32_t n_members,
                           uint32_t* tile_bytes, uint32_t* member_bytes, uint32_t* member_crc, uint32_t* member_isize)
{
    if (!ctx || (n_members && (!depth || !member_elem || !member_n || !tile_bytes || !member_bytes || !member_crc || !member_isize)))
        return GCI_E_INVALID;
    parallel_blocks(ctx->threads, n_members, 1, [&](uint64_t m, uint64_t) {
        uint32_t reg = 0xFFFFFFFFu, len = 0, sum = 0;
        for (uint32_t t = 0; t < DEF_MEMBER_TILES; t++) {
            const uint32_t first = t * DEF_TILE, n_all = member_n[m];
            const uint32_t n = n_all > first ? std::min(DEF_TILE, n_all - first) : 0u;
            BitW o;
            deflate_tile(depth + member_elem[m] + first, n, o, reg, len);
            tile_bytes[m * DEF_MEMBER_TILES + t] = (uint32_t)(o.total >> 3);
            sum += (uint32_t)(o.total >> 3);
        }
        member_bytes[m] = sum + 20u;
        member_crc[m] = reg ^ 0xFFFFFFFFu;
        member_isize[m] = len;
    });
    return GCI_OK;
}

int gci_depth_deflate_write(gci_ctx* ctx, const int32_t* depth, const uint64_t* member_elem, const uint32_t* member_n, uint32_t n_members,
                            const uint32_t* tile_bytes, const uint32_t* member_crc, const uint32_t* member_isize, const uint64_t* member_out,
                            uint8_t* out, uint64_t cap)
{
    if (!ctx || (n_members && (!depth || !member_elem || !member_n || !tile_bytes || !member_crc || !member_isize || !member_out || !out)))
        return GCI_E_INVALID;
    std::atomic<int> bad{0};
    parallel_blocks(ctx->threads, n_members, 1, [&](uint64_t m, uint64_t) {
        uint32_t total = 20u;
        for (uint32_t t = 0; t < DEF_MEMBER_TILES; t++) total += tile_bytes[m * DEF_MEMBER_TILES + t];
        if (member_out[m] + total > cap) { bad = 1; return; }
        uint8_t* h = out + member_out[m];
        const uint8_t head[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF};
        memcpy(h, head, 10);
        uint8_t* w = h + 10;
        for (uint32_t t = 0; t < DEF_MEMBER_TILES; t++) {
            const uint32_t first = t * DEF_TILE, n_all = member_n[m];
            const uint32_t n = n_all > first ? std::min(DEF_TILE, n_all - first) : 0u;
            BitW o;
            o.out = w;
            uint32_t reg = 0, len = 0;
            deflate_tile(depth + member_elem[m] + first, n, o, reg, len);
            w += tile_bytes[m * DEF_MEMBER_TILES + t];
        }
        const uint32_t c = member_crc[m], z = member_isize[m];
        const uint8_t tail[10] = {0x03, 0x00, (uint8_t)c, (uint8_t)(c >> 8), (uint8_t)(c >> 16), (uint8_t)(c >> 24),
                                  (uint8_t)z, (uint8_t)(z >> 8), (uint8_t)(z >> 16), (uint8_t)(z >> 24)};
        memcpy(w, tail, 10);
    });
    return bad ? GCI_E_CAPACITY : GCI_OK;
}

}  // extern "C"

/* ---- this library's own .depth.gz -> track without inflating it (k_depth_gz.hip) --------------------------------------------------------
 * The grammar of include/gci_hip.h, read a bit at a time against RFC 1951's tables; the CRC of a member is taken over the text of its
 * runs, byte by byte: no GF(2) algebra to agree with.  Like the device, a token is only looked at with 20 bits in hand. */
namespace {
const uint16_t DGZ_LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t DGZ_LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t DGZ_DIST_BASE[8] = {1, 2, 3, 4, 5, 7, 9, 13};
const uint8_t DGZ_DIST_EXTRA[8] = {0, 0, 0, 0, 1, 1, 2, 2};

struct DgzBits {
    const uint8_t* raw;
    uint64_t n_bits, at;
    bool has(uint64_t k) const { return n_bits - at >= k; }
    uint32_t bit() { const uint32_t v = (raw[at >> 3] >> (at & 7u)) & 1u; at++; return v; }
    uint32_t value(uint32_t k) { uint32_t v = 0; for (uint32_t i = 0; i < k; i++) v |= bit() << i; return v; }     // LSB first
    uint32_t code(uint32_t k) { uint32_t v = 0; for (uint32_t i = 0; i < k; i++) v = (v << 1) | bit(); return v; }  // Huffman: MSB first
};

struct DgzMember { uint64_t end = 0; uint32_t lines = 0, crc_file = 0, isize_file = 0; };

// on_run(depth, lines) for every run as it closes (false: stop) -> false: not this writer's
template <typename F>
bool dgz_decode(const uint8_t* raw, uint64_t n, uint64_t pos, F on_run, DgzMember& out)
{
    static const uint8_t head[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF};
    if (pos >= n || n - pos < 10 || memcmp(raw + pos, head, 10) != 0) return false;
    DgzBits b{raw, n * 8, (pos + 10) * 8};
    uint32_t blocks = 0, lines = 0;
    bool prev_fixed = false;
    for (;;) {
        if (!b.has(3)) return false;
        const uint32_t bfinal = b.bit(), btype = b.value(2);
        if (btype == 0) {
            if (!prev_fixed || bfinal) return false;
            b.at = (b.at + 7) & ~(uint64_t)7;
            if (!b.has(32)) return false;
            const uint32_t len = b.value(16), nlen = b.value(16);
            if (len != 0 || nlen != 0xFFFFu) return false;
            prev_fixed = false;
            continue;
        }
        if (btype != 1 || ++blocks > GCI_DGZ_MAX_BLOCKS) return false;
        std::string line;                        // the characters literals have spelled of a line not yet closed
        bool spelling = false;
        uint32_t w = 0, run_val = 0, run_lines = 0, partial = 0;   // partial: bytes matches have copied of a line not yet whole
        for (;;) {
            if (!b.has(20)) return false;
            // the fixed code, RFC 1951 3.2.6: 7 bits 0000000 .. 0010111 = 256 .. 279, 8 bits 00110000 .. 10111111 = 0 .. 143,
            // 8 bits 11000000 .. 11000111 = 280 .. 287, 9 bits = 144 .. 255
            uint32_t c = b.code(7), sym;
            if (c <= 0x17u) sym = 256 + c;
            else {
                c = (c << 1) | b.bit();
                if (c >= 0x30u && c <= 0xBFu) sym = c - 0x30u;
                else if (c >= 0xC0u && c <= 0xC7u) sym = 280 + (c - 0xC0u);
                else return false;               // a literal of 144 or more
            }
            if (sym == 256) break;
            if (sym < 256) {
                if (partial) return false;
                if (!spelling) {
                    if (w && !on_run(run_val, run_lines)) return false;
                    w = 0; spelling = true; line.clear();
                }
                if (sym == '\n') {
                    if (line.empty() || line.size() > 10 || (line.size() > 1 && line[0] == '0')) return false;
                    const unsigned long long v = strtoull(line.c_str(), nullptr, 10);
                    if (v > 0x7FFFFFFFull || lines == GCI_DGZ_MAX_LINES) return false;
                    w = (uint32_t)line.size() + 1; run_val = (uint32_t)v; run_lines = 1; lines++;
                    spelling = false;
                } else if (sym >= '0' && sym <= '9') {
                    if (line.size() == 10 || (line.size() == 1 && line[0] == '0')) return false;
                    line.push_back((char)sym);
                } else return false;
                continue;
            }
            if (sym > 285) return false;
            const uint32_t len = DGZ_LEN_BASE[sym - 257] + b.value(DGZ_LEN_EXTRA[sym - 257]);
            const uint32_t dc = b.code(5);
            if (dc >= 8) return false;
            const uint32_t dist = DGZ_DIST_BASE[dc] + b.value(DGZ_DIST_EXTRA[dc]);
            if (spelling || w == 0 || dist != w) return false;
            partial += len;
            const uint32_t whole = partial / w;
            partial %= w;
            if (whole > GCI_DGZ_MAX_LINES - lines) return false;
            run_lines += whole; lines += whole;
        }
        if (spelling || partial) return false;
        if (w && !on_run(run_val, run_lines)) return false;
        prev_fixed = true;
        if (bfinal) break;
    }
    const uint64_t q = (b.at + 7) >> 3;
    if (q > n || n - q < 8) return false;
    auto le32 = [&](uint64_t o) { return (uint32_t)raw[o] | (uint32_t)raw[o + 1] << 8 | (uint32_t)raw[o + 2] << 16 | (uint32_t)raw[o + 3] << 24; };
    out.crc_file = le32(q);
    out.isize_file = le32(q + 4);
    out.end = q + 8;
    out.lines = lines;
    return true;
}
}  // namespace

extern "C" {

int gci_depth_gz_scan(gci_ctx* ctx, const uint8_t* raw, uint64_t n_raw, const uint64_t* cand_pos, uint32_t n_cand, gci_dgz_info* info)
{
    if (!ctx || (n_cand && (!raw || !cand_pos || !info))) return GCI_E_INVALID;
    const uint32_t* T = crc_table();
    parallel_blocks(ctx->threads, n_cand, 1, [&](uint64_t i, uint64_t) {
        uint32_t reg = 0xFFFFFFFFu, text_len = 0, runs = 0;
        DgzMember mem;
        const bool ok = dgz_decode(raw, n_raw, cand_pos[i], [&](uint32_t v, uint32_t n) {
            char line[16];
            const int w = snprintf(line, sizeof line, "%u\n", v);
            for (uint32_t r = 0; r < n; r++)
                for (int k = 0; k < w; k++) reg = T[(reg ^ (uint8_t)line[k]) & 0xFFu] ^ (reg >> 8);
            text_len += n * (uint32_t)w;
            runs++;
            return true;
        }, mem);
        gci_dgz_info o;
        memset(&o, 0, sizeof o);
        o.status = ok ? GCI_DGZ_OK : GCI_DGZ_FOREIGN;
        if (ok) {
            o.end = mem.end; o.lines = mem.lines; o.runs = runs;
            o.crc_ok = (reg ^ 0xFFFFFFFFu) == mem.crc_file;
            o.isize_ok = text_len == mem.isize_file;
        }
        info[i] = o;
    });
    return GCI_OK;
}

int gci_depth_gz_runs(gci_ctx* ctx, const uint8_t* raw, uint64_t n_raw, const gci_dgz_member* members, uint32_t n_members, gci_dgz_run* runs)
{
    if (!ctx || (n_members && (!raw || !members || !runs))) return GCI_E_INVALID;
    parallel_blocks(ctx->threads, n_members, 1, [&](uint64_t m, uint64_t) {
        uint32_t r = 0;
        DgzMember mem;
        (void)dgz_decode(raw, n_raw, members[m].pos, [&](uint32_t v, uint32_t n) {
            if (r >= members[m].runs) return false;
            runs[members[m].run0 + r].depth = (int32_t)v;
            runs[members[m].run0 + r].count = n;
            r++;
            return true;
        }, mem);
    });
    return GCI_OK;
}

int gci_depth_gz_expand(gci_ctx* ctx, const gci_dgz_run* runs, const gci_dgz_member* members, uint32_t n_members, int32_t* track,
                        uint64_t track_n)
{
    if (!ctx || (n_members && (!runs || !members || !track))) return GCI_E_INVALID;
    parallel_blocks(ctx->threads, n_members, 1, [&](uint64_t m, uint64_t) {
        uint64_t k = 0;                          // lines of the member written so far
        for (uint32_t r = 0; r < members[m].runs && k < members[m].lines; r++) {
            const gci_dgz_run& run = runs[members[m].run0 + r];
            for (uint32_t j = 0; j < run.count && k < members[m].lines; j++, k++)
                if (members[m].elem0 + k < track_n) track[members[m].elem0 + k] = run.depth;
        }
    });
    return GCI_OK;
}

}  // extern "C"

/* ---- depth text -> track (k_depth_parse.hip): the same tiles, line ownership, keys and status word, on host threads ------------ */
namespace {
constexpr uint64_t PARSE_TILE = 4096;
inline uint64_t parse_tiles(uint64_t n) { return (n + PARSE_TILE - 1) / PARSE_TILE; }
// f(offset, rank) for every line whose first byte is in the tile, in order; -> the number of those lines
template <typename F>
uint32_t for_each_line(const uint8_t* text, uint64_t n, uint64_t tile, F f)
{
    uint32_t rank = 0;
    for (uint64_t i = tile * PARSE_TILE; i < std::min(n, (tile + 1) * PARSE_TILE); i++)
        if (i == 0 || text[i - 1] == '\n') f(i, rank++);
    return rank;
}
inline void note_first_bad(std::atomic<uint64_t>& first_bad, uint64_t i)
{
    uint64_t cur = first_bad.load();
    while (i < cur && !first_bad.compare_exchange_weak(cur, i)) {}
}
inline void push_key(std::atomic<uint32_t>& slots, uint64_t* keys, uint32_t cap, uint64_t i, uint32_t rank)
{
    const uint32_t s = slots.fetch_add(1);
    if (s < cap) keys[s] = (i << 12) | rank;
}
// the element of the track `line` goes to, through the last segment whose first line is <= line; -1: none
int64_t seg_dest(const int64_t* segs, uint32_t n_segs, uint64_t line, uint64_t track_n)
{
    uint32_t a = 0, b = n_segs;
    while (a < b) { const uint32_t m = (a + b) / 2; if ((uint64_t)segs[3 * m] <= line) a = m + 1; else b = m; }
    if (a == 0) return -1;
    const int64_t* s = segs + 3 * (a - 1);
    if (s[2] < 0 || (int64_t)line >= s[0] + s[1]) return -1;
    const int64_t e = s[2] + ((int64_t)line - s[0]);
    return (uint64_t)e < track_n ? e : -1;
}
// [0-9]{1,10} then '\n' or the end of the text, value <= INT32_MAX -> value, or -1
int64_t strict_value(const uint8_t* text, uint64_t i, uint64_t n)
{
    uint64_t v = 0, d = 0;
    for (; d < 11 && i + d < n && text[i + d] >= '0' && text[i + d] <= '9'; d++) v = v * 10 + (uint64_t)(text[i + d] - '0');
    const bool closed = i + d == n || text[i + d] == '\n';
    return (d >= 1 && d <= 10 && closed && v <= 0x7FFFFFFFull) ? (int64_t)v : -1;
}
}  // namespace

extern "C" {

int gci_depth_text_index(gci_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t* tile_lines, uint64_t* keys, uint32_t cap,
                         uint32_t* n_hdr, uint64_t* bad)
{
    if (!ctx || !n_hdr || !bad || (n && (!text || !tile_lines)) || (cap && !keys)) return GCI_E_INVALID;
    std::atomic<uint32_t> slots{0};
    std::atomic<uint64_t> first_bad{~0ull};
    parallel_blocks(ctx->threads, parse_tiles(n), 64, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t t = lo; t < hi; t++)
            tile_lines[t] = for_each_line(text, n, t, [&](uint64_t i, uint32_t rank) {
                if (text[i] == '>') push_key(slots, keys, cap, i, rank);
                else if (strict_value(text, i, n) < 0) note_first_bad(first_bad, i);
            });
    });
    *n_hdr = slots.load();
    *bad = first_bad.load();
    return GCI_OK;
}

int gci_depth_text_parse(gci_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* tile_line0, const int64_t* segs, uint32_t n_segs,
                         int32_t* track, uint64_t track_n)
{
    if (!ctx || (n && (!text || !tile_line0)) || (n_segs && !segs) || (track_n && !track)) return GCI_E_INVALID;
    if (!n || !n_segs || !track_n) return GCI_OK;
    parallel_blocks(ctx->threads, parse_tiles(n), 64, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t t = lo; t < hi; t++)
            for_each_line(text, n, t, [&](uint64_t i, uint32_t rank) {
                const int64_t e = text[i] == '>' ? -1 : seg_dest(segs, n_segs, tile_line0[t] + rank, track_n);
                if (e < 0) return;
                uint32_t v = 0;
                for (uint64_t d = 0; d < 10 && i + d < n && text[i + d] >= '0' && text[i + d] <= '9'; d++) v = v * 10 + (uint32_t)(text[i + d] - '0');
                track[e] = (int32_t)v;
            });
    });
    return GCI_OK;
}

}  // extern "C"

/* ---- samtools depth text -> track (k_sdepth.hip): the same tiles, line ownership, grammar, keys and status word ------------------ */
namespace {
constexpr uint64_t SD_LINE_MAX = 255;              // bytes of a line with its '\n'
inline bool name_end(uint8_t c) { return c == '\t' || c == '\n'; }
bool sd_strict_line(const uint8_t* text, uint64_t i, uint64_t n)
{
    const uint64_t lim = std::min(n - i, SD_LINE_MAX);
    const uint8_t* b = text + i;
    uint64_t k = 0;
    while (k < lim && b[k] >= 0x21 && b[k] <= 0x7E) k++;
    if (k == 0 || k >= lim || b[k] != '\t') return false;
    k++;
    uint64_t d = 0;
    while (k < lim && d < 11 && b[k] >= '0' && b[k] <= '9') { k++; d++; }
    if (d == 0 || d > 10 || k >= lim || b[k] != '\t') return false;
    k++;
    if (k >= lim) return false;
    const bool zero = b[k] == '0';
    uint64_t v = 0;
    d = 0;
    while (k < lim && d < 11 && b[k] >= '0' && b[k] <= '9') { v = v * 10 + (uint64_t)(b[k] - '0'); k++; d++; }
    if (d == 0 || d > 10 || (zero && d > 1) || v > 0x7FFFFFFFull) return false;
    return i + k == n || (k < lim && b[k] == '\n');
}
// the name of the line at i equals a[0 .. a_len) cut at its first '\t' / '\n' (a_len: the bytes of a that may be read)
bool sd_same_name(const uint8_t* a, uint64_t a_len, bool a_is_name, const uint8_t* text, uint64_t i, uint64_t n)
{
    const uint64_t lim = std::min(n - i, SD_LINE_MAX);
    for (uint64_t k = 0; k < lim; k++) {
        const bool ea = a_is_name ? k >= a_len : name_end(a[k]), ec = name_end(text[i + k]);
        if (ea || ec) return ea && ec;
        if (a[k] != text[i + k]) return false;
    }
    return false;
}
}  // namespace

extern "C" {

int gci_sdepth_index(gci_ctx* ctx, const uint8_t* text, uint64_t n, const uint8_t* prev_name, uint32_t prev_len, uint32_t* tile_lines,
                     uint64_t* keys, uint32_t cap, uint32_t* n_keys, uint64_t* bad)
{
    if (!ctx || !n_keys || !bad || (n && (!text || !tile_lines)) || (cap && !keys) || (prev_len && !prev_name) || prev_len > SD_LINE_MAX)
        return GCI_E_INVALID;
    std::atomic<uint32_t> slots{0};
    std::atomic<uint64_t> first_bad{~0ull};
    parallel_blocks(ctx->threads, parse_tiles(n), 64, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t t = lo; t < hi; t++)
            tile_lines[t] = for_each_line(text, n, t, [&](uint64_t i, uint32_t rank) {
                if (!sd_strict_line(text, i, n)) note_first_bad(first_bad, i);
                bool same;
                if (i == 0) {
                    same = sd_same_name(prev_name, prev_len, true, text, 0, n);
                } else {                                    // the line in front begins at most SD_LINE_MAX bytes back, or equals nothing
                    uint64_t q = i - 1;
                    while (q > 0 && i - q < SD_LINE_MAX + 1 && text[q - 1] != '\n') q--;
                    same = i - q <= SD_LINE_MAX && (q == 0 || text[q - 1] == '\n') && sd_same_name(text + q, 0, false, text, i, n);
                }
                if (!same) push_key(slots, keys, cap, i, rank);
            });
    });
    *n_keys = slots.load();
    *bad = first_bad.load();
    return GCI_OK;
}

int gci_sdepth_parse(gci_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* tile_line0, uint64_t line_base, const int64_t* segs,
                     uint32_t n_segs, int32_t* track, uint64_t track_n)
{
    if (!ctx || (n && (!text || !tile_line0)) || (n_segs && !segs) || (track_n && !track)) return GCI_E_INVALID;
    if (!n || !n_segs || !track_n) return GCI_OK;
    parallel_blocks(ctx->threads, parse_tiles(n), 64, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t t = lo; t < hi; t++)
            for_each_line(text, n, t, [&](uint64_t i, uint32_t rank) {
                const int64_t e = seg_dest(segs, n_segs, line_base + tile_line0[t] + rank, track_n);
                if (e < 0) return;
                uint64_t end = i;                           // the depth column: the digits in front of the line's end
                while (end < n && text[end] != '\n') end++;
                uint32_t v = 0, mul = 1;
                for (uint64_t d = 1; d <= 10 && d <= end && text[end - d] >= '0' && text[end - d] <= '9'; d++, mul *= 10)
                    v += (uint32_t)(text[end - d] - '0') * mul;
                track[e] = (int32_t)v;
            });
    });
    return GCI_OK;
}

}  // extern "C"
