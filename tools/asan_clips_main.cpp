// asan_clips_main.cpp -- the CPU twin's clip functions (gci_bam_clip_size / _write, gci_clip_sites_size / _write) under
// AddressSanitizer and UBSan, as a stand-alone program: two record cases (end operations next to a cut-off stream; a CIGAR longer than
// a chunk with the clip at its very end, and a position near 2^31) and one site case, with the answers written by hand.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/asan_clips_main.cpp -o asan_clips && ./asan_clips
#include "../gci_amd/csrc/cpu/gci_cpu.cpp"

#include <stdio.h>

namespace {

typedef std::pair<uint32_t, uint32_t> Op;             // (code, length)

void put32(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); }

// one record with a one-letter name, l_seq = 0 and no tags, appended to the stream
void add_record(std::vector<uint8_t>& s, std::vector<uint64_t>& offs, int32_t ref_id, int32_t pos, uint16_t flag, const std::vector<Op>& cigar)
{
    offs.push_back(s.size());
    put32(s, (uint32_t)(32 + 2 + 4 * cigar.size()));
    put32(s, (uint32_t)ref_id); put32(s, (uint32_t)pos);
    s.push_back(2); s.push_back(60); s.push_back(0); s.push_back(0);                      // l_read_name, mapq, bin
    s.push_back((uint8_t)cigar.size()); s.push_back((uint8_t)(cigar.size() >> 8));
    s.push_back((uint8_t)flag); s.push_back((uint8_t)(flag >> 8));
    put32(s, 0); put32(s, (uint32_t)-1); put32(s, (uint32_t)-1); put32(s, 0);             // l_seq, next refID, next pos, tlen
    s.push_back('r'); s.push_back(0);
    for (const Op& o : cigar) put32(s, (o.second << 4) | o.first);
}

int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

}  // namespace

int main()
{
    enum { M = 0, I = 1, D = 2, N = 3, S = 4, H = 5 };
    gci_ctx* ctx = nullptr;
    EXPECT(gci_ctx_create(0, nullptr, 0, &ctx) == GCI_OK);
    const int64_t lengths[2] = {1000, 70000};
    EXPECT(gci_layout_set(ctx, 2, lengths) == GCI_OK);
    const int32_t sel[2] = {0, 1};
    uint64_t counts[3], status = 0;
    std::vector<gci_ivl> out(16, gci_ivl{7, 7, 7, 7});

    // case 1: end operations, and a last record that runs past the stream
    {
        std::vector<uint8_t> s(12, 0);
        std::vector<uint64_t> offs;
        add_record(s, offs, 0, 100, 0, {{S, 5}, {M, 10}});
        add_record(s, offs, 0, 200, 0x800, {{H, 5}, {S, 5}, {M, 10}, {S, 5}, {H, 5}});
        add_record(s, offs, 0, 300, 0, {{S, 3}});
        add_record(s, offs, 0, 995, 0, {{S, 9}, {D, 5}, {H, 9}});            // its right site is the contig's last base
        add_record(s, offs, 0, 996, 0, {{M, 5}, {S, 9}});                   // ... one beyond it
        add_record(s, offs, 0, 400, 0x100, {{S, 50}, {M, 5}});
        add_record(s, offs, 0, 500, 0, {{M, 9}});
        s.resize(s.size() - 3);
        EXPECT(gci_bam_clip_size(ctx, s.data(), s.size(), offs.data(), (uint32_t)offs.size(), 1, sel, 2, 0x704, 0, 5, counts, &status) == GCI_OK);
        EXPECT(counts[0] == 4 && counts[1] == 3 && counts[2] == 2);
        EXPECT(status == ((6ull << 8) | 7ull));
        EXPECT(gci_bam_clip_write(ctx, s.data(), s.size(), offs.data(), (uint32_t)offs.size(), 1, out.data(), 4, &status) == GCI_E_CAPACITY && out[0].contig == 7);
        EXPECT(gci_bam_clip_write(ctx, s.data(), s.size(), offs.data(), (uint32_t)offs.size(), 1, out.data(), 5, &status) == GCI_OK);
        const int32_t want[5] = {100, 200, 995, 209, 999};
        for (int k = 0; k < 5; k++) EXPECT(out[k].contig == 0 && out[k].start == want[k] && out[k].end == want[k] && out[k].pad == 0);
        EXPECT(out[5].contig == 7);
        EXPECT(gci_bam_clip_size(ctx, s.data(), s.size(), offs.data(), (uint32_t)offs.size(), 1, sel, 2, 0x704, 0, 0, counts, &status) == GCI_E_INVALID);
    }
    // case 2: 4097 operations with the clip behind the last chunk's edge, and pos + R beyond int32
    {
        std::vector<uint8_t> s(12, 0);
        std::vector<uint64_t> offs;
        std::vector<Op> big(4096, Op(M, 1));
        big[0] = Op(S, 7); big[1] = Op(I, 3); big.push_back(Op(H, 8));
        add_record(s, offs, 1, 10, 0, big);
        add_record(s, offs, 1, 0x7FFFFFF0, 0, {{S, 20}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {S, 20}});
        EXPECT(gci_bam_clip_size(ctx, s.data(), s.size(), offs.data(), (uint32_t)offs.size(), 1, sel, 2, 0x704, 0, 7, counts, &status) == GCI_OK);
        EXPECT(counts[0] == 2 && counts[1] == 1 && counts[2] == 1 && status == ~0ull);
        EXPECT(gci_bam_clip_write(ctx, s.data(), s.size(), offs.data(), (uint32_t)offs.size(), 1, out.data(), 16, &status) == GCI_OK);
        EXPECT(out[0].contig == 1 && out[0].start == 10 && out[1].contig == 1 && out[1].start == 10 + 4094 - 1);
    }
    // the sites of two tracks
    {
        const int64_t total = gci_layout_total(ctx);
        EXPECT(total == 4096 + 73728);
        int32_t *left = nullptr, *right = nullptr;
        EXPECT(gci_malloc(ctx, (size_t)total * 4, (void**)&left) == GCI_OK && gci_malloc(ctx, (size_t)total * 4, (void**)&right) == GCI_OK);
        memset(left, 0, (size_t)total * 4); memset(right, 0, (size_t)total * 4);
        left[0] = 3; right[999] = 4; left[1000] = 9; left[4096] = 2; right[4096] = 3; left[4096 + 69999] = 3; right[total - 1] = 9;
        uint64_t n = 0;
        std::vector<gci_clip_site> sites(8, gci_clip_site{7, 7, 7, 7, 7, 7});
        EXPECT(gci_clip_sites_size(ctx, left, right, nullptr, 3, nullptr, 0, &n) == GCI_OK && n == 4);
        EXPECT(gci_clip_sites_write(ctx, left, right, nullptr, 3, nullptr, 0, sites.data(), 3) == GCI_E_CAPACITY && sites[0].contig == 7);
        EXPECT(gci_clip_sites_write(ctx, left, right, nullptr, 3, nullptr, 0, sites.data(), 8) == GCI_OK);
        const int32_t want[4][4] = {{0, 0, 3, 0}, {0, 999, 0, 4}, {1, 0, 2, 3}, {1, 69999, 3, 0}};
        for (int k = 0; k < 4; k++)
            EXPECT(sites[k].contig == want[k][0] && sites[k].pos == want[k][1] && sites[k].left == want[k][2] && sites[k].right == want[k][3] && sites[k].depth == 0);
        EXPECT(sites[4].contig == 7);
        const gci_window win[2] = {{-5, 1}, {999, total + 100}};
        EXPECT(gci_clip_sites_size(ctx, left, right, left, 4, win, 2, &n) == GCI_OK && n == 1);
        EXPECT(gci_clip_sites_write(ctx, left, right, left, 4, win, 2, sites.data(), 8) == GCI_OK && sites[0].pos == 999 && sites[0].depth == 0);
        EXPECT(gci_clip_sites_size(ctx, left, right, nullptr, 0, nullptr, 0, &n) == GCI_E_INVALID);
        gci_free(ctx, left); gci_free(ctx, right);
    }
    gci_ctx_destroy(ctx);
    printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
