// asan_indels_main.cpp -- the CPU twin's indel functions (gci_bam_indel_size / _write, gci_indel_sites_size / _write) under
// AddressSanitizer and UBSan, as a stand-alone program: three record cases (the thresholds next to a cut-off stream; 4097 operations
// with a D on either side of a chunk's edge; a position near 2^31) and one site case, with the answers written by hand.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/asan_indels_main.cpp -o asan_indels && ./asan_indels
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

bool is(const gci_ivl& v, int32_t contig, int32_t start, int32_t end) { return v.contig == contig && v.start == start && v.end == end && v.pad == 0; }

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

    // case 1: the thresholds, the contig's end, a skipped record, and a last record that runs past the stream
    {
        std::vector<uint8_t> s(12, 0);
        std::vector<uint64_t> offs;
        add_record(s, offs, 0, 100, 0, {{M, 10}, {D, 9}, {M, 10}, {D, 10}, {M, 10}, {I, 9}, {M, 5}, {I, 10}, {M, 5}});      // D at 110 and 129, I behind 148 and 153
        add_record(s, offs, 0, 300, 0x800, {{S, 5}, {M, 5}, {D, 5}, {D, 5}, {N, 30}, {M, 5}});      // 5D5D: two deletions of 5
        add_record(s, offs, 0, 0, 0, {{I, 10}, {M, 3}});                    // at = 0: the site is base 0
        add_record(s, offs, 0, 995, 0, {{M, 4}, {D, 10}, {M, 1}, {I, 10}}); // D from the contig's last base on: one base; the I lies behind the contig
        add_record(s, offs, 0, 400, 0x100, {{M, 5}, {D, 50}, {M, 5}});      // skipped
        add_record(s, offs, 0, 500, 0, {{M, 9}});
        s.resize(s.size() - 3);
        const uint32_t n = (uint32_t)offs.size();
        EXPECT(gci_bam_indel_size(ctx, s.data(), s.size(), offs.data(), n, 1, sel, 2, 0x704, 0, 10, counts, &status) == GCI_OK);
        EXPECT(counts[0] == 4 && counts[1] == 2 && counts[2] == 2);
        EXPECT(status == ((5ull << 8) | 7ull));
        EXPECT(gci_bam_indel_write(ctx, s.data(), s.size(), offs.data(), n, 1, out.data(), 3, &status) == GCI_E_CAPACITY && out[0].contig == 7);
        EXPECT(gci_bam_indel_write(ctx, s.data(), s.size(), offs.data(), n, 1, out.data(), 4, &status) == GCI_OK);
        EXPECT(is(out[0], 0, 129, 138) && is(out[1], 0, 999, 999) && is(out[2], 0, 153, 153) && is(out[3], 0, 0, 0) && out[4].contig == 7);
        EXPECT(gci_bam_indel_size(ctx, s.data(), s.size(), offs.data(), n, 1, sel, 2, 0x704, 0, 5, counts, &status) == GCI_OK);
        EXPECT(counts[0] == 4 && counts[1] == 5 && counts[2] == 3);
        EXPECT(gci_bam_indel_write(ctx, s.data(), s.size(), offs.data(), n, 1, out.data(), 16, &status) == GCI_OK);
        EXPECT(is(out[0], 0, 110, 118) && is(out[1], 0, 129, 138) && is(out[2], 0, 305, 309) && is(out[3], 0, 310, 314) && is(out[4], 0, 999, 999));
        EXPECT(is(out[5], 0, 148, 148) && is(out[6], 0, 153, 153) && is(out[7], 0, 0, 0) && out[8].contig == 7);
        EXPECT(gci_bam_indel_size(ctx, s.data(), s.size(), offs.data(), n, 1, sel, 2, 0x704, 0, 0, counts, &status) == GCI_E_INVALID);
        EXPECT(gci_bam_indel_write(ctx, s.data(), s.size(), offs.data(), n - 1, 1, out.data(), 16, &status) == GCI_E_INVALID);
    }
    // case 2: 4097 operations of one base each, a D as the last operation of chunk 0, one as the first of chunk 1, an I behind chunk 1's edge
    {
        std::vector<uint8_t> s(12, 0);
        std::vector<uint64_t> offs;
        std::vector<Op> big(4097, Op(M, 1));
        big[2047] = Op(D, 20); big[2048] = Op(D, 21); big[4095] = Op(I, 22); big[4096] = Op(D, 23);
        add_record(s, offs, 1, 10, 0, big);
        std::fill(out.begin(), out.end(), gci_ivl{7, 7, 7, 7});
        EXPECT(gci_bam_indel_size(ctx, s.data(), s.size(), offs.data(), 1, 1, sel, 2, 0x704, 0, 20, counts, &status) == GCI_OK);
        EXPECT(counts[0] == 1 && counts[1] == 3 && counts[2] == 1 && status == ~0ull);
        EXPECT(gci_bam_indel_write(ctx, s.data(), s.size(), offs.data(), 1, 1, out.data(), 16, &status) == GCI_OK);
        // 2047 M in front of the first D; then 20 + 21 deleted bases and 2046 more M in front of the I
        EXPECT(is(out[0], 1, 10 + 2047, 10 + 2047 + 19) && is(out[1], 1, 10 + 2067, 10 + 2067 + 20));
        EXPECT(is(out[2], 1, 10 + 2088 + 2046, 10 + 2088 + 2046 + 22) && is(out[3], 1, 10 + 2088 + 2046 - 1, 10 + 2088 + 2046 - 1) && out[4].contig == 7);
    }
    // case 3: positions near and beyond 2^31
    {
        std::vector<uint8_t> s(12, 0);
        std::vector<uint64_t> offs;
        add_record(s, offs, 1, 0x7FFFFFF0, 0, {{M, 5}, {D, 30}, {I, 30}, {N, (1u << 28) - 1}, {D, 30}});
        add_record(s, offs, 1, 50, 0, {{D, 30}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1},
                                      {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {D, 30}, {I, 30}});
        std::fill(out.begin(), out.end(), gci_ivl{7, 7, 7, 7});
        EXPECT(gci_bam_indel_size(ctx, s.data(), s.size(), offs.data(), 2, 1, sel, 2, 0x704, 0, 30, counts, &status) == GCI_OK);
        EXPECT(counts[0] == 2 && counts[1] == 1 && counts[2] == 0 && status == ~0ull);
        EXPECT(gci_bam_indel_write(ctx, s.data(), s.size(), offs.data(), 2, 1, out.data(), 16, &status) == GCI_OK);
        EXPECT(is(out[0], 1, 50, 79) && out[1].contig == 7);
    }
    // the sites of two tracks
    {
        const int64_t total = gci_layout_total(ctx);
        EXPECT(total == 4096 + 73728);
        int32_t *del = nullptr, *ins = nullptr, *depth = nullptr;
        EXPECT(gci_malloc(ctx, (size_t)total * 4, (void**)&del) == GCI_OK && gci_malloc(ctx, (size_t)total * 4, (void**)&ins) == GCI_OK &&
               gci_malloc(ctx, (size_t)total * 4, (void**)&depth) == GCI_OK);
        memset(del, 0, (size_t)total * 4); memset(ins, 0, (size_t)total * 4);
        for (int64_t p = 0; p < total; p++) depth[p] = (int32_t)(p % 50);
        for (int p = 0; p < 3; p++) del[p] = 3;                               // contig 0: 0 - 2
        for (int p = 990; p < 1010; p++) ins[p] = 4;                          // ... 990 - 999, then padding
        del[995] = 6;
        for (int p = 4096; p < 4100; p++) del[p] = 3;                         // contig 1 from its first base: 0 - 3
        for (int p = 4096 + 4090; p < 4096 + 4100; p += 2) { del[p] = 3; ins[p + 1] = 5; }      // either track, across a tile's edge
        del[4096 + 69999] = 3; ins[total - 1] = 9;                            // the contig's last base; padding
        del[4096 + 500] = 2;                                                  // one short of min_reads
        uint64_t n = 0;
        std::vector<gci_indel_site> sites(8, gci_indel_site{7, 7, 7, 7, 7, 7});
        EXPECT(gci_indel_sites_size(ctx, del, ins, depth, 3, nullptr, 0, &n) == GCI_OK && n == 5);
        EXPECT(gci_indel_sites_write(ctx, del, ins, depth, 3, nullptr, 0, sites.data(), 4) == GCI_E_CAPACITY && sites[0].contig == 7);
        EXPECT(gci_indel_sites_write(ctx, del, ins, depth, 3, nullptr, 0, sites.data(), 8) == GCI_OK);
        const int32_t want[5][6] = {{0, 0, 3, 3, 0, 2}, {0, 990, 1000, 6, 4, 49}, {1, 0, 4, 3, 0, 49}, {1, 4090, 4100, 3, 5, 45}, {1, 69999, 70000, 3, 0, 45}};
        for (int k = 0; k < 5; k++)
            EXPECT(sites[k].contig == want[k][0] && sites[k].start == want[k][1] && sites[k].end == want[k][2] && sites[k].del == want[k][3] &&
                   sites[k].ins == want[k][4] && sites[k].depth == want[k][5]);
        EXPECT(sites[5].contig == 7);
        const gci_window win[3] = {{-5, 2}, {2, 995}, {995, total + 100}};    // touching windows cut the runs
        EXPECT(gci_indel_sites_size(ctx, del, ins, nullptr, 4, win, 3, &n) == GCI_OK && n == 7);      // ... and the five lone ins bases of contig 1
        EXPECT(gci_indel_sites_write(ctx, del, ins, nullptr, 4, win, 3, sites.data(), 8) == GCI_OK);
        EXPECT(sites[0].start == 990 && sites[0].end == 995 && sites[0].del == 0 && sites[0].ins == 4 && sites[0].depth == 0);
        EXPECT(sites[1].start == 995 && sites[1].end == 1000 && sites[1].del == 6 && sites[2].contig == 1 && sites[2].start == 4091 && sites[2].end == 4092);
        EXPECT(gci_indel_sites_size(ctx, del, ins, nullptr, 0, nullptr, 0, &n) == GCI_E_INVALID);
        EXPECT(gci_indel_sites_write(ctx, del, ins, depth, 4, win, 3, sites.data(), 8) == GCI_E_INVALID);      // not the depth of the size call
        gci_free(ctx, del); gci_free(ctx, ins); gci_free(ctx, depth);
    }
    gci_ctx_destroy(ctx);
    printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
