// asan_mismatch_main.cpp -- the CPU twin's mismatch functions (gci_fasta_codes, gci_bam_mismatch_size / _write, gci_mismatch_sites_size /
// _write) under AddressSanitizer and UBSan, as a stand-alone program: the malformed and boundary cases -- SEQ in a heap block of its
// exact size, so a base read behind it is reported --, with the answers written by hand.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/asan_mismatch_main.cpp -o asan_mismatch && ./asan_mismatch
#include "../gci_amd/csrc/cpu/gci_cpu.cpp"

#include <stdio.h>

namespace {

typedef std::pair<uint32_t, uint32_t> Op;             // (code, length)

void put32(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); }

// one record with a one-letter name and no tags, appended to the stream: SEQ from the letters of `seq`, QUAL 0xFF
void add_record(std::vector<uint8_t>& s, std::vector<uint64_t>& offs, int32_t ref_id, int32_t pos, uint16_t flag, const std::vector<Op>& cigar,
                const std::string& seq)
{
    const uint32_t l_seq = (uint32_t)seq.size();
    offs.push_back(s.size());
    put32(s, (uint32_t)(32 + 2 + 4 * cigar.size() + (l_seq + 1) / 2 + l_seq));
    put32(s, (uint32_t)ref_id); put32(s, (uint32_t)pos);
    s.push_back(2); s.push_back(60); s.push_back(0); s.push_back(0);                      // l_read_name, mapq, bin
    s.push_back((uint8_t)cigar.size()); s.push_back((uint8_t)(cigar.size() >> 8));
    s.push_back((uint8_t)flag); s.push_back((uint8_t)(flag >> 8));
    put32(s, l_seq); put32(s, (uint32_t)-1); put32(s, (uint32_t)-1); put32(s, 0);         // l_seq, next refID, next pos, tlen
    s.push_back('r'); s.push_back(0);
    for (const Op& o : cigar) put32(s, (o.second << 4) | o.first);
    static const std::string codes = "=ACMGRSVTWYHKDBN";
    for (uint32_t k = 0; k < l_seq; k += 2) {
        const uint32_t hi = (uint32_t)codes.find(seq[k]), lo = k + 1 < l_seq ? (uint32_t)codes.find(seq[k + 1]) : 0u;
        s.push_back((uint8_t)((hi << 4) | lo));
    }
    for (uint32_t k = 0; k < l_seq; k++) s.push_back(0xFF);
}

int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

bool is(const gci_ivl& v, int32_t contig, int32_t p) { return v.contig == contig && v.start == p && v.end == p && v.pad == 0; }

}  // namespace

int main()
{
    enum { M = 0, I = 1, D = 2, N = 3, S = 4, H = 5, EQ = 7, X = 8 };
    gci_ctx* ctx = nullptr;
    EXPECT(gci_ctx_create(0, nullptr, 0, &ctx) == GCI_OK);
    const int64_t lengths[2] = {20, 6};
    EXPECT(gci_layout_set(ctx, 2, lengths) == GCI_OK);
    const int64_t total = gci_layout_total(ctx);
    EXPECT(total == 8192);
    const int32_t sel[2] = {0, 1};
    uint64_t counts[3], status = 0;

    // the assembly: CRLF, a blank line, lower case, N and R, a record left out, no final newline -- in a block of its exact size
    const std::string fa = ">d x\r\nacg\r\n\r\nNRt\r\n>extra\nGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGG\n>c\nACGTACGTAC\nGTACGTACGT";
    uint8_t* text = nullptr;
    EXPECT(gci_malloc(ctx, fa.size(), (void**)&text) == GCI_OK);
    memcpy(text, fa.data(), fa.size());
    const int64_t d0 = (int64_t)fa.find("acg"), e0 = (int64_t)fa.find(">extra"), d1 = e0 + 7, e1 = (int64_t)fa.find(">c"), d2 = e1 + 3;
    const int64_t body[6] = {d0, e0, d1, e1, d2, (int64_t)fa.size()};
    const int64_t dst[3] = {4096, -1, 0};
    std::vector<uint64_t> kept0(2, 0);
    std::vector<uint8_t> codes((size_t)total, 0xEE);
    EXPECT(gci_fasta_codes(ctx, text, fa.size(), body, 3, dst, kept0.data(), codes.data()) == GCI_OK);
    const uint8_t want_c[20] = {1, 2, 4, 8, 1, 2, 4, 8, 1, 2, 4, 8, 1, 2, 4, 8, 1, 2, 4, 8}, want_d[6] = {1, 2, 4, 15, 5, 8};
    EXPECT(!memcmp(codes.data(), want_c, 20) && !memcmp(codes.data() + 4096, want_d, 6) && codes[20] == 0xEE && codes[4102] == 0xEE && codes[4095] == 0xEE);
    const int64_t dst_end[3] = {total - 2, -1, -1};                            // a record that would run over the array's end: cut there
    EXPECT(gci_fasta_codes(ctx, text, fa.size(), body, 3, dst_end, kept0.data(), codes.data()) == GCI_OK && codes[(size_t)total - 1] == 2);
    gci_free(ctx, text);
    for (int64_t p = 20; p < 4096; p++) codes[(size_t)p] = 15;
    for (int64_t p = 4102; p < total; p++) codes[(size_t)p] = 15;

    // the records, the stream in a heap block of its exact size: the last record's SEQ ends 5 bytes (QUAL) in front of the block's end
    std::vector<gci_ivl> out(16, gci_ivl{7, 7, 7, 7});
    {
        std::vector<uint8_t> s(12, 0);
        std::vector<uint64_t> offs;
        add_record(s, offs, 0, 2, 0, {{S, 1}, {M, 5}}, "TGTCCG");                   // 0: base 4 reads C
        add_record(s, offs, 0, 0, 0, {{EQ, 3}, {X, 3}, {M, 2}}, "AGGTACGA");        // 1: base 1 under =, none under X, base 7
        add_record(s, offs, 1, 0, 0, {{M, 6}}, "AGGAAT");                           // 2: G against c; N and R are never compared
        add_record(s, offs, 0, 0, 0, {{M, 4}}, "=NRA");                             // 3: only A against T
        add_record(s, offs, 0, 16, 0, {{M, 8}}, "TTTTTTTT");                        // 4: over the contig's end: A C G T at 16 - 19, three mismatches
        add_record(s, offs, 0, 0, 0, {{M, 4}}, "");                                 // 5: SEQ *: counted, nothing compared
        add_record(s, offs, 0, 0, 0x100, {{M, 4}}, "TTTT");                         // 6: skipped
        add_record(s, offs, 0, 0x7FFFFFF0, 0, {{M, 4}}, "TTTT");                    // 7: beyond the contig
        add_record(s, offs, 0, 4, 0, {{S, 1}, {M, 4}, {I, 1}}, "TTTTT");            // 8: l_seq one less than S + M + I: malformed
        add_record(s, offs, 0, 8, 0, {{M, 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1},
                                      {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {N, (1u << 28) - 1}, {M, 3}}, "TTTT");     // 9: past 2^31
        add_record(s, offs, 0, 8, 0, {{M, 4}}, "TTTTT");                            // 10: l_seq one more
        uint8_t* bam = nullptr;
        EXPECT(gci_malloc(ctx, s.size(), (void**)&bam) == GCI_OK);
        memcpy(bam, s.data(), s.size());
        const uint32_t n = (uint32_t)offs.size();
        EXPECT(gci_bam_mismatch_size(ctx, bam, s.size(), offs.data(), n, 0, sel, 2, 0x704, 0, codes.data(), counts, &status) == GCI_E_INVALID);
        EXPECT(gci_bam_mismatch_size(ctx, bam, s.size(), offs.data(), n, 1, sel, 2, 0x704, 0, codes.data(), counts, &status) == GCI_OK);
        EXPECT(counts[0] == 10 && counts[1] == 9 && counts[2] == 5 + 8 + 4 + 1 + 4 + 1);
        EXPECT(status == ((8ull << 8) | 7ull));
        EXPECT(gci_bam_mismatch_write(ctx, bam, s.size(), offs.data(), n, 1, codes.data(), out.data(), 8, &status) == GCI_E_CAPACITY && out[0].contig == 7);
        EXPECT(gci_bam_mismatch_write(ctx, bam, s.size(), offs.data(), n, 1, codes.data(), out.data(), 9, &status) == GCI_OK);
        EXPECT(is(out[0], 0, 4) && is(out[1], 0, 1) && is(out[2], 0, 7) && is(out[3], 1, 1) && is(out[4], 0, 3));
        EXPECT(is(out[5], 0, 16) && is(out[6], 0, 17) && is(out[7], 0, 18) && is(out[8], 0, 8) && out[9].contig == 7);
        EXPECT(gci_bam_mismatch_write(ctx, bam, s.size(), offs.data(), n - 1, 1, codes.data(), out.data(), 16, &status) == GCI_E_INVALID);
        // the stream cut inside the last record's SEQ: reported, not read
        EXPECT(gci_bam_mismatch_size(ctx, bam, s.size() - 7, offs.data(), n, 1, sel, 2, 0x704, 0, codes.data(), counts, &status) == GCI_OK);
        EXPECT(counts[0] == 9 && counts[1] == 9 && status == ((8ull << 8) | 7ull));
        gci_free(ctx, bam);
    }
    // 4097 operations of one base each: an I as the last operation of chunk 0, a D as the first of chunk 1
    {
        const int64_t big[1] = {5000};
        EXPECT(gci_layout_set(ctx, 1, big) == GCI_OK);
        std::vector<uint8_t> ref((size_t)gci_layout_total(ctx), 1);            // A everywhere
        std::vector<uint8_t> s(12, 0);
        std::vector<uint64_t> offs;
        std::vector<Op> ops(4097, Op(M, 1));
        ops[2047] = Op(I, 1); ops[2048] = Op(D, 2);
        std::string seq(4096, 'A');
        seq[2046] = 'C'; seq[2047] = 'G'; seq[2048] = 'T'; seq[4095] = 'C';    // the base in front of the I, the inserted base, the base behind the D, the last
        add_record(s, offs, 0, 10, 0, ops, seq);
        EXPECT(gci_bam_mismatch_size(ctx, s.data(), s.size(), offs.data(), 1, 1, sel, 1, 0x704, 0, ref.data(), counts, &status) == GCI_OK);
        EXPECT(counts[0] == 1 && counts[1] == 3 && counts[2] == 4095 && status == ~0ull);
        std::fill(out.begin(), out.end(), gci_ivl{7, 7, 7, 7});
        EXPECT(gci_bam_mismatch_write(ctx, s.data(), s.size(), offs.data(), 1, 1, ref.data(), out.data(), 16, &status) == GCI_OK);
        // 2047 M, then the I, then 2 deleted bases: operation 2049 begins at 10 + 2049; the last M at 10 + 2047 + 2 + 2047
        EXPECT(is(out[0], 0, 10 + 2046) && is(out[1], 0, 10 + 2049) && is(out[2], 0, 10 + 4096) && out[3].contig == 7);
    }
    // the sites of two tracks
    {
        const int64_t two[2] = {1000, 70000};
        EXPECT(gci_layout_set(ctx, 2, two) == GCI_OK);
        const int64_t n_el = gci_layout_total(ctx);
        int32_t *mm = nullptr, *depth = nullptr;
        EXPECT(gci_malloc(ctx, (size_t)n_el * 4, (void**)&mm) == GCI_OK && gci_malloc(ctx, (size_t)n_el * 4, (void**)&depth) == GCI_OK);
        memset(mm, 0, (size_t)n_el * 4);
        for (int64_t p = 0; p < n_el; p++) depth[p] = 8;
        for (int p = 0; p < 3; p++) mm[p] = 4;                                // contig 0: 0 - 2
        for (int p = 990; p < 1010; p++) mm[p] = 5;                           // ... 990 - 999, then padding
        mm[995] = 7; depth[995] = 9; mm[997] = 7; depth[997] = 11;            // the maximum twice: the depth of the first
        for (int p = 4096; p < 4100; p++) mm[p] = 4;                          // contig 1 from its first base
        mm[4096 + 69999] = 8; mm[n_el - 1] = 8;                               // the contig's last base; padding
        mm[4096 + 500] = 3; depth[4096 + 500] = 6; mm[4096 + 501] = 500001; depth[4096 + 501] = 1000000; mm[4096 + 502] = 499999; depth[4096 + 502] = 1000000;
        uint64_t n = 0;
        std::vector<gci_mismatch_site> sites(8, gci_mismatch_site{7, 7, 7, 7, 7});
        EXPECT(gci_mismatch_sites_size(ctx, mm, depth, 3, 500000, nullptr, 0, &n) == GCI_OK && n == 5);
        EXPECT(gci_mismatch_sites_write(ctx, mm, depth, 3, 500000, nullptr, 0, sites.data(), 4) == GCI_E_CAPACITY && sites[0].contig == 7);
        EXPECT(gci_mismatch_sites_write(ctx, mm, depth, 3, 500000, nullptr, 0, sites.data(), 8) == GCI_OK);
        const int32_t want[5][5] = {{0, 0, 3, 4, 8}, {0, 990, 1000, 7, 9}, {1, 0, 4, 4, 8}, {1, 500, 502, 500001, 1000000}, {1, 69999, 70000, 8, 8}};
        for (int k = 0; k < 5; k++)
            EXPECT(sites[k].contig == want[k][0] && sites[k].start == want[k][1] && sites[k].end == want[k][2] && sites[k].mismatch == want[k][3] &&
                   sites[k].depth == want[k][4]);
        EXPECT(sites[5].contig == 7);
        const gci_window win[3] = {{-5, 2}, {2, 995}, {995, n_el + 100}};      // touching windows cut the runs
        EXPECT(gci_mismatch_sites_size(ctx, mm, depth, 3, 500000, win, 3, &n) == GCI_OK && n == 7);
        EXPECT(gci_mismatch_sites_write(ctx, mm, depth, 3, 500000, win, 3, sites.data(), 8) == GCI_OK);
        EXPECT(sites[0].start == 0 && sites[0].end == 2 && sites[1].start == 2 && sites[1].end == 3 && sites[2].start == 990 && sites[2].end == 995);
        EXPECT(sites[3].start == 995 && sites[3].end == 1000 && sites[5].contig == 1 && sites[5].start == 500 && sites[5].end == 502);
        EXPECT(gci_mismatch_sites_size(ctx, mm, depth, 0, 500000, nullptr, 0, &n) == GCI_E_INVALID);
        EXPECT(gci_mismatch_sites_size(ctx, mm, depth, 3, 1000001, nullptr, 0, &n) == GCI_E_INVALID);
        EXPECT(gci_mismatch_sites_write(ctx, mm, depth, 3, 500001, win, 3, sites.data(), 8) == GCI_E_INVALID);      // not the fraction of the size call
        gci_free(ctx, mm); gci_free(ctx, depth);
    }
    gci_ctx_destroy(ctx);
    printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
