// A stand-alone program over gci_amd/csrc/cpu/gci_cpu.cpp for tests/test_depth_gz_cpu.py, built with -fsanitize=address,undefined:
// the twin of k_depth_gz.hip on candidates that are no member starts and on members cut short, every buffer a heap block of
// exactly its size so that one byte read beyond it is reported.
//     depth_gz_fuzz <file of members> <position of a whole member in it> <its end>
#include "../gci_amd/csrc/cpu/gci_cpu.cpp"

#include <stdio.h>

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const std::vector<uint8_t> file = slurp(argv[1]);
    const uint64_t pos = strtoull(argv[2], nullptr, 10), end = strtoull(argv[3], nullptr, 10);
    if (file.empty() || end > file.size() || pos >= end) return 2;
    static const uint8_t head[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF};
    gci_ctx* ctx = nullptr;
    if (gci_ctx_create(0, nullptr, 0, &ctx) != GCI_OK) return 3;
    unsigned long accepted = 0, refused = 0;
    // the header stamped at every byte offset: what follows is another member's bits
    for (uint64_t o = 0; o < file.size(); o++) {
        const uint64_t n = file.size();
        uint8_t* raw = (uint8_t*)malloc(n);
        memcpy(raw, file.data(), n);
        for (uint64_t k = 0; k < 10 && o + k < n; k++) raw[o + k] = head[k];
        gci_dgz_info info;
        if (gci_depth_gz_scan(ctx, raw, n, &o, 1, &info) != GCI_OK) return 4;
        if (info.status == GCI_DGZ_OK) {
            if (info.end > n || info.end <= o) { fprintf(stderr, "offset %llu: end %llu of %llu\n", (unsigned long long)o, (unsigned long long)info.end, (unsigned long long)n); return 5; }
            accepted++;
            std::vector<gci_dgz_run> runs(info.runs ? info.runs : 1);
            gci_dgz_member m = {o, 0, 0, info.runs, info.lines};
            std::vector<int32_t> track(info.lines ? info.lines : 1);
            if (gci_depth_gz_runs(ctx, raw, n, &m, 1, runs.data()) != GCI_OK) return 4;
            if (gci_depth_gz_expand(ctx, runs.data(), &m, 1, track.data(), info.lines) != GCI_OK) return 4;
        } else refused++;
        free(raw);
    }
    // a whole member, then cut short at every byte of its last 64
    for (uint64_t cut = 0; cut <= 64 && cut < end - pos; cut++) {
        const uint64_t n = end - pos - cut, zero = 0;
        uint8_t* raw = (uint8_t*)malloc(n);
        memcpy(raw, file.data() + pos, n);
        gci_dgz_info info;
        if (gci_depth_gz_scan(ctx, raw, n, &zero, 1, &info) != GCI_OK) return 4;
        if ((info.status == GCI_DGZ_OK) != (cut == 0) || info.end > n) { fprintf(stderr, "cut %llu: status %u end %llu\n", (unsigned long long)cut, info.status, (unsigned long long)info.end); return 6; }
        free(raw);
    }
    gci_ctx_destroy(ctx);
    printf("accepted %lu refused %lu\n", accepted, refused);
    return 0;
}
