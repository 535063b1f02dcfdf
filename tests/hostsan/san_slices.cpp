// san_slices — the slice cutter of the traceback and the stitch (rp_cut_slices, ks_rpath_kit.h: its host half, which needs
// nothing of the project's and no device) under AddressSanitizer + UBSan.  TEST INFRASTRUCTURE ONLY.
//
//     san_slices BUDGET_ROWS OFF_0 OFF_1 ... OFF_N      (the exclusive scan of the items' rows: N + 1 values, N >= 0)
//
// prints one line: bad=<index or -1> bad_rows=<rows> max_rows=<rows> cut=<a,b,...> first_row=<a,b,...>
// The offsets are handed over in a heap block of exactly N + 1 words, so a read past either end is seen.
#include "../../kmerseek_amd/csrc/ks_rpath_kit.h"
#include <cstdio>
#include <cstdlib>
#include <memory>

static void list(const char *name, const std::vector<uint64_t> &v) {
    std::printf(" %s=", name);
    for (size_t i = 0; i < v.size(); i++) std::printf(i ? ",%llu" : "%llu", (unsigned long long)v[i]);
}

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: san_slices BUDGET_ROWS OFF_0 ... OFF_N\n"); return 2; }
    const uint64_t budget = std::strtoull(argv[1], nullptr, 10), n = (uint64_t)argc - 3;
    std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
    for (uint64_t i = 0; i <= n; i++) off[i] = std::strtoull(argv[2 + i], nullptr, 10);
    const rp_slices Z = rp_cut_slices(off.get(), n, budget);
    std::printf("bad=%lld bad_rows=%llu max_rows=%llu", Z.bad < n ? (long long)Z.bad : -1LL, (unsigned long long)Z.bad_rows,
                (unsigned long long)Z.max_rows);
    list("cut", Z.cut);
    list("first_row", Z.first_row);
    std::printf("\n");
    return 0;
}
