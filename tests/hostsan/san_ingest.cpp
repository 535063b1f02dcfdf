// san_ingest.cpp — stand-alone driver of ksh_sketch_fasta (kmerseek_amd/csrc/ks_ingest.cpp) over the CPU stand-in.
// TEST INFRASTRUCTURE ONLY: built with the host sanitizers by tests/hostsan/build.py, run by tests/test_host_sanitizers_cpu.py.
//
//   san_ingest sketch FASTA K SCALED MOL VALIDATE BATCH PIPELINE OUT NSEEDS JITTER_US [CAPTURE_OUT]
//       sketches FASTA under NSEEDS jitter seeds; every seed must give the same bytes; the result goes to OUT:
//       u64 n_records, u64 n_hashes, u64 offsets[n_records + 1], u64 hashes[], u32 abunds[], u64 names_len, names
//       CAPTURE_OUT: what the packer handed to the device stage: u64 n_records, u64 n_residues, u64 lengths[], residues
//   san_ingest expect FASTA K SCALED MOL VALIDATE BATCH CODE NSEEDS JITTER_US
//       the call must fail with CODE, pipelined and serial, under every seed, with the same message and nothing left allocated
//   san_ingest faults FASTA K SCALED MOL VALIDATE BATCH NSEEDS JITTER_US
//       one clean run counts the stubbed calls; then the first, a middle and the last call of four of them is made to fail in turn
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kmerseek_host_c.h"
#include "stub_common.h"

namespace {
struct Args {
    const char *fasta; uint32_t k, scaled; const char *mol; int validate; uint64_t batch;
};
Args parse(char **v) { return {v[0], (uint32_t)atoi(v[1]), (uint32_t)atoi(v[2]), v[3], atoi(v[4]), strtoull(v[5], nullptr, 10)}; }

int run(const Args &a, int pipeline, ksh_fasta_sketches **out, std::string &msg) {
    char err[512] = {0};
    *out = nullptr;
    const int rc = ksh_sketch_fasta(a.fasta, a.k, a.scaled, a.mol, a.validate, 0, a.batch, pipeline, out, err, sizeof err);
    msg = err;
    return rc;
}

std::string serialise(ksh_fasta_sketches *r) {
    std::string s;
    auto put = [&](const void *p, size_t n) { if (n) s.append((const char *)p, n); };
    const uint64_t n = ksh_fs_n_records(r), nh = ksh_fs_n_hashes(r);
    put(&n, 8); put(&nh, 8);
    put(ksh_fs_offsets(r), (n + 1) * 8);
    put(ksh_fs_hashes(r), nh * 8);
    put(ksh_fs_abunds(r), nh * 4);
    uint64_t len = 0;
    const char *names = ksh_fs_names(r, &len);
    put(&len, 8); put(names, len);
    return s;
}

bool write_file(const char *path, const std::string &s) {
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    return fclose(f) == 0 && ok;
}

int leaked(const char *what) {
    if (stub_live_bytes() == 0) return 0;
    printf("FAIL %s: %llu bytes of stubbed device / pinned memory still allocated\n", what, (unsigned long long)stub_live_bytes());
    return 1;
}

int cmd_sketch(int argc, char **argv) {
    if (argc < 10) return 2;
    const Args a = parse(argv);
    const int pipeline = atoi(argv[6]);
    const char *out_path = argv[7];
    const int nseeds = atoi(argv[8]);
    const unsigned jitter = (unsigned)atoi(argv[9]);
    const char *cap_path = argc > 10 ? argv[10] : nullptr;
    std::string first;
    for (int s = 0; s < nseeds; s++) {
        stub_reset();
        stub_jitter(1000 + (uint64_t)s, jitter);
        stub_capture(cap_path && s == 0);
        ksh_fasta_sketches *r = nullptr;
        std::string msg;
        const int rc = run(a, pipeline, &r, msg);
        stub_capture(0);
        if (rc != 0) { printf("FAIL seed %d: rc %d: %s\n", s, rc, msg.c_str()); return 1; }
        uint64_t n_res = 0, n_win = 0, n_batches = 0;
        ksh_fs_stats(r, &n_res, &n_win, &n_batches, nullptr);
        const std::string bytes = serialise(r);
        if (s == 0) {
            first = bytes;
            printf("n_records=%llu n_hashes=%llu n_residues=%llu n_windows=%llu n_batches=%llu\n", (unsigned long long)ksh_fs_n_records(r),
                   (unsigned long long)ksh_fs_n_hashes(r), (unsigned long long)n_res, (unsigned long long)n_win, (unsigned long long)n_batches);
            if (cap_path) {
                uint64_t nr = 0, nl = 0;
                const uint8_t *res = stub_captured_residues(&nr);
                const uint64_t *len = stub_captured_lengths(&nl);
                std::string c;
                c.append((const char *)&nl, 8); c.append((const char *)&nr, 8);
                if (nl) c.append((const char *)len, nl * 8);
                if (nr) c.append((const char *)res, nr);
                if (!write_file(cap_path, c)) { printf("FAIL cannot write %s\n", cap_path); return 1; }
            }
        } else if (bytes != first) {
            printf("FAIL seed %d: result differs from seed 0\n", s);
            return 1;
        }
        ksh_fs_free(r);
        if (leaked("sketch")) return 1;
    }
    if (!write_file(out_path, first)) { printf("FAIL cannot write %s\n", out_path); return 1; }
    printf("ok %d seeds\n", nseeds);
    return 0;
}

int cmd_expect(int argc, char **argv) {
    if (argc < 9) return 2;
    const Args a = parse(argv);
    const int code = atoi(argv[6]), nseeds = atoi(argv[7]);
    const unsigned jitter = (unsigned)atoi(argv[8]);
    std::string first;
    for (int s = 0; s < nseeds; s++)
        for (int pipeline = 1; pipeline >= 0; pipeline--) {
            stub_reset();
            stub_jitter(2000 + (uint64_t)s, jitter);
            ksh_fasta_sketches *r = nullptr;
            std::string msg;
            const int rc = run(a, pipeline, &r, msg);
            if (rc != code || r) { printf("FAIL seed %d pipeline %d: rc %d (want %d): %s\n", s, pipeline, rc, code, msg.c_str()); ksh_fs_free(r); return 1; }
            if (first.empty()) { first = msg; printf("msg=%s\n", msg.c_str()); }
            else if (msg != first) { printf("FAIL seed %d pipeline %d: message '%s' differs from '%s'\n", s, pipeline, msg.c_str(), first.c_str()); return 1; }
            if (leaked("expect")) return 1;
        }
    printf("ok %d seeds\n", nseeds);
    return 0;
}

int cmd_faults(int argc, char **argv) {
    if (argc < 8) return 2;
    const Args a = parse(argv);
    const int nseeds = atoi(argv[6]);
    const unsigned jitter = (unsigned)atoi(argv[7]);
    static const char *const fns[] = {"hipHostMalloc", "hipMemcpyAsync", "ks_sketch_batch_device", "ks_sketches_copy_to_host"};
    int cases = 0;
    for (int pipeline = 1; pipeline >= 0; pipeline--) {
        // a clean run without jitter counts the calls (the serial path allocates one slot, the pipeline three)
        stub_reset();
        stub_jitter(0, 0);
        ksh_fasta_sketches *r = nullptr;
        std::string msg;
        if (run(a, pipeline, &r, msg) != 0) { printf("FAIL clean run: %s\n", msg.c_str()); return 1; }
        ksh_fs_free(r);
        int total[4];
        for (int f = 0; f < 4; f++) total[f] = stub_call_count(fns[f]);
        for (int f = 0; f < 4; f++) {
            if (total[f] < 3) { printf("FAIL %s is called %d times: no first / middle / last\n", fns[f], total[f]); return 1; }
            // hipHostMalloc: slots grow on demand, so under another interleaving the count may differ: the last call of the
            // clean run is still a call every run makes or the run ends clean before it (both are checked below)
            const int at[3] = {1, (total[f] + 1) / 2, total[f]};
            for (int w = 0; w < 3; w++)
                for (int s = 0; s < nseeds; s++) {
                    stub_reset();
                    stub_jitter(3000 + (uint64_t)s, jitter);
                    stub_fail_nth(fns[f], at[w], 1 /* hipErrorInvalidValue */ + (fns[f][0] == 'k' ? 5 /* KS_ERR_HIP */ : 0));
                    r = nullptr;
                    const int rc = run(a, pipeline, &r, msg);
                    const bool reached = stub_call_count(fns[f]) >= at[w];
                    if (reached ? (rc != 13 || r || msg.empty()) : rc != 0) {
                        printf("FAIL %s call %d of %d, pipeline %d, seed %d: rc %d (%s), the call was %sreached\n", fns[f], at[w], total[f], pipeline, s, rc,
                               msg.c_str(), reached ? "" : "not ");
                        ksh_fs_free(r);
                        return 1;
                    }
                    if (!reached) printf("note %s call %d not reached under seed %d (pipeline %d)\n", fns[f], at[w], s, pipeline);
                    ksh_fs_free(r);
                    if (leaked(fns[f])) return 1;
                    cases++;
                }
            printf("%s: %d calls, failed at 1 / %d / %d, pipeline %d: code 13 each\n", fns[f], total[f], at[1], at[2], pipeline);
        }
    }
    printf("ok %d cases\n", cases);
    return 0;
}
} // namespace

int main(int argc, char **argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc >= 2 && !strcmp(argv[1], "sketch")) return cmd_sketch(argc - 2, argv + 2);
    if (argc >= 2 && !strcmp(argv[1], "expect")) return cmd_expect(argc - 2, argv + 2);
    if (argc >= 2 && !strcmp(argv[1], "faults")) return cmd_faults(argc - 2, argv + 2);
    fprintf(stderr, "usage: san_ingest sketch|expect|faults ... (see the head of san_ingest.cpp)\n");
    return 2;
}
