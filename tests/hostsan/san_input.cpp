// san_input.cpp — stand-alone driver of ksh_input_decompress (kmerseek_amd/csrc/ks_input.cpp).
// TEST INFRASTRUCTURE ONLY: built with the host sanitizers by tests/hostsan/build.py, run by tests/test_host_sanitizers_cpu.py.
//
//   san_input FORMAT FILE PLAIN TMP N_CUTS N_MUTATIONS
//       FILE decodes to the bytes of PLAIN and reports FORMAT; then at least N_CUTS truncations (an even stride over the
//       file) and N_MUTATIONS seeded byte mutations, written to TMP, each decode to some bytes or fail with an error code.
//       A decompressor library that is not on the machine: "skip FORMAT: <reason>", exit 0 (as the product reports it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/kmerseek_host_c.h"

namespace {
bool read_file(const char *path, std::string &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    out.clear();
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}
bool write_file(const char *path, const std::string &s) {
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    return fclose(f) == 0 && ok;
}
// 0 = bytes, 1 = a documented error; -1 = neither
int decode(const char *path, std::string *out, std::string *fmt, std::string *err) {
    uint8_t *data = nullptr;
    uint64_t len = 0;
    char f[16] = {0}, e[256] = {0};
    const int rc = ksh_input_decompress(path, &data, &len, f, sizeof f, e, sizeof e);
    if (fmt) *fmt = f;
    if (err) *err = e;
    if (rc == 0) {
        if (!data) return -1;
        if (out) out->assign((const char *)data, (size_t)len);
        ksh_input_free(data);
        return 0;
    }
    if (data || (rc != 11 && rc != 13) || !e[0]) return -1;
    return 1;
}
} // namespace

int main(int argc, char **argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc < 7) { fprintf(stderr, "usage: san_input FORMAT FILE PLAIN TMP N_CUTS N_MUTATIONS\n"); return 2; }
    const char *format = argv[1], *file = argv[2], *tmp = argv[4];
    const size_t n_cuts = (size_t)atoi(argv[5]);
    const int n_mut = atoi(argv[6]);
    std::string blob, plain, got, fmt, err;
    if (!read_file(file, blob) || !read_file(argv[3], plain)) { printf("FAIL cannot read the inputs\n"); return 1; }
    int r = decode(file, &got, &fmt, &err);
    if (r == 1 && err.find("could not be loaded") != std::string::npos) { printf("skip %s: %s\n", format, err.c_str()); return 0; }
    if (r != 0 || fmt != format || got != plain) {
        printf("FAIL whole file: r %d, format '%s' (want '%s'), %zu bytes (want %zu): %s\n", r, fmt.c_str(), format, got.size(), plain.size(), err.c_str());
        return 1;
    }
    const size_t stride = blob.size() / n_cuts ? blob.size() / n_cuts : 1;
    size_t cuts = 0, cut_err = 0;
    for (size_t cut = 0; cut < blob.size(); cut += stride, cuts++) {
        if (!write_file(tmp, blob.substr(0, cut))) { printf("FAIL cannot write %s\n", tmp); return 1; }
        r = decode(tmp, &got, &fmt, &err);
        if (r < 0) { printf("FAIL cut at %zu: neither bytes nor a documented error (%s)\n", cut, err.c_str()); return 1; }
        // what does decode of a cut archive is a prefix of the whole (a cut between two members, or the plain reader)
        if (r == 0 && fmt == format && strcmp(format, "plain") && plain.compare(0, got.size(), got) != 0) {
            printf("FAIL cut at %zu: %zu bytes that are no prefix of the file's\n", cut, got.size());
            return 1;
        }
        cut_err += (size_t)r;
    }
    if (blob.size() >= n_cuts && cuts < n_cuts) { printf("FAIL only %zu cuts\n", cuts); return 1; }
    uint64_t rng = 0xc0ffee;
    auto next = [&]() { rng = rng * 6364136223846793005ULL + 1442695040888963407ULL; return rng >> 33; };
    size_t mut_err = 0;
    for (int i = 0; i < n_mut; i++) {
        std::string bad = blob;
        const int nb = 1 + (int)(next() % 3);
        for (int j = 0; j < nb; j++) bad[next() % bad.size()] = (char)next();
        if (!write_file(tmp, bad)) { printf("FAIL cannot write %s\n", tmp); return 1; }
        r = decode(tmp, nullptr, nullptr, &err);
        if (r < 0) { printf("FAIL mutation %d: neither bytes nor a documented error (%s)\n", i, err.c_str()); return 1; }
        mut_err += (size_t)r;
    }
    printf("ok %s: %zu bytes -> %zu; %zu cuts (%zu errors), %d mutations (%zu errors)\n", format, blob.size(), plain.size(), cuts, cut_err, n_mut, mut_err);
    return 0;
}
