// san_index.cpp — stand-alone driver of the index object (kmerseek_amd/csrc/ks_host.cpp) over the CPU stand-in.
// TEST INFRASTRUCTURE ONLY: built with the host sanitizers by tests/hostsan/build.py, run by tests/test_host_sanitizers_cpu.py.
//
//   san_index search DIR TARGETS_FASTA QUERY_FASTA MANY_FASTA OUT_JSON NSEEDS JITTER_US
//       index TARGETS (process_fasta, small batches), search QUERY, save / load / equivalence, then MANY (>= 64 records per
//       batch: the validation fan-out) through add_records and process_fasta, and a batch with bad records; JSON -> OUT_JSON
//   san_index hostile DIR N_MUTATIONS
//       one small valid state file; every truncation, every length / count field replaced by 0, 2^32, 2^63, 2^64 - 1 and
//       N_MUTATIONS seeded byte mutations are loaded: each load is an error or a valid index
#include <sys/resource.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kmerseek_host_c.h"
#include "stub_common.h"

namespace {
char g_err[512];

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);       \
            printf(__VA_ARGS__);                              \
            printf(" [err: %s]\n", g_err);                    \
            return 1;                                         \
        }                                                     \
    } while (0)

bool read_file(const std::string &path, std::string &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}
bool write_file(const std::string &path, const std::string &s) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    return fclose(f) == 0 && ok;
}

// (sequence, name) records of a FASTA file of any supported compression: a plain reader for the driver's own use
bool read_fasta(const char *path, std::vector<std::pair<std::string, std::string>> &recs) {
    uint8_t *data = nullptr;
    uint64_t len = 0;
    char fmt[16];
    if (ksh_input_decompress(path, &data, &len, fmt, sizeof fmt, g_err, sizeof g_err) != 0) return false;
    size_t p = 0;
    while (p < len) {
        size_t e = p;
        while (e < len && data[e] != '\n') e++;
        std::string line((const char *)data + p, e - p);
        while (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty() && line[0] == '>') recs.emplace_back(std::string(), line.substr(1));
        else if (!recs.empty()) recs.back().first += line;
        p = e + 1;
    }
    ksh_input_free(data);
    return true;
}

struct Ptrs {
    std::vector<const char *> seq, name;
    explicit Ptrs(const std::vector<std::pair<std::string, std::string>> &r) {
        for (auto &x : r) { seq.push_back(x.first.c_str()); name.push_back(x.second.c_str()); }
    }
};

int search_once(const std::string &dir, const char *targets, const char *query, const char *many, std::string &json_out) {
    const std::string db = dir + "/targets.db";
    ksh_index *ix = nullptr, *back = nullptr;
    CHECK(ksh_index_new(db.c_str(), 16, 5, "hp", 0, 0, 0, &ix, g_err, sizeof g_err) == 0, "ksh_index_new");
    CHECK(ksh_index_process_fasta(ix, targets, 0, 7, g_err, sizeof g_err) == 0, "process_fasta(targets)");
    std::vector<std::pair<std::string, std::string>> q;
    CHECK(read_fasta(query, q) && !q.empty(), "query fasta");
    Ptrs qp(q);
    char *json = nullptr;
    CHECK(ksh_index_search_ex(ix, qp.seq.data(), qp.name.data(), (uint32_t)q.size(), 1, 0.0, &json, g_err, sizeof g_err) == 0 && json, "search_ex");
    json_out = json;
    ksh_string_free(json);
    // process_fasta saved the state: the loaded index is equivalent and answers the same
    CHECK(ksh_index_load(db.c_str(), 0, &back, g_err, sizeof g_err) == 0, "load");
    int eq = 0;
    CHECK(ksh_index_is_equivalent_to(ix, back, &eq, g_err, sizeof g_err) == 0 && eq == 1, "loaded index is not equivalent");
    json = nullptr;
    CHECK(ksh_index_search_ex(back, qp.seq.data(), qp.name.data(), (uint32_t)q.size(), 1, 0.0, &json, g_err, sizeof g_err) == 0 && json, "search_ex(loaded)");
    CHECK(json_out == json, "the loaded index answers differently");
    ksh_string_free(json);
    // a threshold nothing reaches, and an invalid one
    json = nullptr;
    CHECK(ksh_index_search_ex(ix, qp.seq.data(), qp.name.data(), (uint32_t)q.size(), 1, 2.0, &json, g_err, sizeof g_err) == 0 && json && !strcmp(json, "[]"),
          "min_containment 2.0 keeps rows");
    ksh_string_free(json);
    json = nullptr;
    CHECK(ksh_index_search_ex(ix, qp.seq.data(), qp.name.data(), (uint32_t)q.size(), 1, -1.0, &json, g_err, sizeof g_err) != 0 && !json, "min_containment -1 accepted");
    ksh_index_free(back);
    back = nullptr;

    // >= 64 records in one batch: prepare_records fans the validation out over threads
    std::vector<std::pair<std::string, std::string>> m;
    CHECK(read_fasta(many, m) && m.size() >= 128, "many fasta");
    Ptrs mp(m);
    const uint64_t before = ksh_index_signature_count(ix);
    CHECK(ksh_index_add_records(ix, mp.seq.data(), mp.name.data(), (uint32_t)m.size(), 1, g_err, sizeof g_err) == 0, "add_records(many)");
    const uint64_t after = ksh_index_signature_count(ix);
    CHECK(after > before && after <= before + m.size(), "signature count %llu -> %llu", (unsigned long long)before, (unsigned long long)after);
    CHECK(ksh_index_save_state(ix, g_err, sizeof g_err) == 0, "save_state");
    CHECK(ksh_index_load(db.c_str(), 0, &back, g_err, sizeof g_err) == 0, "load after add_records");
    CHECK(ksh_index_is_equivalent_to(ix, back, &eq, g_err, sizeof g_err) == 0 && eq == 1, "loaded index is not equivalent (many)");
    CHECK(ksh_index_is_equivalent_to(back, ix, &eq, g_err, sizeof g_err) == 0 && eq == 1, "equivalence is not symmetric");
    ksh_index_free(back);
    back = nullptr;
    const std::string db2 = dir + "/many.db";
    ksh_index *mx = nullptr;
    CHECK(ksh_index_new(db2.c_str(), 16, 5, "hp", 1, 0, 0, &mx, g_err, sizeof g_err) == 0, "ksh_index_new(many)");
    CHECK(ksh_index_process_fasta(mx, many, 0, 100, g_err, sizeof g_err) == 0, "process_fasta(many)");
    CHECK(ksh_index_signature_count(mx) == after - before, "process_fasta(many) stored %llu signatures, add_records %llu",
          (unsigned long long)ksh_index_signature_count(mx), (unsigned long long)(after - before));
    CHECK(ksh_index_is_equivalent_to(ix, mx, &eq, g_err, sizeof g_err) == 0 && eq == 0, "different indexes are equivalent");
    // several bad records in one fanned-out batch: the first in record order is the one reported, nothing is stored
    std::vector<std::pair<std::string, std::string>> bad = m;
    bad[bad.size() - 2].first.insert(3, "1");
    bad[bad.size() / 2].first.insert(7, "2");
    bad[5].first.insert(11, "3");
    Ptrs bp(bad);
    const int rc = ksh_index_add_records(mx, bp.seq.data(), bp.name.data(), (uint32_t)bad.size(), 1, g_err, sizeof g_err);
    CHECK(rc == 3 && !strcmp(g_err, "Invalid amino acid '3' found at position 12"), "bad batch: rc %d", rc);
    CHECK(ksh_index_signature_count(mx) == after - before, "a failed batch stored signatures");
    g_err[0] = 0;
    ksh_index_free(mx);
    ksh_index_free(ix);
    CHECK(stub_live_bytes() == 0, "%llu bytes of stubbed memory still allocated", (unsigned long long)stub_live_bytes());
    return 0;
}

int cmd_search(int argc, char **argv) {
    if (argc < 7) return 2;
    const std::string dir = argv[0];
    const int nseeds = atoi(argv[5]);
    const unsigned jitter = (unsigned)atoi(argv[6]);
    std::string first;
    for (int s = 0; s < nseeds; s++) {
        stub_reset();
        stub_jitter(4000 + (uint64_t)s, jitter);
        std::string json;
        if (search_once(dir, argv[1], argv[2], argv[3], json)) return 1;
        if (s == 0) first = json;
        else if (json != first) { printf("FAIL seed %d: search rows differ from seed 0\n", s); return 1; }
    }
    if (!write_file(argv[4], first)) { printf("FAIL cannot write %s\n", argv[4]); return 1; }
    printf("ok %d seeds\n", nseeds);
    return 0;
}

// ---- hostile state files ---------------------------------------------------------------------------------------------
// Offsets of every 8-byte length / count field of a valid state file, found by walking the layout save_state writes.
struct Walker {
    const std::string &b;
    size_t p = 8; // behind the magic
    std::vector<size_t> fields;
    bool ok = true;
    uint64_t u64(bool is_len) {
        if (p + 8 > b.size()) { ok = false; return 0; }
        uint64_t v;
        memcpy(&v, b.data() + p, 8);
        if (is_len) fields.push_back(p);
        p += 8;
        return v;
    }
    void skip(uint64_t n) { if (n > b.size() - p) ok = false; else p += (size_t)n; }
    void str() { skip(u64(true)); }
    bool walk() {
        str(); u64(false); u64(false); u64(false);         // moltype, ksize, scaled, store_raw
        skip(u64(true) * 16);                              // combined sketch
        const uint64_t ns = u64(true);
        for (uint64_t s = 0; ok && s < ns; s++) {
            str(); str();                                  // name, md5sum
            skip(u64(true) * 16);                          // mins + abundances
            if (u64(false)) str();                         // raw flag, raw sequence
            const uint64_t nk = u64(true);
            for (uint64_t k = 0; ok && k < nk; k++) {
                u64(false); str();                         // hash, encoded k-mer
                const uint64_t no = u64(true);
                for (uint64_t o = 0; ok && o < no; o++) { str(); skip(u64(true) * 8); }
            }
        }
        return ok && p == b.size();
    }
};

long max_rss_kb() {
    struct rusage u;
    getrusage(RUSAGE_SELF, &u);
    return u.ru_maxrss;
}

// 1 = rejected with an error, 0 = loaded (and freed), -1 = the driver itself failed
int load_one(const std::string &path, const std::string &blob) {
    if (!write_file(path, blob)) return -1;
    ksh_index *ix = nullptr;
    g_err[0] = 0;
    const int rc = ksh_index_load(path.c_str(), 0, &ix, g_err, sizeof g_err);
    if (rc == 0) {
        if (!ix) return -1;
        // a file that loads is a valid index: it can be used
        (void)ksh_index_signature_count(ix);
        char *json = nullptr;
        if (ksh_index_dump_json(ix, 1, &json) != 0) { ksh_index_free(ix); return -1; }
        ksh_string_free(json);
        ksh_index_free(ix);
        return 0;
    }
    return (ix == nullptr && g_err[0]) ? 1 : -1;
}

int cmd_hostile(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[0], db = dir + "/small.db", probe = dir + "/probe.db";
    const int n_mut = atoi(argv[1]);
    ksh_index *ix = nullptr;
    CHECK(ksh_index_new(db.c_str(), 5, 1, "protein", 1, 0, 0, &ix, g_err, sizeof g_err) == 0, "ksh_index_new");
    const char *seqs[3] = {"PLANTANDANIMALGENQMES", "LIVINGALIVE", "ACDEFGHIKLMNPQRSTVWY"}, *names[3] = {"p1", "p2", "p3"};
    CHECK(ksh_index_add_records(ix, seqs, names, 3, 0, g_err, sizeof g_err) == 0, "add_records");
    CHECK(ksh_index_save_state(ix, g_err, sizeof g_err) == 0, "save_state");
    ksh_index_free(ix);
    std::string blob;
    CHECK(read_file(db, blob) && blob.size() > 1024 && blob.size() < 16384, "state file of %zu bytes", blob.size());
    CHECK(load_one(probe, blob) == 0, "the valid file does not load");
    Walker w{blob};
    CHECK(w.walk(), "the driver's walk of the file layout does not end at the end of the file");
    const long rss0 = max_rss_kb();

    size_t rejected = 0, total = 0;
    for (size_t cut = 0; cut < blob.size(); cut++) {
        const int r = load_one(probe, blob.substr(0, cut));
        CHECK(r >= 0, "truncation to %zu bytes", cut);
        CHECK(r == 1, "a file truncated to %zu of %zu bytes loaded", cut, blob.size());
        rejected += (size_t)r; total++;
    }
    printf("truncations: %zu of %zu rejected\n", rejected, total);

    static const uint64_t lies[4] = {0, 1ULL << 32, 1ULL << 63, ~0ULL};
    size_t f_rej = 0, f_tot = 0;
    for (size_t at : w.fields)
        for (uint64_t v : lies) {
            uint64_t old;
            memcpy(&old, blob.data() + at, 8);
            if (old == v) continue;
            std::string bad = blob;
            memcpy(&bad[at], &v, 8);
            const int r = load_one(probe, bad);
            CHECK(r >= 0, "field at %zu = %llu", at, (unsigned long long)v);
            f_rej += (size_t)r; f_tot++;
        }
    printf("fields: %zu length / count fields, %zu of %zu replacements rejected\n", w.fields.size(), f_rej, f_tot);

    uint64_t rng = 0x5eed;
    auto next = [&]() { rng = rng * 6364136223846793005ULL + 1442695040888963407ULL; return rng >> 33; };
    size_t m_rej = 0;
    for (int i = 0; i < n_mut; i++) {
        std::string bad = blob;
        const int nb = 1 + (int)(next() % 3);
        for (int j = 0; j < nb; j++) bad[next() % bad.size()] = (char)next();
        if (next() % 8 == 0) bad.resize(next() % bad.size()); // some are cut as well
        const int r = load_one(probe, bad);
        CHECK(r >= 0, "mutation %d", i);
        m_rej += (size_t)r;
    }
    printf("mutations: %zu of %d rejected (%.1f %%)\n", m_rej, n_mut, n_mut ? 100.0 * (double)m_rej / n_mut : 0.0);
    // No load may allocate the size a field lies about: the smallest lie is 2^32 entries (>= 4 GiB, zero-filled by the
    // containers that would hold it, so resident); the honest loads of a file of a few KB stay far below 1 GiB in all.
    const long grown_kb = max_rss_kb() - rss0;
    printf("peak resident memory grew by %ld KiB\n", grown_kb);
    CHECK(grown_kb < (1L << 20), "resident memory grew by %ld KiB: a lying size was allocated", grown_kb);
    CHECK(stub_live_bytes() == 0, "%llu bytes of stubbed memory still allocated", (unsigned long long)stub_live_bytes());
    printf("ok\n");
    return 0;
}
} // namespace

int main(int argc, char **argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc >= 2 && !strcmp(argv[1], "search")) return cmd_search(argc - 2, argv + 2);
    if (argc >= 2 && !strcmp(argv[1], "hostile")) return cmd_hostile(argc - 2, argv + 2);
    fprintf(stderr, "usage: san_index search|hostile ... (see the head of san_index.cpp)\n");
    return 2;
}
