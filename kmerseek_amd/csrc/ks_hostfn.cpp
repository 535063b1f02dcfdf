// ks_hostfn.cpp — the entry points of the C ABI that touch no device: status text, moltype names, max_hash and the
// validate / resolve pre-step.  Pure host code (no HIP header): the packer threads of ks_ingest.cpp / ks_host.cpp call
// the validator 16 at a time, and a host-only build of the host layer links this file as it stands.
#include <cstdint>
#include <cstring>
#include <exception>
#include <new>

#include "../../include/kmerseek_amd.h"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

namespace {
// The exception guard of the extern "C" boundary for entry points without a context (ks_common.h's ks_guard with
// ctx == nullptr): bad_alloc -> KS_ERR_OOM, anything else -> KS_ERR_HIP; there is no context to carry a message.
template <typename F>
inline int host_guard(F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return KS_ERR_OOM;
    } catch (...) {
        return KS_ERR_HIP;
    }
}
} // namespace

extern "C" const char *ks_status_string(int s) {
    switch (s) {
    case KS_OK: return "ok";
    case KS_ERR_INVALID_MOLTYPE: return "invalid moltype";
    case KS_ERR_INVALID_KSIZE: return "invalid k-mer size";
    case KS_ERR_INVALID_RESIDUE: return "invalid amino acid";
    case KS_ERR_INVALID_ARG: return "invalid argument";
    case KS_ERR_OOM: return "out of device memory";
    case KS_ERR_HIP: return "HIP runtime error";
    case KS_ERR_NO_DEVICE: return "no HIP device";
    case KS_ERR_CAPACITY: return "device list capacity exceeded";
    case KS_ERR_INVALID_SCALED: return "invalid scaled";
    default: return "unknown status";
    }
}

// get_hash_function_from_moltype, src/rust/encoding.rs:17-27
extern "C" int ks_moltype_from_string(const char *name, uint32_t *out) {
    return host_guard([&]() -> int {
    if (!name || !out) return KS_ERR_INVALID_ARG;
    if (!strcmp(name, "protein") || !strcmp(name, "raw")) { *out = KS_PROTEIN; return KS_OK; }
    if (!strcmp(name, "hp")) { *out = KS_HP; return KS_OK; }
    if (!strcmp(name, "dayhoff")) { *out = KS_DAYHOFF; return KS_OK; }
    return KS_ERR_INVALID_MOLTYPE;
    });
}

// sourmash max_hash_for_scaled: (u64::MAX as f64 / scaled as f64) as u64, saturating
extern "C" uint64_t ks_max_hash(uint32_t scaled) {
    if (scaled == 0) return 0;
    if (scaled == 1) return UINT64_MAX;
    double v = 18446744073709551616.0 / (double)scaled;
    if (v >= 18446744073709551616.0) return UINT64_MAX;
    return (uint64_t)v;
}

// ---- host-side pre-step: AminoAcidAmbiguity::validate_and_resolve, src/rust/aminoacid.rs:74-105 ----
static inline u64 splitmix64(u64 *s) {
    u64 z = (*s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

extern "C" int ks_validate_and_resolve(const uint8_t *seq, uint64_t len, int upper, uint64_t rng_seed,
                                       uint8_t *out, uint64_t *out_len, ks_residue_error *err) {
    return host_guard([&]() -> int {
    if ((!seq && len) || !out || !out_len) return KS_ERR_INVALID_ARG;
    // class LUT: 0 invalid, 1 plain valid (20 standard + X U O), 2 stop, 3/4/5 = B/Z/J.  Called from many packer threads
    // at once (ks_ingest.cpp, ks_host.cpp): the table is a function-local static built by its initialiser (C++11
    // guarantees one thread runs it and the others wait), and never written afterwards.
    struct cls_table {
        u8 v[256];
        cls_table() {
            memset(v, 0, sizeof v);
            for (const char *p = "ACDEFGHIKLMNPQRSTVWYXUO"; *p; p++) v[(u8)*p] = 1; // aminoacid.rs:8-14
            v[(u8)'*'] = 2;
            v[(u8)'B'] = 3; v[(u8)'Z'] = 4; v[(u8)'J'] = 5; // aminoacid.rs:32-36
        }
    };
    static const cls_table cls_tab;
    const u8 *cls = cls_tab.v;
    u64 n = 0, rng = rng_seed, bits = 0;
    int nbits = 0;
    for (u64 i = 0; i < len; i++) {
        u8 c = seq[i];
        if (upper && c >= 'a' && c <= 'z') c = (u8)(c - 32); // index.rs:1000
        u8 k = cls[c];
        if (k == 2) { out[n++] = c; break; }                  // aminoacid.rs:79-83
        if (k == 0) {                                         // aminoacid.rs:85-87
            if (err) { err->seq_index = 0; err->position = (u32)(n + 1); err->residue = c; }
            *out_len = n;
            return KS_ERR_INVALID_RESIDUE;
        }
        if (k >= 3) {
            if (nbits == 0) { bits = splitmix64(&rng); nbits = 64; }
            int pick = (int)(bits & 1); bits >>= 1; nbits--;
            static const char *cand[3] = {"DN", "EQ", "IL"};
            c = (u8)cand[k - 3][pick];
        }
        out[n++] = c;
    }
    *out_len = n;
    return KS_OK;
    });
}
