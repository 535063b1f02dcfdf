// ks_translate.hip — six-frame translation of a nucleotide batch on the device, and the translated sketch built on it: the
// protein / dayhoff / hp sketch of DNA that the sourmash / branchwater family makes by translating every record in six frames and
// adding all frames' k-mers to one sketch.  What sourmash's add_sequence does for a protein-type sketch given DNA was restated
// from its documentation, not run: sourmash is not part of the build, and NO PARITY IS CLAIMED (include/kmerseek_amd.h).
//
//   bases     after ASCII upper-casing T = 0, C = 1, A = 2, G = 3, every other byte 4 (invalid).  The complement is code ^ 2.
//   codon     (b1, b2, b3) -> TABLE[16 b1 + 4 b2 + b3], the standard code (NCBI table 1); any invalid base -> 'X'.  '*' and 'X' are
//             residues like any other: nothing is skipped, nothing cuts a frame.
//   frames    record s of L bases becomes sequences 6s + f (forward, the codons of nt[f:]) and 6s + 3 + f (the same on the reverse
//             complement), f = 0, 1, 2, each max(0, (L - f) / 3) residues: one residue buffer + u64 offsets[6n + 1], the batch
//             layout ks_sketch_batch_device reads.  At most 2 L residues per record.
//
//   lengths   k_frame_lens, a lane per record: six u32 lengths, and the offsets checked (0 first, ascending, n_nt last, no record
//             beyond 2^32 - 16 bases: the first bad record comes back with the call's one wait) -> ks_scan_u32_to_u64 -> offsets
//   translate k_translate6, a workgroup per TR_CHUNK bases:
//             1. the chunk's bases and TR_HALO on either side -> 1-byte codes in LDS (four per 32-bit load and LDS store where the
//                input pointer allows)
//             2. for every staged position p the residue of the triple (p, p + 1, p + 2), read forward and read as a codon of the
//                reverse complement (p + 2, p + 1, p complemented) -> two LDS byte arrays.  The 64-byte table sits in LDS.
//             3. a lane per base p of the chunk finds p's record — a binary search over the records the chunk touches, repeated
//                only when p leaves the record of the lane's previous base — and, if the triple at p lies inside the record, owns
//                two output bytes: forward frame (p - a) % 3, index (p - a) / 3; reverse frame t % 3, index t / 3 with
//                t = e - 3 - p counted from the record's END (a, e: the record's bounds).  ONE triple serves both strands: a
//                reverse codon is anchored at its lowest base, so "the codons that start in the chunk" are the same for both.
//             stores: the four residues of an ALIGNED 32-bit word of a frame that lie wholly inside the frame are written as one
//             word by the lane that owns the word's first byte — it reads the other three from LDS, 3 bases apart (9 + 2 bases
//             beyond its own: the halo; the word belongs to the chunk of its first byte's triple).  Bytes of a frame's ragged
//             head and tail are written singly.  Every lane decides this from the destination index alone, so no byte is written
//             twice and none is missed, whatever the chunk boundaries cut.  In a long record 3 of 4 lanes store nothing and the
//             rest store words: 3 runs (forward) + 3 runs (reverse) of consecutive words per wave.
//   Records may be shorter than a codon, hundreds may share a chunk, one may span many; nothing is assumed about alignment of
//   record starts.  All indices that lead to a store are held against the buffer's capacity: offsets that lie cannot make the
//   kernel write outside d_frames.
//
// ks_sketch_translated*: translate into pool scratch -> ks_sketch_device_impl on the 6n frames, unchanged -> ks_union_groups_impl
// with groups of six (the rank path, ks_union.hip) -> a plain ks_sketches of n records.  Scratch: 2 bytes per base + 16, 48 bytes
// per record for the frame offsets, 24 for the lengths; the six-fold sketch; what the union takes (ks_union.hip).
#include "ks_device.h"

#define TR_THREADS 256
#define TR_CHUNK 4096u // bases a workgroup owns
#define TR_HALO 12u    // staged on either side: the last byte of a word lies 9 bases from its first, and a triple is 3 long
#define TR_SPAN (TR_CHUNK + 2 * TR_HALO)
#define TR_MAX_LEN 0xfffffff0ULL
#define TR_BAD_CODE 4u

__device__ const u8 tr_table[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

KS_DEV u32 tr_code(u32 b) {
    b &= 0xdfu; // ASCII upper-casing of the four letters that matter (only 'T' / 't' give 0x54, and so on)
    return b == 'T' ? 0u : b == 'C' ? 1u : b == 'A' ? 2u : b == 'G' ? 3u : TR_BAD_CODE;
}

// six lengths per record; bad[0] = the first record whose offsets are not 0 first, ascending, n_nt last and at most TR_MAX_LEN apart
__global__ __launch_bounds__(256) void k_frame_lens(const u64 *off, u32 n_seqs, u64 n_nt, u32 *lens, unsigned long long *bad) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seqs) return;
    const u64 a = off[s], e = off[s + 1];
    u32 L = 0;
    if (e < a || e > n_nt || e - a > TR_MAX_LEN || (s == 0 && a != 0) || (s == n_seqs - 1 && e != n_nt)) ks_first_bad(bad, 0, s);
    else L = (u32)(e - a);
#pragma unroll
    for (u32 f = 0; f < 3; f++) lens[6 * (u64)s + f] = lens[6 * (u64)s + 3 + f] = L >= f ? (L - f) / 3 : 0u;
}

// `cap`: residues d_frames holds.  foff: the scanned lengths.
__global__ __launch_bounds__(TR_THREADS) void k_translate6(const u8 *nt, const u64 *off, u32 n_seqs, u64 n_nt, const u64 *foff, u8 *frames, u64 cap) {
    __shared__ __attribute__((aligned(16))) u8 s_code[TR_SPAN + 4]; // s_code[i]: the base at c0 - TR_HALO + i
    __shared__ u8 s_fwd[TR_SPAN], s_rev[TR_SPAN];                    // the residue of the triple that begins there
    __shared__ u8 s_tab[64];
    __shared__ u32 s_rec[2];
    const u32 tid = threadIdx.x;
    const u64 c0 = (u64)blockIdx.x * TR_CHUNK;
    const u32 n_own = (u32)(n_nt - c0 < TR_CHUNK ? n_nt - c0 : TR_CHUNK); // bases of this chunk (>= 1: the grid covers n_nt)

    if (tid < 64) s_tab[tid] = tr_table[tid];
    if (tid == 0) { // the records the chunk touches (empty records at its borders do no harm: no base is theirs)
        const u32 lo = ks_last_le_u64(off, 0, n_seqs - 1, c0);
        s_rec[0] = lo;
        s_rec[1] = ks_last_le_u64(off, lo, n_seqs - 1, c0 + n_own - 1);
    }
    // 1. codes.  Position c0 - TR_HALO + i for i in [0, TR_SPAN); c0 and TR_HALO are multiples of 4, so words of the input are
    // words of s_code.  A word is loaded whole when the pointer is aligned and all four bases exist.
    const bool words = ((uintptr_t)nt & 3u) == 0;
    for (u32 w = tid; w < TR_SPAN / 4; w += TR_THREADS) {
        const u64 p = c0 + 4 * (u64)w - TR_HALO; // (wraps below 0 in the first chunk: then p >= n_nt, as for bases past the end)
        u32 packed;
        if (words && p < n_nt && p + 3 < n_nt) {
            const u32 v = *(const u32 *)(nt + p);
            packed = tr_code(v & 255u) | (tr_code((v >> 8) & 255u) << 8) | (tr_code((v >> 16) & 255u) << 16) | (tr_code(v >> 24) << 24);
        } else {
            packed = 0;
#pragma unroll
            for (u32 k = 0; k < 4; k++) {
                const u64 q = p + k;
                packed |= (q < n_nt ? tr_code(nt[q]) : TR_BAD_CODE) << (8 * k);
            }
        }
        *(u32 *)(s_code + 4 * w) = packed;
    }
    if (tid == 0) *(u32 *)(s_code + TR_SPAN) = TR_BAD_CODE * 0x01010101u; // (the triples of the last two staged positions read it)
    __syncthreads();
    // 2. both readings of every staged triple
    for (u32 i = tid; i < TR_SPAN; i += TR_THREADS) {
        const u32 b1 = s_code[i], b2 = s_code[i + 1], b3 = s_code[i + 2];
        const bool ok = (b1 | b2 | b3) < TR_BAD_CODE;
        s_fwd[i] = ok ? s_tab[16 * b1 + 4 * b2 + b3] : (u8)'X';
        s_rev[i] = ok ? s_tab[16 * (b3 ^ 2u) + 4 * (b2 ^ 2u) + (b1 ^ 2u)] : (u8)'X';
    }
    __syncthreads();
    // 3. a lane per base
    const u32 r_lo = s_rec[0], r_hi = s_rec[1];
    u32 s = r_lo;
    u64 a = 1, e = 0, fo[6] = {0, 0, 0, 0, 0, 0}; // (a > e: no record yet)
    for (u32 i = tid; i < n_own; i += TR_THREADS) {
        const u64 p = c0 + i;
        if (p < a || p >= e) {
            s = ks_last_le_u64(off, r_lo, r_hi, p);
            a = off[s]; e = off[s + 1];
#pragma unroll
            for (u32 f = 0; f < 6; f++) fo[f] = foff[6 * (u64)s + f];
        }
        if (p < a || p + 2 >= e || e - a > TR_MAX_LEN) continue; // no triple of the record begins here (or the offsets lie)
        const u32 L = (u32)(e - a), pos = (u32)(p - a), j = TR_HALO + i;
        { // forward: bytes idx .. idx + 3 of the frame are the triples at p, p + 3, p + 6, p + 9
            const u32 f = pos % 3, idx = pos / 3, len = (L - f) / 3;
            const u64 D = (f == 0 ? fo[0] : f == 1 ? fo[1] : fo[2]) + idx;
            const u32 k = (u32)D & 3u;
            if (idx >= k && idx - k + 3 < len) {
                if (k == 0 && D + 4 <= cap)
                    *(u32 *)(frames + D) = (u32)s_fwd[j] | ((u32)s_fwd[j + 3] << 8) | ((u32)s_fwd[j + 6] << 16) | ((u32)s_fwd[j + 9] << 24);
            } else if (D < cap) frames[D] = s_fwd[j];
        }
        { // reverse: counted from the record's end, bytes idx .. idx + 3 are the triples at p, p - 3, p - 6, p - 9
            const u32 t = L - 3 - pos, f = t % 3, idx = t / 3, len = (L - f) / 3;
            const u64 D = (f == 0 ? fo[3] : f == 1 ? fo[4] : fo[5]) + idx;
            const u32 k = (u32)D & 3u;
            if (idx >= k && idx - k + 3 < len) {
                if (k == 0 && D + 4 <= cap)
                    *(u32 *)(frames + D) = (u32)s_rev[j] | ((u32)s_rev[j - 3] << 8) | ((u32)s_rev[j - 6] << 16) | ((u32)s_rev[j - 9] << 24);
            } else if (D < cap) frames[D] = s_rev[j];
        }
    }
}

// d_frames holds `cap` residues, d_foff 6 n_seqs + 1 offsets.  One wait: the residue count and the first bad record come back with it.
static int translate_run(ks_ctx *ctx, const u8 *d_nt, const u64 *d_offs, u32 n_seqs, u64 n_nt, u8 *d_frames, u64 cap, u64 *d_foff, u64 *n_res) {
    *n_res = 0;
    const u64 n6 = 6 * (u64)n_seqs;
    if (n_seqs == 0) {
        if (n_nt) return ks_fail(ctx, KS_ERR_INVALID_ARG, "translate6: %llu bases in a batch of 0 records", (unsigned long long)n_nt);
        KS_HIP(ctx, hipMemsetAsync(d_foff, 0, sizeof(u64), ctx->stream));
        return ks_stream_wait(ctx);
    }
    ks_scratch sc(ctx);
    u32 *lens = nullptr;
    ks_ctl ctl; // word 0: the first record with bad offsets
    KS_TRY(sc.alloc(&lens, (size_t)n6));
    KS_TRY(ctl.init(ctx, sc, KS_PIN_TRANSLATE, 1, 1));
    KS_LAUNCH(ctx, "frame_lens", k_frame_lens, (n_seqs + 255) / 256, 256, d_offs, n_seqs, n_nt, lens, ctl.words());
    KS_TRY(ks_scan_u32_to_u64(ctx, lens, d_foff, n6));
    if (n_nt) {
        const u64 grid = (n_nt + TR_CHUNK - 1) / TR_CHUNK;
        if (grid > 0x7fffffffULL) return ks_fail(ctx, KS_ERR_CAPACITY, "translate6: %llu bases in one batch", (unsigned long long)n_nt);
        KS_LAUNCH(ctx, "translate6", k_translate6, (u32)grid, TR_THREADS, d_nt, d_offs, n_seqs, n_nt, (const u64 *)d_foff, d_frames, cap);
    }
    u64 *const total = ctx->h_pin + KS_PIN_TRANSLATE + 2;
    KS_TRY(ks_stream_wait_fetch_scans(ctx, {ctl.fetch(), ks_fetch_words(d_foff + n6, total, 2)}));
    if (ctl.bad(0))
        return ks_fail(ctx, KS_ERR_INVALID_ARG, "translate6: offsets must start at 0, ascend and end at n_nt, a record holds at most 2^32 - 16 bases (record %llu)",
                       (unsigned long long)ctl[0]);
    if (*total > cap) return ks_fail(ctx, KS_ERR_HIP, "internal error: %llu residues from %llu bases", (unsigned long long)*total, (unsigned long long)n_nt);
    *n_res = *total;
    return KS_OK;
}

// what both entry points refuse before any device work
static int translate_args_check(ks_ctx *ctx, const char *what, const u8 *d_nt, const u64 *d_offs, u32 n_seqs, u64 n_nt) {
    if (!d_offs || (!d_nt && n_nt)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (6 * (u64)n_seqs > 0xffffffffULL) return ks_fail(ctx, KS_ERR_CAPACITY, "%s: the six frames of %u records do not fit 32-bit sequence ids", what, n_seqs);
    if (n_nt > (1ULL << 62)) return ks_fail(ctx, KS_ERR_CAPACITY, "%s: %llu bases in one batch", what, (unsigned long long)n_nt);
    return KS_OK;
}

extern "C" uint64_t ks_translate6_bound(uint64_t n_nt) { return n_nt > (~0ULL >> 1) ? ~0ULL : 2 * n_nt; }
extern "C" uint32_t ks_debug_translate_chunk(void) { return TR_CHUNK; }

extern "C" int ks_translate6_device(ks_ctx *ctx, const uint8_t *d_nt, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_nt, uint8_t *d_frames,
                                    uint64_t *d_frame_offsets, uint64_t *n_residues_out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    if (n_residues_out) *n_residues_out = 0;
    KS_TRY(translate_args_check(ctx, "translate6", d_nt, d_offsets, n_seqs, n_nt));
    if (!d_frame_offsets || !n_residues_out || (!d_frames && n_nt)) return ks_fail(ctx, KS_ERR_INVALID_ARG, "translate6: NULL argument");
    if (((uintptr_t)d_frames & 15) != 0) return ks_fail(ctx, KS_ERR_INVALID_ARG, "translate6: d_frames must be 16-byte aligned");
    KS_HIP(ctx, hipSetDevice(ctx->device));
    return translate_run(ctx, d_nt, d_offsets, n_seqs, n_nt, d_frames, ks_translate6_bound(n_nt), d_frame_offsets, n_residues_out);
    });
}

int ks_sketch_translated_impl(ks_ctx *ctx, const u8 *d_nt, const u64 *d_offs, u32 n_seqs, u64 n_nt, u32 max_seq_len, const ks_params *p,
                              ks_sketches **out) {
    if (!out) return ks_fail(ctx, KS_ERR_INVALID_ARG, "sketch_translated: out is NULL");
    *out = nullptr;
    KS_TRY(ks_check_params(ctx, p));
    KS_TRY(translate_args_check(ctx, "sketch_translated", d_nt, d_offs, n_seqs, n_nt));
    KS_HIP(ctx, hipSetDevice(ctx->device));
    ks_scratch sc(ctx);
    u8 *frames = nullptr;
    u64 *foff = nullptr, n_res = 0;
    const u64 cap = ks_translate6_bound(n_nt);
    KS_TRY(sc.alloc(&frames, (size_t)cap + 16)); // (+ 16: the sketch tiles load whole 16-byte words)
    KS_TRY(sc.alloc(&foff, 6 * (size_t)n_seqs + 1));
    KS_TRY(translate_run(ctx, d_nt, d_offs, n_seqs, n_nt, frames, cap, foff, &n_res));
    // the six-fold sketch lives until the union has read it
    struct six_owner { ks_sketches *s = nullptr; ~six_owner() { ks_sketches_free(s); } } six;
    const u32 frame_bound = max_seq_len ? (max_seq_len / 3 ? max_seq_len / 3 : 1u) : 0u;
    KS_TRY(ks_sketch_device_impl(ctx, frames, foff, 6 * n_seqs, n_res, frame_bound, p, 0, 0, 0, &six.s));
    std::vector<u32> groups((size_t)n_seqs + 1);
    for (u32 s = 0; s <= n_seqs; s++) groups[s] = 6 * s;
    return ks_union_groups_impl(ctx, six.s, groups.data(), n_seqs, out);
}

extern "C" int ks_sketch_translated_device(ks_ctx *ctx, const uint8_t *d_nt, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_nt,
                                           uint32_t max_seq_len, const ks_params *params, ks_sketches **out) {
    return ks_guard(ctx, [&]() -> int {
    if (!ctx) return KS_ERR_INVALID_ARG;
    return ks_sketch_translated_impl(ctx, d_nt, d_offsets, n_seqs, n_nt, max_seq_len, params, out);
    });
}
