/*
 * kmerseek_amd.h — C ABI of the MI355X (gfx950) protein k-mer sketch-and-search engine.
 *
 * This is the drop-in boundary for the one hot path of seanome/kmerseek:
 *   sketch : sliding-window k-mer -> reduced-alphabet re-encode -> MurmurHash3_x64_128.h1 (seed 42)
 *            -> FracMinHash keep-below-threshold -> per-sequence sorted unique hashes + abundances
 *   search : sorted-hash set intersection of every query sketch against an index of target sketches
 *
 * The reference has no FFI seam of its own for this path (sourmash / branchwater are linked-in
 * Rust crates).  Each entry point below names the reference interface it replaces; a Rust
 * `extern "C"` block or a Python ctypes stub binds them 1:1.
 *
 * Conventions
 *   - every function returns a ks_status (0 = ok) unless documented otherwise; nothing throws
 *     or aborts across this boundary — every entry point that can allocate runs its body inside an
 *     exception guard (std::bad_alloc -> KS_ERR_OOM, anything else -> KS_ERR_HIP "internal error");
 *     ks_last_error(ctx) gives the message of the last failure.  Reference convention: every failure
 *     is a value (src/rust/errors.rs:8-24).
 *   - a ks_ctx owns one HIP device + one stream + a grow-only device workspace.  It is NOT
 *     thread-safe: use one context per host thread (the reference's `&self` + rayon fan-out,
 *     src/rust/index.rs:990-1005, becomes one batched call).
 *   - inputs are caller-owned and only read during the call; outputs are library-owned opaque
 *     objects, released with the matching *_free.  All calls are synchronous on return unless
 *     the name ends in _async.
 *   - there is no CPU fallback: without a HIP device ks_ctx_create fails with KS_ERR_NO_DEVICE.
 */
#ifndef KMERSEEK_AMD_H
#define KMERSEEK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KS_ABI_VERSION 1

typedef enum ks_status {
    KS_OK = 0,
    KS_ERR_INVALID_MOLTYPE = 1, /* IndexError::InvalidMoltype, src/rust/errors.rs:8-9; text of encoding.rs:22-25 */
    KS_ERR_INVALID_KSIZE = 2,   /* IndexError::InvalidKsize, src/rust/errors.rs:20-21 */
    KS_ERR_INVALID_RESIDUE = 3, /* IndexError::InvalidAminoAcid(char, pos), src/rust/errors.rs:14-15 */
    KS_ERR_INVALID_ARG = 4,
    KS_ERR_OOM = 5,
    KS_ERR_HIP = 6,
    KS_ERR_NO_DEVICE = 7,
    KS_ERR_CAPACITY = 8,        /* a device-side list (hit pairs) outgrew its hard cap */
    KS_ERR_INVALID_SCALED = 9
} ks_status;

/* get_hash_function_from_moltype / get_encoding_fn_from_moltype, src/rust/encoding.rs:17-53;
 * PyProteinEncoding Raw/Dayhoff/HP, src/rust/lib.rs:29-65. */
typedef enum ks_moltype { KS_PROTEIN = 0, KS_DAYHOFF = 1, KS_HP = 2 } ks_moltype;

#define KS_SEED_DEFAULT 42ull /* pub const SEED, src/rust/signature.rs:12 */
#define KS_MAX_KSIZE 128u

/* KmerMinHash::new(scaled, 3*ksize, hashfn, seed, track_abundance=true, num=0),
 * src/rust/signature.rs:120-131.  ksize is the PROTEIN k (the sourmash ksize is 3*ksize). */
typedef struct ks_params {
    uint32_t ksize;   /* 1..KS_MAX_KSIZE */
    uint32_t scaled;  /* >= 1; max_hash as ks_max_hash() */
    uint32_t moltype; /* ks_moltype */
    uint32_t flags;   /* reserved, 0 */
    uint64_t seed;    /* KS_SEED_DEFAULT */
} ks_params;

typedef struct ks_ctx ks_ctx;
typedef struct ks_sketches ks_sketches; /* device-resident CSR: offsets[n+1], hashes u64, abund u32 */
typedef struct ks_index ks_index;       /* device-resident inverted index: postings sorted by hash */
typedef struct ks_hits ks_hits;         /* device-resident COO (qid, tid, intersect, n_weighted) */
typedef struct ks_kmerpos ks_kmerpos;   /* device-resident (seq, start, hash) triples */
typedef struct ks_matchpos ks_matchpos; /* device-resident CSR over hit rows: (query start, target start) of shared k-mers */
typedef struct ks_regions ks_regions;   /* device-resident CSR over hit rows: the colinear regions those pairs chain into */
typedef struct ks_raligns ks_raligns;   /* device-resident CSR over hit rows: those regions aligned with gaps (banded affine X-drop) */
typedef struct ks_cigars ks_cigars;     /* device-resident CSR over regions: the path of each alignment as BAM-encoded CIGAR ops */
typedef struct ks_rscores ks_rscores;   /* device-resident CSR over hit rows: those regions scored and extended (ungapped X-drop) */

/* ---- library / context ------------------------------------------------------------------ */

uint32_t ks_abi_version(void);
const char *ks_status_string(int status);

/* "protein" | "raw" | "hp" | "dayhoff" -> ks_moltype (src/rust/encoding.rs:17-27).
 * Returns KS_ERR_INVALID_MOLTYPE for anything else. */
int ks_moltype_from_string(const char *name, uint32_t *moltype_out);

/* sourmash max_hash_for_scaled as used by KmerMinHash::new (src/rust/signature.rs:124-131). */
uint64_t ks_max_hash(uint32_t scaled);

/* hip_stream: a hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream), or NULL
 * to let the context create its own non-blocking stream.  The device's default (null) stream cannot be named by NULL here:
 * pass hipStreamLegacy ((hipStream_t)1) for it — kmerseek_amd/engine.py does that for a caller that hands over the 0
 * torch reports for its default stream. */
int ks_ctx_create(int device, void *hip_stream, ks_ctx **out);
void ks_ctx_destroy(ks_ctx *ctx);
const char *ks_last_error(const ks_ctx *ctx);
void *ks_ctx_stream(const ks_ctx *ctx); /* the hipStream_t all kernels are launched on */
int ks_ctx_synchronize(ks_ctx *ctx);
/* device workspace pool: blocks held, bytes held / in use, hipMalloc calls so far (0 new ones in steady state) */
int ks_ctx_pool_stats(const ks_ctx *ctx, uint64_t *n_blocks, uint64_t *bytes_held, uint64_t *bytes_in_use,
                      uint64_t *n_mallocs);

/* How often this context had to repeat a sketch batch (results are identical either way; a repeat only costs time):
 * out[0] = launches repeated because a tile look-back gave up waiting (dispatch order was not blockIdx order; the context
 *          then takes tile ids from an atomic ticket for good: out[1] = 1),
 * out[2] = batches repeated with plain tiles because a compacting tile (scaled > 1) kept more hashes than its LDS lists take,
 * out[3] = batches repeated with window-count sized outputs because they kept more hashes than the expected 1/scaled,
 * out[4] = shared-tile launches whose tiles took the start of their CSR slots from the tile plan instead of a look-back across
 *          tiles (scaled = 1, packed tiles: a sequence's slot is as long as its k-mer windows; a path, not a repeat). */
int ks_ctx_sketch_stats(const ks_ctx *ctx, uint64_t out[5]); /* (five words — four before out[4] was added: size the array) */
/* The same for ks_search: out[0] = searches that ran their join twice because the match list outgrew its first guess
 * (the list is sized from the previous search of the context), out[1] = searches whose row pass was repeated with
 * ticket-ordered tiles because a look-back gave up (the context then uses tickets for good), out[2] = searches whose rows
 * came from the aggregate pass over the match sort's first level (taken while the previous search of the context had many
 * matches per row; a path, not a repeat), out[3] = searches in which that pass gave up (a region with more rows than its
 * table holds) and the sort was resumed, out[4] = searches whose join ran the table kernel (taken while the join buckets are
 * expected to hold few query postings — behind a filtered partition: few survivors, by the previous filtered search of the
 * context; a path, not a repeat). */
int ks_ctx_search_stats(const ks_ctx *ctx, uint64_t out[5]); /* (five words — four before out[4] was added: size the array) */
/* ks_sketch_search_device on this context: out[0] = calls whose sketch read-back was folded into the search's first wait,
 * out[1] = calls that had to be repeated with the two plain calls (skewed hashes, an economy that did not fit), out[2] = calls
 * whose rows came from the aggregate pass (out[2] of ks_ctx_search_stats rose during the call), out[3] = calls whose join ran
 * the table kernel (out[4] of ks_ctx_search_stats rose). */
int ks_ctx_fused_stats(const ks_ctx *ctx, uint64_t out[4]); /* (four words — three before out[3] was added) */
/* The presence filter of the searches on this context (a fingerprint-layout index carries a two-bit filter over hash prefixes; the
 * partition of the query postings drops those the bitmap rules out): out[0] = query postings the filtered partitions read,
 * out[1] = postings they dropped.  Results never depend on the filter; KS_DEBUG_QFILTER = 0 / 1 forces it off / on. */
int ks_ctx_qfilter_stats(const ks_ctx *ctx, uint64_t out[2]);
/* Diagnostics: the KS_DEBUG_* environment variables (they force the rarely taken paths in the tests; results never
 * depend on them) are read once, when the context is created — never on the per-call path.  This reads them again. */
int ks_ctx_reload_debug_env(ks_ctx *ctx);
/* Self-test of the exception guard, callable without a device: a body that throws `what` ("bad_alloc", "runtime", "other";
 * anything else throws nothing) runs behind the guard; returns the status that came out of it. */
int ks_debug_guard_selftest(const char *what);

/* Plain device buffers for callers that have no HIP binding of their own (the *_device entry points take raw
 * device pointers): 256-byte aligned allocations on ctx's device, stream-ordered copies that return when done. */
int ks_dev_malloc(ks_ctx *ctx, uint64_t bytes, void **out);
int ks_dev_free(ks_ctx *ctx, void *ptr);
int ks_dev_upload(ks_ctx *ctx, void *dst_device, const void *src_host, uint64_t bytes);
int ks_dev_download(ks_ctx *ctx, void *dst_host, const void *src_device, uint64_t bytes);

/* Pinned (page-locked) host memory.  Host buffers handed to this library are copied in one DMA at link rate when they are
 * pinned (ks_host_alloc, hipHostMalloc, hipHostRegister); pageable ones go through the context's double-buffered pinned
 * staging with a few host copy threads.  Callers that want sketches / k-mer tables back should receive them in pinned arrays. */
int ks_host_alloc(ks_ctx *ctx, uint64_t bytes, void **out);
int ks_host_free(ks_ctx *ctx, void *ptr);

/* ---- host-side pre-step ------------------------------------------------------------------ */

typedef struct ks_residue_error {
    uint32_t seq_index; /* index of the offending record in the batch */
    uint32_t position;  /* 1-based, in the OUTPUT so far (src/rust/aminoacid.rs:86) */
    uint8_t residue;
} ks_residue_error;

/* AminoAcidAmbiguity::validate_and_resolve (src/rust/aminoacid.rs:74-105) on one record:
 * accepts the 20 standard residues + X U O * + B Z J; truncates after the first '*' (inclusive);
 * B->D|N, Z->E|Q, J->I|L chosen by a SplitMix64 stream seeded with rng_seed (the reference draws
 * from rand::rng(), aminoacid.rs:48 — non-reproducible by construction).
 * upper != 0 first upper-cases ASCII (the FASTA path, src/rust/index.rs:1000).
 * out must hold len bytes.  Returns KS_OK or KS_ERR_INVALID_RESIDUE (err filled, seq_index = 0). */
int ks_validate_and_resolve(const uint8_t *seq, uint64_t len, int upper, uint64_t rng_seed,
                            uint8_t *out, uint64_t *out_len, ks_residue_error *err);

/* ---- sketch ------------------------------------------------------------------------------- */

/* Replaces the rayon loop of process_batch_parallel (src/rust/index.rs:984-1016) around
 * ProteinSignature::add_protein -> sourmash KmerMinHash::add_protein (src/rust/signature.rs:273-282),
 * and branchwater do_manysketch(singleton=True) (src/python/kmerseek/sketch.py:33-39).
 *
 * residues   : n_seqs sequences concatenated, 1 byte per residue (ASCII), HOST memory
 * seq_offsets: n_seqs+1 ascending byte offsets into residues, HOST memory
 * Residues are hashed as given after ASCII upper-casing (what sourmash does internally); run
 * ks_validate_and_resolve first for the Rust-path semantics.
 * Result: per sequence, ascending unique hashes h with 0 < h <= max_hash and abund = number of
 * windows of that sequence hashing to h. */
int ks_sketch_batch(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets,
                    uint32_t n_seqs, const ks_params *params, ks_sketches **out);

/* Same, with residues / seq_offsets already resident in device memory (HBM) on ctx's device.
 * n_residues = seq_offsets[n_seqs].  max_seq_len: an upper bound on the longest sequence of the batch, or 0.
 * With a bound the launches are planned on the host and the call synchronises once, at its end; with 0 the
 * library measures the batch first (one more device->host round trip, and a tile stride fitted to the batch).
 * A bound smaller than the longest sequence is detected and fails with KS_ERR_INVALID_ARG (no output). */
int ks_sketch_batch_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets,
                           uint32_t n_seqs, uint64_t n_residues, uint32_t max_seq_len,
                           const ks_params *params, ks_sketches **out);

/* Sketch a QUERY batch that is about to be searched against `index` (sketch parameters are the index's).  Same result
 * as ks_sketch_batch_device; in addition the sketch kernel writes the batch's postings already partitioned on the hash
 * bits the join against this index consumes, so the following ks_search skips its first partition pass (the sketch
 * kernel is ALU-bound: the extra writes ride on idle memory pipes).  If the hashes are too skewed for the fixed-size
 * regions the postings are dropped and ks_search partitions as usual — results are identical either way. */
int ks_sketch_queries_device(ks_ctx *ctx, const ks_index *index, const uint8_t *d_residues,
                             const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                             uint32_t max_seq_len, ks_sketches **out);

/* ks_sketch_queries_device + ks_search in ONE call, for callers that sketch a batch only to search it — what the
 * reference does per query file (src/python/kmerseek/search.py:125-141 after sketch.py:28-40; batches of 1000 records in
 * src/rust/main.rs:130).  Same sketches, same hits as the two calls; the host waits for the device twice instead of three
 * times (the wait at the end of the sketch is folded into the search's first one: ~25 us per call, which is what a small
 * batch or a 1/8 query shard notices).  *sketches_out may be NULL: the sketches are then freed before returning. */
int ks_sketch_search_device(ks_ctx *ctx, const ks_index *index, const uint8_t *d_residues,
                            const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                            uint32_t max_seq_len, ks_sketches **sketches_out, ks_hits **hits_out);
/* The same from host arrays (the layout ks_sketch_batch takes): upload, sketch, search. */
int ks_sketch_search(ks_ctx *ctx, const ks_index *index, const uint8_t *residues, const uint64_t *seq_offsets,
                     uint32_t n_seqs, ks_sketches **sketches_out, ks_hits **hits_out);

uint32_t ks_sketches_n_seqs(const ks_sketches *s);
uint64_t ks_sketches_n_hashes(const ks_sketches *s);
uint64_t ks_sketches_n_windows(const ks_sketches *s); /* k-mer windows hashed to build it */
/* != 0 if ks_sketch_queries_device's partitioned postings are attached: 1 = 12-byte postings (hash, sequence id),
 * 2 = 10-byte postings (the fingerprint join of big indexes at scaled = 1: 8 hash bits are implied by the region) */
int ks_sketches_has_postings(const ks_sketches *s);
void ks_sketches_params(const ks_sketches *s, ks_params *out);
/* device pointers (valid until ks_sketches_free): offsets u64[n+1], hashes u64[], abund u32[] — the plain CSR.  (Inside the
 * library a fresh batch is a CSR of slots: a sequence that repeats a k-mer leaves a gap behind its distinct hashes.  The first
 * of these calls — like ks_sketches_copy_to_host, ks_index_build, ks_sketches_union — closes the gaps of such a batch with one
 * gather on the context's stream and waits for it; a batch without repeats is a plain CSR as it stands.  NULL with the reason
 * in ks_last_error if that pass fails.) */
const uint64_t *ks_sketches_device_offsets(const ks_sketches *s);
const uint64_t *ks_sketches_device_hashes(const ks_sketches *s);
const uint32_t *ks_sketches_device_abunds(const ks_sketches *s);
/* any of the three host pointers may be NULL */
int ks_sketches_copy_to_host(ks_ctx *ctx, const ks_sketches *s, uint64_t *offsets,
                             uint64_t *hashes, uint32_t *abunds);
/* upload an existing CSR (e.g. sketches loaded from a .sig.zip) so it can be indexed / searched */
int ks_sketches_from_host(ks_ctx *ctx, const uint64_t *offsets, const uint64_t *hashes,
                          const uint32_t *abunds, uint32_t n_seqs, const ks_params *params,
                          ks_sketches **out);
/* Union of all sequences' sketches with abundances summed per hash, returned as ONE sequence: the
 * "combined minhash" that ProteomeIndex::store_signatures maintains (src/rust/index.rs:800-830,
 * add_many_with_abund under a mutex there).  Abundance sums saturate at 2^32-1. */
int ks_sketches_union(ks_ctx *ctx, const ks_sketches *in, ks_sketches **out);
void ks_sketches_free(ks_sketches *s);

/* ---- translated search: nucleotide input for the protein / dayhoff / hp sketches ---------------------------------------- */

/* Six-frame translation of a nucleotide batch on the device: what lets contigs, reads and unannotated genomes be searched
 * against a protein database.  The sourmash / branchwater family does this inside add_sequence for a protein-type sketch given
 * DNA; sourmash is not part of this build, the semantics below were restated from its documentation and NO PARITY IS CLAIMED.
 * For a record of L bases, taken as bytes after ASCII upper-casing:
 *   base codes  T = 0, C = 1, A = 2, G = 3; every other byte is invalid (N, U, the IUPAC codes and gaps included)
 *   codon       (b1, b2, b3) -> TABLE[16 b1 + 4 b2 + b3], TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
 *               (the standard code, NCBI table 1); a codon with an invalid base gives 'X'.  '*' and 'X' are residues like any
 *               other: they are not skipped and do not cut the frame (the sketch hashes whatever byte it is given).
 *   reverse     rc[i] = comp(nt[L - 1 - i]), A <-> T, C <-> G, any other byte maps to itself
 *   frames      forward frame f in {0, 1, 2}: the codons of nt[f:], max(0, (L - f) / 3) residues, a trailing partial codon
 *               dropped; reverse frame f: the same on rc[f:]
 * Record s becomes the six sequences 6 s + f (forward) and 6 s + 3 + f (reverse) of ONE contiguous residue buffer with u64
 * offsets [6 n_seqs + 1] — the batch layout ks_sketch_batch_device, ks_kmer_positions_device and ks_sketch_queries_device read.
 * A window that starts at `start` of forward frame f covers the bases from f + 3 start on, one of reverse frame f the bases from
 * L - f - 3 (start + ksize) on.  d_nt / d_offsets: device, n_seqs + 1 ascending offsets from 0 to n_nt.
 * KS_ERR_INVALID_ARG: NULL arguments, d_frames not 16-byte aligned (both before any device work); offsets that do not start at
 * 0, ascend and end at n_nt, or a record beyond 2^32 - 16 bases (found on the device: the output is then incomplete, nothing is
 * written outside it).  KS_ERR_CAPACITY: 6 n_seqs does not fit a u32.  One stream, one wait, synchronous on return. */
uint64_t ks_translate6_bound(uint64_t n_nt);          /* residues the frames of n_nt bases can need: 2 * n_nt */
int ks_translate6_device(ks_ctx *ctx, const uint8_t *d_nt, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_nt,
                         uint8_t *d_frames /* caller-owned, >= bound, 16-byte aligned */,
                         uint64_t *d_frame_offsets /* caller-owned, 6 * n_seqs + 1 */, uint64_t *n_residues_out);
/* The translated sketch: record s's sketch is the union of its six frame sketches at `params` (ksize stays the PROTEIN k), the
 * abundances of a hash summed over the frames and saturating at 2^32 - 1 as in ks_sketches_union.  A record shorter than
 * 3 * ksize bases has an empty sketch; a palindromic record counts each window twice.  The result is a plain ks_sketches:
 * n_seqs records, n_windows the sum over the frames, no postings attached — ks_search, ks_index_build, the hit-list passes and
 * ks_corpus_build take it unchanged.  max_seq_len: an upper bound on the longest record IN BASES, or 0 to have the batch
 * measured; the frames are sketched under the bound max_seq_len / 3, and one that is too small fails as it does in
 * ks_sketch_batch_device.  Parameters, NULL arguments and the u32 range of 6 n_seqs are checked before any device work.  The
 * frames and the six-fold sketch live in the context's pool and are given back before the call returns. */
int ks_sketch_translated_device(ks_ctx *ctx, const uint8_t *d_nt, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_nt,
                                uint32_t max_seq_len /* in bases, 0 = measure */, const ks_params *params, ks_sketches **out);
/* the same from host arrays (the layout ks_sketch_batch takes, with bases for residues) */
int ks_sketch_translated(ks_ctx *ctx, const uint8_t *nt, const uint64_t *offsets, uint32_t n_seqs, const ks_params *params,
                         ks_sketches **out);
/* Union by group: sketch g of the result is the ascending distinct hashes of the sketches [group_offsets[g], group_offsets[g + 1])
 * of `in`, abundances summed per hash and saturating at 2^32 - 1 — ks_sketches_union folds a whole set into one sketch, this
 * folds consecutive runs: the six frames of a record, or all proteins of a genome into the proteome-sized query ks_hits_gather
 * has a path for.  group_offsets: HOST, n_groups + 1 entries, 0 first, the set's sequence count last, never descending.  The
 * result is a dense CSR of n_groups sketches with the input's params and n_windows; an empty group gives an empty sketch, a
 * group of one a copy, n_groups == 0 (on an empty set) a valid empty set.  Groups of at most ks_debug_union_rank_max() members
 * are merged by binary-search ranks in one kernel, larger ones by two stable radix sorts; the result never depends on the path
 * (KS_DEBUG_UNION_PATH = 1 / 2 force the rank / the sort path for the tests).
 * KS_ERR_INVALID_ARG (before any device work): NULL arguments, an input of another context, group_offsets that do not start at
 * 0, end at the sequence count and ascend.  KS_ERR_CAPACITY: 2^32 - 2 or more hashes.  One stream, one wait; scratch from the
 * pool: 32 bytes per input hash on the rank path, 56 on the sort path. */
int ks_sketches_union_groups(ks_ctx *ctx, const ks_sketches *in, const uint32_t *group_offsets, uint32_t n_groups, ks_sketches **out);
uint32_t ks_debug_translate_chunk(void);   /* bases one workgroup of the translate kernel owns: the tests put record ends around it */
uint32_t ks_debug_union_rank_max(void);    /* largest group the rank path takes */

/* ---- low-complexity masking: mask, split and the masked sketch ---------------------------------------------------------- */

/* A low-complexity filter applied before sketching, as the search tools of the BLAST family apply SEG.  The rule is THIS
 * LIBRARY'S OWN, defined in integers: the first stage of SEG (trigger windows, extension over contiguous windows) without the
 * second-stage trimming.  NCBI seg is not part of this build and NO PARITY IS CLAIMED.
 *   classes     a residue's class is its letter without case (26), '*' (1) or "any other byte" (1): 28 classes.  X and * are
 *               classes like any other.
 *   window      W residues.  T[c] = floor(c log2(c) 65536 + 0.5), T[0] = 0 (a committed table).  The window of record r that
 *               starts at p is valid iff p + W <= end(r); its complexity is e(p) = T[W] - sum over classes of T[count], W * 65536
 *               times its Shannon entropy in bits.
 *   thresholds  in millibits: lo1(p) iff e(p) <= floor(k1 W 65536 / 1000) (the trigger), lo2(p) likewise with k2 >= k1 (the
 *               extension).  Invalid windows are neither.
 *   hysteresis  a run is a maximal stretch of consecutive window starts with lo2 (it cannot cross a record: the last W - 1
 *               starts of a record are invalid); it is hot iff it holds a lo1 window.  A hot run [i, j) masks the residues
 *               [i, j - 1 + W).  Nothing else is masked.
 *   segments    of a record: its maximal stretches of unmasked residues of at least min_len residues, in order; possibly none.
 * Everything is integer arithmetic: the result does not depend on the launch geometry.
 * ks_mask_opts: window 0 means 12; window, k1 and k2 ALL 0 (and opts == NULL) mean the defaults 12 / 2200 / 2500; otherwise k1
 * and k2 are taken as given (k1 = k2 = 0 masks exactly the windows of one class).  KS_ERR_INVALID_ARG, before any device work:
 * window outside [2, KS_MASK_MAX_WINDOW], k2 < k1, NULL arguments; found on the device and named in the message: offsets that do
 * not start at 0, ascend and end at n_residues, a record beyond 2^32 - 16 residues.  KS_ERR_CAPACITY: 2^32 - 64 or more
 * residues in one batch.  One stream, one wait per call, synchronous on return. */
#define KS_MASK_MAX_WINDOW 32
typedef struct ks_mask_opts { uint32_t window, k1_millibits, k2_millibits; } ks_mask_opts;
typedef struct ks_mask ks_mask;
typedef struct ks_segments ks_segments;
int ks_mask_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                   const ks_mask_opts *opts, ks_mask **out);
/* the same from host arrays (the layout ks_sketch_batch takes) */
int ks_mask_batch(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs, const ks_mask_opts *opts,
                  ks_mask **out);
uint32_t ks_mask_n_seqs(const ks_mask *m);
uint64_t ks_mask_n_residues(const ks_mask *m);
uint64_t ks_mask_n_masked(const ks_mask *m);
const uint8_t *ks_mask_device_mask(const ks_mask *m);            /* n_residues bytes, 1 = masked */
const uint32_t *ks_mask_device_masked_counts(const ks_mask *m);  /* n_seqs */
int ks_mask_copy_to_host(ks_ctx *ctx, const ks_mask *m, uint8_t *mask, uint32_t *masked_counts); /* either may be NULL */
void ks_mask_free(ks_mask *m);
/* The segments of a batch under a mask made from it (same n_seqs and n_residues, or KS_ERR_INVALID_ARG): seg_record and
 * seg_start (relative to the record) per segment, the segments' residues as one compacted buffer with u64 offsets — the batch
 * layout every *_device sketch entry reads, 16-byte aligned — and per record the range of its segments.  min_len 0 counts as 1. */
int ks_mask_split_device(ks_ctx *ctx, const ks_mask *mask, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs,
                         uint64_t n_residues, uint32_t min_len, ks_segments **out);
uint64_t ks_segments_n_segs(const ks_segments *s);
uint64_t ks_segments_n_residues(const ks_segments *s);
uint32_t ks_segments_n_records(const ks_segments *s);
const uint32_t *ks_segments_device_seg_record(const ks_segments *s);
const uint32_t *ks_segments_device_seg_start(const ks_segments *s);
const uint64_t *ks_segments_device_seg_offsets(const ks_segments *s);   /* n_segs + 1 */
const uint8_t *ks_segments_device_residues(const ks_segments *s);
const uint32_t *ks_segments_device_group_offsets(const ks_segments *s); /* n_records + 1 */
int ks_segments_copy_to_host(ks_ctx *ctx, const ks_segments *s, uint32_t *seg_record, uint32_t *seg_start, uint64_t *seg_offsets,
                             uint8_t *residues, uint32_t *group_offsets);
void ks_segments_free(ks_segments *s);
/* The masked sketch: the hashes of exactly those windows of a record that contain no masked residue, abundances counted over
 * those windows — mask, split at min_len = ksize, ks_sketch_batch_device on the segments, ks_sketches_union_groups by record.
 * The result is a plain ks_sketches of n_seqs records; n_windows is the sum over the segments; a record without a segment has
 * an empty sketch.  Records with more than ks_debug_union_rank_max() segments send the batch's union down its sort path.
 * max_seq_len as in ks_sketch_batch_device.  All scratch goes back to the context's pool before the call returns. */
int ks_sketch_masked_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs, uint64_t n_residues,
                            uint32_t max_seq_len, const ks_params *params, const ks_mask_opts *opts, ks_sketches **out);
int ks_sketch_masked(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets, uint32_t n_seqs, const ks_params *params,
                     const ks_mask_opts *opts, ks_sketches **out);
/* ks_kmer_positions_device on the segments, every triple carried back to its record: seq = the segment's record, start counted
 * from the record's first residue, ordered by (seq, start) — the table that agrees with a masked sketch in ks_match_positions. */
int ks_kmer_positions_masked_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs,
                                    uint64_t n_residues, const ks_params *params, const ks_mask_opts *opts, ks_kmerpos **out);
uint32_t ks_debug_mask_chunk(void);        /* residues one workgroup of the mask kernels owns: the tests put runs around it */

/* ---- k-mer positions ----------------------------------------------------------------------- */

/* Replaces ProteomeIndex::process_kmers (src/rust/index.rs:749-786): for every window whose hash
 * is in the sequence's sketch emit (seq, start, hash), ordered by (seq, start).  With the
 * FracMinHash rule "in the sketch" == "0 < h <= max_hash", so no membership scan is needed.
 * The host groups triples into KmerInfo{encoded_kmer, original_kmer -> [positions]} (src/rust/kmer.rs:6-12). */
int ks_kmer_positions(ks_ctx *ctx, const uint8_t *residues, const uint64_t *seq_offsets,
                      uint32_t n_seqs, const ks_params *params, ks_kmerpos **out);
/* Same, with the batch already resident in device memory (d_residues 16-byte aligned, n_residues = seq_offsets[n_seqs]). */
int ks_kmer_positions_device(ks_ctx *ctx, const uint8_t *d_residues, const uint64_t *d_seq_offsets, uint32_t n_seqs,
                             uint64_t n_residues, const ks_params *params, ks_kmerpos **out);
uint64_t ks_kmerpos_count(const ks_kmerpos *p);
void ks_kmerpos_params(const ks_kmerpos *p, ks_params *out); /* the parameters the table was made with */
int ks_kmerpos_copy_to_host(ks_ctx *ctx, const ks_kmerpos *p, uint32_t *seq, uint32_t *start,
                            uint64_t *hash);
void ks_kmerpos_free(ks_kmerpos *p);

/* ---- index + search ------------------------------------------------------------------------ */

/* Builds the inverted index over target sketches: postings (hash, tid, abund) sorted by hash.
 * Stands where `kmerseek index` / do_index builds its search structure (src/python/kmerseek/index.py:55-74);
 * the targets' per-sequence sizes and abundance totals are kept for the ratio columns. */
int ks_index_build(ks_ctx *ctx, const ks_sketches *targets, ks_index **out);
uint32_t ks_index_n_targets(const ks_index *ix);
uint64_t ks_index_n_postings(const ks_index *ix);
void ks_index_free(ks_index *ix);

/* Replaces branchwater do_manysearch(threshold=0, output_all=False) (src/python/kmerseek/search.py:125-141):
 * for every (query, target) pair with at least one shared hash emits
 *   qid, tid, intersect = |mins_q ∩ mins_t|, n_weighted = Σ target abundance over the shared hashes,
 * sorted by (qid, tid).  Pair results are identical to a pairwise sorted merge of the sketches. */
int ks_search(ks_ctx *ctx, const ks_index *index, const ks_sketches *queries, ks_hits **out);
uint64_t ks_hits_count(const ks_hits *h);
uint64_t ks_hits_n_pair_instances(const ks_hits *h); /* Σ_h q(h)·t(h): matched (posting, posting) pairs */
/* how the query postings were grouped for the join (results are identical on every path):
 * 0 the sketch kernel's regions were the buckets; 1 regions + one histogram-free bucket scatter;
 * 2 regions + one dense radix pass (a bucket overflowed); 3 dense radix partition from the CSR (no postings attached) */
int ks_hits_partition_path(const ks_hits *h);
/* Bytes per query posting inside the join buckets of the search that produced h: 12 (hash u64 + sequence id u32), 10 (the
 * sketch kernel's 10-byte form kept through the bucket scatter), 9 (join prefixes of 16 bits: the bucket implies two hash bytes
 * and carries two bytes of the sequence id there), 0 (the search ran without the histogram-free bucket scatter).  Diagnostic. */
int ks_hits_bucket_posting_bytes(const ks_hits *h);
int ks_hits_copy_to_host(ks_ctx *ctx, const ks_hits *h, uint32_t *qid, uint32_t *tid,
                         uint32_t *intersect, uint64_t *n_weighted);
/* Device-resident COO columns (valid until ks_hits_free; ks_hits_count entries each) — what a multi-GPU caller hands to
 * RCCL without a host round trip (hit lists of shards are disjoint and only concatenated). */
const uint32_t *ks_hits_device_qid(const ks_hits *h);
const uint32_t *ks_hits_device_tid(const ks_hits *h);
const uint32_t *ks_hits_device_intersect(const ks_hits *h);
const uint64_t *ks_hits_device_n_weighted(const ks_hits *h);
/* Device-to-device copy of the columns into caller-owned device buffers (e.g. the send block of an all-gather), with
 * qid_base / tid_base added to the ids (a shard's local numbering -> global).  Asynchronous on ctx's stream; any
 * destination may be NULL. */
int ks_hits_copy_to_device(ks_ctx *ctx, const ks_hits *h, uint32_t qid_base, uint32_t tid_base, uint32_t *d_qid,
                           uint32_t *d_tid, uint32_t *d_intersect, uint64_t *d_n_weighted);
/* Transport form of the rows for a multi-GPU exchange: one 64-bit word per row,
 *     qid << (tbits + 2v) | tid << 2v | intersect << v | n_weighted,   v = (64 - qbits - tbits) / 2,
 * ids in global numbering (qid_base / tid_base added; qbits / tbits = bits of the GLOBAL id ranges, qbits + tbits <= 48).
 * A row whose intersect or n_weighted needs more than v bits carries all-ones in both value fields and is appended to the
 * escape list (row index, intersect, n_weighted; *d_n_esc counts them, also past esc_cap — the caller sizes a repeat).
 * 8 bytes per row instead of 20 over xGMI.  Asynchronous on ctx's stream; *d_n_esc must be zero on entry. */
int ks_hits_pack64_to_device(ks_ctx *ctx, const ks_hits *h, uint32_t qid_base, uint32_t tid_base, int qbits, int tbits,
                             uint64_t *d_packed, uint32_t *d_esc_row, uint32_t *d_esc_intersect, uint64_t *d_esc_n_weighted,
                             uint32_t *d_n_esc, uint32_t esc_cap);
/* The receiving side: n transport words (device) -> the four columns (device, caller-owned).  Escaped rows come out with
 * all-ones in both value fields; the caller patches them from the gathered escape lists.  Asynchronous on ctx's stream. */
int ks_hits_unpack64_device(ks_ctx *ctx, const uint64_t *d_packed, uint64_t n, int qbits, int tbits, uint32_t *d_qid,
                            uint32_t *d_tid, uint32_t *d_intersect, uint64_t *d_n_weighted);
/* Index-sharded exchange, global (qid, tid) order: the gathered rows are n_blocks rank blocks (block r = block_rows[r] rows,
 * host array), each ordered by (qid, tid), the ranks' target ranges ascending.  One counting merge (per (query, rank) run
 * lengths by binary search -> exclusive scan -> one move) writes them ordered by (qid, tid) into the caller-owned output
 * columns (device, sum(block_rows) entries; must not alias the inputs).  qid values must be < n_queries: a row that is not
 * has no place in the merged order, and the call fails with KS_ERR_INVALID_ARG (outputs then incomplete) instead of leaving a
 * gap.  Returns after the move has run (one wait on ctx's stream: the count of such rows comes back with it).
 * (Rows per query as branchwater manysearch lists them: src/python/kmerseek/search.py:125-141.) */
int ks_hits_merge_by_qid_device(ks_ctx *ctx, const uint32_t *d_qid, const uint32_t *d_tid, const uint32_t *d_intersect,
                                const uint64_t *d_n_weighted, const uint64_t *block_rows, uint32_t n_blocks, uint32_t n_queries,
                                uint32_t *d_out_qid, uint32_t *d_out_tid, uint32_t *d_out_intersect, uint64_t *d_out_n_weighted);
void ks_hits_free(ks_hits *h);

/* ---- search options (opt-in; the entries above are these with opts == NULL) --------------------------------------------- */

/* Per row, the statistics of the target abundances of the shared hashes that the manysearch columns average_abund /
 * median_abund / std_abund need (src/python/kmerseek/search.py:125-141): with it the match records of a row are sorted by
 * abundance too, and one pass over them computes
 *   median2 = 2 x the median (exact: the middle value doubled for an odd count, the sum of the two middle values otherwise),
 *   ss      = the sum of (a - mean)^2 over the row in f64, with sum += a, mean = sum / n, ss += (a - mean) * (a - mean)
 *             evaluated in that order over the ascending abundances (no contraction into fma): bit-identical to a host
 *             loop that does the same.  std = sqrt(ss / n) and mean = n_weighted / n stay with the caller. */
#define KS_SEARCH_ABUND_STATS 1u
typedef struct ks_search_opts {
    uint32_t flags;         /* KS_SEARCH_* */
    uint32_t reserved;      /* 0 */
    double min_containment; /* keep a row iff (double)intersect / (double)|q| >= this (|q| = the query's distinct hashes);
                               0 keeps every row.  Negative or NaN: KS_ERR_INVALID_ARG.  Kept rows stay in (qid, tid) order. */
} ks_search_opts;
/* ks_search / ks_sketch_search_device / ks_sketch_search with options.  opts == NULL or all zero: exactly the plain call.
 * Options are checked before any device work. */
int ks_search_ex(ks_ctx *ctx, const ks_index *index, const ks_sketches *queries, const ks_search_opts *opts, ks_hits **out);
int ks_sketch_search_device_ex(ks_ctx *ctx, const ks_index *index, const uint8_t *d_residues, const uint64_t *d_seq_offsets,
                               uint32_t n_seqs, uint64_t n_residues, uint32_t max_seq_len, const ks_search_opts *opts,
                               ks_sketches **sketches_out, ks_hits **hits_out);
int ks_sketch_search_ex(ks_ctx *ctx, const ks_index *index, const uint8_t *residues, const uint64_t *seq_offsets,
                        uint32_t n_seqs, const ks_search_opts *opts, ks_sketches **sketches_out, ks_hits **hits_out);
/* 1 if h was produced with KS_SEARCH_ABUND_STATS (the two columns below exist), else 0 */
int ks_hits_has_abund_stats(const ks_hits *h);
/* device columns (ks_hits_count entries, valid until ks_hits_free), NULL without KS_SEARCH_ABUND_STATS */
const uint64_t *ks_hits_device_median2(const ks_hits *h);
const double *ks_hits_device_abund_ss(const ks_hits *h);
/* either destination may be NULL; KS_ERR_INVALID_ARG for hits without the statistics */
int ks_hits_copy_abund_stats_to_host(ks_ctx *ctx, const ks_hits *h, uint64_t *median2, double *ss);

/* ---- match positions: where each hit's shared k-mers lie ------------------------------------------------------------------ */

/* Replaces the k-mer join of `kmerseek search --extract-kmers` (src/python/kmerseek/search.py:195-240: query and target k-mer
 * tables joined on the hash, restricted to the search hits): for every row r = (qid, tid) of `hits`, the multiset
 *     { (a.start, b.start) : a in q_pos, a.seq = qid, b in t_pos, b.seq = tid, a.hash = b.hash }
 * ordered by (query start, target start) — a hash that repeats m times in the query and n times in the target gives m x n
 * pairs.  q_pos / t_pos: the ks_kmer_positions* tables of the query batch and of the targets `hits` was searched on, made
 * with the same ks_params (else KS_ERR_INVALID_ARG); hits: from any search entry, thresholded ones included — equal hashes of
 * a (query, target) pair that is not a row of `hits` give no pair.  Every row of a search shares a hash, so it owns at least
 * one pair (at least `intersect`, exactly `intersect` when neither sequence repeats a k-mer): a row without pairs means the
 * three inputs do not belong together, and the call fails with KS_ERR_INVALID_ARG.
 * Result (device-resident):
 *   row_offsets u64[n_rows + 1]  row r owns pairs [row_offsets[r], row_offsets[r + 1]);  n_rows = ks_hits_count(hits)
 *   q_start, t_start u32[n_pairs]
 *   q_lo, q_hi, t_lo, t_hi u32[n_rows]  per row the smallest start and the largest start + ksize on either side: the
 *                                query_start / match_start of the reference's stitched row and an upper bound of its *_end
 * One stream, synchronous on return; all scratch comes from the context's pool. */
typedef struct ks_matchpos_opts {
    uint32_t flags;     /* none defined: 0 */
    uint32_t reserved;  /* 0 */
    uint64_t max_pairs; /* refuse more than this many pairs; 0 = the library's own limit (what the device memory and one sort
                           take).  The pairs are counted — as the join finds them, before the rows a thresholded search dropped
                           are taken out: that many have to be materialised — BEFORE the pair arrays are allocated; beyond the
                           limit the call fails with KS_ERR_CAPACITY and ks_last_error carries the count (low-complexity hp
                           k-mers make the sum of q(h) x t(h) explode: the caller can say no). */
} ks_matchpos_opts;
/* opts == NULL: the defaults.  Options are checked before any device work. */
int ks_match_positions(ks_ctx *ctx, const ks_kmerpos *q_pos, const ks_kmerpos *t_pos, const ks_hits *hits,
                       const ks_matchpos_opts *opts, ks_matchpos **out);
uint64_t ks_matchpos_n_rows(const ks_matchpos *m);
uint64_t ks_matchpos_n_pairs(const ks_matchpos *m);
/* hit-row slices the call ran in (1 unless row index + both starts need more than 64 key bits).  Diagnostic. */
uint32_t ks_matchpos_n_slices(const ks_matchpos *m);
/* device pointers, valid until ks_matchpos_free */
const uint64_t *ks_matchpos_device_row_offsets(const ks_matchpos *m);
const uint32_t *ks_matchpos_device_q_start(const ks_matchpos *m);
const uint32_t *ks_matchpos_device_t_start(const ks_matchpos *m);
const uint32_t *ks_matchpos_device_q_lo(const ks_matchpos *m);
const uint32_t *ks_matchpos_device_q_hi(const ks_matchpos *m);
const uint32_t *ks_matchpos_device_t_lo(const ks_matchpos *m);
const uint32_t *ks_matchpos_device_t_hi(const ks_matchpos *m);
/* any destination may be NULL */
int ks_matchpos_copy_to_host(ks_ctx *ctx, const ks_matchpos *m, uint64_t *row_offsets, uint32_t *q_start, uint32_t *t_start,
                             uint32_t *q_lo, uint32_t *q_hi, uint32_t *t_lo, uint32_t *t_hi);
void ks_matchpos_free(ks_matchpos *m);

/* ---- match regions: each hit's pairs chained by diagonal ------------------------------------------------------------------- */

/* The last step before the reference's output line, `query:start-end` found in `target:start-end`: every hit row's pairs
 * chained into maximal colinear regions.  The reference's stitcher (src/python/kmerseek/search.py:37-121) takes all pairs of
 * a match for ONE contiguous colinear run and returns a wrong region when they are not (two unrelated k-mers, a multi-domain
 * protein); this pass returns every run.  All arithmetic is in integers.
 *   pair of hit row r: (a, b) = (query start, target start); its diagonal d = b - a (signed); the pairs of a row are distinct
 *   region: a maximal set of pairs of one row and one d in which, sorted by a, consecutive pairs satisfy
 *           a_next - a_prev <= ksize + max_gap   (max_gap = 0: the windows overlap or abut)
 *   ksize: that of the tables the ks_matchpos was made from.
 * Per region:
 *   q_start = the smallest a;  t_start = q_start + d
 *   length  = the largest a + ksize - q_start — the same on both sides: the region is [q_start, q_start + length) in the
 *             query and [t_start, t_start + length) in the target, 0-based half-open as the reference's columns
 *   n_kmers = the number of pairs
 *   covered = sum over consecutive pairs of min(ksize, a_next - a_prev), + ksize: the residues under at least one shared
 *             window (= length when max_gap = 0)
 * Regions with fewer than min_kmers pairs are dropped after chaining (0 and 1 keep everything); a row may keep none.
 * Result (device-resident):
 *   row_offsets u64[n_rows + 1]   row r owns regions [row_offsets[r], row_offsets[r + 1]);  n_rows = ks_matchpos_n_rows(mp)
 *   q_start, t_start, length, n_kmers, covered u32[n_regions]    inside a row ordered by (q_start, t_start)
 * The result never depends on the internal path (slices, sort variant, wave or workgroup).  A ks_matchpos without rows or
 * pairs gives a valid empty result.  max_gap is clamped so that ksize + max_gap stays a u32.
 * KS_ERR_INVALID_ARG: non-zero flags / reserved (checked before any device work), NULL arguments, an input of another
 * context.  KS_ERR_CAPACITY: the diagonal and the start fill the 64-bit sort key on their own (starts beyond 2^31), or more
 * than 2^38 / ksize pairs (only reachable with ksize > 64).
 * One stream, synchronous on return, two host waits (the region count comes back with the first); all scratch comes from the
 * context's pool: 52 bytes per pair. */
typedef struct ks_regions_opts {
    uint32_t flags;     /* none defined: 0 */
    uint32_t min_kmers; /* drop regions with fewer pairs; 0 = 1 = keep all */
    uint32_t max_gap;   /* residues two consecutive windows of a region may leave uncovered between them */
    uint32_t reserved;  /* 0 */
} ks_regions_opts;
/* opts == NULL: the defaults (min_kmers 1, max_gap 0) */
int ks_match_regions(ks_ctx *ctx, const ks_matchpos *mp, const ks_regions_opts *opts, ks_regions **out);
uint64_t ks_regions_n_rows(const ks_regions *r);
uint64_t ks_regions_n_regions(const ks_regions *r);
/* hit-row slices the chaining ran in (1 unless row index, diagonal and start need more than 64 key bits).  Diagnostic. */
uint32_t ks_regions_n_slices(const ks_regions *r);
/* device pointers, valid until ks_regions_free */
const uint64_t *ks_regions_device_row_offsets(const ks_regions *r);
const uint32_t *ks_regions_device_q_start(const ks_regions *r);
const uint32_t *ks_regions_device_t_start(const ks_regions *r);
const uint32_t *ks_regions_device_length(const ks_regions *r);
const uint32_t *ks_regions_device_n_kmers(const ks_regions *r);
const uint32_t *ks_regions_device_covered(const ks_regions *r);
/* any destination may be NULL */
int ks_regions_copy_to_host(ks_ctx *ctx, const ks_regions *r, uint64_t *row_offsets, uint32_t *q_start, uint32_t *t_start,
                            uint32_t *length, uint32_t *n_kmers, uint32_t *covered);
void ks_regions_free(ks_regions *r);

/* ---- region scores: how good is a region?  Substitution-matrix score and ungapped X-drop extension ------------------------- */

/* Scores every region of a ks_regions under a substitution matrix and, on request, extends it without gaps in both
 * directions under an X-drop rule (the ungapped stage of every seed-and-extend search).  The reference prints the `query`,
 * `alpha` and `match` strings of a stitched region (src/python/kmerseek/search.py:61-121) and leaves the judging to the eye;
 * for hp and dayhoff the seeds match in the reduced alphabet only, so the identity in the real alphabet is what this adds.
 * All arithmetic is in integers: the result is bit-exact against a host loop.
 *   regions: a ks_regions R;  hits: the ks_hits H whose rows it was chained for — row r = (qid, tid),
 *            ks_regions_n_rows(R) == ks_hits_count(H)
 *   the query and the target residue batches on the device (d_res, d_offsets u64[n + 1], n_seqs, n_residues): the layout
 *   ks_sketch_batch_device and ks_kmer_positions_device read
 * Residue class of a byte x, after ASCII upper-casing (only a-z change): 'A'..'Z' -> 0..25, '*' -> 26, every other byte -> 27.
 * Matrix: int8 M[KS_RSCORE_ALPHABET][KS_RSCORE_ALPHABET], row-major, a caller-owned HOST array; the row is the query's class,
 * the column the target's; it need not be symmetric.  matrix == NULL: M[x][y] = (x == y) ? +1 : -1.
 * A position pair (i in the query sequence, j in the target sequence): s = M[class(q[i])][class(t[j])]; it is an identity iff
 * the two upper-cased bytes are equal, a positive iff s > 0.
 * Region g of row r: a = q_start, b = t_start, n = length; Lq, Lt the lengths of the two sequences.
 *   core        the n pairs (a + i, b + i);  core_score = the sum of s over them (i64)
 *   right extension (only with KS_RSCORE_EXTEND): e_max = min(Lq - (a + n), Lt - (b + n));
 *               S_0 = 0, S_j = S_(j-1) + s(a + n + j - 1, b + n + j - 1) for j = 1 .. e_max;  B_j = max(S_0 .. S_j);
 *               J = the smallest j >= 1 with B_j - S_j > x_drop, or e_max if there is none;
 *               right_ext = the smallest j in [0, J] with S_j == B_J (the shortest extension wins a tie);  right_score = B_J
 *   left extension: the mirror image on the pairs (a - j, b - j), j = 1 .. min(a, b)
 *   without the flag both extensions are 0
 * Result (device-resident), the same CSR over hit rows and the same order as R (row_offsets is a copy of R's):
 *   q_start = a - left_ext, t_start = b - left_ext, length = left_ext + n + right_ext   u32[n_regions]
 *   score = left_score + core_score + right_score                                        i64[n_regions]
 *   identities, positives   u32[n_regions]  counted over the extended span
 *   core_identities         u32[n_regions]  counted over the core alone
 * Extended regions of one row may overlap or coincide: nothing is merged or de-duplicated here (ks_rscores_cull, below, does
 * that).  The result never depends on
 * the launch geometry or on how many positions a wave examines per step.  An R without rows or regions gives a valid empty
 * result.
 * KS_ERR_INVALID_ARG: unknown flags / a non-zero reserved field (checked before any device work, also with ctx == NULL), NULL
 * arguments, an input of another context, ks_regions_n_rows(R) != ks_hits_count(H); a region that does not lie inside its two
 * sequences (a + n > Lq or b + n > Lt) or a qid / tid beyond its batch — the inputs do not belong together: ks_last_error
 * names the first such row, and nothing is read outside the batches.
 * One stream, synchronous on return, one host wait; all scratch comes from the context's pool. */
#define KS_RSCORE_ALPHABET 28
#define KS_RSCORE_EXTEND 1u
typedef struct ks_rscore_opts {
    uint32_t flags;        /* KS_RSCORE_EXTEND */
    uint32_t x_drop;       /* used with KS_RSCORE_EXTEND; 0 stops at the first step below the best */
    const int8_t *matrix;  /* HOST, 28 x 28 row-major, or NULL: +1 / -1 */
    uint64_t reserved;     /* 0 */
} ks_rscore_opts;
/* opts == NULL: the defaults (no extension, the +1 / -1 matrix) */
int ks_regions_score(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits,
                     const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res,
                     const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res,
                     const ks_rscore_opts *opts, ks_rscores **out);
uint64_t ks_rscores_n_rows(const ks_rscores *s);
uint64_t ks_rscores_n_regions(const ks_rscores *s);
/* device pointers, valid until ks_rscores_free */
const uint64_t *ks_rscores_device_row_offsets(const ks_rscores *s);
const uint32_t *ks_rscores_device_q_start(const ks_rscores *s);
const uint32_t *ks_rscores_device_t_start(const ks_rscores *s);
const uint32_t *ks_rscores_device_length(const ks_rscores *s);
const int64_t *ks_rscores_device_score(const ks_rscores *s);
const uint32_t *ks_rscores_device_identities(const ks_rscores *s);
const uint32_t *ks_rscores_device_positives(const ks_rscores *s);
const uint32_t *ks_rscores_device_core_identities(const ks_rscores *s);
/* any destination may be NULL */
int ks_rscores_copy_to_host(ks_ctx *ctx, const ks_rscores *s, uint64_t *row_offsets, uint32_t *q_start, uint32_t *t_start,
                            uint32_t *length, int64_t *score, uint32_t *identities, uint32_t *positives, uint32_t *core_identities);
void ks_rscores_free(ks_rscores *s);
/* positions one wave examines per extension step: the tests place terminations around it */
uint32_t ks_debug_rscore_step(void);

/* ---- region alignments: one gapped alignment per region (banded affine-gap extension under an X-drop rule) ---------------- */

/* Extends every region of a ks_regions WITH gaps, from the middle pair of its seed to both sides: the gapped stage of a
 * seed-and-extend search, behind the ungapped one of ks_regions_score.  An indel moves a match to a neighbouring diagonal and
 * ks_match_regions then reports fragments; this gives each of them the one alignment it belongs to — its score, extents,
 * identities, gap count — in the real alphabet.  The path itself is ks_regions_traceback's, below: the result records the
 * options it was made with for it.  All arithmetic is in integers: the result is bit-exact against a host loop
 * (tests/ralign_ref.py).
 * Inputs, residue classes, the matrix (caller-owned HOST int8 M[28][28], NULL: +1 / -1), identities (equal upper-cased bytes)
 * and positives (s > 0): those of ks_regions_score, above.
 * Options: band = W in [0, 31]; gap_open = o and gap_extend = e in [0, 255], a gap of L residues costs o + L * e;
 * x_drop <= 2^20; flags 0.
 * Region with seed (a, b, n), n >= 1: the anchor is the pair (ai, bj) = (a + n / 2, b + n / 2) (integer division).  The
 * alignment is the anchor pair, a right extension over Q = q[ai + 1 ...], T = t[bj + 1 ...] and a left extension — the same
 * function — over the reversed prefixes Q = q[ai - 1], q[ai - 2], ...; T = t[bj - 1], ...
 * One extension over Q_1 .. Q_X and T_1 .. T_Y lives on the cells (x, y), 0 <= x <= X, 0 <= y <= Y, |y - x| <= W; every other
 * cell does not exist and is never a source:
 *   H~(0, 0) = 0
 *   F(x, y)  = max(H(x - 1, y) - o - e, F(x - 1, y) - e)                   on a tie the continued gap
 *   D(x, y)  = H(x - 1, y - 1) + M[class(Q_x)][class(T_y)]
 *   H~(x, y) = max(D, F)                                                   on a tie D
 *   E(x, y)  = max over existing y' < y of H~(x, y') - o - (y - y') * e    on a tie the largest y'
 *   H(x, y)  = max(H~, E)                                                  on a tie H~
 * (E reads H~ only: for o >= 0 the scores are those of the three-matrix Gotoh recurrence over the same band.)  Every cell
 * carries the counts of the path that made it through the same choices: identities, positives, gap_opens, gaps (residues).
 *   R_x = max over y of H(x, y);  B_x = max(R_0 .. R_x);
 *   J = the first x >= 1 with B_x - R_x > x_drop, or the last row that has a cell (a row-level X-drop: no cell is pruned)
 *   the extension's result is the cell of rows 0 .. J with the largest H, on a tie the smallest x, then the smallest y:
 *   its (x, y), its H and its counts.  With W = 0 this is the ungapped rule of ks_regions_score started at the anchor.
 * Result (device-resident), the same CSR over hit rows and the same order as R (row_offsets is a copy of R's):
 *   q_start = ai - x_left, q_length = x_left + 1 + x_right, t_start = bj - y_left, t_length = y_left + 1 + y_right   u32
 *   score = M[anchor pair] + left + right                                                                            i64
 *   identities, positives (the anchor pair included), gap_opens, gaps, aln_length = aligned pairs + gaps              u32
 * Alignments of one row may overlap or coincide: nothing is merged here (ks_raligns_cull, below, keeps one of each).  The result
 * never depends on the launch geometry or on
 * ks_debug_ralign_chunk().  An R without rows or regions gives a valid empty result.
 * KS_ERR_INVALID_ARG: an option out of range or unknown flags (checked before any device work, also with ctx == NULL), and
 * everything ks_regions_score refuses, with the same check: ks_last_error names the first bad row, nothing is read outside
 * the batches.  KS_ERR_CAPACITY: a hit row with regions whose query or target sequence is longer than 2^20 residues (the bound
 * that keeps the dynamic program in 32 bits); ks_last_error names the first such row.
 * One stream, one launch, synchronous on return, one host wait; all scratch comes from the context's pool. */
#define KS_RALIGN_MAX_BAND 31u
#define KS_RALIGN_MAX_GAP_COST 255u
#define KS_RALIGN_MAX_X_DROP (1u << 20)
typedef struct ks_ralign_opts {
    const int8_t *matrix;  /* HOST, 28 x 28 row-major, or NULL: +1 / -1 */
    uint32_t band;         /* W <= KS_RALIGN_MAX_BAND */
    uint32_t gap_open;     /* o <= KS_RALIGN_MAX_GAP_COST */
    uint32_t gap_extend;   /* e <= KS_RALIGN_MAX_GAP_COST */
    uint32_t x_drop;       /* <= KS_RALIGN_MAX_X_DROP */
    uint32_t flags;        /* 0 */
} ks_ralign_opts;
/* opts == NULL: band 16, gap_open 11, gap_extend 1, x_drop 30, the +1 / -1 matrix */
int ks_regions_align(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits,
                     const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res,
                     const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res,
                     const ks_ralign_opts *opts, ks_raligns **out);
uint64_t ks_raligns_n_rows(const ks_raligns *s);
uint64_t ks_raligns_n_regions(const ks_raligns *s);
/* device pointers, valid until ks_raligns_free */
const uint64_t *ks_raligns_device_row_offsets(const ks_raligns *s);
const uint32_t *ks_raligns_device_q_start(const ks_raligns *s);
const uint32_t *ks_raligns_device_q_length(const ks_raligns *s);
const uint32_t *ks_raligns_device_t_start(const ks_raligns *s);
const uint32_t *ks_raligns_device_t_length(const ks_raligns *s);
const int64_t *ks_raligns_device_score(const ks_raligns *s);
const uint32_t *ks_raligns_device_identities(const ks_raligns *s);
const uint32_t *ks_raligns_device_positives(const ks_raligns *s);
const uint32_t *ks_raligns_device_gap_opens(const ks_raligns *s);
const uint32_t *ks_raligns_device_gaps(const ks_raligns *s);
const uint32_t *ks_raligns_device_aln_length(const ks_raligns *s);
/* any destination may be NULL */
int ks_raligns_copy_to_host(ks_ctx *ctx, const ks_raligns *s, uint64_t *row_offsets, uint32_t *q_start, uint32_t *q_length,
                            uint32_t *t_start, uint32_t *t_length, int64_t *score, uint32_t *identities, uint32_t *positives,
                            uint32_t *gap_opens, uint32_t *gaps, uint32_t *aln_length);
void ks_raligns_free(ks_raligns *s);
/* rows of the dynamic program whose residues one wave stages at once: the tests place terminations around it */
uint32_t ks_debug_ralign_chunk(void);

/* ---- region traceback: the path of every region alignment, as a CIGAR ------------------------------------------------------ */

/* Walks back the alignment of every region of a ks_raligns and reports its path: what a PAF / SAM `cg` tag, a printed
 * alignment or a mask of the aligned residues needs.  ks_regions_align fixes the path by the tie rules of its recurrence
 * (above) and reports four counts of it; this reports the path those are counts of.  All arithmetic is in integers: the result
 * is bit-exact against a host loop (tests/rtrace_ref.py).
 *   regions, hits and the two residue batches: what ks_regions_align took;  alignments: the ks_raligns S it returned.
 * S records the options it was made with (band, gap_open, gap_extend, x_drop, a copy of the matrix): the traceback runs the
 * same program and cannot be given others.
 * Region g with seed (a, b, n) and anchor (ai, bj) = (a + n / 2, b + n / 2): the end cells of its two extensions follow from S:
 *   x_left = ai - q_start, x_right = q_length - 1 - x_left;  y_left = bj - t_start, y_right = t_length - 1 - y_left
 * The path of one extension goes from its end cell back to (0, 0) by the choices the recurrence made:
 *   at H(x, y):   E if H took E — a jump to H~(x, y'), y' the source of E, y - y' target residues — else H~(x, y)
 *   at H~(x, y):  D — one aligned pair, to H(x - 1, y - 1) — if H~ took D, else F(x, y)
 *   at F(x, y):   one query residue; to F(x - 1, y) if F continued the gap, else to H(x - 1, y)
 *   at H(0, y), y > 0: an E of y residues from (0, 0)
 * with the ties as above: F prefers the continued gap, H~ prefers D, E the largest y', H prefers H~.
 * The alignment is the left path in forward sequence order, the anchor pair, the right path.  Its columns, the query as the
 * read and the target as the reference: an aligned pair is M; a query residue without a target residue is I; a target residue
 * without a query residue is D.  With KS_RTRACE_EQX an aligned pair is = where the two upper-cased bytes are equal and X where
 * they are not.  Adjacent equal columns are one op, the anchor merges with the runs beside it; an op is len << 4 | code with
 * the BAM codes M = 0, I = 1, D = 2, = = 7, X = 8 (len <= 2^21 + 31 < 2^28).
 * Result (device-resident): a CSR over the regions in the order of S: op_offsets u64[n_regions + 1], ops u32[n_ops].
 * For every region: the ops' lengths sum to aln_length; pairs + I = q_length; pairs + D = t_length; the number of I and D ops
 * is gap_opens (the recurrence never splits a run; an I run beside a D run is two opens) and their lengths sum to gaps; with
 * KS_RTRACE_EQX the = columns are identities; re-scoring the ops under the matrix and the gap costs gives score and positives.
 * The result never depends on the launch geometry, on ks_debug_ralign_chunk() / ks_debug_rtrace_stage() or on
 * max_scratch_bytes.  An S without rows or regions gives a valid empty result (op_offsets = {0}).
 * Scratch: one byte per cell of the band for the rows between the two end cells — 64 bytes per row, q_length - 1 rows (each
 * side's rounded up to an even number) per region.  max_scratch_bytes (0: 1 GiB) bounds it: the regions run in slices of
 * consecutive regions whose rows fit.  KS_ERR_CAPACITY: a single region that does not fit (ks_last_error names it), and what
 * ks_regions_align refuses with it.
 * KS_ERR_INVALID_ARG: unknown flags / a non-zero reserved field (checked before any device work, also with ctx == NULL);
 * everything ks_regions_align refuses, with the same checks; an S whose row or region count is not that of `regions` (checked
 * on the host before any device work); an S that does not belong to these regions and batches — an extent outside its
 * sequence, an anchor outside the extent, an end cell outside the band, or a path whose length or score is not the
 * alignment's: ks_last_error names the first such region.  The extent and anchor checks run before anything is indexed by
 * them: no combination of arguments that passes the host checks reads or writes outside the batches and the scratch.
 * One stream, synchronous on return, three host waits (the layout, the op count, the ops); all memory comes from the
 * context's pool. */
#define KS_RTRACE_EQX 1u
typedef struct ks_rtrace_opts {
    uint32_t flags;             /* KS_RTRACE_EQX */
    uint32_t reserved;          /* 0 */
    uint64_t max_scratch_bytes; /* direction scratch of one slice; 0: 1 GiB */
} ks_rtrace_opts;
/* opts == NULL: M / I / D ops, 1 GiB */
int ks_regions_traceback(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits,
                         const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res,
                         const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res,
                         const ks_raligns *alignments, const ks_rtrace_opts *opts, ks_cigars **out);
uint64_t ks_cigars_n_rows(const ks_cigars *c);
uint64_t ks_cigars_n_regions(const ks_cigars *c);
uint64_t ks_cigars_n_ops(const ks_cigars *c);
/* diagnostic: the direction scratch the call allocated, and the slices it ran in */
uint64_t ks_cigars_scratch_bytes(const ks_cigars *c);
uint32_t ks_cigars_n_slices(const ks_cigars *c);
/* device pointers, valid until ks_cigars_free */
const uint64_t *ks_cigars_device_op_offsets(const ks_cigars *c);
const uint32_t *ks_cigars_device_ops(const ks_cigars *c);
/* any destination may be NULL */
int ks_cigars_copy_to_host(ks_ctx *ctx, const ks_cigars *c, uint64_t *op_offsets, uint32_t *ops);
void ks_cigars_free(ks_cigars *c);
/* rows of directions one wave stages at once for the walk: the tests place end cells around it */
uint32_t ks_debug_rtrace_stage(void);

/* ---- region cull: one row per distinct alignment of a hit, best first ------------------------------------------------------ */

/* What every seed-and-extend search closes its extension stage with (HSP culling): of the regions of one hit row, those that
 * a better region of the same row covers are removed.  ks_regions_align gives every fragment an indel splits a match into the
 * one alignment they belong to — the same alignment, once per fragment; a repeat gives alignments inside alignments.  This
 * pass keeps one of each and says which region stands for which.  It is a pass over extents and scores only: it reads no
 * residues.  The same pass serves a ks_raligns (both sides have their own length) and a ks_rscores (the ungapped extended
 * regions: one length for both sides).  All arithmetic is in integers, in 64 bits.
 * Input: a CSR over hit rows and five columns per region:
 *   row_offsets u64[n_rows + 1];  q_start, q_length, t_start, t_length u32[n];  score i64[n]
 *   region g is [q_start, q_start + q_length) in the query and [t_start, t_start + t_length) in the target.
 * Options: overlap_pct = P in [1, 100], 0 means 100;  max_per_row = N, 0 means no limit;  min_score, used only with the flag
 * KS_RCULL_MIN_SCORE.
 * Priority inside a row: g comes before h iff score[g] > score[h], or the scores are equal and g < h by input index.
 * covers(k, g) holds iff  ovq * 100 >= P * q_length[g]  and  ovt * 100 >= P * t_length[g],  where
 *   ovq = max(0, min(qe_k, qe_g) - max(qs_k, qs_g))  (qe = q_start + q_length, in u64) and ovt is the same on the target.
 * The relation is relative to g, the region being removed: it is not symmetric.  With P = 100 it means "g lies inside k on
 * both sequences".  Overlap on one sequence alone never covers: that is a repeat.
 * The regions of a row are decided in priority order, each by the first rule that applies:
 *   1. with the flag, score[g] < min_score: dropped, keeper[g] = KS_RCULL_NONE.  Such a region never covers anything.
 *   2. a kept region of the row covers g: removed; keeper[g] = the first such kept region in priority order.
 *   3. the row already keeps N regions (N > 0): dropped, keeper[g] = KS_RCULL_NONE.
 *   4. otherwise g is kept and keeper[g] = g.
 * The pass is greedy, not transitive: a removed region covers nothing.  If A removes B and only B would have covered C, C is kept.
 * Result (device-resident):
 *   row_offsets u64[n_rows + 1]   a CSR of the kept regions over the same hit rows
 *   per kept region: src_region u32, its input index — ascending inside a row, so the input's (q_start, t_start) order
 *                    survives; rank u32, 0 is the row's best kept region; n_merged u32, the input regions that name it as
 *                    keeper, itself included
 *   keeper u32[n]                 one per input region
 *   row_best_score f64[n_rows]    (double)score of the row's rank-0 region, NaN for a row that keeps none: exactly a d_score
 *                                 column for ks_hits_best with KS_BEST_SCORE, which ranks NaN last
 * The sum of n_merged plus the regions with keeper KS_RCULL_NONE is n.  The result does not depend on the path a row took
 * (KS_DEBUG_CULL_PATH = 1 / 2 / 3 force every row of at most 64 regions onto a wave / every row onto a workgroup / that with a
 * small LDS capacity, for the tests) or on the launch geometry.  An input without rows or regions gives a valid empty result.
 * Culling a culled list again with the same P, no limit and no min_score keeps everything with n_merged = 1.
 * KS_ERR_INVALID_ARG: unknown flags, a non-zero reserved field or P > 100 (checked before any device work, also with
 * ctx == NULL); NULL arguments; an object of another context; row_offsets that is not a non-decreasing CSR from 0 to n — a plan
 * kernel checks this before anything is indexed by it, ks_last_error names the first bad row; a region with a length of 0
 * (the first such region is named).  KS_ERR_CAPACITY: 2^32 - 2 or more rows, more than 2^32 - 1 regions.
 * One stream, synchronous on return, one host wait (the kept count and the bad-row words come back with it); all memory comes
 * from the context's pool: 28 bytes of scratch per region and 24 per hit row. */
typedef struct ks_rcull ks_rcull;
#define KS_RCULL_NONE 0xffffffffu
#define KS_RCULL_MIN_SCORE 1u
typedef struct ks_rcull_opts {
    uint32_t overlap_pct;  /* P in [1, 100]; 0 = 100 */
    uint32_t max_per_row;  /* N; 0 = no limit */
    int64_t  min_score;    /* used with KS_RCULL_MIN_SCORE */
    uint32_t flags;        /* KS_RCULL_MIN_SCORE */
    uint32_t reserved;     /* 0 */
} ks_rcull_opts;
/* opts == NULL: P = 100, no limit, no min_score.  d_t_length == NULL: the target lengths are the query lengths. */
int ks_regions_cull_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint32_t *d_q_start, const uint32_t *d_q_length,
                           const uint32_t *d_t_start, const uint32_t *d_t_length, const int64_t *d_score, uint64_t n_rows,
                           uint64_t n_regions, const ks_rcull_opts *opts, ks_rcull **out);
/* the same on the columns of an object: the alignments' extents and score; the extended regions' placement, `length` for both
 * sides, and score */
int ks_raligns_cull(ks_ctx *ctx, const ks_raligns *alignments, const ks_rcull_opts *opts, ks_rcull **out);
int ks_rscores_cull(ks_ctx *ctx, const ks_rscores *scores, const ks_rcull_opts *opts, ks_rcull **out);
uint64_t ks_rcull_n_rows(const ks_rcull *c);
uint64_t ks_rcull_n_regions(const ks_rcull *c); /* of the input */
uint64_t ks_rcull_n_kept(const ks_rcull *c);
/* device pointers, valid until ks_rcull_free */
const uint64_t *ks_rcull_device_row_offsets(const ks_rcull *c);
const uint32_t *ks_rcull_device_src_region(const ks_rcull *c);
const uint32_t *ks_rcull_device_rank(const ks_rcull *c);
const uint32_t *ks_rcull_device_n_merged(const ks_rcull *c);
const uint32_t *ks_rcull_device_keeper(const ks_rcull *c);
const double *ks_rcull_device_row_best_score(const ks_rcull *c);
/* any destination may be NULL */
int ks_rcull_copy_to_host(ks_ctx *ctx, const ks_rcull *c, uint64_t *row_offsets, uint32_t *src_region, uint32_t *rank,
                          uint32_t *n_merged, uint32_t *keeper, double *row_best_score);
void ks_rcull_free(ks_rcull *c);
/* The object of the kept regions only: every column gathered by src_region, row_offsets from the cull.  ks_raligns_take
 * carries the recorded options and the matrix: a taken ks_regions with a taken ks_raligns is a valid input of
 * ks_regions_traceback, which then traces only what was kept.  KS_ERR_INVALID_ARG: NULL arguments, an object of another
 * context, an object whose row or region count is not that of the cull's input.  Synchronous on return. */
int ks_regions_take(ks_ctx *ctx, const ks_regions *regions, const ks_rcull *cull, ks_regions **out);
int ks_rscores_take(ks_ctx *ctx, const ks_rscores *scores, const ks_rcull *cull, ks_rscores **out);
int ks_raligns_take(ks_ctx *ctx, const ks_raligns *alignments, const ks_rcull *cull, ks_raligns **out);
/* regions of a row the workgroup path holds in LDS (returned) and that capacity under KS_DEBUG_CULL_PATH = 3 (*small_rows,
 * may be NULL): the tests place rows around them */
uint32_t ks_debug_rcull_lds_rows(uint32_t *small_rows);

/* ---- region chain: one colinear chain of alignments per hit ------------------------------------------------------------------ */

/* What a seed-and-extend search does after the cull to say how the local alignments of one hit fit together (BLAST's HSP
 * linking, the chains behind qcovs, MMseqs2 -c, CD-HIT -aS / -aL): per hit row the set of regions that can all be true at once —
 * ascending on BOTH sequences — with the largest sum of scores minus link costs.  Two alignments on either side of a long
 * insertion chain; two domains in swapped order do not.  Like the cull it reads extents and scores only, no residues, and
 * serves a ks_raligns and a ks_rscores alike.  The intended input is what the cull kept (ks_raligns_take), any other is taken.
 * Input: a CSR over hit rows and five columns per region, as for ks_regions_cull_device:
 *   row_offsets u64[n_rows + 1];  q_start, q_length, t_start, t_length u32[n];  score i64[n]
 *   d_t_length == NULL: the target lengths are the query lengths.  d_identities, d_aln_length u32[n]: either may be NULL;
 *   they are only summed over the chain.
 * Options (opts == NULL: all zero): max_gap (0: no limit), max_overlap, link_cost <= 2^30, skew_cost and overlap_cost <= 2^16;
 * flags and reserved must be 0.
 * All arithmetic is in signed 64 bits; an end is start + length.  follows(a, b) holds iff
 *   q_start[a] < q_start[b], t_start[a] < t_start[b], q_end[a] < q_end[b], t_end[a] < t_end[b]  and, with
 *   dq = q_start[b] - q_end[a], dt = t_start[b] - t_end[a], ov = max(0, -dq, -dt):
 *   ov <= max_overlap  and  (max_gap == 0 or max(dq, dt, 0) <= max_gap).
 * cost(a, b) = link_cost + skew_cost * |dq - dt| + overlap_cost * ov.
 * Per hit row:
 *   best[i] = score[i] + max(0, max over j with follows(j, i) of best[j] - cost(j, i))
 *   a link is taken only when best[j] - cost(j, i) > 0; among equal maxima pred[i] is the smallest input index j;
 *   pred[i] = KS_RCHAIN_NONE: the chain starts at i.
 *   The row's chain ends at the region of the largest best (ties: the smaller input index) and is walked back along pred.
 * follows needs a strictly smaller q_start: any order by q_start is a valid evaluation order, and equal starts never link.
 * Result (device-resident):
 *   row_offsets u64[n_rows + 1], src_region u32[n_chained]   the members of each row's chain in chain order (ascending
 *                                                            q_start); a row without regions has none
 *   best i64[n], pred u32[n]                                 per input region
 *   per hit row:
 *   chain_score i64          the best of the end region, 0 for a row without regions
 *   q_start, q_length, t_start, t_length u32   the span from the first member's start to the last member's end, zeros for an
 *                            empty row
 *   q_aligned, t_aligned u32 the length of the union of the members' intervals: starts and ends both ascend strictly along a
 *                            chain, so it is the first member's length plus, over successive members a, b,
 *                            end[b] - max(start[b], end[a])
 *   identities, aln_length u64   the sums of the optional columns over the members, 0 where the column was not passed
 *   row_chain_score f64      (double)chain_score, NaN for an empty row: exactly a d_score column for ks_hits_best with
 *                            KS_BEST_SCORE and for the cluster passes
 * Every member but the first has its predecessor as pred; chain_score is the sum of the members' scores minus the sum of the
 * link costs.  The result does not depend on the path a row took (KS_DEBUG_CHAIN_PATH = 1 / 2 / 3 force every row of at most 64
 * regions onto a wave / every row onto a workgroup / that with a small LDS capacity, for the tests) or on the launch geometry.
 * An input without rows or regions gives a valid empty result.
 * KS_ERR_INVALID_ARG: an option out of range, unknown flags or a non-zero reserved field (checked before any device work, also
 * with ctx == NULL); NULL arguments; an object of another context; row_offsets that is not a non-decreasing CSR from 0 to n
 * (ks_last_error names the first bad row); a region with a length of 0, with an end beyond 0xffffffff or with |score| > 2^30 —
 * with that bound and the cost bounds no sum can leave 64 bits — (the plan kernel names the first such region).
 * KS_ERR_CAPACITY: 2^32 - 2 or more rows, more than 2^32 - 1 regions.
 * One stream, synchronous on return, one host wait (the chained count and the bad words come back with it); all memory comes
 * from the context's pool: 24 bytes of scratch per region and 24 per hit row. */
typedef struct ks_rchain ks_rchain;
#define KS_RCHAIN_NONE 0xffffffffu
typedef struct ks_rchain_opts {
    uint32_t max_gap;      /* the longest gap between two members on either sequence; 0 = no limit */
    uint32_t max_overlap;  /* the longest overlap of two members on either sequence */
    uint32_t link_cost;    /* per link, <= 2^30 */
    uint32_t skew_cost;    /* per position of |dq - dt|, <= 2^16 */
    uint32_t overlap_cost; /* per overlapping position, <= 2^16 */
    uint32_t flags;        /* 0 */
    uint32_t reserved[2];  /* 0 */
} ks_rchain_opts;
int ks_regions_chain_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint32_t *d_q_start, const uint32_t *d_q_length,
                            const uint32_t *d_t_start, const uint32_t *d_t_length, const int64_t *d_score,
                            const uint32_t *d_identities, const uint32_t *d_aln_length, uint64_t n_rows, uint64_t n_regions,
                            const ks_rchain_opts *opts, ks_rchain **out);
/* the same on the columns of an object: the alignments' extents, score, identities and aln_length; the extended regions'
 * placement, `length` for both sides and as aln_length, score and identities */
int ks_raligns_chain(ks_ctx *ctx, const ks_raligns *alignments, const ks_rchain_opts *opts, ks_rchain **out);
int ks_rscores_chain(ks_ctx *ctx, const ks_rscores *scores, const ks_rchain_opts *opts, ks_rchain **out);
uint64_t ks_rchain_n_rows(const ks_rchain *c);
uint64_t ks_rchain_n_regions(const ks_rchain *c); /* of the input */
uint64_t ks_rchain_n_chained(const ks_rchain *c);
/* device pointers, valid until ks_rchain_free */
const uint64_t *ks_rchain_device_row_offsets(const ks_rchain *c);
const uint32_t *ks_rchain_device_src_region(const ks_rchain *c);
const int64_t *ks_rchain_device_best(const ks_rchain *c);
const uint32_t *ks_rchain_device_pred(const ks_rchain *c);
const int64_t *ks_rchain_device_chain_score(const ks_rchain *c);
const uint32_t *ks_rchain_device_q_start(const ks_rchain *c);
const uint32_t *ks_rchain_device_q_length(const ks_rchain *c);
const uint32_t *ks_rchain_device_t_start(const ks_rchain *c);
const uint32_t *ks_rchain_device_t_length(const ks_rchain *c);
const uint32_t *ks_rchain_device_q_aligned(const ks_rchain *c);
const uint32_t *ks_rchain_device_t_aligned(const ks_rchain *c);
const uint64_t *ks_rchain_device_identities(const ks_rchain *c);
const uint64_t *ks_rchain_device_aln_length(const ks_rchain *c);
const double *ks_rchain_device_row_chain_score(const ks_rchain *c);
const double *ks_rchain_device_row_coverage(const ks_rchain *c); /* NULL before ks_rchain_coverage */
/* any destination may be NULL */
int ks_rchain_copy_to_host(ks_ctx *ctx, const ks_rchain *c, uint64_t *row_offsets, uint32_t *src_region, int64_t *best,
                           uint32_t *pred, int64_t *chain_score, uint32_t *q_start, uint32_t *q_length, uint32_t *t_start,
                           uint32_t *t_length, uint32_t *q_aligned, uint32_t *t_aligned, uint64_t *identities,
                           uint64_t *aln_length, double *row_chain_score);
void ks_rchain_free(ks_rchain *c);
/* Fills the chain's column row_coverage f64[n_rows], owned by the chain (a later call overwrites it): how much of its two
 * sequences the chain of each hit row covers.  hits: the hit list the chained regions belong to (its qid / tid name the
 * sequences); d_q_off u64[n_q + 1], d_t_off u64[n_t + 1]: the sequence offsets ks_regions_align takes.  mode: 0 q_aligned /
 * len(query), 1 t_aligned / len(target), 2 the smaller of the two, 3 the larger — one IEEE f64 division of two integers per
 * side.  NaN for a row without a chain or a sequence of length 0.
 * KS_ERR_INVALID_ARG: NULL arguments, an object of another context, mode > 3, hits of another row count, an id beyond n_q / n_t,
 * an aligned length beyond its sequence's (ks_last_error names the first such row); a refused call leaves no column.
 * Synchronous on return, one host wait. */
int ks_rchain_coverage(ks_ctx *ctx, ks_rchain *chain, const ks_hits *hits, const uint64_t *d_q_off, uint32_t n_q,
                       const uint64_t *d_t_off, uint32_t n_t, uint32_t mode);
/* copies row_coverage to the host; KS_ERR_INVALID_ARG before the first ks_rchain_coverage */
int ks_rchain_coverage_to_host(ks_ctx *ctx, const ks_rchain *c, double *row_coverage);
/* regions of a row the workgroup path holds in LDS (returned) and that capacity under KS_DEBUG_CHAIN_PATH = 3 (*small_rows,
 * may be NULL): the tests place rows around them */
uint32_t ks_debug_rchain_lds_rows(uint32_t *small_rows);

/* ---- frame fold: the hits of a translated search per (record, strand, target), regions in bases -------------------------- */

/* A search whose queries are the 6 n frames of ks_translate6_device (record s: 6 s + f forward, 6 s + 3 + f on the reverse
 * complement, f = 0, 1, 2) answers per frame, in residues of that frame.  The fold puts the rows of one strand's three frames
 * against one target into ONE row and their regions onto one coordinate, the strand's bases, so that ks_regions_chain_device
 * links across frames: two alignments in different frames on either side of a frameshift become one chain (blastx, DIAMOND -F).
 * Input: frame_hits, ordered by (qid, tid) as every search returns them; d_nt_offsets u64[n_records + 1], the record offsets
 * in bases (L_s: the length of record s); a CSR of regions over the hit rows as ks_regions_chain_device takes it (row_offsets
 * u64[n_rows + 1]; q_start, q_length, t_start, t_length u32[n]; d_t_length == NULL: the target lengths are the query lengths)
 * and the pass-through columns d_score i64[n], d_identities, d_aln_length u32[n], each of which may be NULL.  opts: flags and
 * reserved, all zero (NULL: the defaults).
 * Folded rows: one per distinct (2 s + strand, tid) that has at least one frame row (strand = 0 for frames 0 - 2, 1 for 3 - 5),
 * ordered by (2 s + strand, tid).  TWO objects come back, both NULL after any failure:
 *   *out_hits   a ks_hits with qid = 2 s + strand, tid, intersect = the sum of the member rows' (saturating at 2^32 - 1),
 *               n_weighted = their u64 sum; no statistics columns; n_pair_instances, partition_path and bucket_posting_bytes
 *               are the input's.  A hit list like any other: ks_hits_best with KS_BEST_SCORE and a chain's row_chain_score.
 *   *out        a ks_ffold:
 *   src_row u32[3 n_folded]      entry 3 r + j: the input row of frame 3 strand + j of folded row r, or KS_FFOLD_NONE
 *   row_offsets u64[n_folded + 1]   the CSR of the folded regions: a folded row's regions are those of its frame-0 row, then
 *                                of its frame-1 row, then frame 2, each in input order
 *   per folded region:
 *   src_region u32               the input region
 *   frame u8                     0 .. 5
 *   nt_length u32                3 q_length
 *   s_start u32                  f + 3 q_start: the start in the strand's own orientation (on the record for strand 0, on its
 *                                reverse complement for strand 1); the coordinate to chain on
 *   nt_start u32                 the start on the record as given: s_start forward, L_s - f - 3 (q_start + q_length) reverse
 *   t_start3, t_length3 u32      3 t_start, 3 t_length: the target in the same unit, so that the chain's |dq - dt| is in bases
 *   score i64, identities, aln_length u32   the input columns through src_region; NULL where the input column was NULL
 * An empty hit list, records without rows and rows without regions give valid (empty or shorter) results; n_regions of the
 * result is n of the input.  The result does not depend on the launch geometry.
 * KS_ERR_INVALID_ARG: unknown flags or a non-zero reserved field (checked first, also with ctx == NULL); NULL arguments; an
 * object of another context; and, ks_last_error naming the first offending record, row or region: d_nt_offsets that do not
 * start at 0 and ascend; a record beyond 2^32 - 16 bases; a qid >= 6 n_records; rows not strictly ascending by (qid, tid);
 * row_offsets that is not a non-decreasing CSR from 0 to n; a region whose q_start + q_length exceeds its frame's length
 * max(0, (L_s - f) / 3); a region whose 3 (t_start + t_length) exceeds 2^32 - 1.
 * KS_ERR_CAPACITY: 2^32 - 2 or more rows, more than 2^32 - 1 regions.
 * One stream, synchronous on return, one host wait (the folded row count and the bad words come back with it); all memory
 * comes from the context's pool: 32 bytes of scratch per hit row.  The folded count is known only after the wait: the folded
 * hit list, src_row and row_offsets are allocated for as many rows as the INPUT has (src_row for three times as many) and keep
 * those blocks until the objects are freed, though n_folded rows are used — up to three times what they need where all three
 * frames of every strand hit. */
typedef struct ks_ffold ks_ffold;
#define KS_FFOLD_NONE 0xffffffffu
typedef struct ks_ffold_opts {
    uint32_t flags;       /* 0 */
    uint32_t reserved[3]; /* 0 */
} ks_ffold_opts;
int ks_frames_fold_device(ks_ctx *ctx, const ks_hits *frame_hits, const uint64_t *d_nt_offsets, uint32_t n_records,
                          const uint64_t *d_row_offsets, const uint32_t *d_q_start, const uint32_t *d_q_length,
                          const uint32_t *d_t_start, const uint32_t *d_t_length, const int64_t *d_score,
                          const uint32_t *d_identities, const uint32_t *d_aln_length, uint64_t n_regions,
                          const ks_ffold_opts *opts, ks_hits **out_hits, ks_ffold **out);
/* the same on the columns of an object made for the rows of frame_hits: the extended regions' placement, `length` for both
 * sides and as aln_length, score and identities; the alignments' extents, score, identities and aln_length */
int ks_rscores_fold_frames(ks_ctx *ctx, const ks_hits *frame_hits, const uint64_t *d_nt_offsets, uint32_t n_records,
                           const ks_rscores *scores, const ks_ffold_opts *opts, ks_hits **out_hits, ks_ffold **out);
int ks_raligns_fold_frames(ks_ctx *ctx, const ks_hits *frame_hits, const uint64_t *d_nt_offsets, uint32_t n_records,
                           const ks_raligns *alignments, const ks_ffold_opts *opts, ks_hits **out_hits, ks_ffold **out);
uint64_t ks_ffold_n_rows(const ks_ffold *f);     /* folded rows */
uint64_t ks_ffold_n_regions(const ks_ffold *f);
uint64_t ks_ffold_n_src_rows(const ks_ffold *f); /* hit rows of the input */
/* device pointers, valid until ks_ffold_free */
const uint32_t *ks_ffold_device_src_row(const ks_ffold *f);
const uint64_t *ks_ffold_device_row_offsets(const ks_ffold *f);
const uint32_t *ks_ffold_device_src_region(const ks_ffold *f);
const uint8_t *ks_ffold_device_frame(const ks_ffold *f);
const uint32_t *ks_ffold_device_nt_length(const ks_ffold *f);
const uint32_t *ks_ffold_device_s_start(const ks_ffold *f);
const uint32_t *ks_ffold_device_nt_start(const ks_ffold *f);
const uint32_t *ks_ffold_device_t_start3(const ks_ffold *f);
const uint32_t *ks_ffold_device_t_length3(const ks_ffold *f);
const int64_t *ks_ffold_device_score(const ks_ffold *f);          /* NULL: the fold was made without that column, as the two below */
const uint32_t *ks_ffold_device_identities(const ks_ffold *f);
const uint32_t *ks_ffold_device_aln_length(const ks_ffold *f);
/* any destination may be NULL; the destination of a column the fold does not have is left as it is */
int ks_ffold_copy_to_host(ks_ctx *ctx, const ks_ffold *f, uint32_t *src_row, uint64_t *row_offsets, uint32_t *src_region,
                          uint8_t *frame, uint32_t *nt_length, uint32_t *s_start, uint32_t *nt_start, uint32_t *t_start3,
                          uint32_t *t_length3, int64_t *score, uint32_t *identities, uint32_t *aln_length);
void ks_ffold_free(ks_ffold *f);

/* ---- region stitch: the chain of a hit as ONE gapped alignment with one CIGAR ---------------------------------------------- */

/* What a seed-and-extend search closes its alignment stage with (minimap2 fills between chained anchors, BLAST links HSPs,
 * MMseqs2 realigns the diagonal range): the members of each hit row's chain keep their paths, what lies between two consecutive
 * members is aligned globally, and the row becomes one alignment — one CIGAR, one score, a PAF / SAM record.  All arithmetic is
 * in integers: the result is bit-exact against a host loop (tests/rstitch_ref.py).
 *   chain: a ks_rchain;  alignments: the ks_raligns it was computed from (the intended input: ks_raligns_take of the cull);
 *   cigars: the ks_cigars traced from exactly those alignments (the same regions in the same order);  hits and the two residue
 *   batches: what ks_regions_align took.  The matrix, gap_open = o and gap_extend = e are those recorded in `alignments`; its
 *   band and x_drop are not used.
 * Options: max_fill in [0, 4096], 0 means 1024;  flags: KS_RSTITCH_EQX;  max_scratch_bytes, 0 means 1 GiB;  reserved 0.
 * Per hit row the chain lists the members m_0 .. m_(k-1) (src_region, in chain order); an end is start + length.
 * Trim: for i >= 1, member i loses the smallest number c of leading columns such that the query position is >= q_end[m_(i-1)]
 *   and the target position is >= t_end[m_(i-1)] (the ORIGINAL ends of the member before it; tails are never trimmed; with the
 *   chain's max_overlap 0 nothing is trimmed).  c may be all of its columns: the member then contributes nothing and its end
 *   still stands.  The trimmed member starts at (q', t').
 * Link i: X = q' - q_end[m_(i-1)], Y = t' - t_end[m_(i-1)] (both >= 0).  X = Y = 0: nothing;  Y = 0: I x X;  X = 0: D x Y;
 *   min(X, Y) <= 63 and max(X, Y) <= max_fill: FILLED, below;  otherwise OPEN: I x X, then D x Y.
 * Fill: the recurrence of ks_regions_align (above: H~, F, D, E, H and every tie rule) on the whole rectangle — every cell
 *   0 <= x <= |Q|, 0 <= y <= |T| exists, no band, no X-drop — with the end cell (|Q|, |T|) walked back to (0, 0) by the rules of
 *   ks_regions_traceback.  T is the SHORTER stretch (X == Y: the target's), Q the longer.  A pair always scores
 *   M[class(query residue)][class(target residue)].  Where T is the target stretch an F step is I and an E jump of L is D x L;
 *   where T is the query stretch (roles swapped) an F step is D and an E jump of L is I x L.  The optimal score does not depend
 *   on the orientation, the choice among co-optimal paths does: the orientation is part of the contract.
 * Splice: the ops of m_0, link 1, the trimmed m_1, ...; adjacent equal ops merge, joints included (an I run beside a D run
 *   stays two ops).  The pairs of a fill are M; with KS_RSTITCH_EQX they are = / X by upper-cased byte equality, and the
 *   members' ops must then hold no M — without the flag no = or X.  An op is len << 4 | code, as in ks_cigars.
 * Result (device-resident): a CSR over the hit rows, op_offsets u64[n_rows + 1] and ops u32[n_ops], and per hit row the columns
 *   of that alignment, re-scored over the residues:
 *   q_start, q_length, t_start, t_length u32   from the first member's start to the last member's end: the chain's span
 *   score i64                = sum of M[pair] - sum over the I / D ops of (o + L * e)
 *   identities, positives, gap_opens (the I and D ops after merging), gaps, aln_length u32
 *   n_members, n_filled, n_open, n_trimmed (columns removed) u32
 *   row_score f64            (double)score, NaN for a row without members: a d_score column for ks_hits_best with
 *                            KS_BEST_SCORE and for the cluster passes
 *   A row without members has no ops and zeros.  A row of one member has that member's ops and exactly its alignment's columns.
 * The result never depends on the launch geometry, on ks_debug_rstitch_stage() or on max_scratch_bytes.
 * Scratch: 64 bytes per row of Q of every filled link (rounded up to an even number of rows).  max_scratch_bytes bounds it: the
 * members run in slices of consecutive members whose links fit.
 * KS_ERR_INVALID_ARG, before any device work and also with ctx == NULL: max_fill > 4096, unknown flags, a non-zero reserved
 * field.  Then: NULL arguments; an object of another context; row or region counts of chain, alignments, cigars and hits that
 * disagree.  Found on the device before anything is indexed by it, ks_last_error names the first offender: a src_region outside
 * its row's alignments; a qid / tid or sequence outside its batch; an extent outside its sequence; a member whose ops do not
 * consume exactly its q_length / t_length; the M / = / X mismatch; a member that ends before the member in front of it on
 * either sequence.
 * KS_ERR_CAPACITY: a single filled link whose directions do not fit max_scratch_bytes; what ks_regions_align refuses with it
 * (a chained hit row with a sequence of more than 2^20 residues).
 * One stream, synchronous on return, three host waits (the layout, the op count, the result); all memory comes from the
 * context's pool. */
typedef struct ks_hitalns ks_hitalns;
#define KS_RSTITCH_EQX 1u
#define KS_RSTITCH_MAX_FILL 4096u
typedef struct ks_rstitch_opts {
    uint32_t max_fill;          /* the longer side of a filled rectangle at most; 0: 1024; at most 4096 */
    uint32_t flags;             /* KS_RSTITCH_EQX */
    uint64_t max_scratch_bytes; /* direction scratch of one slice; 0: 1 GiB */
    uint32_t reserved[2];       /* 0 */
} ks_rstitch_opts;
/* opts == NULL: the defaults */
int ks_regions_stitch(ks_ctx *ctx, const ks_rchain *chain, const ks_raligns *alignments, const ks_cigars *cigars, const ks_hits *hits,
                      const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res,
                      const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res,
                      const ks_rstitch_opts *opts, ks_hitalns **out);
uint64_t ks_hitalns_n_rows(const ks_hitalns *a);
uint64_t ks_hitalns_n_ops(const ks_hitalns *a);
/* diagnostic: the direction scratch the call allocated, and the slices it ran in */
uint64_t ks_hitalns_scratch_bytes(const ks_hitalns *a);
uint32_t ks_hitalns_n_slices(const ks_hitalns *a);
/* device pointers, valid until ks_hitalns_free */
const uint64_t *ks_hitalns_device_op_offsets(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_ops(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_q_start(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_q_length(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_t_start(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_t_length(const ks_hitalns *a);
const int64_t *ks_hitalns_device_score(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_identities(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_positives(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_gap_opens(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_gaps(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_aln_length(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_n_members(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_n_filled(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_n_open(const ks_hitalns *a);
const uint32_t *ks_hitalns_device_n_trimmed(const ks_hitalns *a);
const double *ks_hitalns_device_row_score(const ks_hitalns *a);
/* any destination may be NULL */
int ks_hitalns_copy_to_host(ks_ctx *ctx, const ks_hitalns *a, uint64_t *op_offsets, uint32_t *ops, uint32_t *q_start, uint32_t *q_length,
                            uint32_t *t_start, uint32_t *t_length, int64_t *score, uint32_t *identities, uint32_t *positives,
                            uint32_t *gap_opens, uint32_t *gaps, uint32_t *aln_length, uint32_t *n_members, uint32_t *n_filled,
                            uint32_t *n_open, uint32_t *n_trimmed, double *row_score);
void ks_hitalns_free(ks_hitalns *a);
/* rows of directions one wave stages at once for the walk of a fill: the tests place rectangles around it */
uint32_t ks_debug_rstitch_stage(void);

/* ---- frame stitch: the chain of a translated hit as ONE alignment of the strand's bases, frameshifts marked ------------------ */

/* What a translated search is run for (blastx, DIAMOND -F): per (record strand, protein) one alignment of the strand's bases
 * against the protein, the frameshift marked at its place and paid for in the score.  The chain of ks_regions_chain_device on a
 * ks_ffold links alignments that lie in different frames; this pass joins their traced paths across the frames into one CIGAR
 * in codon columns and re-scores it over the residues.  All arithmetic is in integers: the result is bit-exact against a host
 * loop (tests/fstitch_ref.py).
 *   fold: a ks_ffold made from gapped alignments (ks_raligns_fold_frames);  folded_hits: the fold's hit list (qid = 2 record +
 *   strand, tid);  chain: the ks_rchain of the fold's columns (one row per folded row, src_region indexes the folded regions);
 *   alignments: the ks_raligns the fold was made of (fold.src_region indexes it: typically ks_raligns_take of the cull);
 *   cigars: the ks_cigars traced from exactly those alignments;  the frame batch: the residues of ks_translate6_device (6 n
 *   sequences, what ks_regions_align took as queries);  the target batch.  The matrix, gap_open = o and gap_extend = e are those
 *   recorded in `alignments`.
 * Options: max_fill in [0, 4096], 0 means 1024;  flags: KS_RSTITCH_EQX;  frameshift_cost, taken as given, at most 2^16 (the
 *   caller's parameter like the matrix; opts == NULL: 15, the value DIAMOND's manual suggests for -F);  max_scratch_bytes, 0
 *   means 1 GiB;  reserved 0.
 * Coordinates: a strand base position p reads the codon that is residue p / 3 of frame sequence 6 record + 3 strand + p % 3
 *   (the fold's s_start = f + 3 q_start with f < 3: one rule addresses every frame).  An end is start + length.
 * Trim (the rule of ks_regions_stitch, in bases): member i >= 1 loses the fewest leading columns such that its strand position is
 *   >= the ORIGINAL strand end s_start + nt_length of member i - 1 and its target position >= that member's original target end;
 *   a query-consuming column moves the strand position by 3.  Tails are never trimmed; a member may lose every column, its end
 *   still stands.  A backward shift therefore shows as a trimmed codon followed by a forward skip.
 * Link i: E, T_e the previous member's original ends, (p', t') the trimmed member's start; X = p' - E bases, Y = t' - T_e
 *   residues, c = X / 3, r = X % 3 (r != 0 exactly when the two members' frames differ).  Two parts:
 *   1. the protein link of ks_regions_stitch on the rectangle (c, Y) — nothing, I x c, D x Y, FILLED (min <= 63, max <= max_fill;
 *      the same orientation and tie rules) or OPEN (I x c, then D x Y) — whose query stretch is the c codons read in the PREVIOUS
 *      member's frame directly after its end: residues [E / 3, E / 3 + c) of frame E % 3;
 *   2. if r != 0, ONE frameshift op of length r directly before the next member: r strand bases skipped, no codon, no target
 *      residue, BAM code 3 (N), KS_CIGAR_FSHIFT.
 *   The pass does NOT search for the best place of the shift inside a link.
 * Splice: the ops of m_0, link 1, the trimmed m_1, ...; adjacent equal ops merge across joints; an N op never merges with
 *   anything, another N included.  KS_RSTITCH_EQX as in ks_regions_stitch.  M, = and X are one codon against one residue, I a
 *   codon without a residue, D a residue without a codon:  3 (pairs + I) + sum of N = nt_length,  pairs + D = t_length.
 *   Worked examples (a gene of n codons, its two parts aligned in two frames, no chance match beside the shift):
 *     one base inserted after codon m      X = 1, Y = 0            mM 1N (n - m)M
 *     one base of codon m deleted          X = 2, Y = 1, c = 0     mM 1D 2N (n - m - 1)M
 * Result (device-resident): a CSR over the folded rows, op_offsets u64[n_rows + 1] and ops u32[n_ops] (len << 4 | code), and per
 *   folded row:
 *   s_start, nt_length u32     strand bases: the first member's start to the last member's end
 *   nt_start u32               bases on the record as given: the first member's nt_start on strand 0, the last member's on strand 1
 *   t_start, t_length u32      residues of the target
 *   score i64                  = sum of M[pair] - sum over the I / D ops of (o + L e) - frameshift_cost x (number of N ops)
 *   identities, positives, gap_opens (I and D ops), gaps (their columns), aln_length (columns; N is not counted) u32
 *   n_members, n_filled, n_open, n_trimmed (columns removed), n_frameshifts (N ops) u32
 *   row_score f64              (double)score, NaN for a row without members: a d_score column for ks_hits_best on folded_hits
 *   A row whose chain lies in one frame has no N op: its ops, score and counts are what ks_regions_stitch gives for the same
 *   members on that frame's residues.  A row without members has no ops and zeros.
 * The result never depends on the launch geometry, on ks_debug_rstitch_stage() or on max_scratch_bytes.  Scratch as in
 * ks_regions_stitch: 64 bytes per row of the longer side of every filled link, in slices that fit max_scratch_bytes.
 * KS_ERR_INVALID_ARG, before any device work and also with ctx == NULL: max_fill > 4096, frameshift_cost > 2^16, unknown flags,
 * a non-zero reserved field.  Then: NULL arguments; an object of another context; row or region counts of fold, chain, folded
 * hits, alignments and cigars that disagree.  Found on the device before anything is indexed by it, ks_last_error names the
 * first offender: a chain src_region outside its folded row's regions; a fold src_region >= the alignments' region count; a fold
 * that is not of these alignments (s_start != frame % 3 + 3 q_start, nt_length != 3 q_length, t_start3 != 3 t_start, t_length3
 * != 3 t_length); frame / 3 != qid & 1; a frame sequence id >= n_f or a tid >= n_t or a sequence outside its batch; an extent
 * outside its sequence; ops that do not consume exactly the member's extents; the M / = / X mismatch; a member that ends before
 * the member in front of it on the strand or the target.
 * KS_ERR_CAPACITY: a chained row with a frame or target sequence of more than 2^20 residues; one filled link whose directions
 * do not fit max_scratch_bytes.
 * A refused call leaves no object and nothing held in the pool.  One stream, synchronous on return, three host waits.
 * Not built: the search for the best shift position inside a link; genetic codes other than table 1; E-values of the stitched
 * alignment; members without traced paths (ungapped ks_rscores); folding both strands. */
typedef struct ks_framealns ks_framealns;
#define KS_CIGAR_FSHIFT 3u
#define KS_FSTITCH_MAX_COST 65536u
typedef struct ks_fstitch_opts {
    uint32_t max_fill;          /* the longer side of a filled rectangle at most; 0: 1024; at most 4096 */
    uint32_t flags;             /* KS_RSTITCH_EQX */
    uint32_t frameshift_cost;   /* subtracted per N op; at most 65536 */
    uint32_t reserved;          /* 0 */
    uint64_t max_scratch_bytes; /* direction scratch of one slice; 0: 1 GiB */
} ks_fstitch_opts;
/* opts == NULL: the defaults, frameshift_cost 15 */
int ks_frames_stitch(ks_ctx *ctx, const ks_ffold *fold, const ks_hits *folded_hits, const ks_rchain *chain, const ks_raligns *alignments,
                     const ks_cigars *cigars, const uint8_t *d_f_res, const uint64_t *d_f_offs, uint32_t n_f, uint64_t n_f_res,
                     const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res, const ks_fstitch_opts *opts,
                     ks_framealns **out);
uint64_t ks_framealns_n_rows(const ks_framealns *a);
uint64_t ks_framealns_n_ops(const ks_framealns *a);
/* diagnostic: the direction scratch the call allocated, and the slices it ran in */
uint64_t ks_framealns_scratch_bytes(const ks_framealns *a);
uint32_t ks_framealns_n_slices(const ks_framealns *a);
/* device pointers, valid until ks_framealns_free */
const uint64_t *ks_framealns_device_op_offsets(const ks_framealns *a);
const uint32_t *ks_framealns_device_ops(const ks_framealns *a);
const uint32_t *ks_framealns_device_s_start(const ks_framealns *a);
const uint32_t *ks_framealns_device_nt_length(const ks_framealns *a);
const uint32_t *ks_framealns_device_nt_start(const ks_framealns *a);
const uint32_t *ks_framealns_device_t_start(const ks_framealns *a);
const uint32_t *ks_framealns_device_t_length(const ks_framealns *a);
const int64_t *ks_framealns_device_score(const ks_framealns *a);
const uint32_t *ks_framealns_device_identities(const ks_framealns *a);
const uint32_t *ks_framealns_device_positives(const ks_framealns *a);
const uint32_t *ks_framealns_device_gap_opens(const ks_framealns *a);
const uint32_t *ks_framealns_device_gaps(const ks_framealns *a);
const uint32_t *ks_framealns_device_aln_length(const ks_framealns *a);
const uint32_t *ks_framealns_device_n_members(const ks_framealns *a);
const uint32_t *ks_framealns_device_n_filled(const ks_framealns *a);
const uint32_t *ks_framealns_device_n_open(const ks_framealns *a);
const uint32_t *ks_framealns_device_n_trimmed(const ks_framealns *a);
const uint32_t *ks_framealns_device_n_frameshifts(const ks_framealns *a);
const double *ks_framealns_device_row_score(const ks_framealns *a);
/* any destination may be NULL */
int ks_framealns_copy_to_host(ks_ctx *ctx, const ks_framealns *a, uint64_t *op_offsets, uint32_t *ops, uint32_t *s_start, uint32_t *nt_length,
                              uint32_t *nt_start, uint32_t *t_start, uint32_t *t_length, int64_t *score, uint32_t *identities,
                              uint32_t *positives, uint32_t *gap_opens, uint32_t *gaps, uint32_t *aln_length, uint32_t *n_members,
                              uint32_t *n_filled, uint32_t *n_open, uint32_t *n_trimmed, uint32_t *n_frameshifts, double *row_score);
void ks_framealns_free(ks_framealns *a);

/* ---- coverage: per-residue depth and profile of many alignments, per-sequence breadth ---------------------------------------- */

/* What the alignments are for once there are many of them: taken together, what do they say about a sequence?  Every pass above
 * works inside one hit row; this one reduces ACROSS the rows onto the residues of one batch — the breadth-of-coverage filter of a
 * read-to-protein pipeline ("is this protein present" is how much of it the reads cover, and how deep), the per-position depth
 * that shows a query's domains, and the per-position residue counts that every conservation score, consensus or PSSM starts
 * from.  Everything but the two quotients is an integer and exact (tests/pileup_ref.py restates it in plain loops).
 *   The call takes ENTRIES.  An entry is a run of CIGAR ops (len << 4 | BAM code, the query as the read, as in ks_cigars) that
 *   belongs to a hit row (qid, tid) of `hits`, with a start position on each side, counted from the sequence's first residue.
 *   A SIDE is chosen, KS_PILEUP_QUERY or KS_PILEUP_TARGET: the entry's sequence is qid or tid of its row in that side's batch;
 *   the OTHER side is the remaining one.
 * How the ops consume the two sides:
 *   M, =, X   PAIR COLUMNS: one residue on both sides
 *   I         the query only;      D   the target only
 *   N         (code 3, KS_CIGAR_FSHIFT) nothing on the target.  On the query side it stands for skipped bases of a strand, which
 *             no residue batch holds: N is legal only where the query side is not read — side == KS_PILEUP_TARGET without the
 *             profile.
 *   An op of length 0 consumes nothing and covers nothing.
 * Per residue p of the side's batch (n_residues of them, batch coordinates offsets[seq] + position):
 *   depth[p] u32            the pair columns, over all entries taken, that place p.  An entry places a residue at most once;
 *                           entries of one row that overlap each count.
 *   counts[p * 28 + c] u32  with KS_PILEUP_PROFILE: those columns whose residue on the OTHER side has class c — the 28 classes of
 *                           ks_residue_composition_device and the score matrices (A..Z without case, '*', everything else).
 *                           For every p the 28 counts sum to depth[p].  Without the flag the column has no entries
 *                           (ks_pileup_n_profile == 0).
 * Per sequence s of the side's batch (n_seqs):
 *   length u32;  n_alignments u32  entries taken with at least one pair column on s;  covered u32  positions with depth > 0;
 *   max_depth u32;  depth_sum u64;  breadth f64 = covered / length;  mean_depth f64 = depth_sum / length — both the correctly
 *   rounded f64 quotient of the two integers (what numpy gives), NaN for an empty sequence.
 * Worked examples (one entry, starts 0, depth of the side):
 *   2M1I2M   query side: 5 residues, depth 1 1 0 1 1 (the inserted residue has no column);  target side: 4 residues, 1 1 1 1
 *   2M1D2M   query side: 4 residues, 1 1 1 1;  target side: 5 residues, 1 1 0 1 1
 *   41M1N59M target side: 100 residues of depth 1 — the N moves nothing there
 * Arguments of ks_pileup_device:
 *   d_row_offsets u64[n_rows + 1]: the CSR of the entries over the hit rows, or NULL: one entry per row (n_entries == n_rows);
 *   d_op_offsets u64[n_entries + 1], d_ops u32[n_ops]: the CSR of the ops over the entries;
 *   d_start u32[n_entries]: the entries' starts on the chosen side;  d_other_start: on the other side (profile only, else NULL);
 *   d_row_mask u8[n_rows] or NULL: the entries of a row with 0 are skipped (nothing of them is read: a top-k selection of rows);
 *   hits: n_rows rows, read for qid and tid;  d_offsets, n_seqs, n_res: the side's batch (its residues are not read);
 *   d_o_res, d_o_offsets, n_o_seqs, n_o_res: the other batch (profile only, else NULL / 0).
 * The result never depends on the launch geometry, on the order the entries are processed in or on an internal path: every add
 * is an integer add (KS_DEBUG_PILEUP_PATH = 1 / 2 send every sequence's reduction to a wave / to a workgroup, for the tests).
 * KS_ERR_INVALID_ARG, options first, before any device work and also with ctx == NULL: unknown flags, a side that is neither,
 * a non-zero reserved, KS_PILEUP_PROFILE without the other batch or without d_other_start.  Then: NULL arguments; an object of
 * another context; n_rows that is not the hit list's row count; entries without rows.  Then KS_ERR_CAPACITY: n_res >= 2^32 - 1
 * (one 32-bit scan takes fewer), 2^32 - 2 or more rows or entries, more than 2^32 - 1 ops.  Then, found on the device before
 * anything is indexed by it, the first kind that occurs, its lowest index named in ks_last_error:
 *   a row CSR, then op offsets, that descend or do not end at their count (the index of the offset);
 *   a hit row whose id lies beyond its batch (the other batch only with the profile);
 *   an entry with an op code outside M I D N = X, or an N where the query side is read;
 *   an entry whose ops consume more of either sequence than it has from its start (the other side only with the profile);
 *   an entry on a sequence whose offsets descend or pass its batch;  a sequence of the side's batch with such offsets.
 * Whatever the inputs hold, nothing is read or written outside the batches, the entries and the result's arrays.  A refused
 * call leaves no object and nothing held in the pool.  One stream, synchronous on return, one host wait.  Scratch from the
 * pool: 8 bytes per residue of the side's batch and 8 per sequence.
 * Not built: depth in bases on the query side of frame alignments.  (Weights per entry — Henikoff's, a score, an abundance —
 * and the pileup that sums them: ks_wpileup_device, below.  Consensus and PSSM columns from the counts:
 * ks_profile_build_device, below.) */
typedef struct ks_pileup ks_pileup;
#define KS_PILEUP_QUERY   0u
#define KS_PILEUP_TARGET  1u
#define KS_PILEUP_PROFILE 1u /* flags: also counts[p][class of the other side's residue] */
typedef struct ks_pileup_opts {
    uint32_t flags;    /* KS_PILEUP_PROFILE */
    uint32_t side;     /* KS_PILEUP_QUERY | KS_PILEUP_TARGET */
    uint64_t reserved; /* 0 */
} ks_pileup_opts;
/* opts == NULL: the depth of the query side */
int ks_pileup_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint64_t *d_op_offsets, const uint32_t *d_ops, uint64_t n_rows,
                     uint64_t n_entries, uint64_t n_ops, const uint32_t *d_start, const uint32_t *d_other_start, const uint8_t *d_row_mask,
                     const ks_hits *hits, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res,
                     const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res,
                     const ks_pileup_opts *opts, ks_pileup **out);
/* The three kinds of alignments the passes above make, piled up (thin wrappers, as ks_rscores_stats over ks_scores_stats_device).
 * ks_cigars_pileup: the entries are the regions of `cigars`; the row CSR and the starts come from `alignments`, the ks_raligns
 * they were traced from (equal counts).  ks_hitalns_pileup: one entry per hit row, the stitched alignment; a row without members
 * has no ops and adds nothing.  ks_frames_pileup: one entry per folded row of a translated search on `fold_hits`, TARGET SIDE
 * ONLY — M and D move the protein by one, I and N by nothing; KS_PILEUP_QUERY and KS_PILEUP_PROFILE are refused by name with the
 * options (depth in bases on a strand is not built). */
int ks_cigars_pileup(ks_ctx *ctx, const ks_cigars *cigars, const ks_raligns *alignments, const ks_hits *hits, const uint8_t *d_row_mask,
                     const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets,
                     uint32_t n_o_seqs, uint64_t n_o_res, const ks_pileup_opts *opts, ks_pileup **out);
int ks_hitalns_pileup(ks_ctx *ctx, const ks_hitalns *stitched, const ks_hits *hits, const uint8_t *d_row_mask, const uint64_t *d_offsets,
                      uint32_t n_seqs, uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs,
                      uint64_t n_o_res, const ks_pileup_opts *opts, ks_pileup **out);
int ks_frames_pileup(ks_ctx *ctx, const ks_framealns *frame_alignments, const ks_hits *fold_hits, const uint8_t *d_row_mask,
                        const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res, const ks_pileup_opts *opts, ks_pileup **out);
uint32_t ks_pileup_n_seqs(const ks_pileup *p);
uint64_t ks_pileup_n_residues(const ks_pileup *p);
/* entries of `counts`: 28 x n_residues with KS_PILEUP_PROFILE, else 0 */
uint64_t ks_pileup_n_profile(const ks_pileup *p);
/* device pointers, valid until ks_pileup_free */
const uint32_t *ks_pileup_device_depth(const ks_pileup *p);
const uint32_t *ks_pileup_device_counts(const ks_pileup *p);
const uint32_t *ks_pileup_device_length(const ks_pileup *p);
const uint32_t *ks_pileup_device_n_alignments(const ks_pileup *p);
const uint32_t *ks_pileup_device_covered(const ks_pileup *p);
const uint32_t *ks_pileup_device_max_depth(const ks_pileup *p);
const uint64_t *ks_pileup_device_depth_sum(const ks_pileup *p);
const double *ks_pileup_device_breadth(const ks_pileup *p);
const double *ks_pileup_device_mean_depth(const ks_pileup *p);
/* any destination may be NULL */
int ks_pileup_copy_to_host(ks_ctx *ctx, const ks_pileup *p, uint32_t *depth, uint32_t *counts, uint32_t *length, uint32_t *n_alignments,
                           uint32_t *covered, uint32_t *max_depth, uint64_t *depth_sum, double *breadth, double *mean_depth);
void ks_pileup_free(ks_pileup *p);
/* the longest sequence a wave reduces; a longer one goes to a workgroup (the tests place sequences around it) */
void ks_debug_pileup_limits(uint32_t *wave_max);

/* ---- sequence weights: one weight per entry of a pileup, and the pileup that sums them ---------------------------------------- */

/* 312 near-copies of one homolog piled up on a query say one thing 312 times.  The two passes here let a profile count them as
 * what they are: ks_entry_weights_device gives every entry a weight that is small where the entry agrees with many others,
 * ks_wpileup_device sums such weights — or any others: a score, an abundance — where the pileup counts entries.
 * A weight is a u32 in units of 2^-30: KS_WEIGHT_ONE is the weight 1.  All of it is integer arithmetic and exact
 * (tests/pweights_ref.py restates it in plain loops).  For every argument the passes share with ks_pileup_device the contract is
 * that call's, word for word: the entries, the hit list, the mask, the side and the batches, the refusals in their order and
 * the offender they name.
 *
 * ks_entry_weights_device: position-based (Henikoff) weights, adapted to local alignments; the rule is this project's own.
 *   It reads the other side as a pileup with KS_PILEUP_PROFILE does (the other batch and d_other_start are needed), and
 *   d_counts u32[n_res * 28]: the counts of an unweighted pileup with KS_PILEUP_PROFILE of the SAME entries, mask and side.
 *   flags: KS_PWEIGHTS_INCLUDE_QUERY — the sequence the entries lie on is one more member of each of its columns; d_res, the
 *   side's residues, is then read (else it may be NULL).
 *   Per residue p of the side's batch:  cnt[j] = counts[p * 28 + j];  with the flag cnt[class(res[p])] += 1;
 *     k_p = #{j of all 28 : cnt[j] > 0}.
 *   Per entry e that is TAKEN — its row is not masked, its ops passed the pileup's judgement, it has np_e >= 1 pair columns:
 *     S_e = sum over its pair columns (p, c = the class of the other side's residue) of floor(KS_WEIGHT_ONE / ((u64)k_p * cnt[c])),
 *           a u64 sum of u64 integer divisions (a term may be 0);
 *     weight[e] = (u32)(S_e / np_e), the mean column term;  n_cols[e] = np_e.
 *     weight[e] <= KS_WEIGHT_ONE, with equality exactly when the entry is alone in each of its columns.
 *   An entry that is not taken has weight 0 and n_cols 0; nothing of a masked row is read.
 *   Worked example: query side, query ACDE, three entries 4M at start 0 against ACDE, ACDE, AGDK, no flag.  Columns 0 and 2:
 *   k = 1, cnt = 3, every term 357913941.  Columns 1 and 3: k = 2; cnt = 2 for the two that agree, 268435456 each; cnt = 1 for
 *   the odd one, 536870912.  S = 1252698794, 1252698794, 1789569706;  weight = 313174698, 313174698, 447392426.
 *   Refused as ks_pileup_device refuses, in its order; unknown flags with the options; a NULL d_counts, or a NULL d_res with the
 *   flag, with the NULL arguments.  Then, found on the device: a taken entry with a column whose cnt[c] is 0 — the counts were
 *   not made from these entries — KS_ERR_INVALID_ARG, the lowest such entry named.  A refused call leaves no object and nothing
 *   held in the pool.  One host wait.  Scratch: one byte per residue of the side's batch.
 * ks_cigars_pileup_weights: the same for the regions of `cigars` (with the `alignments` they were traced from) and the `pileup`
 *   made from them, which must hold counts and be of the side's batch.
 *
 * ks_wpileup_device, ks_cigars_pileup_weighted, ks_hitalns_pileup_weighted: their siblings' arguments and d_weight
 *   u32[n_entries] (NULL only without entries).  Every column of the unweighted call is made, identically, and
 *   wdepth[p] u64            the sum of the weights of the entries that place p (an entry counts once per column it places p in);
 *   wcounts[p * 28 + c] u64  with KS_PILEUP_PROFILE: the same by the class of the other side's residue; the 28 sum to wdepth[p].
 *   An entry of weight 0 adds to the unweighted columns and not to these.  Fewer than 2^32 entries of a u32 weight cannot wrap
 *   a u64; the adds are 64-bit integer atomics, no order shows.  ks_wpileup_n_weighted: the entries of wdepth, 0 for an object
 *   of the unweighted entry points (whose wdepth and wcounts pointers are NULL).  ks_frames_pileup has no weighted form.
 * (The functions that take a ks_pileup here are named ks_wpileup_*: what a weighted pileup has beyond ks_pileup_*.) */
typedef struct ks_pweights ks_pweights;
#define KS_WEIGHT_ONE (1u << 30)
#define KS_PWEIGHTS_INCLUDE_QUERY 1u
int ks_entry_weights_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint64_t *d_op_offsets, const uint32_t *d_ops, uint64_t n_rows,
                             uint64_t n_entries, uint64_t n_ops, const uint32_t *d_start, const uint32_t *d_other_start, const uint8_t *d_row_mask,
                             const ks_hits *hits, const uint8_t *d_res, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res,
                             const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res, const uint32_t *d_counts,
                             uint32_t side, uint32_t flags, ks_pweights **out);
int ks_cigars_pileup_weights(ks_ctx *ctx, const ks_cigars *cigars, const ks_raligns *alignments, const ks_pileup *pileup, const ks_hits *hits,
                             const uint8_t *d_row_mask, const uint8_t *d_res, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res,
                             const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res, uint32_t side, uint32_t flags,
                             ks_pweights **out);
uint64_t ks_pweights_n_entries(const ks_pweights *w);
/* device pointers, valid until ks_pweights_free */
const uint32_t *ks_pweights_device_weight(const ks_pweights *w);
const uint32_t *ks_pweights_device_n_cols(const ks_pweights *w);
/* any destination may be NULL */
int ks_pweights_copy_to_host(ks_ctx *ctx, const ks_pweights *w, uint32_t *weight, uint32_t *n_cols);
void ks_pweights_free(ks_pweights *w);
int ks_wpileup_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const uint64_t *d_op_offsets, const uint32_t *d_ops, uint64_t n_rows,
                              uint64_t n_entries, uint64_t n_ops, const uint32_t *d_start, const uint32_t *d_other_start, const uint8_t *d_row_mask,
                              const ks_hits *hits, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res,
                              const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs, uint64_t n_o_res,
                              const uint32_t *d_weight, const ks_pileup_opts *opts, ks_pileup **out);
int ks_cigars_pileup_weighted(ks_ctx *ctx, const ks_cigars *cigars, const ks_raligns *alignments, const ks_hits *hits, const uint8_t *d_row_mask,
                              const uint64_t *d_offsets, uint32_t n_seqs, uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets,
                              uint32_t n_o_seqs, uint64_t n_o_res, const uint32_t *d_weight, const ks_pileup_opts *opts, ks_pileup **out);
int ks_hitalns_pileup_weighted(ks_ctx *ctx, const ks_hitalns *stitched, const ks_hits *hits, const uint8_t *d_row_mask, const uint64_t *d_offsets,
                               uint32_t n_seqs, uint64_t n_res, const uint8_t *d_o_res, const uint64_t *d_o_offsets, uint32_t n_o_seqs,
                               uint64_t n_o_res, const uint32_t *d_weight, const ks_pileup_opts *opts, ks_pileup **out);
uint64_t ks_wpileup_n_weighted(const ks_pileup *p);
const uint64_t *ks_wpileup_device_wdepth(const ks_pileup *p);
const uint64_t *ks_wpileup_device_wcounts(const ks_pileup *p);
/* wdepth u64[n_weighted], wcounts u64[28 x n_weighted with the profile, else 0]; any destination may be NULL */
int ks_wpileup_copy_to_host(ks_ctx *ctx, const ks_pileup *p, uint64_t *wdepth, uint64_t *wcounts);

/* ---- position-specific scores: a profile of the query batch, and the region passes against it ------------------------------- */

/* The counts of a query-side pileup (KS_PILEUP_PROFILE) made into one row of 28 scores per query residue, and the three region
 * passes run against those rows where they took a matrix: M[class(Q_x)][class(T_y)] becomes P[position of Q_x][class(T_y)].
 * A candidate that a reduced-alphabet seed brought in and a BLOSUM row scores poorly is re-scored by what the query's confident
 * alignments say about each of its positions.  Seeding stays exact k-mer matching.
 *
 * The build rule is this project's own, in committed constants and a fixed order of f64 operations, bit-exact against a host
 * loop (tests/profile_ref.py).  No log or exp runs on the device: the caller brings the likelihood ratios R and a table of
 * ascending thresholds, and a score is the number of thresholds at or below the position's ratio r.
 * ks_profile_opts, all HOST data:
 *   matrix      int8[28][28], the fallback (NULL: +1 / -1);  bg f64[28], each >= 0: a class with bg == 0 is UNMODELLED;
 *   ratio       f64[28][28], R[j][c];  beta f64 >= 0, the weight of the pseudo-counts;
 *   thresholds  f64[n_thr], strictly ascending, n_thr <= KS_PROFILE_MAX_THRESHOLDS;  base i32;
 *   flags       KS_PROFILE_INCLUDE_QUERY;  reserved 0.
 * Per residue p of the batch, a = the class of q_res[p], J = the modelled classes, cnt[j] = counts[p * 28 + j]:
 *   n0 = sum over j in J of cnt[j] (u64).  n0 == 0: the row is matrix[a][.], n_obs[p] = 0.
 *   Otherwise, with KS_PROFILE_INCLUDE_QUERY and a in J, cnt[a] += 1;  n = sum over J of cnt;  n_obs[p] = min(n, 2^32 - 1).
 *   c not in J: scores[p][c] = matrix[a][c].
 *   c in J, in f64, every operation rounded on its own (no fused multiply-add), in exactly this order:
 *     g = sum over j in J, ascending, of (f64)cnt[j] * R[j][c], from 0.0;  t = g / (f64)n;  t = bg[c] * t;  t = beta * t;
 *     num = (f64)cnt[c] + t;  den = (f64)n + beta;  r = (num / den) / bg[c];
 *     scores[p][c] = clamp(base + #{k : thresholds[k] <= r}, -127, 127)        (a NaN r is at or above no threshold)
 *   consensus[p]: depth[p] == 0: the residue's own byte, ASCII upper-cased.  Otherwise the class with the largest count once the
 *     residue's own class has been counted once more (all 28 classes, whatever the flag), ties to the smaller class, as that
 *     class's letter: 'A' .. 'Z', '*', and 'X' for class 27.
 * Result: scores int8[n_residues * 28] (the accessor and copy_to_host hand them out as bytes), consensus u8[n_residues],
 * n_obs u32[n_residues]; the object records the fallback matrix.
 * ks_profile_build_device: d_counts u32[n_q_res * 28] and d_depth u32[n_q_res] as ks_pileup_device makes them on the query side,
 * the query batch (d_q_res, d_q_offs u64[n_q + 1], n_q, n_q_res).  ks_profile_build_pileup: the same from a ks_pileup that was
 * made with KS_PILEUP_PROFILE on a batch of n_q sequences and n_q_res residues.  ks_profile_from_host: a profile whose rows the
 * caller brings (scores int8[n_q_res * 28]; consensus, n_obs: NULL for zeros; matrix: the fallback to record, NULL: +1 / -1).
 * KS_ERR_INVALID_ARG, in this order: the options, before any device work and also with ctx == NULL — unknown flags, a non-zero
 * reserved, thresholds that do not ascend strictly, a NaN among bg, ratio, beta or the thresholds, a negative bg or beta, n_thr
 * beyond the maximum, a missing bg, ratio or (n_thr != 0) thresholds;  NULL pointers, an object of another context, a pileup
 * without the profile or of another batch;  n_q_res that is not d_q_offs[n_q] (read before anything is indexed by it).  A
 * refused call leaves no object.  One stream, synchronous on return. */
typedef struct ks_profile ks_profile;
#define KS_PROFILE_INCLUDE_QUERY 1u
#define KS_PROFILE_MAX_THRESHOLDS 254u
typedef struct ks_profile_opts {
    const int8_t *matrix;     /* host, [28][28] or NULL */
    const double *bg;         /* host, [28] */
    const double *ratio;      /* host, [28][28] */
    double beta;
    const double *thresholds; /* host, [n_thr] */
    uint32_t n_thr;
    int32_t base;
    uint32_t flags;           /* KS_PROFILE_INCLUDE_QUERY */
    uint32_t reserved;        /* 0 */
} ks_profile_opts;
int ks_profile_build_device(ks_ctx *ctx, const uint32_t *d_counts, const uint32_t *d_depth, const uint8_t *d_q_res, const uint64_t *d_q_offs,
                            uint32_t n_q, uint64_t n_q_res, const ks_profile_opts *opts, ks_profile **out);
int ks_profile_build_pileup(ks_ctx *ctx, const ks_pileup *pileup, const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q,
                            uint64_t n_q_res, const ks_profile_opts *opts, ks_profile **out);
int ks_profile_from_host(ks_ctx *ctx, const int8_t *scores, const uint8_t *consensus, const uint32_t *n_obs, uint32_t n_q, uint64_t n_q_res,
                         const int8_t *matrix, ks_profile **out);
uint32_t ks_profile_n_seqs(const ks_profile *p);
uint64_t ks_profile_n_residues(const ks_profile *p);
/* entries of `scores`: 28 x n_residues */
uint64_t ks_profile_n_scores(const ks_profile *p);
/* device pointers, valid until ks_profile_free.  scores: the int8 values as the bytes they are (every column accessor of the
 * result objects is one of five unsigned / 64-bit element types): read them as int8_t */
const uint8_t *ks_profile_device_scores(const ks_profile *p);
const uint8_t *ks_profile_device_consensus(const ks_profile *p);
const uint32_t *ks_profile_device_n_obs(const ks_profile *p);
/* any destination may be NULL */
int ks_profile_copy_to_host(ks_ctx *ctx, const ks_profile *p, uint8_t *scores, uint8_t *consensus, uint32_t *n_obs);
void ks_profile_free(ks_profile *p);

/* The WEIGHTED build: the same options, rows, consensus and n_obs from a weighted pileup of the query side — counts, wcounts
 * (ks_wpileup_device with KS_PILEUP_PROFILE, e.g. under the weights of ks_entry_weights_device) and depth.  The
 * observed frequencies are the weighted ones, and the amount of evidence behind them is k, the number of distinct classes seen
 * at the column, not the number of sequences: 312 copies of one residue are one observation against beta.
 * Per residue p, a = the class of q_res[p], J = the modelled classes, cnt[j] = counts[p * 28 + j]:
 *   n0 = sum over j in J of cnt[j] (u64).  n0 == 0: the row is matrix[a][.], n_obs[p] = 0.
 *   Otherwise, with KS_PROFILE_INCLUDE_QUERY and a in J, cnt[a] += 1;  n = sum over J of cnt;  k = #{j in J : cnt[j] > 0};
 *   W_j = wcounts[p * 28 + j] (u64), and with the flag and a in J  W_a += floor(KS_WEIGHT_ONE / ((u64)k * cnt[a])), the query's
 *   own column term;  W = sum over J of W_j, an exact u64.  W == 0: the row is matrix[a][.], n_obs[p] = 0.
 *   Else n_obs[p] = min(n, 2^32 - 1).  c not in J: scores[p][c] = matrix[a][c].
 *   c in J, in f64, every operation rounded on its own (no fused multiply-add), in exactly this order:
 *     x_j = ((f64)W_j / (f64)W) * (f64)k  for j in J;
 *     g = sum over j in J, ascending, of x_j * R[j][c], from 0.0;  t = g / (f64)k;  t = bg[c] * t;  t = beta * t;
 *     num = x_c + t;  den = (f64)k + beta;  r = (num / den) / bg[c];
 *     scores[p][c] = clamp(base + #{k' : thresholds[k'] <= r}, -127, 127)       (a NaN r is at or above no threshold)
 *   consensus[p]: depth[p] == 0: the residue's own byte, ASCII upper-cased.  Otherwise, over all 28 classes and whatever the
 *     flag: cq[j] = counts[p * 28 + j], cq[a] += 1;  kq = #{j : cq[j] > 0};  V_j = wcounts[p * 28 + j],
 *     V_a += floor(KS_WEIGHT_ONE / ((u64)kq * cq[a])) — the query's column term under ks_entry_weights_device's rule with
 *     KS_PWEIGHTS_INCLUDE_QUERY;  the class with the largest V, ties to the smaller class, as that class's letter.
 * ks_profile_build_weighted_device: d_counts u32[n_q_res * 28], d_wcounts u64[n_q_res * 28], d_depth u32[n_q_res].
 * ks_profile_build_weighted_pileup: the same from a ks_pileup of the weighted entry points made with KS_PILEUP_PROFILE; one of
 * the unweighted entry points (ks_wpileup_n_weighted == 0) is refused by name.  Everything else as the two builds above. */
int ks_profile_build_weighted_device(ks_ctx *ctx, const uint32_t *d_counts, const uint64_t *d_wcounts, const uint32_t *d_depth,
                                     const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q, uint64_t n_q_res, const ks_profile_opts *opts,
                                     ks_profile **out);
int ks_profile_build_weighted_pileup(ks_ctx *ctx, const ks_pileup *pileup, const uint8_t *d_q_res, const uint64_t *d_q_offs, uint32_t n_q,
                                     uint64_t n_q_res, const ks_profile_opts *opts, ks_profile **out);

/* The three region passes against a profile of the QUERY batch.  The contract of each is its sibling's, word for word —
 * recurrence, tie rules, X-drop, counts, ops, refusals — with one difference: a pair (Q_x, T_y) scores
 * P[q_offs[qid] + position of Q_x][class(T_y)], the anchor pair included.  Identities still compare upper-cased bytes, positives
 * are still s > 0.  Both forms are one code path with two scorers, so a tie never differs between them: a profile whose row p is
 * matrix[class(q_res[p])][.] gives the sibling's result bit for bit.  opts->matrix is not read.
 * A ks_raligns made here records that it is profile-made (ks_raligns_by_profile) and the profile's fallback matrix; the cull's
 * take and the chain, which read extents and scores only, carry the mark through.  The passes that read residues under a matrix
 * — ks_regions_traceback, ks_regions_stitch, ks_frames_stitch, ks_raligns_fold_frames, ks_raligns_stats, ks_cigars_pileup —
 * refuse a profile-made ks_raligns by name, before any device work.
 * Also KS_ERR_INVALID_ARG, before any device work: a NULL profile, one of another context, one whose n_residues is not n_q_res;
 * for ks_regions_traceback_profile an `alignments` that is not profile-made.
 * Not built: profile seeds; stitch, E-values or fold with profile alignments; a profile on the target side. */
int ks_regions_score_profile(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res, const uint64_t *d_q_offs,
                             uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res,
                             const ks_profile *profile, const ks_rscore_opts *opts, ks_rscores **out);
int ks_regions_align_profile(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res, const uint64_t *d_q_offs,
                             uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t, uint64_t n_t_res,
                             const ks_profile *profile, const ks_ralign_opts *opts, ks_raligns **out);
int ks_regions_traceback_profile(ks_ctx *ctx, const ks_regions *regions, const ks_hits *hits, const uint8_t *d_q_res, const uint64_t *d_q_offs,
                                 uint32_t n_q, uint64_t n_q_res, const uint8_t *d_t_res, const uint64_t *d_t_offs, uint32_t n_t,
                                 uint64_t n_t_res, const ks_raligns *alignments, const ks_profile *profile, const ks_rtrace_opts *opts,
                                 ks_cigars **out);
/* 1: the alignments were made by ks_regions_align_profile (or taken from such); 0 otherwise */
int ks_raligns_by_profile(const ks_raligns *s);

/* ---- alignment statistics: bit scores and E-values per hit ------------------------------------------------------------------- */

/* Every stage of the region pipeline ends in a raw integer score; these passes make it comparable across queries, databases
 * and compositions (Karlin & Altschul 1990; composition-based statistics: Schaeffer et al. 2001, BLAST -comp_based_stats 1).
 * The gapped (lambda, K) of a matrix and its gap costs cannot be derived here: the caller brings them, as it brings the matrix.
 *
 * 1. Residue composition of a batch.  The class of a byte is the one of ks_regions_score: after ASCII upper-casing A-Z are
 *    0-25, '*' is 26, every other byte 27.  Result (device-resident): counts u32[n_seqs][28], length u32[n_seqs] and
 *    totals u64[28] over the batch.  All integers: the result never depends on the path a sequence took — a wave per sequence
 *    of at most wave_max residues, a workgroup with a private LDS histogram per sequence of at most group_max, a longer one
 *    split over several workgroups that add to its 28 counters with integer atomics (KS_DEBUG_COMP_PATH = 1 | 2 | 3 sends every
 *    sequence one way, read when the context is made and by ks_ctx_reload_debug_env; ks_debug_rcomp_limits gives the two
 *    thresholds).  An empty batch and empty sequences are valid.  KS_ERR_INVALID_ARG: offsets that descend or pass n_res (the
 *    first such sequence is named);  KS_ERR_CAPACITY: a sequence of 2^32 residues or more.  Built once per database and reused. */
typedef struct ks_rcomp ks_rcomp;
int ks_residue_composition_device(ks_ctx *ctx, const uint8_t *d_res, const uint64_t *d_offs, uint32_t n_seqs, uint64_t n_res,
                                  ks_rcomp **out);
uint32_t ks_rcomp_n_seqs(const ks_rcomp *c);
uint64_t ks_rcomp_n_residues(const ks_rcomp *c);
/* device pointers, valid until ks_rcomp_free */
const uint32_t *ks_rcomp_device_counts(const ks_rcomp *c);
const uint64_t *ks_rcomp_device_totals(const ks_rcomp *c);
const uint32_t *ks_rcomp_device_length(const ks_rcomp *c);
/* any destination may be NULL */
int ks_rcomp_copy_to_host(ks_ctx *ctx, const ks_rcomp *c, uint32_t *counts, uint64_t *totals, uint32_t *length);
void ks_rcomp_free(ks_rcomp *c);
/* the longest sequence a wave takes and the longest one workgroup takes: the tests place lengths around them */
void ks_debug_rcomp_limits(uint32_t *wave_max, uint32_t *group_max);

/* 2. Ungapped Karlin-Altschul parameters, on the host, f64, no context.  matrix: 28 x 28 (the query's class is the row), NULL:
 *    +1 / -1.  freq_q, freq_t: 28 non-negative weights each, of which only the 20 standard classes count (those of
 *    ACDEFGHIKLMNPQRSTVWY), renormalised to 1 over them.  P(s) = the sum of fq[i] * ft[j] over the standard (i, j) with
 *    M[i][j] = s.  lambda: the positive root of sum P(s) e^(lambda s) = 1.  H = lambda * sum s P(s) e^(lambda s).  K by the
 *    series of Karlin & Altschul as BLAST evaluates it: delta = the gcd of the scores with P(s) > 0, scores divided by delta,
 *    lambda' = lambda * delta, P_k the k-fold convolution of P,
 *      sigma = sum over k >= 1 of (1 / k) * [sum over j < 0 of P_k(j) e^(lambda' j) + sum over j >= 0 of P_k(j)]
 *      K = -exp(-2 sigma) / ((H / lambda') * expm1(-lambda'))
 *    summed until a term falls below 2^-60, for at most 400 terms.  Any of lambda, K, H may be NULL.
 *    KS_ERR_INVALID_ARG (ks_karlin_last_error, per thread, says which): NULL, negative or non-finite weights, or none on a
 *    standard class; no positive score has positive probability; the expected score is >= 0; the 400 terms did not suffice
 *    ("expected score too close to zero"). */
int ks_karlin_ungapped(const int8_t *matrix, const double *freq_q, const double *freq_t, double *lambda, double *K, double *H);
const char *ks_karlin_last_error(void);

/* 3. The statistics of a column of scores: per hit row r = (q, t) a composition-based rescaling of the score, per entry (a
 *    region, an alignment, a stitched hit) a bit score and an E-value.
 *    Options: flags KS_ASTATS_NO_COMPOSITION | KS_ASTATS_PAIRWISE | KS_ASTATS_ALLOW_UNGAPPED;  matrix: HOST 28 x 28 or NULL
 *    (+1 / -1; for ks_raligns_stats and ks_hitalns_stats NULL or byte-equal to the one recorded in `alignments`, which is
 *    used);  lambda, K: both 0: the library's ungapped values, else both > 0: the caller's, typically gapped;  background: HOST
 *    f64[28] or NULL: t_comp's totals;  ratio_min, ratio_max: 0 and 0 mean 0.5 and 1.0 (BLAST's bounds for the lambda ratio as
 *    far as they can be restated; no parity is claimed);  db_residues, 0: the residues of t_comp;  db_seqs, 0: t_comp's
 *    sequences;  length_adjust, default 0;  reserved 0.
 *    ks_raligns_stats and ks_hitalns_stats refuse lambda == 0 without KS_ASTATS_ALLOW_UNGAPPED: ungapped parameters understate
 *    gapped E-values, and nothing here does that silently.
 *    Per call, on the host: smin and smax over the standard 20 x 20 block of the matrix (KS_ERR_INVALID_ARG if smax <= 0 or
 *    smin >= 0);  lambda_std — and K_std where no parameters are given — from ks_karlin_ungapped(matrix, background,
 *    background);  lambda_c, K_c: the caller's values, or those two.
 *    Per hit row, exact: cq, ct = the standard-class counts of the two sequences;  h_s = the sum of cq[i] * ct[j] over the
 *    standard (i, j) with M[i][j] = s, in u64;  N = sum h_s.  A row with a sequence of more than 2^20 residues is
 *    KS_ERR_CAPACITY, so N <= 2^40 and every coefficient below is exact in f64.  The row is REGULAR when N > 0, sum s * h_s < 0
 *    and some s > 0 has h_s > 0 — three integer tests.  For a regular row, with d = smax - smin,
 *      f(x) = sum over s of h_s x^(smax - s)  -  N x^smax
 *    — sum h_s x^(-s) = N, the equation of lambda_r in x = e^(-lambda_r), times x^smax: positive below the root, negative from
 *    there to the trivial root 1 — (integer coefficients combined per power, then converted to f64), evaluated by Horner from the
 *    highest power d down in f64, one rounding per operation, no contraction.  Bisection: lo = 0.0, hi = 1.0;  mid = 0.5 * (lo + hi), stop if mid == lo or
 *    mid == hi or after 128 steps, f(mid) > 0 ? lo = mid : hi = mid;  x_r = lo — e^(-lambda_r) of the pair.  A row that is not
 *    regular has status KS_ASTATS_ROW_FALLBACK and x_r = 0.0.  status and x are bit-identical to that loop on a host
 *    (tests/astats_ref.py), whatever the launch geometry.
 *    Per hit row, f64: lambda_r = -log(x_r);  ratio_r = min(max(lambda_r / lambda_std, ratio_min), ratio_max);  1 for fallback
 *    rows, and for every row under KS_ASTATS_NO_COMPOSITION (status KS_ASTATS_ROW_SKIPPED, x = 0.0: no histogram is made, and
 *    t_comp may be NULL when db_residues, db_seqs and background are given and KS_ASTATS_PAIRWISE is not; q_comp is always
 *    needed: its lengths are m).
 *    Per entry e of row r with score S:  S' = ratio_r * (double)S;  bit_score = (lambda_c * S' - ln K_c) / ln 2;
 *      evalue = (K_c * (double)N_eff) * (double)m_eff * exp(-lambda_c * S'),  m_eff = max(Lq - length_adjust, 1),
 *      N_eff = max(db_residues - db_seqs * length_adjust, 1) in saturating integers; with KS_ASTATS_PAIRWISE
 *      N_eff = max(Lt - length_adjust, 1).  Lq, Lt: the length columns of the compositions.
 *    Result (device-resident): per row status u8, x f64, lambda_ratio f64, row_bit_score f64 (the largest bit score of the
 *    row's entries) and row_evalue f64 (the smallest E-value) — NaN for a row without entries; d_score columns for
 *    ks_hits_best with KS_BEST_SCORE and the cluster passes;  per entry bit_score and evalue f64.  Scalars: lambda_std,
 *    lambda_used, K_used, params_source (0 computed, 1 caller), n_fallback.
 *    d_row_offsets: u64[n_rows + 1], the CSR of the n scores over the hit rows, or NULL: one score per hit row (n == n_rows).
 *    KS_ERR_INVALID_ARG, before any device work and also with ctx == NULL: unknown flags, a non-zero reserved field, exactly
 *    one of lambda and K set, negative or NaN lambda, K or ratios, ratio_min > ratio_max, the matrix conflict, the refusal of
 *    ungapped parameters.  Then: NULL arguments; objects of another context; row counts that disagree with `hits`; a
 *    row_offsets that is no CSR from 0 to n; a qid or tid beyond its composition (ks_last_error names the first such row).
 *    One stream, synchronous on return, one host wait; all scratch comes from the context's pool. */
typedef struct ks_astats ks_astats;
#define KS_ASTATS_NO_COMPOSITION 1u
#define KS_ASTATS_PAIRWISE 2u
#define KS_ASTATS_ALLOW_UNGAPPED 4u
#define KS_ASTATS_ROW_REGULAR 0u
#define KS_ASTATS_ROW_FALLBACK 1u
#define KS_ASTATS_ROW_SKIPPED 2u
#define KS_ASTATS_MAX_SEQ_LEN (1u << 20)
typedef struct ks_astats_opts {
    uint32_t flags;         /* KS_ASTATS_* */
    uint32_t length_adjust; /* taken off every sequence length; default 0 */
    const int8_t *matrix;   /* HOST, 28 x 28; NULL: +1 / -1 */
    double lambda, K;       /* both 0: the ungapped values of the matrix; else both > 0 */
    const double *background; /* HOST, f64[28]; NULL: t_comp's totals */
    double ratio_min, ratio_max; /* 0 and 0: 0.5 and 1.0 */
    uint64_t db_residues;   /* 0: the residues of t_comp */
    uint64_t db_seqs;       /* 0: the sequences of t_comp */
    uint64_t reserved;      /* 0 */
} ks_astats_opts;
/* opts == NULL: the defaults */
int ks_scores_stats_device(ks_ctx *ctx, const uint64_t *d_row_offsets, const int64_t *d_score, uint64_t n_rows, uint64_t n,
                           const ks_hits *hits, const ks_rcomp *q_comp, const ks_rcomp *t_comp, const ks_astats_opts *opts,
                           ks_astats **out);
int ks_rscores_stats(ks_ctx *ctx, const ks_rscores *scores, const ks_hits *hits, const ks_rcomp *q_comp, const ks_rcomp *t_comp,
                     const ks_astats_opts *opts, ks_astats **out);
int ks_raligns_stats(ks_ctx *ctx, const ks_raligns *alignments, const ks_hits *hits, const ks_rcomp *q_comp, const ks_rcomp *t_comp,
                     const ks_astats_opts *opts, ks_astats **out);
int ks_hitalns_stats(ks_ctx *ctx, const ks_hitalns *stitched, const ks_raligns *alignments, const ks_hits *hits, const ks_rcomp *q_comp,
                     const ks_rcomp *t_comp, const ks_astats_opts *opts, ks_astats **out);
uint64_t ks_astats_n_rows(const ks_astats *s);
uint64_t ks_astats_n_entries(const ks_astats *s);
uint64_t ks_astats_n_fallback(const ks_astats *s);
double ks_astats_lambda_std(const ks_astats *s);
double ks_astats_lambda_used(const ks_astats *s);
double ks_astats_k_used(const ks_astats *s);
uint32_t ks_astats_params_source(const ks_astats *s);
/* device pointers, valid until ks_astats_free */
const uint8_t *ks_astats_device_status(const ks_astats *s);
const double *ks_astats_device_x(const ks_astats *s);
const double *ks_astats_device_lambda_ratio(const ks_astats *s);
const double *ks_astats_device_bit_score(const ks_astats *s);
const double *ks_astats_device_evalue(const ks_astats *s);
const double *ks_astats_device_row_bit_score(const ks_astats *s);
const double *ks_astats_device_row_evalue(const ks_astats *s);
/* any destination may be NULL */
int ks_astats_copy_to_host(ks_ctx *ctx, const ks_astats *s, uint8_t *status, double *x, double *lambda_ratio, double *bit_score,
                           double *evalue, double *row_bit_score, double *row_evalue);
void ks_astats_free(ks_astats *s);

/* ---- significance: does a hit's overlap mean anything? --------------------------------------------------------------------- */

/* Replaces the two sums behind the columns that branchwater multisearch adds with "calculate probability of overlap between
 * target and query" switched on (src/python/kmerseek/search.py:144-158): prob_overlap and tf_idf_score.
 *
 * Corpus table of a sketch set S, one entry per distinct hash h of S, ascending:
 *   abund_sum(h) u64  the abundances of h summed over the sketches that hold it — exact, no saturation (ks_sketches_union
 *                     saturates at 2^32 - 1; this does not)
 *   doc_freq(h)  u32  the number of sketches that hold h
 *   total(S)     u64  all abundances of S summed
 * n_docs counts every sketch of the set, empty ones included. */
typedef struct ks_corpus ks_corpus;
int ks_corpus_build(ks_ctx *ctx, const ks_sketches *sketches, ks_corpus **out);
uint64_t ks_corpus_n_hashes(const ks_corpus *c);
uint32_t ks_corpus_n_docs(const ks_corpus *c);
uint64_t ks_corpus_total_abund(const ks_corpus *c);
/* any destination may be NULL */
int ks_corpus_copy_to_host(ks_ctx *ctx, const ks_corpus *c, uint64_t *hashes, uint64_t *abund_sum, uint32_t *doc_freq);
void ks_corpus_free(ks_corpus *c);

/* Per row r = (q, t) of `hits`, over the hashes q and t share, in ascending hash order, starting from 0.0:
 *   prob_overlap[r] += ((double)abund_sum_Q(h) / (double)total(Q)) * ((double)abund_sum_T(h) / (double)total(T))
 *   tf_idf[r]       += ((double)abund_q(h) / (double)(sum of q's abundances)) * idf[doc_freq_T(h)]
 *   idf[d] = log(((double)1 + n_targets) / ((double)1 + d)) + 1.0      natural log, evaluated on the host (libm) and uploaded
 * in IEEE f64, every operation rounded on its own (no fma contraction, no reassociation): bit-identical to a host loop that
 * does the same.  The columns derived from them stay with the caller (kmerseek_amd/wire.py):
 *   prob_overlap_adjusted = prob_overlap * (double)(n_queries * n_targets);
 *   containment_adjusted = ((double)intersect / (double)|q|) / prob_overlap_adjusted, and its log10.
 * queries / targets: the sets `hits` was searched on, made with the same ks_params; q_corpus / t_corpus: their corpus tables
 * (n_docs must equal the set's sequence count); hits: from any search entry, thresholded ones included.  The row pass counts
 * the shared hashes it adds: a count that is not the row's intersect, or an id beyond a set, means the inputs do not belong
 * together — KS_ERR_INVALID_ARG, and ks_last_error names the first such row.  A query whose abundances sum to 0 (or a set
 * whose total is 0) divides 0 by 0: its rows hold NaN.  One stream, synchronous on return; scratch comes from the pool. */
typedef struct ks_signif ks_signif;
typedef struct ks_signif_opts {
    uint32_t flags;    /* none defined: 0 */
    uint32_t reserved; /* 0 */
} ks_signif_opts;
/* opts == NULL: the defaults.  Options are checked before any device work. */
int ks_hits_significance(ks_ctx *ctx, const ks_sketches *queries, const ks_sketches *targets, const ks_corpus *q_corpus,
                         const ks_corpus *t_corpus, const ks_hits *hits, const ks_signif_opts *opts, ks_signif **out);
uint64_t ks_signif_n_rows(const ks_signif *s);
/* device columns (ks_signif_n_rows entries, valid until ks_signif_free) */
const double *ks_signif_device_prob_overlap(const ks_signif *s);
const double *ks_signif_device_tf_idf(const ks_signif *s);
/* either destination may be NULL */
int ks_signif_copy_to_host(ks_ctx *ctx, const ks_signif *s, double *prob_overlap, double *tf_idf);
void ks_signif_free(ks_signif *s);

/* ---- best hits per query: top-k by a rank key ------------------------------------------------------------------------------ */

/* The k best rows of every query of an existing hit list (BLAST's max_target_seqs), as a pass of its own: it composes with a
 * thresholded search, with the ks_hits_significance columns as the rank key and with a gathered multi-GPU hit list.
 * Sizes: |q| and |t| are the distinct hash counts of the row's query and target sketch.  `queries` may be NULL for
 * KS_BEST_INTERSECT and KS_BEST_SCORE, `targets` unless the key needs |t|; a non-NULL set's sequence count bounds the ids.
 * Scores are f64 with one rounding per operation (the division is correctly rounded: a host computes the same bits).
 * Order inside one query: row a beats row b iff score(a) > score(b), or the scores are equal and tid(a) < tid(b); -0.0 equals
 * +0.0, NaN compares below every number (-inf included) and NaNs are equal to each other.
 * rank(r) = the number of rows of r's query that beat r; a row is kept iff rank < k.  Ranks inside a query are therefore
 * 0, 1, 2 ... without gaps, and ties at the cut are settled by the smaller tid.
 * *out: a new ks_hits with the kept rows STILL ordered by (qid, tid) (a valid input of ks_match_positions and
 * ks_hits_significance), all four row columns, the two statistics columns if the input has them, and per row `rank` and
 * `src_row`, the row's index in the input list (a caller gathers its own per-row columns through it).  n_pair_instances,
 * partition_path and bucket_posting_bytes are copied.  The input is unchanged and stays valid.  An empty input, or queries
 * without rows, give an empty or shorter list; with k at or above the longest query's row count the output is the input plus
 * the two columns.
 * KS_ERR_INVALID_ARG (options first, before any device work, also with ctx == NULL): k == 0; an unknown rank_by; non-zero
 * flags / reserved; d_score NULL with KS_BEST_SCORE or non-NULL without it; a needed set NULL; then: sets of different
 * ks_params; a qid or tid beyond its set; a |q| or |t| of 0 on a row whose key needs it (ks_last_error names the first such
 * row).  One stream, one wait (the kept count comes back with it); scratch comes from the pool. */
#define KS_BEST_INTERSECT          0u  /* score = (double)intersect (same order as the query's containment: |q| is common to a query's rows) */
#define KS_BEST_TARGET_CONTAINMENT 1u  /* (double)intersect / (double)|t| */
#define KS_BEST_MAX_CONTAINMENT    2u  /* (double)intersect / (double)min(|q|, |t|) */
#define KS_BEST_JACCARD            3u  /* (double)intersect / (double)(|q| + |t| - intersect), the denominator in u64 */
#define KS_BEST_SCORE              4u  /* d_score[r]: a caller-owned device column of ks_hits_count(hits) doubles */
typedef struct ks_best_opts {
    uint32_t rank_by;  /* KS_BEST_* */
    uint32_t k;        /* rows kept per query, >= 1 */
    uint32_t flags;    /* 0 */
    uint32_t reserved; /* 0 */
} ks_best_opts;
int ks_hits_best(ks_ctx *ctx, const ks_hits *hits, const ks_sketches *queries, const ks_sketches *targets,
                 const double *d_score, const ks_best_opts *opts, ks_hits **out);
/* device columns (ks_hits_count entries, valid until ks_hits_free); NULL unless h came from ks_hits_best */
const uint32_t *ks_hits_device_rank(const ks_hits *h);
const uint32_t *ks_hits_device_src_row(const ks_hits *h);
/* either destination may be NULL; KS_ERR_INVALID_ARG for hits that did not come from ks_hits_best */
int ks_hits_copy_best_to_host(ks_ctx *ctx, const ks_hits *h, uint32_t *rank, uint32_t *src_row);

/* ---- gather: the greedy non-redundant targets of every query ----------------------------------------------------------------- */

/* Per query the shortest greedy list of targets that together explain its hashes (the `gather` / `fastmultigather` step of the
 * sourmash / branchwater tools): every target is credited only with the hashes no earlier target covered.  `hits` comes from
 * any search of `queries` against an index of `targets`; thresholded and ks_hits_best lists are valid (a missing row simply is
 * not a candidate).  For every query q with at least one row, in integers only:
 *   R_0 = the distinct hashes of q.  Round i = 0, 1, ...: for every row r of q not yet picked, c_i(r) = |R_i and hashes(tid(r))|;
 *   r* = the row with the largest c_i, ties to the smaller tid (the earlier row).  The query stops when
 *   c_i(r*) < max(min_unique, 1), or i == max_results != 0, or no row is left.  Otherwise r* is kept with
 *     rank = i, unique_intersect = c_i(r*), unique_weighted = the sum of q's abundances over R_i and hashes(t*) (u64, no
 *     saturation), R_(i+1) = R_i without hashes(t*), remaining = |R_(i+1)|.
 * *out: a new ks_hits, built as ks_hits_best builds one: the kept rows STILL ordered by (qid, tid) (a valid input of
 * ks_match_positions, ks_hits_significance and ks_hits_best), the four row columns, the two statistics columns if the input has
 * them, `rank` and `src_row` (the accessors of ks_hits_best and ks_hits_copy_best_to_host work on it) and the three gather
 * columns.  n_pair_instances, partition_path and bucket_posting_bytes are copied; the input is unchanged and stays valid.  An
 * empty hit list gives a valid empty result.  Passes that copy rows (ks_hits_best, the containment threshold) do NOT carry the
 * three gather columns: their output has src_row, through which a caller gathers them.
 * The result never depends on the internal path, the launch geometry or the order in which waves ran: every comparison is on
 * the integer key (count << 32) | ~row, the weighted sum is an integer sum.  (KS_DEBUG_GATHER_PATH = 1 / 2 / 3 force every
 * query onto the wave path / the workgroup path / the workgroup path with its live bitmap in global memory, for the tests.)
 * KS_ERR_INVALID_ARG, options first (before any device work, also with ctx == NULL): non-zero flags / reserved; then NULL
 * arguments, inputs of another context, sets of different ks_params; then, found on the device: a qid or tid beyond its set,
 * and a row whose round-0 count is not its `intersect` — hits and sketches do not belong together (ks_last_error names the
 * first such row).  2^32 - 2 or more rows: KS_ERR_CAPACITY.
 * One stream, one wait (the kept count and the bad-row words come back with it), synchronous on return.  Scratch from the pool:
 * 56 bytes per hit row (+ 16 per query for the segment lists), 4 bytes per shared hash — sized by the list's
 * n_pair_instances, the sum of a search's intersect column — and 1 bit per query hash. */
typedef struct ks_gather_opts {
    uint32_t min_unique;   /* stop a query when the best remaining target would add fewer new hashes; 0 = 1 */
    uint32_t max_results;  /* rows kept per query at most; 0 = no limit */
    uint32_t flags;        /* 0 */
    uint32_t reserved;     /* 0 */
} ks_gather_opts;
/* opts == NULL: the defaults */
int ks_hits_gather(ks_ctx *ctx, const ks_hits *hits, const ks_sketches *queries, const ks_sketches *targets,
                   const ks_gather_opts *opts, ks_hits **out);
/* device columns (ks_hits_count entries, valid until ks_hits_free); NULL unless h came from ks_hits_gather */
const uint32_t *ks_hits_device_unique_intersect(const ks_hits *h);
const uint32_t *ks_hits_device_remaining(const ks_hits *h);
const uint64_t *ks_hits_device_unique_weighted(const ks_hits *h);
/* any destination may be NULL; KS_ERR_INVALID_ARG for hits that did not come from ks_hits_gather */
int ks_hits_copy_gather_to_host(ks_ctx *ctx, const ks_hits *h, uint32_t *unique_intersect, uint32_t *remaining,
                                uint64_t *unique_weighted);

/* ---- clusters: the connected components of an all-vs-all hit list ---------------------------------------------------------- */

/* What an all-vs-all search is run for: which sequences belong together (the `pairwise` + `cluster` step of the sourmash /
 * branchwater tools).  The nodes are 0 .. n-1, the sequences of ONE set; `hits` comes from searching that set against an index
 * of the same set, so qid and tid are both ids in it.  Any hit list in that id space is valid: the output of a thresholded
 * search or of ks_hits_best too, where only one direction of a pair may survive.
 *   row r = (q, t) is an undirected edge iff q != t and score(r) >= threshold
 *   score: the KS_BEST_* keys of ks_hits_best, bit for bit (one device function computes both); |q| and |t| are the distinct
 *          hash counts of nodes[q] and nodes[t].  A NaN score is never an edge; -0.0 equals +0.0; threshold -inf passes
 *          every row that is not NaN.
 *   `nodes` may be NULL for KS_BEST_INTERSECT and KS_BEST_SCORE: n then comes from opts->n_nodes.
 * Clusters are the connected components; a node without an edge is a cluster of one.  An empty hit list gives n singletons.
 * Result (device-resident, every value an integer):
 *   label u32[n]                  the smallest node id of the node's cluster
 *   cluster_id u32[n]             clusters numbered 0 .. n_clusters-1 by ascending smallest member
 *   offsets u64[n_clusters + 1], members u32[n]    the CSR of the clusters in that order, members ascending inside a cluster
 *   representative u32[n_clusters]   with `nodes` the member with the most distinct hashes, ties to the smaller id; without,
 *                                 the smallest member
 *   n_edges: the rows that passed the threshold, self rows and both directions counted as they occur.
 * The result never depends on the internal path (wave-uniform or lane-per-row hooking), the launch geometry or the order in
 * which waves ran: the union-find links by node id alone and everything after it is integer counting and sorting
 * (KS_DEBUG_CLUSTER_PATH = 1 / 2 force the lane-per-row / the wave-uniform hooking for the tests; unset: lane per row).  The
 * input is unchanged and stays valid.
 * KS_ERR_INVALID_ARG (options first, before any device work, also with ctx == NULL): an unknown similarity; non-zero flags /
 * reserved; a NaN threshold; d_score NULL with KS_BEST_SCORE or non-NULL without it; `nodes` NULL where the key needs sizes;
 * n_nodes that is neither 0 nor the node set's sequence count; then: a qid or tid >= n; a size of 0 on a row whose key needs
 * it (ks_last_error names the first such row).  One stream, one wait (the scalars come back with it); scratch comes from the
 * pool: 36 bytes per node, none per row. */
typedef struct ks_clusters ks_clusters;
typedef struct ks_cluster_opts {
    uint32_t similarity; /* KS_BEST_INTERSECT | _TARGET_CONTAINMENT | _MAX_CONTAINMENT | _JACCARD | _SCORE: the same scores, bit for bit, as ks_hits_best */
    uint32_t n_nodes;    /* used only when nodes == NULL; with nodes != NULL it must be 0 or ks_sketches_n_seqs(nodes) */
    double   threshold;  /* a row is an edge iff score >= threshold (NaN scores never are); NaN threshold: KS_ERR_INVALID_ARG */
    uint32_t flags;      /* 0 */
    uint32_t reserved;   /* 0 */
} ks_cluster_opts;
int ks_hits_cluster(ks_ctx *ctx, const ks_hits *hits, const ks_sketches *nodes, const double *d_score,
                    const ks_cluster_opts *opts, ks_clusters **out);
uint32_t ks_clusters_n_nodes(const ks_clusters *c);
uint32_t ks_clusters_n_clusters(const ks_clusters *c);
uint64_t ks_clusters_n_edges(const ks_clusters *c);
/* members of the biggest cluster */
uint32_t ks_clusters_largest(const ks_clusters *c);
/* device pointers, valid until ks_clusters_free */
const uint32_t *ks_clusters_device_label(const ks_clusters *c);
const uint32_t *ks_clusters_device_cluster_id(const ks_clusters *c);
const uint64_t *ks_clusters_device_offsets(const ks_clusters *c);
const uint32_t *ks_clusters_device_members(const ks_clusters *c);
const uint32_t *ks_clusters_device_representative(const ks_clusters *c);
/* any destination may be NULL */
int ks_clusters_copy_to_host(ks_ctx *ctx, const ks_clusters *c, uint32_t *label, uint32_t *cluster_id, uint64_t *offsets,
                             uint32_t *members, uint32_t *representative);
void ks_clusters_free(ks_clusters *c);

/* ---- clusters: greedy representative clustering of an all-vs-all hit list ------------------------------------------------ */

/* The connected components chain: on proteins a multi-domain sequence links families that share nothing, and at the thresholds
 * people use one component swallows the set.  This pass clusters the way CD-HIT's incremental clustering and the greedy
 * set-cover modes of MMseqs2 / linclust do: around representatives.  Nodes, rows, edges and scores are those of
 * ks_hits_cluster: row r = (q, t) is an undirected edge iff q != t and score(r) >= threshold, rows of one direction only are
 * valid, a NaN score is never an edge, -0.0 equals +0.0.
 *   priority: a total order of the nodes.  With `nodes`: more distinct hashes first, ties to the smaller id; without: the
 *          smaller id first.
 *   representatives: the nodes are taken in priority order; a node is a representative iff none of its neighbours of higher
 *          priority is one.  (The lexicographically first maximal independent set of the graph under that order: unique.)
 *   assignment: every other node has a representative among its neighbours.  KS_GREEDY_ASSIGN_FIRST joins the one of highest
 *          priority (CD-HIT's default).  KS_GREEDY_ASSIGN_BEST joins the representative at the other end of the passing row
 *          with the largest score — rows (v, u) and (u, v) are each a candidate, with their own score; ties go to the
 *          representative of higher priority.
 * So every member has a passing row with its representative and no passing row joins two representatives; under
 * KS_GREEDY_ASSIGN_FIRST a representative also has the highest priority of its cluster (ASSIGN_BEST may prefer the better row
 * of a representative of lower priority).  No reference tool is restated here: no parity is claimed.
 * Result: a ks_clusters, read through the accessors above (device-resident, every value an integer):
 *   label u32[n]                  the node's representative; a representative labels itself
 *   cluster_id u32[n]             clusters numbered 0 .. n_clusters-1 by ascending representative id
 *   offsets u64[n_clusters + 1], members u32[n]    the CSR of the clusters in that order, members ascending inside a cluster
 *   representative u32[n_clusters]   the cluster's representative
 *   n_edges, n_clusters, largest  as for ks_hits_cluster (n_edges: the rows that passed, self rows and both directions
 *                                 counted as they occur)
 *   ks_clusters_n_rounds          the rounds the pass took (a diagnostic: it may depend on the schedule; nothing else does)
 * The pass runs in rounds: in each, every undecided node that no undecided neighbour of higher priority blocks is decided, and
 * the edges both of whose ends are still undecided go on to the next round.  The number of rounds is the depth of the
 * dependency chain — small on real data, n on a path in priority order — so once few edges are live one workgroup finishes all
 * remaining rounds in one launch (KS_DEBUG_GREEDY_PATH = 1 forces rounds over the whole grid only, 2 that single workgroup
 * straight after the first round, for the tests).  The result never depends on the path, the launch geometry or the order in
 * which waves ran.  The input is unchanged and stays valid.
 * KS_ERR_INVALID_ARG, in the order of ks_hits_cluster (options first, before any device work, also with ctx == NULL): non-zero
 * flags; an unknown assign mode; an unknown similarity; a NaN threshold; d_score NULL with KS_BEST_SCORE or non-NULL without
 * it; `nodes` NULL where the key needs sizes; n_nodes that is neither 0 nor the node set's sequence count; then: a qid or tid
 * >= n; a size of 0 on a row whose key needs it (ks_last_error names the first such row).  One stream; the host looks at the
 * undecided count once per few rounds.  Scratch comes from the pool: 60 bytes per node, 8 bytes per hit row and 8 bytes per
 * passing non-self row (the two live-edge lists). */
#define KS_GREEDY_ASSIGN_FIRST 0u
#define KS_GREEDY_ASSIGN_BEST  1u
typedef struct ks_greedy_opts {
    uint32_t similarity; /* KS_BEST_INTERSECT | _TARGET_CONTAINMENT | _MAX_CONTAINMENT | _JACCARD | _SCORE: the same scores, bit for bit, as ks_hits_best / ks_hits_cluster */
    uint32_t n_nodes;    /* as in ks_cluster_opts: used only when nodes == NULL; with nodes != NULL it must be 0 or ks_sketches_n_seqs(nodes) */
    double   threshold;  /* a row is an edge iff score >= threshold (NaN scores never are); NaN threshold: KS_ERR_INVALID_ARG */
    uint32_t assign;     /* KS_GREEDY_ASSIGN_FIRST | KS_GREEDY_ASSIGN_BEST */
    uint32_t flags;      /* 0 */
} ks_greedy_opts;
int ks_hits_cluster_greedy(ks_ctx *ctx, const ks_hits *hits, const ks_sketches *nodes, const double *d_score,
                           const ks_greedy_opts *opts, ks_clusters **out);
/* rounds a ks_hits_cluster_greedy result took; 0 for a ks_hits_cluster result */
uint32_t ks_clusters_n_rounds(const ks_clusters *c);
/* live edges at or below which one workgroup finishes the greedy rounds (the tests size an edge list on either side of it) */
uint32_t ks_debug_greedy_tail_edges(void);

/* ---- test hooks: the device-wide primitives, called directly ----------------------------------
 * The exclusive scans, the stable LSD radix sort and the MSD match sort that the passes above stand on, on arrays the caller
 * chooses (tests/test_gpu_prims.py).  Not part of the product interface.  For all of them: the pointers are the caller's device
 * memory on ctx's device unless marked HOST; the arguments are checked on the host before anything is launched
 * (KS_ERR_INVALID_ARG: a NULL, n >= 2^32 - 1, a value outside the range named below); scratch comes from the context's pool and
 * goes back; the call returns when the work is done and fails with KS_ERR_HIP when a scan's look-back gave up. */
/* kind 0: exclusive scan u32 -> u64, d_out has n + 1 entries (d_out[n] = the total; the sum must stay below 2^38), d_total is not
 * used.  kind 1: exclusive scan u32 -> u32 (sums wrap at 2^32) of a copy of d_in in d_out (n entries), in place there;
 * d_total (may be NULL) receives the total.  kind 2: kind 0 without the bound on the sum (never the one-launch path). */
int ks_debug_scan(ks_ctx *ctx, int kind, const uint32_t *d_in, void *d_out, uint64_t n, uint32_t *d_total);
/* The one-launch scans number their tiles from a counter that grows for the life of the context; a tile's status word lives in
 * slot (number mod 2^20) of a ring that is never cleared and carries the number's low 24 bits as its tag.  This sets the number
 * the next such scan starts at (the ring and the counter are made if the context has none yet; the ring keeps its words).  The
 * caller answers for a state the counter could have reached by counting: a word left in a slot must not carry the tag the new
 * numbering expects there, i.e. no earlier scan on this context used a number that is equal mod 2^24 to one about to be used
 * unless the slot was rewritten in between (by counting, 2^20 tiles before at the latest). */
int ks_debug_scan_seek(ks_ctx *ctx, uint32_t global_tile);
/* *base = the number the next one-launch scan starts at: it advances by a scan's tile count (ceil(n / 2048)) iff the scan took the
 * one-launch path (a single tile, n == 0 and KS_DEBUG_SCAN_3PASS do not) */
int ks_debug_scan_ticket(ks_ctx *ctx, uint32_t *base);
/* Stable LSD passes over n (key u64, value) records, one 8-bit digit per listed shift: shifts (HOST) holds n_shifts (1 .. 8)
 * values in 0 .. 56.  vbytes 0 (keys only, d_vals / d_vals_out not used), 4 or 8 picks the value width.  vbytes 4 only:
 * pfxK != 0 — the digits are bits [shift, shift + 8) of umulhi(key >> 32, pfxK) instead of the key's; seg_len != NULL — the input
 * of the first pass lies in seg_regions regions seg_cap records apart, seg_len[r] of them filled (their sum must be n).
 * alias_in != 0: the input is first copied into one of the two scratch pairs and sorted from there (the in-place form).
 * The sorted records are copied to d_keys_out / d_vals_out (n entries each), wherever the passes left them. */
int ks_debug_radix_sort(ks_ctx *ctx, int vbytes, const uint64_t *d_keys, const void *d_vals, uint64_t n, const int *shifts,
                        int n_shifts, uint32_t pfxK, const uint32_t *seg_len, uint64_t seg_cap, uint32_t seg_regions,
                        int alias_in, uint64_t *d_keys_out, void *d_vals_out);
/* The match sort, in place: d_keys ordered on key bits [lo_bit, lo_bit + nbits), the order among equal keys unspecified
 * (0 <= lo_bit, 1 <= nbits <= 64 - lo_bit).  seg_count != NULL (HOST, n_segs entries, 1 .. 64): the list lies in n_segs segments
 * seg_cap records apart, seg_count[s] of them filled (their sum must be n, d_keys spans n_segs * seg_cap records); the sorted list
 * is dense, d_keys[0, n).  info (HOST) = { done, bits of the second partition level, buckets, buckets that went to the large-bucket
 * kernel }.  done == 0 (and the other three): this sort does not apply (n < 65,536, nbits <= 16 or KS_DEBUG_PAIRS_LSD) and the
 * list is untouched. */
int ks_debug_msd_sort(ks_ctx *ctx, uint64_t *d_keys, uint64_t n, int lo_bit, int nbits, const uint32_t *seg_count, uint32_t n_segs,
                      uint64_t seg_cap, uint32_t info[4]);

/* ---- measurement --------------------------------------------------------------------------- */

/* Per-kernel HIP-event timing on ctx's stream.  enable: 0 off; 1 events bracket every launch (~20 us of idle queue
 * around each: for an untimed diagnostic pass); 2 only the sketch tile kernel — the one a step's roofline is quoted
 * for — so that a timed region pays for one bracket per batch. */
typedef struct ks_kernel_time {
    char name[48];
    uint64_t launches;
    double total_ms;
} ks_kernel_time;
int ks_timing_enable(ks_ctx *ctx, int enable);
int ks_timing_reset(ks_ctx *ctx);
/* resolves pending events (synchronizes the stream) and copies up to cap rows; *n = rows available */
int ks_timing_get(ks_ctx *ctx, ks_kernel_time *rows, uint32_t cap, uint32_t *n);

/* The two ceilings SURVEY.md section 8(d) asks bench.py to print beside the HBM roofline, measured on ctx's device:
 *   gmul_per_s    - 64-bit integer multiplies per second / 1e9 (MurmurHash3 needs 8 per window for k <= 16),
 *   copy_gb_per_s - device-to-device hipMemcpy rate, bytes read + bytes written per second / 1e9,
 *   nominal_gb_per_s - memoryClockRate x memoryBusWidth of the device properties (DDR: x2) / 1e9. */
int ks_bench_device_rates(ks_ctx *ctx, double *gmul_per_s, double *copy_gb_per_s, double *nominal_gb_per_s);
/* random 8-byte gathers per second from a 134 MB table ([0]) and from a 2 MB table ([1]): the ceiling of a table-lookup hash
 * for the two-letter hp alphabet (see DESIGN.md for why the multiplies win) */
int ks_bench_gather_rates(ks_ctx *ctx, double gathers_per_s[2]);

#ifdef __cplusplus
}
#endif
#endif /* KMERSEEK_AMD_H */
