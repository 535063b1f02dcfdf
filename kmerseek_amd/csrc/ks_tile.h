// ks_tile.h — the tile kit: what a kernel needs to stage a tile of residues in LDS and hash its k-mer windows.
// Shared by the sketch tiles (ks_sketch.hip), the slab path for sequences longer than a tile (ks_sketch_long.hip) and the
// k-mer position table (ks_kmerpos.hip): the tile's sizes, the sketch launch arguments (sk_args), the two staging steps
// (sk_load16, sk_encode16), the window hash in its compile-time (sk_hash_window) and run-time (sk_hash_window_rt) forms,
// and the search for the sequence that holds a position (sk_seq_beyond).
#pragma once
#include "ks_device.h"

#ifndef SK_THREADS
#define SK_THREADS 512
#endif
#define SK_E 8
#define SK_TILE (SK_THREADS * SK_E) // 4096 LDS positions
#define SK_PAD 160                  // >= KS_MAX_KSIZE + 24: slack behind the last residue for word reads
#define SK_SEQ_CAP 254 // sequence boundaries of a tile staged in LDS (tiles with more fall back to global reads)

// the arguments of a sketch launch: k_sketch_tiles takes one, the slab path one inside its own (sk_long_args), k_place_long one
struct sk_args {
    const u8 *res;
    const u64 *offs;
    u32 n_seqs;
    u64 n_res;
    u32 k;
    u64 seed;
    u64 max_hash;
    u32 sfix;     // floor(2^48 / ((max_hash >> 32) + 1)): bucket multiplier = (n_windows * sfix) >> 16
    const u8 *lut; // 256-byte encode table for this moltype
    u32 upper_only; // the table only upper-cases (moltype protein): applied arithmetically
    u32 R;         // tile stride in residues (see sk_r_cand_host, ks_sketch.hip); 0 = packed tiles (tile_g0 gives each tile's first residue)
    const u64 *tile_g0; // packed tiles: 16-byte aligned residue offset the tile's LDS window starts at
    const u64 *tile_wbase; // packed tiles, no hash threshold, or NULL: k-mer windows of all sequences before the tile's first = where its
                           // CSR slots begin (slots as long as the sequences' windows: no look-back across tiles, no tile status words)
    u32 span;      // residues a shared tile covers from tile * R: SK_TILE, or more for the compacting variant (scaled > 1)
    u32 c_div, c_rcp; // compacting variant: bucket space is positions / c_div (c_rcp = ceil(2^32 / c_div))
    u64 out_cap;   // capacity of out_hash / out_abund (MODE 0): writes beyond it are dropped and the host repeats larger
    u32 use_ticket; // tile ids from the atomic ticket (1) or from blockIdx.x (0)
    u32 debug_qcap;      // diagnostics (KS_DEBUG_QCAP): capacity of the bucket lists of phase 3 (0 = what fits)
    u32 debug_skip_tile; // diagnostics (KS_DEBUG_LOOKBACK_SKIP): this tile never publishes — its successors' spins really expire
    u32 le_cap;    // a sequence whose LOCAL end lies beyond this is not this launch's business
    u32 max_len_tile; // ... nor is one longer than this (packed tiles: PK_MAX_LEN, so that "long" means the same everywhere)
    const u32 *seq_list; // MODE 0: tile_first[n_tiles + 1] (tile -> first sequence); MODE 1: the medium sequences
    const u32 *n_list;   // MODE 1: device-resident length of seq_list
    u32 n_list_cap;      // ... and the allocated length (the smaller one counts)
    // MODE 0 writes the final CSR directly: hashes / abunds at csr positions, csr[s] per sequence
    u64 *out_hash;  // MODE 0: final hashes [n_windows]; MODE 1: lg_hash [n_res] (run of sequence s starts at offs[s])
    u32 *out_abund;
    u64 *csr;       // [n_seqs + 1] final CSR offsets (MODE 0)
    u64 *total_out; // MODE 0: the batch's kept-hash total once more, next to the other words the host reads back
    u32 *counts;    // [n_seqs] DISTINCT hashes of every sequence (ks_sketches::d_counts): written by whoever sketches the sequence
    u32 *kept;      // [n_seqs] kept hashes (repeats included) of medium / long sequences (written by MODE 1 / k_sketch_long, read by
                    // MODE 0: a deferred sequence's slot in the CSR is as long as its kept count)
    u64 *drops_out; // kept hashes that repeat an earlier one of their sequence, summed over the batch (slots the CSR leaves empty)
    // decoupled look-back across tiles (MODE 0)
    unsigned long long *tile_status; // [n_tiles] (flag << 62) | value; flag 1 = tile aggregate, 2 = inclusive prefix
    u32 *ticket;    // [0] dynamic tile id, [1] status bits: 1 = a bounded spin expired, 2 = postings not emitted for some tile,
                    //     4 = a compacting tile kept more hashes (or holds more sequences) than its LDS lists take
    u32 n_tiles;
    const u32 *n_tiles_dev; // MODE 0, optional: the tiles there really are (a launch sized by an upper bound: the rest return)
    // optional: postings (hash, sequence) partitioned on the low 8 bits of the join prefix into <= 256 fixed-capacity
    // regions, written while the vector ALU is the bottleneck — the query side's first partition pass of ks_search
    u64 *part_keys;   // [256 * part_cap] or NULL
    u32 *part_vals;
    u32 *part_cursor; // [256] records placed per region so far
    u64 part_cap;
    u32 part_K, part_mask; // region = ks_join_prefix(h, part_K) & part_mask
    u32 part_kshift;       // != 0: part_K = 2^(32 - part_kshift), the prefix is a shift (sk_digit)
    u32 part_s;            // != 0: 10-byte postings (ks_sketches::part_s): sequence id bits 0..7 ride in hash bits [part_s, part_s + 8)
    u32 part_sub_shift;    // sub-regions per region = 1 << shift; a workgroup writes sub-region blockIdx.x & (that - 1)
};

// bucket multiplier: bucket = umulhi(h >> 32, mul) < n_windows for every kept h (h <= max_hash)
KS_DEV u32 sk_bucket_mul(u32 nw, u32 sfix) {
    u64 m = ((u64)nw * sfix) >> 16;
    return m > 0xffffffffULL ? 0xffffffffu : (u32)m;
}

// hash of the window that starts at LDS byte `pos8 + I` where pos8 is 8-byte aligned.  KC != 0: k is the compile-time
// constant KC (the launches of the common k-mer sizes): the block loop, the tail branches and the byte masks fold away and a
// tail of <= 4 bytes multiplies as a 32-bit value — ~56 instead of ~90 vector instructions per window at k = 10, where
// the hash phase is what the vector ALU is busy with (profiles/).
template <int I, int KC = 0>
KS_DEV u64 sk_hash_window(const u64 *w /* LDS words starting at pos8 */, u32 k_rt, u64 seed) {
    const u32 k = KC ? (u32)KC : k_rt;
    ks_murmur m;
    m.init(seed);
    const u32 nb = k >> 4, t = k & 15;
    u32 j = 0;
    for (u32 b = 0; b < nb; b++, j += 2) {
        u64 a0 = w[j], a1 = w[j + 1], a2 = w[j + 2];
        m.block(ks_funnel<I>(a0, a1), ks_funnel<I>(a1, a2));
    }
    if (t) {
        u64 a0 = w[j], a1 = w[j + 1], a2 = w[j + 2];
        u64 k1 = ks_funnel<I>(a0, a1), k2 = ks_funnel<I>(a1, a2);
        if (t > 8) k2 &= ks_mask_bytes(t - 8); else { k1 &= ks_mask_bytes(t); k2 = 0; }
        m.tail(k1, k2, t);
    }
    return m.finish((u64)k);
}

// ... and of the window at byte `byte_shift` (< 8, known only at run time) of w[0]: the same loop with run-time funnel shifts
// (the slab path, whose windows start wherever the sequence does)
KS_DEV u64 sk_hash_window_rt(const u64 *w, u32 byte_shift, u32 k, u64 seed) {
    ks_murmur m;
    m.init(seed);
    const u32 nb = k >> 4, t = k & 15;
    u32 jj = 0;
    for (u32 bl = 0; bl < nb; bl++, jj += 2)
        m.block(ks_funnel_rt(w[jj], w[jj + 1], byte_shift), ks_funnel_rt(w[jj + 1], w[jj + 2], byte_shift));
    if (t) {
        u64 k1 = ks_funnel_rt(w[jj], w[jj + 1], byte_shift), k2 = ks_funnel_rt(w[jj + 1], w[jj + 2], byte_shift);
        if (t > 8) k2 &= ks_mask_bytes(t - 8); else { k1 &= ks_mask_bytes(t); k2 = 0; }
        m.tail(k1, k2, t);
    }
    return m.finish((u64)k);
}

// h[i] = hash of the window at byte pos8 + H + i, i < NW (the calls stay unrolled: every offset is a compile-time constant)
template <int H, int NW, int KC = 0, int I = 0>
KS_DEV void sk_hash_windows(u64 *h, const u64 *w, u32 k_rt, u64 seed) {
    if constexpr (I < NW) {
        h[I] = sk_hash_window<H + I, KC>(w, k_rt, seed);
        sk_hash_windows<H, NW, KC, I + 1>(h, w, k_rt, seed);
    }
}

// Staging a tile's residues, 16 B per lane, is two steps so that a kernel can REQUEST the bytes early and store them later:
// 16 residue bytes at g (16-byte aligned), zero-filled behind the batch ...
KS_DEV uint4 sk_load16(const u8 *res, u64 n_res, u64 g) {
#ifdef SK_NT_RES
    if (g + 16 <= n_res) { const u32 *p4 = (const u32 *)(res + g); return make_uint4(__builtin_nontemporal_load(p4), __builtin_nontemporal_load(p4 + 1), __builtin_nontemporal_load(p4 + 2), __builtin_nontemporal_load(p4 + 3)); }
#else
    if (g + 16 <= n_res) return *(const uint4 *)(res + g);
#endif
    u32 t[4] = {0, 0, 0, 0};
    for (u32 b = 0; b < 16 && g + b < n_res; b++) t[b >> 2] |= (u32)res[g + b] << (8 * (b & 3));
    return make_uint4(t[0], t[1], t[2], t[3]);
}
// ... and the 16 bytes through the encode table (256 bytes in LDS)
KS_DEV uint4 sk_encode16(uint4 v, const u8 *lut_s, bool upper_only /* uniform */) {
    const u32 in[4] = {v.x, v.y, v.z, v.w};
    u32 o[4];
    if (upper_only) { // moltype protein: the table only upper-cases — four bytes at a time, no table, no barrier for it
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const u32 y = in[d] & 0x7f7f7f7fu; // (no carry between bytes: 0x7f + 0x1f < 0x100)
            const u32 lower = (y + 0x1f1f1f1fu) & ~(y + 0x05050505u) & ~in[d] & 0x80808080u; // bytes in 'a' .. 'z'
            o[d] = in[d] ^ (lower >> 2);
        }
    } else {
#pragma unroll
        for (int d = 0; d < 4; d++)
            o[d] = (u32)lut_s[in[d] & 255u] | ((u32)lut_s[(in[d] >> 8) & 255u] << 8) |
                   ((u32)lut_s[(in[d] >> 16) & 255u] << 16) | ((u32)lut_s[in[d] >> 24] << 24);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// first s in [lo, hi) whose local end `end_of(s)` lies beyond `key` (hi if there is none): the sequence that holds position key
template <typename EndOf>
KS_DEV u32 sk_seq_beyond(u32 lo, u32 hi, u32 key, EndOf end_of) {
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (end_of(mid) > key) hi = mid; else lo = mid + 1;
    }
    return lo;
}
