// ks_fstitch.hip — ks_frames_stitch: the chain of every folded row of a translated search (ks_ffold.hip, ks_rchain.hip) made into
// ONE alignment of the strand's bases against the target protein: one CIGAR in codon columns with explicit frameshift ops,
// re-scored over the residues (include/kmerseek_amd.h has the contract).  The pass is ks_stitch_kit.h — plan, slices, fill, emit,
// rescore and their driver, the program of ks_rstitch.hip and not a copy — under the coordinates below: the query axis is the
// strand's bases, a column that consumes the query moves the position by 3.
//
// A strand base position p reads the codon that is residue p / 3 of frame sequence 6 record + 3 strand + p % 3: the fold's
// s_start = f + 3 q_start, f < 3, makes one rule address every frame.  M, = and X are a codon against a residue, I a codon without
// a residue, D a residue without a codon, N (KS_CIGAR_FSHIFT) r = 1 or 2 skipped bases.  The worked examples, a gene of n codons
// whose two parts are aligned in two frames:
//   one base inserted after codon m     X = 1, Y = 0          mM 1N (n - m)M
//   one base of codon m deleted         X = 2, Y = 1, c = 0   mM 1D 2N (n - m - 1)M
// The pass does not search for the place of the shift inside a link: the N op stands directly before the next member.
#include "ks_stitch_kit.h"

struct fs_policy {
    static constexpr u32 UNIT = 3;
    struct ext {
        const u64 *f_offs; const u32 *f_src; const u8 *f_frame; // the fold: n_rows + 1, n_fregions
        const u32 *f_ntlen, *f_sstart, *f_ntstart, *f_ts3, *f_tl3;
        u32 n_fregions, fcost;
    };
    struct spans { u32 *s_start, *nt_length, *nt_start, *n_frameshifts; };
    typedef ks_framealns result;
    struct link {
        u32 g, trim, kop, krem; // the words of ks_stitch_kit.h, and
        u32 c, r, Y;            // r: the skipped bases of the link (X = 3 c + r)
        u32 cls, ncol;
        u32 E, pte;             // the previous member's ends: strand bases, target residues
        u32 pad;
    };

    // c_src[j] must lie inside the folded row's regions, the fold's region name an alignment and lie in a frame of the row's strand;
    // the thread's own member also: the fold's columns are those of that alignment, and all three frames of the strand exist
    template <bool NAME> static KS_DEV bool member(const st_args &A, const ext &F, u32 row, u32 j, u32 q, u32 t, st_member &M) {
        const u32 fg = A.c_src[j];
        if (fg >= F.n_fregions || fg < F.f_offs[row] || fg >= F.f_offs[row + 1]) {
            if (NAME) ks_first_bad(A.bad, ST_BAD_SRC, j);
            return false;
        }
        const u32 g = F.f_src[fg], frame = F.f_frame[fg];
        if (g >= A.n_regions) {
            if (NAME) ks_first_bad(A.bad, ST_BAD_FSRC, fg);
            return false;
        }
        if (frame >= 6u || frame / 3u != (q & 1u)) {
            if (NAME) ks_first_bad(A.bad, ST_BAD_STRAND, fg);
            return false;
        }
        const u64 s6 = 6ULL * (q >> 1) + 3u * (q & 1u);
        M = st_member{g, (u32)s6 + frame % 3u, frame % 3u};
        if (!NAME) return true;
        const u64 qs = A.a_qs[g], ql = A.a_ql[g], ts = A.a_ts[g], tl = A.a_tl[g];
        if ((u64)F.f_sstart[fg] != frame % 3u + 3u * qs || (u64)F.f_ntlen[fg] != 3u * ql || (u64)F.f_ts3[fg] != 3u * ts || (u64)F.f_tl3[fg] != 3u * tl) {
            ks_first_bad(A.bad, ST_BAD_FOLD, fg);
            return false;
        }
        if (s6 + 3u > A.n_q || t >= A.n_t) { ks_first_bad(A.bad, ST_BAD_ROW, row); return false; }
        return true;
    }
    static KS_DEV u32 seq_at(u32 q, u32 p) { return 6u * (q >> 1) + 3u * (q & 1u) + p % 3u; }
    static KS_DEV void keep(link &L, u32 r, u32 E, u32 pte) { L.r = r; L.E = E; L.pte = pte; }
    static KS_DEV void ends_of(const st_args &, const link *links, u32 j, u32 &E, u32 &pte) { // (wave-uniform j)
        E = ks_readfirst(links[j].E); pte = ks_readfirst(links[j].pte);
    }
    static KS_DEV void write_spans(const st_args &A, const ext &F, const spans &Z, u32 r, u64 b, u64 e, u32, u32, u32 n_shift) {
        u32 ss = 0, se = 0, ns = 0;
        if (e > b) {
            const u32 f0 = A.c_src[b], f1 = A.c_src[e - 1];
            ss = F.f_sstart[f0]; se = F.f_sstart[f1] + F.f_ntlen[f1];
            ns = (A.qid[r] & 1u) ? F.f_ntstart[f1] : F.f_ntstart[f0];
        }
        Z.s_start[r] = ss; Z.nt_length[r] = se - ss; Z.nt_start[r] = ns; Z.n_frameshifts[r] = n_shift;
    }
    static spans spans_of(result *R) { return spans{R->d_s_start, R->d_nt_length, R->d_nt_start, R->d_n_frameshifts}; }
    static const u32 *axis_start(const result *R) { return R->d_s_start; }

    static constexpr const char *pass = "frame stitch";
    static constexpr u32 pin = KS_PIN_FSTITCH;
    static constexpr const char *k_plan = "fstitch_plan", *k_fill = "fstitch_fill", *k_count = "fstitch_count", *k_ops = "fstitch_ops",
                                *k_rescore = "fstitch_rescore";
    static constexpr const char *budget_fmt = "frame stitch: the link in front of chain member %llu needs %llu bytes of directions, max_scratch_bytes allows %llu";
    static constexpr const char *walk_fmt = "frame stitch: internal error: the fill in front of chain member %llu did not walk back to its origin";
    // the plan's refusals: `who` is the first offender of ST_BAD_* `why`
    static int refuse(ks_ctx *ctx, u32 why, unsigned long long who, bool eqx, u64 n_regions, const ks_res_batch &Q, const ks_res_batch &T) {
        switch (why) {
        case ST_BAD_SRC:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: chain member %llu names a region outside its folded row's regions: the chain was not made on this fold", who);
        case ST_BAD_FSRC:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: folded region %llu names an alignment beyond the %llu of the alignments: the fold was not made of these alignments",
                           who, (unsigned long long)n_regions);
        case ST_BAD_FOLD:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: folded region %llu does not hold its alignment's extents (s_start = frame %% 3 + 3 q_start, nt_length = 3 q_length, t_start3 = 3 t_start, t_length3 = 3 t_length): the fold was not made of these alignments", who);
        case ST_BAD_STRAND:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: folded region %llu lies in a frame of the other strand than its folded row's: fold and folded hits do not belong together", who);
        case ST_BAD_ROW:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: folded row %llu names a frame sequence beyond the %u of the frame batch, a target beyond the %u of the target batch, or a sequence outside its batch",
                           who, Q.n_seqs, T.n_seqs);
        case ST_BAD_LEN: return ks_fail(ctx, KS_ERR_CAPACITY, "frame stitch: folded row %llu has a frame or target sequence of more than 2^20 residues", who);
        case ST_BAD_EXT:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: the alignment of region %llu does not lie inside its two sequences: alignments, hits and batches do not belong together", who);
        case ST_BAD_OPS:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: the ops of region %llu do not consume exactly its q_length and t_length: the CIGARs were not traced from these alignments", who);
        case ST_BAD_CODE:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, eqx ? "frame stitch: KS_RSTITCH_EQX is set and the ops of region %llu hold M: trace with KS_RTRACE_EQX"
                                                        : "frame stitch: the ops of region %llu hold = or X: set KS_RSTITCH_EQX", who);
        default: // ST_BAD_ASC
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "frame stitch: chain member %llu ends before the member in front of it on the strand or on the target: the chain was not made on this fold", who);
        }
    }
};

int ks_frames_stitch_impl(ks_ctx *ctx, const ks_ffold *F, const ks_hits *H, const ks_rchain *K, const ks_raligns *S, const ks_cigars *G,
                          const ks_res_batch &Q, const ks_res_batch &T, u32 max_fill, u32 flags, u32 frameshift_cost, u64 max_scratch_bytes,
                          ks_framealns *R) {
    const fs_policy::ext X{F->d_row_offsets, F->d_src_region, F->d_frame, F->d_nt_length, F->d_s_start, F->d_nt_start, F->d_t_start3, F->d_t_length3,
                           (u32)F->n_regions, frameshift_cost};
    return st_run<fs_policy>(ctx, K, S, G, H, Q, T, max_fill, flags, max_scratch_bytes, X, R);
}
