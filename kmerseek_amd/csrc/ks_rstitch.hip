// ks_rstitch.hip — ks_regions_stitch: the chain of every hit row (ks_rchain.hip) made into ONE gapped alignment with one CIGAR
// (include/kmerseek_amd.h has the contract).  The pass is ks_stitch_kit.h — plan, slices, fill, emit, rescore and their driver —
// under the plain coordinates below: the query axis is the query's residues, a chain member names its alignment itself, and
// every member of a row lies in the row's one query sequence.
#include "ks_stitch_kit.h"

struct rs_policy {
    static constexpr u32 UNIT = 1;
    struct ext { const u64 *a_offs; };                     // the alignments' rows: n_rows + 1
    struct spans { u32 *q_start, *q_length; };
    typedef ks_hitalns result;
    struct link { u32 trim, kop, krem, c, Y, cls, ncol, g; }; // (the words of ks_stitch_kit.h: 32 bytes)

    // c_src[j] must lie inside the row's alignments (the member in front: inside the alignments)
    template <bool NAME> static KS_DEV bool member(const st_args &A, const ext &F, u32 row, u32 j, u32 q, u32 t, st_member &M) {
        const u32 g = A.c_src[j];
        if (g >= A.n_regions || (NAME && (g < F.a_offs[row] || g >= F.a_offs[row + 1]))) {
            if (NAME) ks_first_bad(A.bad, ST_BAD_SRC, j);
            return false;
        }
        if (NAME && (q >= A.n_q || t >= A.n_t)) { ks_first_bad(A.bad, ST_BAD_ROW, row); return false; }
        M = st_member{g, q, 0u};
        return true;
    }
    static KS_DEV u32 seq_at(u32 q, u32) { return q; }
    static KS_DEV void keep(link &, u32, u32, u32) {}
    static KS_DEV void ends_of(const st_args &A, const link *, u32 j, u32 &E, u32 &pte) { // (wave-uniform j)
        const u32 gp = ks_readfirst(A.c_src[j - 1]);
        E = ks_readfirst(A.a_qs[gp]) + ks_readfirst(A.a_ql[gp]); pte = ks_readfirst(A.a_ts[gp]) + ks_readfirst(A.a_tl[gp]);
    }
    static KS_DEV void write_spans(const st_args &A, const ext &, const spans &Z, u32 r, u64 b, u64 e, u32 g0, u32 g1, u32) {
        const u32 qs = e > b ? A.a_qs[g0] : 0u, qe = e > b ? A.a_qs[g1] + A.a_ql[g1] : 0u;
        Z.q_start[r] = qs; Z.q_length[r] = qe - qs;
    }
    static spans spans_of(result *R) { return spans{R->d_q_start, R->d_q_length}; }
    static const u32 *axis_start(const result *R) { return R->d_q_start; }

    static constexpr const char *pass = "region stitch";
    static constexpr u32 pin = KS_PIN_RSTITCH;
    static constexpr const char *k_plan = "rstitch_plan", *k_fill = "rstitch_fill", *k_count = "rstitch_count", *k_ops = "rstitch_ops",
                                *k_rescore = "rstitch_rescore";
    static constexpr const char *budget_fmt = "region stitch: the link in front of chain member %llu needs %llu bytes of directions, max_scratch_bytes allows %llu";
    static constexpr const char *walk_fmt = "region stitch: internal error: the fill in front of chain member %llu did not walk back to its origin";
    // the plan's refusals: `who` is the first offender of ST_BAD_* `why`
    static int refuse(ks_ctx *ctx, u32 why, unsigned long long who, bool eqx, u64, const ks_res_batch &Q, const ks_res_batch &T) {
        switch (why) {
        case ST_BAD_SRC:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region stitch: chain member %llu names a region outside its hit row's alignments: the chain was not made from these alignments", who);
        case ST_BAD_ROW: return rk_fail_bad_row(ctx, pass, who, Q, T);
        case ST_BAD_LEN: return ks_fail(ctx, KS_ERR_CAPACITY, "region stitch: hit row %llu has a query or target sequence of more than 2^20 residues", who);
        case ST_BAD_EXT:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region stitch: the alignment of region %llu does not lie inside its two sequences: alignments, hits and batches do not belong together", who);
        case ST_BAD_OPS:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region stitch: the ops of region %llu do not consume exactly its q_length and t_length: the CIGARs were not traced from these alignments", who);
        case ST_BAD_CODE:
            return ks_fail(ctx, KS_ERR_INVALID_ARG, eqx ? "region stitch: KS_RSTITCH_EQX is set and the ops of region %llu hold M: trace with KS_RTRACE_EQX"
                                                        : "region stitch: the ops of region %llu hold = or X: set KS_RSTITCH_EQX", who);
        default: // ST_BAD_ASC (the frame stitch's words are never raised)
            return ks_fail(ctx, KS_ERR_INVALID_ARG, "region stitch: chain member %llu ends before the member in front of it on one of the sequences: the chain was not made from these alignments", who);
        }
    }
};

int ks_regions_stitch_impl(ks_ctx *ctx, const ks_rchain *K, const ks_raligns *S, const ks_cigars *G, const ks_hits *H, const ks_res_batch &Q,
                           const ks_res_batch &T, u32 max_fill, u32 flags, u64 max_scratch_bytes, ks_hitalns *R) {
    return st_run<rs_policy>(ctx, K, S, G, H, Q, T, max_fill, flags, max_scratch_bytes, rs_policy::ext{S->d_row_offsets}, R);
}

extern "C" uint32_t ks_debug_rstitch_stage(void) { return RP_STAGE; }
