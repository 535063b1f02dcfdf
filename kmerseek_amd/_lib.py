"""ctypes binding of libkmerseek_amd.so (include/kmerseek_amd.h).

There is deliberately no fallback: if the HIP library is missing or fails to load, every entry
point raises.  The CPU checker used by the tests lives outside this package and is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# KMERSEEK_AMD_LIB selects another build of the same library (kernel-tuning variants); never a fallback
SO_PATH = os.environ.get("KMERSEEK_AMD_LIB") or os.path.join(HERE, "libkmerseek_amd.so")

KS_OK = 0
KS_ERR_INVALID_MOLTYPE = 1
KS_ERR_INVALID_KSIZE = 2
KS_ERR_INVALID_RESIDUE = 3
KS_ERR_INVALID_ARG = 4
KS_ERR_OOM = 5
KS_ERR_HIP = 6
KS_ERR_NO_DEVICE = 7
KS_ERR_CAPACITY = 8
KS_ERR_INVALID_SCALED = 9

KS_PROTEIN, KS_DAYHOFF, KS_HP = 0, 1, 2
KS_SEED_DEFAULT = 42


class ks_params(C.Structure):
    _fields_ = [("ksize", C.c_uint32), ("scaled", C.c_uint32), ("moltype", C.c_uint32),
                ("flags", C.c_uint32), ("seed", C.c_uint64)]


class ks_residue_error(C.Structure):
    _fields_ = [("seq_index", C.c_uint32), ("position", C.c_uint32), ("residue", C.c_uint8)]


KS_SEARCH_ABUND_STATS = 1


class ks_search_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("min_containment", C.c_double)]


class ks_matchpos_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("max_pairs", C.c_uint64)]


class ks_regions_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("min_kmers", C.c_uint32), ("max_gap", C.c_uint32), ("reserved", C.c_uint32)]


KS_RSCORE_ALPHABET = 28
KS_RSCORE_EXTEND = 1


class ks_rscore_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("x_drop", C.c_uint32), ("matrix", C.POINTER(C.c_int8)), ("reserved", C.c_uint64)]


KS_RALIGN_MAX_BAND = 31
KS_RALIGN_MAX_GAP_COST = 255
KS_RALIGN_MAX_X_DROP = 1 << 20


class ks_ralign_opts(C.Structure):
    _fields_ = [("matrix", C.POINTER(C.c_int8)), ("band", C.c_uint32), ("gap_open", C.c_uint32), ("gap_extend", C.c_uint32),
                ("x_drop", C.c_uint32), ("flags", C.c_uint32)]


KS_RTRACE_EQX = 1


class ks_rtrace_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("max_scratch_bytes", C.c_uint64)]


KS_RCULL_NONE = 0xFFFFFFFF
KS_RCULL_MIN_SCORE = 1


class ks_rcull_opts(C.Structure):
    _fields_ = [("overlap_pct", C.c_uint32), ("max_per_row", C.c_uint32), ("min_score", C.c_int64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


KS_RCHAIN_NONE = 0xFFFFFFFF


class ks_rchain_opts(C.Structure):
    _fields_ = [("max_gap", C.c_uint32), ("max_overlap", C.c_uint32), ("link_cost", C.c_uint32), ("skew_cost", C.c_uint32),
                ("overlap_cost", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


KS_FFOLD_NONE = 0xFFFFFFFF


class ks_ffold_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


KS_RSTITCH_EQX = 1
KS_RSTITCH_MAX_FILL = 4096


class ks_rstitch_opts(C.Structure):
    _fields_ = [("max_fill", C.c_uint32), ("flags", C.c_uint32), ("max_scratch_bytes", C.c_uint64), ("reserved", C.c_uint32 * 2)]


KS_CIGAR_FSHIFT = 3
KS_FSTITCH_MAX_COST = 65536


class ks_fstitch_opts(C.Structure):
    _fields_ = [("max_fill", C.c_uint32), ("flags", C.c_uint32), ("frameshift_cost", C.c_uint32), ("reserved", C.c_uint32),
                ("max_scratch_bytes", C.c_uint64)]


KS_PILEUP_QUERY, KS_PILEUP_TARGET, KS_PILEUP_PROFILE = 0, 1, 1
KS_WEIGHT_ONE, KS_PWEIGHTS_INCLUDE_QUERY = 1 << 30, 1


class ks_pileup_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("side", C.c_uint32), ("reserved", C.c_uint64)]


KS_PROFILE_INCLUDE_QUERY = 1
KS_PROFILE_MAX_THRESHOLDS = 254


class ks_profile_opts(C.Structure):
    _fields_ = [("matrix", C.POINTER(C.c_int8)), ("bg", C.POINTER(C.c_double)), ("ratio", C.POINTER(C.c_double)), ("beta", C.c_double),
                ("thresholds", C.POINTER(C.c_double)), ("n_thr", C.c_uint32), ("base", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


KS_ASTATS_NO_COMPOSITION, KS_ASTATS_PAIRWISE, KS_ASTATS_ALLOW_UNGAPPED = 1, 2, 4
KS_ASTATS_ROW_REGULAR, KS_ASTATS_ROW_FALLBACK, KS_ASTATS_ROW_SKIPPED = 0, 1, 2
KS_ASTATS_MAX_SEQ_LEN = 1 << 20


class ks_astats_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("length_adjust", C.c_uint32), ("matrix", C.POINTER(C.c_int8)), ("lambda_", C.c_double),
                ("K", C.c_double), ("background", C.POINTER(C.c_double)), ("ratio_min", C.c_double), ("ratio_max", C.c_double),
                ("db_residues", C.c_uint64), ("db_seqs", C.c_uint64), ("reserved", C.c_uint64)]


class ks_signif_opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32)]


KS_BEST_INTERSECT, KS_BEST_TARGET_CONTAINMENT, KS_BEST_MAX_CONTAINMENT, KS_BEST_JACCARD, KS_BEST_SCORE = 0, 1, 2, 3, 4


class ks_best_opts(C.Structure):
    _fields_ = [("rank_by", C.c_uint32), ("k", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ks_cluster_opts(C.Structure):
    _fields_ = [("similarity", C.c_uint32), ("n_nodes", C.c_uint32), ("threshold", C.c_double), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


KS_GREEDY_ASSIGN_FIRST, KS_GREEDY_ASSIGN_BEST = 0, 1


class ks_greedy_opts(C.Structure):
    _fields_ = [("similarity", C.c_uint32), ("n_nodes", C.c_uint32), ("threshold", C.c_double), ("assign", C.c_uint32),
                ("flags", C.c_uint32)]


class ks_gather_opts(C.Structure):
    _fields_ = [("min_unique", C.c_uint32), ("max_results", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


KS_MASK_MAX_WINDOW = 32


class ks_mask_opts(C.Structure):
    _fields_ = [("window", C.c_uint32), ("k1_millibits", C.c_uint32), ("k2_millibits", C.c_uint32)]


class ks_kernel_time(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double)]


_vp = C.c_void_p
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_pp = C.POINTER(C.c_void_p)
_parp = C.POINTER(ks_params)

# name -> (restype, argtypes); mirrors include/kmerseek_amd.h one to one
SIGNATURES = {
    "ks_abi_version": (C.c_uint32, []),
    "ks_status_string": (C.c_char_p, [C.c_int]),
    "ks_moltype_from_string": (C.c_int, [C.c_char_p, _u32p]),
    "ks_max_hash": (C.c_uint64, [C.c_uint32]),
    "ks_ctx_create": (C.c_int, [C.c_int, _vp, _pp]),
    "ks_ctx_destroy": (None, [_vp]),
    "ks_last_error": (C.c_char_p, [_vp]),
    "ks_ctx_stream": (_vp, [_vp]),
    "ks_ctx_synchronize": (C.c_int, [_vp]),
    "ks_ctx_sketch_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64 * 5)]),
    "ks_ctx_search_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64 * 5)]),
    "ks_ctx_fused_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64 * 4)]),
    "ks_ctx_qfilter_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64 * 2)]),
    "ks_ctx_reload_debug_env": (C.c_int, [_vp]),
    "ks_debug_guard_selftest": (C.c_int, [C.c_char_p]),
    "ks_host_alloc": (C.c_int, [_vp, C.c_uint64, _pp]),
    "ks_host_free": (C.c_int, [_vp, _vp]),
    "ks_dev_malloc": (C.c_int, [_vp, C.c_uint64, _pp]),
    "ks_dev_free": (C.c_int, [_vp, _vp]),
    "ks_dev_upload": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "ks_dev_download": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "ks_ctx_pool_stats": (C.c_int, [_vp, _u64p, _u64p, _u64p, _u64p]),
    "ks_validate_and_resolve": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int, C.c_uint64, C.c_char_p, _u64p,
                                          C.POINTER(ks_residue_error)]),
    "ks_sketch_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _parp, _pp]),
    "ks_sketch_batch_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, _parp, _pp]),
    "ks_sketch_queries_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, _pp]),
    "ks_sketch_search_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, _pp, _pp]),
    "ks_sketch_search": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _pp, _pp]),
    "ks_sketches_has_postings": (C.c_int, [_vp]),
    "ks_sketches_n_seqs": (C.c_uint32, [_vp]),
    "ks_sketches_n_hashes": (C.c_uint64, [_vp]),
    "ks_sketches_n_windows": (C.c_uint64, [_vp]),
    "ks_sketches_params": (None, [_vp, _parp]),
    "ks_sketches_device_offsets": (_vp, [_vp]),
    "ks_sketches_device_hashes": (_vp, [_vp]),
    "ks_sketches_device_abunds": (_vp, [_vp]),
    "ks_sketches_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "ks_sketches_from_host": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _parp, _pp]),
    "ks_sketches_union": (C.c_int, [_vp, _vp, _pp]),
    "ks_sketches_free": (None, [_vp]),
    "ks_translate6_bound": (C.c_uint64, [C.c_uint64]),
    "ks_translate6_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, _u64p]),
    "ks_sketch_translated_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, _parp, _pp]),
    "ks_sketch_translated": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _parp, _pp]),
    "ks_sketches_union_groups": (C.c_int, [_vp, _vp, _u32p, C.c_uint32, _pp]),
    "ks_debug_translate_chunk": (C.c_uint32, []),
    "ks_debug_union_rank_max": (C.c_uint32, []),
    "ks_mask_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, C.POINTER(ks_mask_opts), _pp]),
    "ks_mask_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(ks_mask_opts), _pp]),
    "ks_mask_n_seqs": (C.c_uint32, [_vp]),
    "ks_mask_n_residues": (C.c_uint64, [_vp]),
    "ks_mask_n_masked": (C.c_uint64, [_vp]),
    "ks_mask_device_mask": (_vp, [_vp]),
    "ks_mask_device_masked_counts": (_vp, [_vp]),
    "ks_mask_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp]),
    "ks_mask_free": (None, [_vp]),
    "ks_mask_split_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, _pp]),
    "ks_segments_n_segs": (C.c_uint64, [_vp]),
    "ks_segments_n_residues": (C.c_uint64, [_vp]),
    "ks_segments_n_records": (C.c_uint32, [_vp]),
    "ks_segments_device_seg_record": (_vp, [_vp]),
    "ks_segments_device_seg_start": (_vp, [_vp]),
    "ks_segments_device_seg_offsets": (_vp, [_vp]),
    "ks_segments_device_residues": (_vp, [_vp]),
    "ks_segments_device_group_offsets": (_vp, [_vp]),
    "ks_segments_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ks_segments_free": (None, [_vp]),
    "ks_sketch_masked_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, _parp, C.POINTER(ks_mask_opts), _pp]),
    "ks_sketch_masked": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _parp, C.POINTER(ks_mask_opts), _pp]),
    "ks_kmer_positions_masked_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, _parp, C.POINTER(ks_mask_opts), _pp]),
    "ks_debug_mask_chunk": (C.c_uint32, []),
    "ks_kmer_positions": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _parp, _pp]),
    "ks_kmer_positions_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, _parp, _pp]),
    "ks_kmerpos_count": (C.c_uint64, [_vp]),
    "ks_kmerpos_params": (None, [_vp, _parp]),
    "ks_kmerpos_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "ks_kmerpos_free": (None, [_vp]),
    "ks_index_build": (C.c_int, [_vp, _vp, _pp]),
    "ks_index_n_targets": (C.c_uint32, [_vp]),
    "ks_index_n_postings": (C.c_uint64, [_vp]),
    "ks_index_free": (None, [_vp]),
    "ks_search": (C.c_int, [_vp, _vp, _vp, _pp]),
    "ks_hits_count": (C.c_uint64, [_vp]),
    "ks_hits_n_pair_instances": (C.c_uint64, [_vp]),
    "ks_hits_partition_path": (C.c_int, [_vp]),
    "ks_hits_bucket_posting_bytes": (C.c_int, [_vp]),
    "ks_hits_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ks_hits_device_qid": (_vp, [_vp]),
    "ks_hits_device_tid": (_vp, [_vp]),
    "ks_hits_device_intersect": (_vp, [_vp]),
    "ks_hits_device_n_weighted": (_vp, [_vp]),
    "ks_hits_copy_to_device": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp]),
    "ks_hits_pack64_to_device": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_uint32]),
    "ks_hits_unpack64_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "ks_hits_merge_by_qid_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp]),
    "ks_hits_free": (None, [_vp]),
    "ks_search_ex": (C.c_int, [_vp, _vp, _vp, C.POINTER(ks_search_opts), _pp]),
    "ks_sketch_search_device_ex": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(ks_search_opts), _pp,
                                             _pp]),
    "ks_sketch_search_ex": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.POINTER(ks_search_opts), _pp, _pp]),
    "ks_hits_has_abund_stats": (C.c_int, [_vp]),
    "ks_hits_device_median2": (_vp, [_vp]),
    "ks_hits_device_abund_ss": (_vp, [_vp]),
    "ks_hits_copy_abund_stats_to_host": (C.c_int, [_vp, _vp, _vp, _vp]),
    "ks_match_positions": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(ks_matchpos_opts), _pp]),
    "ks_matchpos_n_rows": (C.c_uint64, [_vp]),
    "ks_matchpos_n_pairs": (C.c_uint64, [_vp]),
    "ks_matchpos_n_slices": (C.c_uint32, [_vp]),
    "ks_matchpos_device_row_offsets": (_vp, [_vp]),
    "ks_matchpos_device_q_start": (_vp, [_vp]),
    "ks_matchpos_device_t_start": (_vp, [_vp]),
    "ks_matchpos_device_q_lo": (_vp, [_vp]),
    "ks_matchpos_device_q_hi": (_vp, [_vp]),
    "ks_matchpos_device_t_lo": (_vp, [_vp]),
    "ks_matchpos_device_t_hi": (_vp, [_vp]),
    "ks_matchpos_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ks_matchpos_free": (None, [_vp]),
    "ks_match_regions": (C.c_int, [_vp, _vp, C.POINTER(ks_regions_opts), _pp]),
    "ks_regions_n_rows": (C.c_uint64, [_vp]),
    "ks_regions_n_regions": (C.c_uint64, [_vp]),
    "ks_regions_n_slices": (C.c_uint32, [_vp]),
    "ks_regions_device_row_offsets": (_vp, [_vp]),
    "ks_regions_device_q_start": (_vp, [_vp]),
    "ks_regions_device_t_start": (_vp, [_vp]),
    "ks_regions_device_length": (_vp, [_vp]),
    "ks_regions_device_n_kmers": (_vp, [_vp]),
    "ks_regions_device_covered": (_vp, [_vp]),
    "ks_regions_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ks_regions_free": (None, [_vp]),
    "ks_regions_score": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64,
                                   C.POINTER(ks_rscore_opts), _pp]),
    "ks_rscores_n_rows": (C.c_uint64, [_vp]),
    "ks_rscores_n_regions": (C.c_uint64, [_vp]),
    "ks_rscores_device_row_offsets": (_vp, [_vp]),
    "ks_rscores_device_q_start": (_vp, [_vp]),
    "ks_rscores_device_t_start": (_vp, [_vp]),
    "ks_rscores_device_length": (_vp, [_vp]),
    "ks_rscores_device_score": (_vp, [_vp]),
    "ks_rscores_device_identities": (_vp, [_vp]),
    "ks_rscores_device_positives": (_vp, [_vp]),
    "ks_rscores_device_core_identities": (_vp, [_vp]),
    "ks_rscores_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ks_rscores_free": (None, [_vp]),
    "ks_debug_rscore_step": (C.c_uint32, []),
    "ks_regions_align": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64,
                                   C.POINTER(ks_ralign_opts), _pp]),
    "ks_raligns_n_rows": (C.c_uint64, [_vp]),
    "ks_raligns_n_regions": (C.c_uint64, [_vp]),
    "ks_raligns_device_row_offsets": (_vp, [_vp]),
    "ks_raligns_device_q_start": (_vp, [_vp]),
    "ks_raligns_device_q_length": (_vp, [_vp]),
    "ks_raligns_device_t_start": (_vp, [_vp]),
    "ks_raligns_device_t_length": (_vp, [_vp]),
    "ks_raligns_device_score": (_vp, [_vp]),
    "ks_raligns_device_identities": (_vp, [_vp]),
    "ks_raligns_device_positives": (_vp, [_vp]),
    "ks_raligns_device_gap_opens": (_vp, [_vp]),
    "ks_raligns_device_gaps": (_vp, [_vp]),
    "ks_raligns_device_aln_length": (_vp, [_vp]),
    "ks_raligns_copy_to_host": (C.c_int, [_vp] * 13),
    "ks_raligns_free": (None, [_vp]),
    "ks_debug_ralign_chunk": (C.c_uint32, []),
    "ks_regions_traceback": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, _vp,
                                       C.POINTER(ks_rtrace_opts), _pp]),
    "ks_cigars_n_rows": (C.c_uint64, [_vp]),
    "ks_cigars_n_regions": (C.c_uint64, [_vp]),
    "ks_cigars_n_ops": (C.c_uint64, [_vp]),
    "ks_cigars_scratch_bytes": (C.c_uint64, [_vp]),
    "ks_cigars_n_slices": (C.c_uint32, [_vp]),
    "ks_cigars_device_op_offsets": (_vp, [_vp]),
    "ks_cigars_device_ops": (_vp, [_vp]),
    "ks_cigars_copy_to_host": (C.c_int, [_vp] * 4),
    "ks_cigars_free": (None, [_vp]),
    "ks_debug_rtrace_stage": (C.c_uint32, []),
    "ks_regions_cull_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, C.c_uint64, C.POINTER(ks_rcull_opts), _pp]),
    "ks_raligns_cull": (C.c_int, [_vp, _vp, C.POINTER(ks_rcull_opts), _pp]),
    "ks_rscores_cull": (C.c_int, [_vp, _vp, C.POINTER(ks_rcull_opts), _pp]),
    "ks_rcull_n_rows": (C.c_uint64, [_vp]),
    "ks_rcull_n_regions": (C.c_uint64, [_vp]),
    "ks_rcull_n_kept": (C.c_uint64, [_vp]),
    "ks_rcull_device_row_offsets": (_vp, [_vp]),
    "ks_rcull_device_src_region": (_vp, [_vp]),
    "ks_rcull_device_rank": (_vp, [_vp]),
    "ks_rcull_device_n_merged": (_vp, [_vp]),
    "ks_rcull_device_keeper": (_vp, [_vp]),
    "ks_rcull_device_row_best_score": (_vp, [_vp]),
    "ks_rcull_copy_to_host": (C.c_int, [_vp] * 8),
    "ks_rcull_free": (None, [_vp]),
    "ks_regions_take": (C.c_int, [_vp, _vp, _vp, _pp]),
    "ks_rscores_take": (C.c_int, [_vp, _vp, _vp, _pp]),
    "ks_raligns_take": (C.c_int, [_vp, _vp, _vp, _pp]),
    "ks_debug_rcull_lds_rows": (C.c_uint32, [_u32p]),
    "ks_regions_chain_device": (C.c_int, [_vp] * 9 + [C.c_uint64, C.c_uint64, C.POINTER(ks_rchain_opts), _pp]),
    "ks_raligns_chain": (C.c_int, [_vp, _vp, C.POINTER(ks_rchain_opts), _pp]),
    "ks_rscores_chain": (C.c_int, [_vp, _vp, C.POINTER(ks_rchain_opts), _pp]),
    "ks_rchain_n_rows": (C.c_uint64, [_vp]),
    "ks_rchain_n_regions": (C.c_uint64, [_vp]),
    "ks_rchain_n_chained": (C.c_uint64, [_vp]),
    "ks_rchain_device_row_offsets": (_vp, [_vp]),
    "ks_rchain_device_src_region": (_vp, [_vp]),
    "ks_rchain_device_best": (_vp, [_vp]),
    "ks_rchain_device_pred": (_vp, [_vp]),
    "ks_rchain_device_chain_score": (_vp, [_vp]),
    "ks_rchain_device_q_start": (_vp, [_vp]),
    "ks_rchain_device_q_length": (_vp, [_vp]),
    "ks_rchain_device_t_start": (_vp, [_vp]),
    "ks_rchain_device_t_length": (_vp, [_vp]),
    "ks_rchain_device_q_aligned": (_vp, [_vp]),
    "ks_rchain_device_t_aligned": (_vp, [_vp]),
    "ks_rchain_device_identities": (_vp, [_vp]),
    "ks_rchain_device_aln_length": (_vp, [_vp]),
    "ks_rchain_device_row_chain_score": (_vp, [_vp]),
    "ks_rchain_device_row_coverage": (_vp, [_vp]),
    "ks_rchain_copy_to_host": (C.c_int, [_vp] * 16),
    "ks_rchain_free": (None, [_vp]),
    "ks_rchain_coverage": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32]),
    "ks_rchain_coverage_to_host": (C.c_int, [_vp, _vp, _vp]),
    "ks_debug_rchain_lds_rows": (C.c_uint32, [_u32p]),
    "ks_frames_fold_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32] + [_vp] * 8 + [C.c_uint64, C.POINTER(ks_ffold_opts), _pp, _pp]),
    "ks_rscores_fold_frames": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.POINTER(ks_ffold_opts), _pp, _pp]),
    "ks_raligns_fold_frames": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.POINTER(ks_ffold_opts), _pp, _pp]),
    "ks_ffold_n_rows": (C.c_uint64, [_vp]),
    "ks_ffold_n_regions": (C.c_uint64, [_vp]),
    "ks_ffold_n_src_rows": (C.c_uint64, [_vp]),
    "ks_ffold_device_src_row": (_vp, [_vp]),
    "ks_ffold_device_row_offsets": (_vp, [_vp]),
    "ks_ffold_device_src_region": (_vp, [_vp]),
    "ks_ffold_device_frame": (_vp, [_vp]),
    "ks_ffold_device_nt_length": (_vp, [_vp]),
    "ks_ffold_device_s_start": (_vp, [_vp]),
    "ks_ffold_device_nt_start": (_vp, [_vp]),
    "ks_ffold_device_t_start3": (_vp, [_vp]),
    "ks_ffold_device_t_length3": (_vp, [_vp]),
    "ks_ffold_device_score": (_vp, [_vp]),
    "ks_ffold_device_identities": (_vp, [_vp]),
    "ks_ffold_device_aln_length": (_vp, [_vp]),
    "ks_ffold_copy_to_host": (C.c_int, [_vp] * 14),
    "ks_ffold_free": (None, [_vp]),
    "ks_regions_stitch": (C.c_int, [_vp] * 5 + [_vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, C.POINTER(ks_rstitch_opts), _pp]),
    "ks_hitalns_n_rows": (C.c_uint64, [_vp]),
    "ks_hitalns_n_ops": (C.c_uint64, [_vp]),
    "ks_hitalns_scratch_bytes": (C.c_uint64, [_vp]),
    "ks_hitalns_n_slices": (C.c_uint32, [_vp]),
    "ks_hitalns_device_op_offsets": (_vp, [_vp]),
    "ks_hitalns_device_ops": (_vp, [_vp]),
    "ks_hitalns_device_q_start": (_vp, [_vp]),
    "ks_hitalns_device_q_length": (_vp, [_vp]),
    "ks_hitalns_device_t_start": (_vp, [_vp]),
    "ks_hitalns_device_t_length": (_vp, [_vp]),
    "ks_hitalns_device_score": (_vp, [_vp]),
    "ks_hitalns_device_identities": (_vp, [_vp]),
    "ks_hitalns_device_positives": (_vp, [_vp]),
    "ks_hitalns_device_gap_opens": (_vp, [_vp]),
    "ks_hitalns_device_gaps": (_vp, [_vp]),
    "ks_hitalns_device_aln_length": (_vp, [_vp]),
    "ks_hitalns_device_n_members": (_vp, [_vp]),
    "ks_hitalns_device_n_filled": (_vp, [_vp]),
    "ks_hitalns_device_n_open": (_vp, [_vp]),
    "ks_hitalns_device_n_trimmed": (_vp, [_vp]),
    "ks_hitalns_device_row_score": (_vp, [_vp]),
    "ks_hitalns_copy_to_host": (C.c_int, [_vp] * 19),
    "ks_hitalns_free": (None, [_vp]),
    "ks_debug_rstitch_stage": (C.c_uint32, []),
    "ks_frames_stitch": (C.c_int, [_vp] * 6 + [_vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, C.POINTER(ks_fstitch_opts), _pp]),
    "ks_framealns_n_rows": (C.c_uint64, [_vp]),
    "ks_framealns_n_ops": (C.c_uint64, [_vp]),
    "ks_framealns_scratch_bytes": (C.c_uint64, [_vp]),
    "ks_framealns_n_slices": (C.c_uint32, [_vp]),
    "ks_framealns_device_op_offsets": (_vp, [_vp]),
    "ks_framealns_device_ops": (_vp, [_vp]),
    "ks_framealns_device_s_start": (_vp, [_vp]),
    "ks_framealns_device_nt_length": (_vp, [_vp]),
    "ks_framealns_device_nt_start": (_vp, [_vp]),
    "ks_framealns_device_t_start": (_vp, [_vp]),
    "ks_framealns_device_t_length": (_vp, [_vp]),
    "ks_framealns_device_score": (_vp, [_vp]),
    "ks_framealns_device_identities": (_vp, [_vp]),
    "ks_framealns_device_positives": (_vp, [_vp]),
    "ks_framealns_device_gap_opens": (_vp, [_vp]),
    "ks_framealns_device_gaps": (_vp, [_vp]),
    "ks_framealns_device_aln_length": (_vp, [_vp]),
    "ks_framealns_device_n_members": (_vp, [_vp]),
    "ks_framealns_device_n_filled": (_vp, [_vp]),
    "ks_framealns_device_n_open": (_vp, [_vp]),
    "ks_framealns_device_n_trimmed": (_vp, [_vp]),
    "ks_framealns_device_n_frameshifts": (_vp, [_vp]),
    "ks_framealns_device_row_score": (_vp, [_vp]),
    "ks_framealns_copy_to_host": (C.c_int, [_vp] * 21),
    "ks_framealns_free": (None, [_vp]),
    "ks_pileup_device": (C.c_int, [_vp] * 4 + [C.c_uint64] * 3 + [_vp] * 5 + [C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64,
                                   C.POINTER(ks_pileup_opts), _pp]),
    "ks_cigars_pileup": (C.c_int, [_vp] * 6 + [C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, C.POINTER(ks_pileup_opts), _pp]),
    "ks_hitalns_pileup": (C.c_int, [_vp] * 5 + [C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, C.POINTER(ks_pileup_opts), _pp]),
    "ks_frames_pileup": (C.c_int, [_vp] * 5 + [C.c_uint32, C.c_uint64, C.POINTER(ks_pileup_opts), _pp]),
    "ks_profile_build_device": (C.c_int, [_vp] * 5 + [C.c_uint32, C.c_uint64, C.POINTER(ks_profile_opts), _pp]),
    "ks_profile_build_pileup": (C.c_int, [_vp] * 4 + [C.c_uint32, C.c_uint64, C.POINTER(ks_profile_opts), _pp]),
    "ks_profile_build_weighted_device": (C.c_int, [_vp] * 6 + [C.c_uint32, C.c_uint64, C.POINTER(ks_profile_opts), _pp]),
    "ks_profile_build_weighted_pileup": (C.c_int, [_vp] * 4 + [C.c_uint32, C.c_uint64, C.POINTER(ks_profile_opts), _pp]),
    "ks_profile_from_host": (C.c_int, [_vp] * 4 + [C.c_uint32, C.c_uint64, _vp, _pp]),
    "ks_profile_n_seqs": (C.c_uint32, [_vp]),
    "ks_profile_n_residues": (C.c_uint64, [_vp]),
    "ks_profile_n_scores": (C.c_uint64, [_vp]),
    "ks_profile_device_scores": (_vp, [_vp]),
    "ks_profile_device_consensus": (_vp, [_vp]),
    "ks_profile_device_n_obs": (_vp, [_vp]),
    "ks_profile_copy_to_host": (C.c_int, [_vp] * 5),
    "ks_profile_free": (None, [_vp]),
    "ks_regions_score_profile": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, _vp,
                                           C.POINTER(ks_rscore_opts), _pp]),
    "ks_regions_align_profile": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, _vp,
                                           C.POINTER(ks_ralign_opts), _pp]),
    "ks_regions_traceback_profile": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp,
                                               C.POINTER(ks_rtrace_opts), _pp]),
    "ks_raligns_by_profile": (C.c_int, [_vp]),
    "ks_pileup_n_seqs": (C.c_uint32, [_vp]),
    "ks_pileup_n_residues": (C.c_uint64, [_vp]),
    "ks_pileup_n_profile": (C.c_uint64, [_vp]),
    "ks_pileup_device_depth": (_vp, [_vp]),
    "ks_pileup_device_counts": (_vp, [_vp]),
    "ks_pileup_device_length": (_vp, [_vp]),
    "ks_pileup_device_n_alignments": (_vp, [_vp]),
    "ks_pileup_device_covered": (_vp, [_vp]),
    "ks_pileup_device_max_depth": (_vp, [_vp]),
    "ks_pileup_device_depth_sum": (_vp, [_vp]),
    "ks_pileup_device_breadth": (_vp, [_vp]),
    "ks_pileup_device_mean_depth": (_vp, [_vp]),
    "ks_pileup_copy_to_host": (C.c_int, [_vp] * 11),
    "ks_pileup_free": (None, [_vp]),
    "ks_entry_weights_device": (C.c_int, [_vp] * 4 + [C.c_uint64] * 3 + [_vp] * 6 + [C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, _vp,
                                           C.c_uint32, C.c_uint32, _pp]),
    "ks_cigars_pileup_weights": (C.c_int, [_vp] * 8 + [C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, _pp]),
    "ks_pweights_n_entries": (C.c_uint64, [_vp]),
    "ks_pweights_device_weight": (_vp, [_vp]),
    "ks_pweights_device_n_cols": (_vp, [_vp]),
    "ks_pweights_copy_to_host": (C.c_int, [_vp] * 4),
    "ks_pweights_free": (None, [_vp]),
    "ks_wpileup_device": (C.c_int, [_vp] * 4 + [C.c_uint64] * 3 + [_vp] * 5 + [C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, _vp,
                                            C.POINTER(ks_pileup_opts), _pp]),
    "ks_cigars_pileup_weighted": (C.c_int, [_vp] * 6 + [C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, _vp, C.POINTER(ks_pileup_opts), _pp]),
    "ks_hitalns_pileup_weighted": (C.c_int, [_vp] * 5 + [C.c_uint32, C.c_uint64, _vp, _vp, C.c_uint32, C.c_uint64, _vp, C.POINTER(ks_pileup_opts), _pp]),
    "ks_wpileup_n_weighted": (C.c_uint64, [_vp]),
    "ks_wpileup_device_wdepth": (_vp, [_vp]),
    "ks_wpileup_device_wcounts": (_vp, [_vp]),
    "ks_wpileup_copy_to_host": (C.c_int, [_vp] * 4),
    "ks_debug_pileup_limits": (None, [_u32p]),
    "ks_residue_composition_device": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, _pp]),
    "ks_rcomp_n_seqs": (C.c_uint32, [_vp]),
    "ks_rcomp_n_residues": (C.c_uint64, [_vp]),
    "ks_rcomp_device_counts": (_vp, [_vp]),
    "ks_rcomp_device_totals": (_vp, [_vp]),
    "ks_rcomp_device_length": (_vp, [_vp]),
    "ks_rcomp_copy_to_host": (C.c_int, [_vp] * 5),
    "ks_rcomp_free": (None, [_vp]),
    "ks_debug_rcomp_limits": (None, [_u32p, _u32p]),
    "ks_karlin_ungapped": (C.c_int, [C.POINTER(C.c_int8), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ks_karlin_last_error": (C.c_char_p, []),
    "ks_scores_stats_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint64, _vp, _vp, _vp, C.POINTER(ks_astats_opts), _pp]),
    "ks_rscores_stats": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(ks_astats_opts), _pp]),
    "ks_raligns_stats": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(ks_astats_opts), _pp]),
    "ks_hitalns_stats": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ks_astats_opts), _pp]),
    "ks_astats_n_rows": (C.c_uint64, [_vp]),
    "ks_astats_n_entries": (C.c_uint64, [_vp]),
    "ks_astats_n_fallback": (C.c_uint64, [_vp]),
    "ks_astats_lambda_std": (C.c_double, [_vp]),
    "ks_astats_lambda_used": (C.c_double, [_vp]),
    "ks_astats_k_used": (C.c_double, [_vp]),
    "ks_astats_params_source": (C.c_uint32, [_vp]),
    "ks_astats_device_status": (_vp, [_vp]),
    "ks_astats_device_x": (_vp, [_vp]),
    "ks_astats_device_lambda_ratio": (_vp, [_vp]),
    "ks_astats_device_bit_score": (_vp, [_vp]),
    "ks_astats_device_evalue": (_vp, [_vp]),
    "ks_astats_device_row_bit_score": (_vp, [_vp]),
    "ks_astats_device_row_evalue": (_vp, [_vp]),
    "ks_astats_copy_to_host": (C.c_int, [_vp] * 9),
    "ks_astats_free": (None, [_vp]),
    "ks_corpus_build": (C.c_int, [_vp, _vp, _pp]),
    "ks_corpus_n_hashes": (C.c_uint64, [_vp]),
    "ks_corpus_n_docs": (C.c_uint32, [_vp]),
    "ks_corpus_total_abund": (C.c_uint64, [_vp]),
    "ks_corpus_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "ks_corpus_free": (None, [_vp]),
    "ks_hits_significance": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ks_signif_opts), _pp]),
    "ks_signif_n_rows": (C.c_uint64, [_vp]),
    "ks_signif_device_prob_overlap": (_vp, [_vp]),
    "ks_signif_device_tf_idf": (_vp, [_vp]),
    "ks_signif_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp]),
    "ks_signif_free": (None, [_vp]),
    "ks_hits_best": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(ks_best_opts), _pp]),
    "ks_hits_device_rank": (_vp, [_vp]),
    "ks_hits_device_src_row": (_vp, [_vp]),
    "ks_hits_copy_best_to_host": (C.c_int, [_vp, _vp, _vp, _vp]),
    "ks_hits_gather": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(ks_gather_opts), _pp]),
    "ks_hits_device_unique_intersect": (_vp, [_vp]),
    "ks_hits_device_remaining": (_vp, [_vp]),
    "ks_hits_device_unique_weighted": (_vp, [_vp]),
    "ks_hits_copy_gather_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "ks_hits_cluster": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(ks_cluster_opts), _pp]),
    "ks_clusters_n_nodes": (C.c_uint32, [_vp]),
    "ks_clusters_n_clusters": (C.c_uint32, [_vp]),
    "ks_clusters_n_edges": (C.c_uint64, [_vp]),
    "ks_clusters_largest": (C.c_uint32, [_vp]),
    "ks_clusters_device_label": (_vp, [_vp]),
    "ks_clusters_device_cluster_id": (_vp, [_vp]),
    "ks_clusters_device_offsets": (_vp, [_vp]),
    "ks_clusters_device_members": (_vp, [_vp]),
    "ks_clusters_device_representative": (_vp, [_vp]),
    "ks_clusters_copy_to_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ks_clusters_free": (None, [_vp]),
    "ks_hits_cluster_greedy": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(ks_greedy_opts), _pp]),
    "ks_clusters_n_rounds": (C.c_uint32, [_vp]),
    "ks_debug_greedy_tail_edges": (C.c_uint32, []),
    "ks_debug_scan": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint64, _vp]),
    "ks_debug_scan_seek": (C.c_int, [_vp, C.c_uint32]),
    "ks_debug_scan_ticket": (C.c_int, [_vp, _u32p]),
    "ks_debug_radix_sort": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint64, C.POINTER(C.c_int), C.c_int, C.c_uint32, _vp, C.c_uint64,
                                      C.c_uint32, C.c_int, _vp, _vp]),
    "ks_debug_msd_sort": (C.c_int, [_vp, _vp, C.c_uint64, C.c_int, C.c_int, _u32p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32 * 4)]),
    "ks_timing_enable": (C.c_int, [_vp, C.c_int]),
    "ks_timing_reset": (C.c_int, [_vp]),
    "ks_timing_get": (C.c_int, [_vp, C.POINTER(ks_kernel_time), C.c_uint32, _u32p]),
    "ks_bench_gather_rates": (C.c_int, [_vp, C.POINTER(C.c_double * 2)]),
    "ks_bench_device_rates": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

_lib = None


class KmerseekLibraryError(RuntimeError):
    pass


def load():
    """dlopen the HIP library; raises KmerseekLibraryError (never falls back) if it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise KmerseekLibraryError(
            f"{SO_PATH} not found: build it with `python -m kmerseek_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64, and whichever copy is mapped first serves
    # both.  If this library pulled in /opt/rocm's copy BEFORE torch was imported, a later `import torch` would bring a
    # second runtime and ks_ctx_create would then see "no HIP device" (measured: bench.py, round 2).  So when torch is
    # installed and the process may use it (device memory, streams, torch.distributed), let it load first.
    if "torch" not in sys.modules and os.environ.get("KS_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    try:
        L = C.CDLL(SO_PATH)
    except OSError as e:  # missing libamdhip64 etc.
        raise KmerseekLibraryError(f"cannot load {SO_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            raise KmerseekLibraryError(f"{SO_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L
