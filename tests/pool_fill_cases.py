"""What tests/test_gpu_poisoned_pool.py runs on a poisoned pool (KS_DEBUG_POOL_FILL), and what it may leave out.

CASES is the table: (module, function, parameter sets).  Every function is a reference-compared test of the suite, called as it is.
Its `ctx` and every other fixture of its module are made by the module's own fixture functions while the variable is set (so they
are poisoned, and torn down the module's way, caches of device objects included); a test that makes its own context does the same.  A
parameter set maps the argument names of one of the function's own pytest.mark.parametrize marks, written as they are there
("k,scaled,mol"), or the name of a parametrised fixture of its module ("mode_ctx"), to one of the values listed there, or to
Nth(i), the i-th of them where the value is too long to repeat.  Nothing else may be passed: tests/test_pool_fill_cpu.py checks the
table against the functions without a device.

tests/pool_fill_exempt.py is the complement: every prototype of include/kmerseek_amd.h that the table need not reach, with the
reason.  A prototype in neither fails the last test of the GPU file, so a new pass joins the table."""
import importlib
import inspect
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ENV = "KS_DEBUG_POOL_FILL"
FILLS = (0, 255)


class Nth:
    """The i-th value of the parametrisation it stands in for."""

    def __init__(self, i):
        self.i = i

    def __repr__(self):
        return f"Nth({self.i})"


PATHS3 = [{"path": p} for p in (None, "1", "2")]
MODES3 = [{"mode_ctx": m} for m in (None, "1", "2")]

CASES = [
    # ---- sketch ---------------------------------------------------------------------------------------------------------------
    ("test_gpu_parity", "test_sketch_vs_oracle_synthetic", [{"k,scaled,mol": (5, 1, "hp")}, {"k,scaled,mol": (16, 5, "dayhoff")},
                                                            {"k,scaled,mol": (33, 3, "hp")}]),
    ("test_gpu_parity", "test_sketch_ragged_and_edge_inputs", [{}]),
    ("test_gpu_parity", "test_sketches_with_repeats_are_a_plain_csr_at_the_boundary", [{}]),
    ("test_gpu_parity", "test_sketch_sort_phases_on_repeats_crowded_buckets_and_tiny_sequences", [{}]),
    ("test_gpu_parity", "test_sketch_only_long_sequences", [{}]),
    ("test_gpu_parity", "test_sketch_empty_batches", [{}]),
    ("test_gpu_parity", "test_compacting_tiles_and_bounded_outputs_fall_back_exactly", [{}]),
    ("test_gpu_planned_slots", "test_proteins_across_tiles_and_chunks", [{"mol,k": ("protein", 10)}, {"mol,k": ("hp", 5)}]),
    ("test_gpu_planned_slots", "test_repeated_kmers_leave_gapped_slots", [{"mol,k": ("protein", 7)}]),
    ("test_gpu_planned_slots", "test_sequences_without_windows_interleaved", [{"mol,k": ("hp", 5), "empty_ends": True}]),
    ("test_gpu_planned_slots", "test_query_side_postings_and_hits", [{"lookback": False}, {"lookback": True}]),
    ("test_gpu_mask", "test_mask_bytes_and_counts", [{"W,k1,k2": (12, 2200, 2500)}]),
    ("test_gpu_mask", "test_split_arrays", [{"min_len": 7}]),
    ("test_gpu_mask", "test_sketch_masked_matches_the_oracle", [{"mol,k,scaled": ("protein", 7, 1), "path": None},
                                                                {"mol,k,scaled": ("hp", 24, 5), "path": "1"},
                                                                {"mol,k,scaled": ("dayhoff", 16, 5), "path": "2"}]),
    ("test_gpu_mask", "test_masked_positions", [{"mol,k,scaled": ("protein", 7, 1)}]),
    ("test_gpu_translate", "test_translate6_bytes_and_offsets", [{}]),
    ("test_gpu_translate", "test_sketch_translated_matches_the_oracle", [{"mol,k,scaled": ("protein", 7, 1), "path": None},
                                                                         {"mol,k,scaled": ("hp", 24, 5), "path": "1"},
                                                                         {"mol,k,scaled": ("dayhoff", 16, 5), "path": "2"}]),
    ("test_gpu_forced_paths", "test_ticket_repeat_counts_repeated_kmers_once", [{"mol,k,scaled": ("hp", 5, 1)}]),
    ("test_gpu_parity", "test_kmer_positions_vs_oracle", [{}]),
    ("test_gpu_parity", "test_kmer_positions_ragged_and_tile_edges", [{}]),
    ("test_gpu_translate", "test_union_groups_crafted", PATHS3),
    ("test_gpu_translate", "test_union_groups_of_a_device_sketch_with_repeats", PATHS3),
    ("test_gpu_crafted_search", "test_union_equals_the_reference", [{"name": "union_saturation"}, {"name": "row_lengths"}]),
    ("test_gpu_parity", "test_sketches_from_host_roundtrip", [{}]),
    # ---- search ---------------------------------------------------------------------------------------------------------------
    ("test_gpu_parity", "test_index_build_paths_agree", [{"nt,k,scaled,mol": (3, 5, 1, "protein")}, {"nt,k,scaled,mol": (2500, 7, 1, "hp")}]),
    ("test_gpu_parity", "test_index_of_one_or_two_postings_on_both_build_paths", [{"targets": Nth(i)} for i in range(4)]),
    ("test_gpu_parity", "test_index_kats", [{}]),
    ("test_gpu_parity", "test_search_vs_oracle", [{"k,scaled,mol,nt,nq": (5, 1, "hp", 120, 90)},
                                                  {"k,scaled,mol,nt,nq": (7, 1, "protein", 2000, 1500)}]),
    ("test_gpu_parity", "test_golden_search", [{}]),
    ("test_gpu_parity", "test_search_self_and_empty", [{}]),
    ("test_gpu_parity", "test_join_fingerprints_segments_and_retry_are_exact", [{"k,scaled,mol,nt,nq": (5, 1, "hp", 150, 120)}]),
    ("test_gpu_parity", "test_join_kernels_agree_on_heavily_repeated_hashes", [{}]),
    ("test_gpu_parity", "test_nine_byte_bucket_postings_equal_plain_search", [{"sparse": "0"}, {"sparse": "1"}]),
    ("test_gpu_forced_paths", "test_long_sequences_as_queries_of_the_one_call_search",
     [{"batch": "random", "setting,no_compact": ("protein", False), "fmt": "10"}, {"batch": "homopolymer", "setting,no_compact": ("dayhoff", True), "fmt": "12"}]),
    ("test_gpu_parity", "test_presorted_query_postings_equal_plain_search", [{"k,scaled,mol,nt,nq": (5, 1, "hp", 150, 120)},
                                                                             {"k,scaled,mol,nt,nq": (10, 1, "protein", 300, 2000)}]),
    ("test_gpu_crafted_search", "test_family_under_knob_set", [{"name,knob": ("prefix_edges_s1", k)} for k in
                                                               ("default", "key_columns", "fp_staged", "fp_sparse", "fp_sparse_segs",
                                                                "index_lsd", "pairs_lsd")]),
    ("test_gpu_crafted_search", "test_copy_to_device_round_trips", [{"name": "one_bucket"}]),
    ("test_gpu_qfilter", "test_index_of_one_and_two_postings", [{"n_postings": 1}, {"n_postings": 2}]),
    ("test_gpu_qfilter", "test_hand_made_index_on_the_bitmaps_edges", [{"sparse": "0"}, {"sparse": "1"}]),
    ("test_gpu_qfilter2", "test_self_batch_drops_nothing", [{"occ": 3}, {"occ": 6}]),
    ("test_gpu_qfilter2", "test_the_filter_is_what_it_says", [{"width": 9, "sparse": "0"}, {"width": 12, "sparse": "1"}]),
    ("test_gpu_parity", "test_search_slices_the_queries_when_the_records_are_too_wide", [{}]),
    ("test_gpu_parity", "test_search_slices_the_queries_when_the_match_list_is_too_long", [{}]),
    ("test_gpu_parity", "test_one_call_sketch_search_equals_the_two_calls", [{"k,scaled,mol,nt,nq,env": Nth(5)}, {"k,scaled,mol,nt,nq,env": Nth(6)}]),
    ("test_gpu_parity", "test_one_call_sketch_search_edge_batches", [{}]),
    ("test_gpu_rows_aggregate", "test_aggregate_rows_equal_sorted_rows_and_oracle", [{"batch": "few", "segs": False}, {"batch": "few", "segs": True}]),
    ("test_gpu_rows_aggregate", "test_hand_made_sketches_sum_beyond_32_bits_and_sparse_regions", [{}]),
    ("test_gpu_rows_aggregate", "test_min_containment_on_both_paths", [{"min_c": 0.5}]),
    ("test_gpu_rows_aggregate", "test_query_slices", [{}]),
    ("test_gpu_search_rows", "test_stats_match_the_host_replica", [{"name": "hp5"}, {"name": "protein10"}]),
    ("test_gpu_search_rows", "test_threshold_keeps_the_rows_of_the_host_test", [{"name": "hp5"}]),
    ("test_gpu_search_rows", "test_forced_paths", [{"name": "hp5", "knob": k} for k in range(7)]),
    ("test_gpu_search_rows", "test_forced_ticket_repeat_with_stats_and_threshold", [{}]),
    ("test_gpu_search_rows", "test_object_api_rows_and_threshold", [{}]),
    # ---- hit-list passes ------------------------------------------------------------------------------------------------------
    ("test_gpu_signif", "test_golden_rows_through_context_significance", [{}]),
    ("test_gpu_signif", "test_crafted_sketches_on_both_row_paths", [{}]),
    ("test_gpu_signif", "test_row_lengths_family_on_both_row_paths", [{}]),
    ("test_gpu_signif", "test_corpus_tables", [{}]),
    ("test_gpu_signif", "test_corpora_passed_in_give_the_same_columns", [{}]),
    ("test_gpu_best", "test_segment_length_ladder", [{"mode": m} for m in (None, "1", "2", "3")]),
    ("test_gpu_best", "test_all_ties_keep_the_smallest_tids", [{"mode": m} for m in (None, "1", "2", "3")]),
    ("test_gpu_best", "test_external_score_column", [{"mode": None}]),
    ("test_gpu_cluster", "test_random_graphs", [{"kind": "sparse", "path": None}, {"kind": "dense", "path": "1"}, {"kind": "sparse", "path": "2"}]),
    ("test_gpu_cluster", "test_chains", [{"kind": "chain_permuted", "path": p} for p in (None, "1", "2")]),
    ("test_gpu_cluster", "test_representative", [{"path": None}]),
    ("test_gpu_greedy", "test_random_graphs", [{"kind": "sparse", "path": None}, {"kind": "dense", "path": "1"}, {"kind": "sparse", "path": "2"}]),
    ("test_gpu_greedy", "test_stars", [{"kind": "star_high", "path": p} for p in (None, "1", "2")]),
    ("test_gpu_greedy", "test_edge_list_around_the_tail_threshold", [{"path": None}]),
    ("test_gpu_gather", "test_hand_made_segments", [{}]),
    ("test_gpu_gather", "test_segment_length_ladder", [{}]),
    ("test_gpu_gather", "test_row_length_edges", [{}]),
    ("test_gpu_gather", "test_staggered_windows_around_a_chunk_edge", [{}]),
    ("test_gpu_exchange", "test_pack_unpack_field_widths", [{"ctx": "own_stream", "which,qbits,tbits": ("big", 20, 12)}, {"ctx": "own_stream", "which,qbits,tbits": ("two", 1, 2)}]),
    ("test_gpu_exchange", "test_pack_flags_an_id_one_beyond_its_field", [{"ctx": "own_stream", "qbits,tbits": (20, 12)}]),
    ("test_gpu_exchange", "test_unpack_at_pointer_offsets_between_guards", [{"ctx": "own_stream", "at,c": (257, 257)}]),
    ("test_gpu_exchange", "test_counting_merge_equals_stable_argsort", [{"ctx": "own_stream", "name": n} for n in ("w3", "empty_middle", "scan_2x1025", "scan_64x33")]),
    ("test_gpu_exchange", "test_exchange_on_different_shards", [{"ctx": "own_stream", "name": "w3_shard_order"}, {"ctx": "own_stream", "name": "w3_escapes_gather"}]),
    ("test_gpu_exchange", "test_device_block_equals_the_host_packing_of_dist", [{"ctx": "own_stream", "case": "two"}]),
    # ---- regions --------------------------------------------------------------------------------------------------------------
    ("test_gpu_matchpos", "test_search_extract_kmers_device_equals_the_golden_rows", [{}]),
    ("test_gpu_matchpos", "test_repeats_give_m_times_n_pairs_in_one_row", [{}]),
    ("test_gpu_matchpos", "test_forced_row_slices_give_the_same_result", [{}]),
    ("test_gpu_matchpos", "test_table_objects_agree_with_the_fetching_calls", [{}]),
    ("test_gpu_regions", "test_golden_seven_regions_from_the_device", [{}]),
    ("test_gpu_regions", "test_repeat_rows_next_to_ordinary_rows", [{}]),
    ("test_gpu_regions", "test_gap_boundary_substitutions_and_an_insertion", [{}]),
    ("test_gpu_regions", "test_forced_slices_and_sort_variants_give_the_same_result", [{}]),
    ("test_gpu_region_scores", "test_golden", [{"k,scaled,mol,n_regions": (15, 5, "hp", 17)}]),
    ("test_gpu_region_scores", "test_crafted_extension_lengths", [{"side": 1}, {"side": -1}]),
    ("test_gpu_region_scores", "test_many_regions_in_one_row_next_to_rows_with_none", [{}]),
    ("test_gpu_region_align", "test_terminations_and_ends_around_the_chunk", [{"side": 1}]),
    ("test_gpu_region_align", "test_indels_at_the_band_edge", [{"W": 16}]),
    ("test_gpu_region_align", "test_tie_heavy_fuzz", [{"gap_open,gap_extend": (1, 1)}]),
    ("test_gpu_region_trace", "test_indels_at_the_band_edge", [{"W": 16}]),
    ("test_gpu_region_trace", "test_end_cells_around_the_chunk", [{"side": -1}]),
    ("test_gpu_region_trace", "test_tie_heavy_fuzz", [{"gap_open,gap_extend": (0, 1)}]),
    ("test_gpu_region_trace", "test_slices_under_a_small_budget", [{}]),
    ("test_gpu_profile", "test_equivalence_around_the_chunk", [{"side": 1}]),
    ("test_gpu_profile", "test_equivalence_on_indels_ties_and_an_asymmetric_matrix", [{}]),
    ("test_gpu_profile", "test_position_specific_rows_move_the_diagonal_and_the_x_drop", [{}]),
    ("test_gpu_profile", "test_position_specific_fuzz", [{}]),
    ("test_gpu_region_cull", "test_fixed_cases", MODES3),
    ("test_gpu_region_cull", "test_synthetic_rows", [{"mode_ctx": None, "which,opts": Nth(0)}, {"mode_ctx": "1", "which,opts": Nth(3)},
                                                     {"mode_ctx": "2", "which,opts": Nth(5)}]),
    ("test_gpu_region_cull", "test_object_entry_points_against_the_reference", [{}]),
    ("test_gpu_region_cull", "test_take_gathers_every_column", [{}]),
    ("test_gpu_region_chain", "test_fixed_cases", MODES3),
    ("test_gpu_region_chain", "test_synthetic_rows", [{"mode_ctx": None, "which,opts": Nth(0)}, {"mode_ctx": "1", "which,opts": Nth(2)},
                                                      {"mode_ctx": "2", "which,opts": Nth(5)}]),
    ("test_gpu_region_chain", "test_object_entry_points_against_the_reference", [{}]),
    ("test_gpu_region_chain", "test_coverage_bit_for_bit", [{}]),
    ("test_gpu_region_stitch", "test_fixed_pairs", [{}]),
    ("test_gpu_region_stitch", "test_rows_of_0_1_2_and_9_members", [{}]),
    ("test_gpu_region_stitch", "test_fuzz_whole_and_in_slices", [{"i": 0}]),
    ("test_gpu_ffold", "test_synthetic_fold_equals_reference", [{"variant": v} for v in ("full", "bare", "no_t_length")]),
    ("test_gpu_ffold", "test_planted_frameshifts_end_to_end", [{}]),
    ("test_gpu_frame_stitch", "test_worked_examples", [{}]),
    ("test_gpu_frame_stitch", "test_rows_of_0_1_2_and_9_members", [{}]),
    ("test_gpu_frame_stitch", "test_fuzz_whole_and_in_slices", [{"i": 0}]),
    ("test_gpu_frame_stitch", "test_single_frame_rows_equal_stitch_chains_and_row_score_ranks", [{}]),
    # ---- coverage and PSSM ----------------------------------------------------------------------------------------------------
    ("test_gpu_pileup", "test_cases_equal_the_reference", [{"name": n} for n in ("boundary", "lane_tails", "csr", "fuzz", "rstitch_stitched", "fstitch")]),
    ("test_gpu_pileup", "test_row_masks", [{"which": "every_second"}]),
    ("test_gpu_pileup", "test_csr_and_one_entry_per_row_agree", [{}]),
    ("test_gpu_pileup", "test_golden_pair_through_the_wire", [{}]),
    ("test_gpu_pileup", "test_planted_contigs_through_the_wire", [{}]),
    ("test_gpu_pileup", "test_forced_paths_around_the_limit", MODES3),
    ("test_gpu_pweights", "test_worked_examples", [{}]),
    ("test_gpu_pweights", "test_weights_and_weighted_pileup_equal_the_reference", [{"name": n} for n in ("lane_tails", "csr", "fuzz")]),
    ("test_gpu_pweights", "test_fuzz_under_random_weights_on_every_path", [{"mode": "1"}, {"mode": "2"}]),
    ("test_gpu_pweights", "test_the_wrappers_on_the_stitch_cases", [{}]),
    ("test_gpu_pweights", "test_wbuild_small_batches", [{"include_query": True}, {"include_query": False}]),
    ("test_gpu_pweights", "test_wbuild_from_a_pileup_and_its_refusals", [{}]),
    ("test_gpu_profile", "test_build_small_batches", [{"include_query": True}, {"include_query": False}]),
    ("test_gpu_profile", "test_build_fuzz", [{}]),
    ("test_gpu_profile", "test_build_from_a_pileup_and_its_refusals", [{}]),
    ("test_gpu_astats", "test_composition_every_path", MODES3),
    ("test_gpu_astats", "test_random_rows_bit_identical", [{"name": "random"}]),
    ("test_gpu_astats", "test_crafted_fallback_rows", [{"name": "pm1"}]),
    ("test_gpu_astats", "test_golden_end_to_end", [{}]),
    # ---- primitives: one size on each side of a tile boundary for each scan kind, LSD with 4- and 8-byte values, MSD -------------
    ("test_gpu_prims", "test_scan_sizes", [{"kind": k, "knob": None, "n": n} for k in (0, 1, 2) for n in (2048, 2049)]
     + [{"kind": k, "knob": "1", "n": 4097} for k in (0, 1, 2)]),
    ("test_gpu_prims", "test_lsd_sizes", [{"vbytes": v, "alias": a, "n": n} for v, a in ((4, 0), (8, 1)) for n in (8192, 8193)]),
    ("test_gpu_prims", "test_msd_uniform", [{"nbits,lo_bit": (24, 0), "n": 65537}, {"nbits,lo_bit": (40, 12), "n": 65536}]),
    ("test_gpu_prims", "test_msd_skew_into_the_large_bucket_kernel", [{"skew": "one_bucket_6000", "nbits,lo_bit": (32, 12), "lds_cap": None},
                                                                      {"skew": "all_equal", "nbits,lo_bit": (24, 0), "lds_cap": "64"}]),
    ("test_gpu_prims", "test_scan_ring_end_tag_period_and_ticket_wrap", [{}]),
    # ---- refusals: a stale first-offender word is the wrong answer here ----------------------------------------------------------
    ("test_gpu_ffold", "test_refusals_name_the_first_offender", [{"kind,index,change": Nth(i)} for i in (1, 3, 5, 8, 10, 11)]),
    ("test_gpu_pileup", "test_refusals_name_the_first_offender", [{}]),
    ("test_gpu_pileup", "test_frame_alignments_refuse_the_query_side_and_the_profile_by_name", [{}]),
    ("test_gpu_region_stitch", "test_errors", [{}]),
    ("test_gpu_frame_stitch", "test_refusals_name_the_first_offender", [{}]),
    ("test_gpu_gather", "test_refusals_leave_the_context_usable", [{}]),
    ("test_gpu_best", "test_refusals_leave_the_context_usable", [{}]),
    ("test_gpu_region_chain", "test_errors", [{}]),
    ("test_gpu_region_cull", "test_errors", [{}]),
    ("test_gpu_pweights", "test_counts_of_other_entries_are_refused", [{}]),
]

# ---- the complement ----------------------------------------------------------------------------------------------------------------
def declared():
    """Every ks_* prototype of include/kmerseek_amd.h (the helper of tests/test_abi.py)."""
    import test_abi
    return test_abi.declared_functions()


def exempt():
    """{name: reason} of the prototypes the table need not reach (tests/pool_fill_exempt.py)."""
    import pool_fill_exempt
    return dict(pool_fill_exempt.EXEMPT)


# ---- the table against the functions -------------------------------------------------------------------------------------------------
BUILTIN = ("monkeypatch", "tmp_path", "request")


def load(module):
    return importlib.import_module(module)


def is_fixture(obj):
    return hasattr(obj, "_fixture_function_marker") or hasattr(obj, "_pytestfixturefunction")


def fixture_marker(obj):
    return getattr(obj, "_fixture_function_marker", None) or getattr(obj, "_pytestfixturefunction")


def fixture_function(obj):
    """The plain function behind a pytest.fixture (pytest refuses a direct call of the fixture itself)."""
    if hasattr(obj, "_get_wrapped_function"):
        return obj._get_wrapped_function()
    if hasattr(obj, "__pytest_wrapped__"):
        return obj.__pytest_wrapped__.obj
    return obj.__wrapped__


def parametrisations(fn):
    """{argnames as written: [values]} of the function's pytest.mark.parametrize marks."""
    out = {}
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            out[m.args[0] if isinstance(m.args[0], str) else ",".join(m.args[0])] = [getattr(v, "values", v) for v in m.args[1]]
    return out


def conftest_fixtures():
    import conftest
    return {n for n in dir(conftest) if is_fixture(getattr(conftest, n))}


def resolve(module, fn, pset):
    """(keyword arguments from the parametrize marks, {fixture: its parameter}) of one parameter set; ValueError names what does not fit."""
    marks, kw, fparams = parametrisations(fn), {}, {}
    for key, val in pset.items():
        if key in marks:
            values = marks[key]
            if isinstance(val, Nth):
                if not 0 <= val.i < len(values):
                    raise ValueError(f"{key}: {val} of {len(values)} values")
                val = values[val.i]
            elif val not in values:
                raise ValueError(f"{key}: {val!r} is none of the function's own values")
            names = [a.strip() for a in key.split(",")]
            kw.update(zip(names, val) if len(names) > 1 else [(names[0], val)])
        elif is_fixture(getattr(module, key, None)) and fixture_marker(getattr(module, key)).params is not None:
            if val not in tuple(fixture_marker(getattr(module, key)).params):
                raise ValueError(f"{key}: {val!r} is no parameter of the fixture")
            fparams[key] = val
        else:
            raise ValueError(f"{key}: neither a parametrize mark nor a parametrised fixture of the function")
    missing = [k for k in marks if k not in pset]
    if missing:
        raise ValueError(f"no value for {missing}")
    return kw, fparams


def sources(module, fn, pset):
    """{argument: where its value comes from} for one call: 'param', 'builtin', 'conftest', 'fixture' (of the module, `ctx` among them;
    its own arguments included under 'fixture:<name>.<arg>'), or 'unknown'."""
    kw, fparams = resolve(module, fn, pset)
    conf, out = conftest_fixtures(), {}

    def walk(prefix, f, given):
        for a in inspect.signature(f).parameters:
            name = prefix + a
            if a in given:
                out[name] = "param"
            elif a in BUILTIN:
                out[name] = "builtin"
            elif is_fixture(getattr(module, a, None)):
                fx = getattr(module, a)
                if fixture_marker(fx).params is not None and a not in fparams:
                    out[name] = "unknown"
                    continue
                out[name] = "fixture"
                walk(f"fixture:{a}.", fixture_function(fx), {})
            elif a in conf:
                out[name] = "conftest"
            else:
                out[name] = "unknown"

    walk("", fn, kw)
    return out


def case_id(module, function, pset):
    def show(v):
        s = repr(v) if not isinstance(v, str) else v
        return re.sub(r"[^A-Za-z0-9_.+-]+", "_", s).strip("_")[:40]
    tail = "-".join(show(v) for v in pset.values())
    return f"{module[len('test_gpu_'):]}::{function[len('test_'):]}" + (f"[{tail}]" if tail else "")


def expand():
    """[(id, module, function, parameter set)] of the whole table, ids unique."""
    out, seen = [], set()
    for module, function, psets in CASES:
        for pset in psets:
            cid = case_id(module, function, pset)
            assert cid not in seen, cid
            seen.add(cid)
            out.append((cid, module, function, pset))
    return out
