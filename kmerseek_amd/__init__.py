"""kmerseek_amd — MI355X-native protein k-mer sketch-and-search (the hot path of seanome/kmerseek).

All compute lives in libkmerseek_amd.so (hand-written HIP for gfx950) behind the C ABI of
include/kmerseek_amd.h.  There is no CPU fallback: importing is cheap, but any call needs the
built library and a GPU.
"""
from ._lib import KmerseekLibraryError, SO_PATH  # noqa: F401
from .engine import (AlignmentStats, Composition, Context, Corpus, EntryWeights, FrameFold, HitAlignments, Hits, Index, InvalidAminoAcid, KmerPositions, KmerseekError, Mask, MatchPositions, Profile, ProfileParams, Regions,  # noqa: F401
                     RegionAlignments, RegionChain, RegionCigars, RegionCull, RegionScores, Segments, Significance, Sketches, KS_WEIGHT_ONE, SEED, karlin_ungapped, make_params, max_hash, moltype_id, pack, profile_params, validate_and_resolve)

__all__ = ["Context", "Sketches", "Index", "Hits", "KmerPositions", "MatchPositions", "Regions", "RegionScores", "RegionAlignments", "RegionCigars", "RegionCull", "RegionChain", "FrameFold", "HitAlignments", "Composition", "EntryWeights", "Profile", "ProfileParams", "AlignmentStats", "Corpus", "Significance", "Mask", "Segments", "KmerseekError", "InvalidAminoAcid", "KmerseekLibraryError",
           "KS_WEIGHT_ONE", "SEED", "karlin_ungapped", "make_params", "max_hash", "moltype_id", "pack", "profile_params", "validate_and_resolve", "SO_PATH"]
