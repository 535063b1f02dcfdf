"""Object wrappers over the C ABI (include/kmerseek_amd.h): Context, Sketches, Index, Hits.

Host arrays are numpy; device-resident inputs are passed as raw pointers (e.g. ``tensor.data_ptr()``),
so nothing here depends on torch.  All compute happens in the HIP library.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import types
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import ks_params

MOLTYPES = {"protein": _lib.KS_PROTEIN, "raw": _lib.KS_PROTEIN, "dayhoff": _lib.KS_DAYHOFF, "hp": _lib.KS_HP}
MOLTYPE_NAMES = {_lib.KS_PROTEIN: "protein", _lib.KS_DAYHOFF: "dayhoff", _lib.KS_HP: "hp"}
SEED = _lib.KS_SEED_DEFAULT  # src/rust/signature.rs:12


class KmerseekError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


class InvalidAminoAcid(KmerseekError):
    """IndexError::InvalidAminoAcid(char, position) — src/rust/errors.rs:14-15."""

    def __init__(self, char: str, position: int, seq_index: int = 0):
        super().__init__(_lib.KS_ERR_INVALID_RESIDUE, f"Invalid amino acid '{char}' found at position {position}")
        self.char, self.position, self.seq_index = char, position, seq_index


def moltype_id(moltype: str) -> int:
    L = _lib.load()
    out = C.c_uint32(0)
    st = L.ks_moltype_from_string(moltype.encode(), C.byref(out))
    if st != _lib.KS_OK:
        # message of src/rust/encoding.rs:22-25
        raise KmerseekError(st, f"Invalid moltype: {moltype}, only 'protein', 'hp', or 'dayhoff' are supported")
    return out.value


def make_params(ksize: int, scaled: int, moltype: str, seed: int = SEED) -> ks_params:
    return ks_params(ksize=int(ksize), scaled=int(scaled), moltype=moltype_id(moltype), flags=0, seed=int(seed))


def max_hash(scaled: int) -> int:
    return int(_lib.load().ks_max_hash(int(scaled)))


def validate_and_resolve(seq: bytes, upper: bool = False, rng_seed: int = 0) -> bytes:
    """Host pre-step (src/rust/aminoacid.rs:74-105); raises InvalidAminoAcid."""
    L = _lib.load()
    out = C.create_string_buffer(len(seq) + 1)
    out_len = C.c_uint64(0)
    err = _lib.ks_residue_error()
    st = L.ks_validate_and_resolve(seq, len(seq), 1 if upper else 0, rng_seed, out, C.byref(out_len), C.byref(err))
    if st == _lib.KS_ERR_INVALID_RESIDUE:
        raise InvalidAminoAcid(chr(err.residue), err.position)
    if st != _lib.KS_OK:
        raise KmerseekError(st, L.ks_status_string(st).decode())
    return out.raw[:out_len.value]


def pack(seqs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """Concatenate records into (residues u8, offsets u64[n+1]) — the batch layout of the C ABI."""
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    res = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy() if len(seqs) else np.zeros(0, np.uint8)
    return res, offs


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _matrix28(matrix) -> Optional[np.ndarray]:
    """A substitution matrix as the C ABI takes it (contiguous int8 [28, 28]), or None."""
    if matrix is None:
        return None
    m = np.asarray(matrix)
    if m.shape != (_lib.KS_RSCORE_ALPHABET, _lib.KS_RSCORE_ALPHABET) or m.dtype != np.int8:
        raise ValueError("matrix must be an int8 array of shape (28, 28)")
    return np.ascontiguousarray(m)


def _int_in(name: str, v, top: int, shown: Optional[str] = None) -> int:
    """v as an int in [0, top], or ValueError "<name> = <v> is not an integer in [0, <top>]" (shown: the bound as the text says it)."""
    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= top:
        raise ValueError(f"{name} = {v} is not an integer in " + (shown or f"[0, {top}]"))
    return int(v)


def _profile_or_matrix(profile, matrix):
    """profile= of a region pass: a Profile or None, exclusive with matrix=; returns it."""
    if profile is not None and not isinstance(profile, Profile):
        raise TypeError("profile= takes a Profile (Context.build_profile)")
    if profile is not None and matrix is not None:
        raise ValueError("profile= and matrix= are exclusive: a pair scores under the one or the other")
    return profile


PILEUP_SIDES = {"query": _lib.KS_PILEUP_QUERY, "target": _lib.KS_PILEUP_TARGET}
KS_WEIGHT_ONE = _lib.KS_WEIGHT_ONE  # the weight 1 of an entry: weights are u32 in units of 2^-30


def _pileup_opts(side: str, profile: bool):
    """ks_pileup_opts of Context.pileup / pileup_device, or ValueError for a side that is neither."""
    if side not in PILEUP_SIDES:
        raise ValueError(f"side = {side!r} is neither \"query\" nor \"target\"")
    return _lib.ks_pileup_opts(_lib.KS_PILEUP_PROFILE if profile else 0, PILEUP_SIDES[side], 0)


def karlin_ungapped(matrix, freq_q, freq_t) -> Tuple[float, float, float]:
    """ks_karlin_ungapped: (lambda, K, H) of `matrix` (int8 [28, 28], None: +1 / -1) without gaps under the residue-class
    weights freq_q and freq_t (28 each, of which the 20 standard classes count, renormalised).  Host only, no context."""
    L = _lib.load()
    m = _matrix28(matrix)
    fq = np.ascontiguousarray(freq_q, dtype=np.float64); ft = np.ascontiguousarray(freq_t, dtype=np.float64)
    if fq.shape != (_lib.KS_RSCORE_ALPHABET,) or ft.shape != (_lib.KS_RSCORE_ALPHABET,):
        raise ValueError("freq_q and freq_t must hold 28 weights each")
    lam, K, H = C.c_double(0), C.c_double(0), C.c_double(0)
    dp = C.POINTER(C.c_double)
    st = L.ks_karlin_ungapped(m.ctypes.data_as(C.POINTER(C.c_int8)) if m is not None else None, fq.ctypes.data_as(dp), ft.ctypes.data_as(dp),
                              C.byref(lam), C.byref(K), C.byref(H))
    if st != _lib.KS_OK:
        raise KmerseekError(st, "karlin_ungapped: " + (L.ks_karlin_last_error() or L.ks_status_string(st)).decode())
    return lam.value, K.value, H.value


STANDARD_CLASSES = tuple(ord(c) - 65 for c in "ACDEFGHIKLMNPQRSTVWY")  # the 20 residue classes karlin_ungapped counts


class ProfileParams:
    """The options of Context.build_profile (ks_profile_opts), all host data: matrix int8 [28, 28] (the fallback; None: +1 / -1),
    bg f64 [28] >= 0 (a class with bg == 0 is unmodelled), ratio f64 [28, 28] (R[j][c]), beta >= 0, thresholds f64 [n <= 254]
    strictly ascending, base (the score below the first threshold) and include_query.  include/kmerseek_amd.h has the rule;
    profile_params makes them from a matrix.  ValueError for what the library would refuse."""

    def __init__(self, matrix, bg, ratio, beta: float, thresholds, base: int, include_query: bool = True):
        A = _lib.KS_RSCORE_ALPHABET
        self.matrix = _matrix28(matrix)
        self.bg = np.ascontiguousarray(bg, dtype=np.float64)
        self.ratio = np.ascontiguousarray(ratio, dtype=np.float64)
        self.thresholds = np.ascontiguousarray(thresholds, dtype=np.float64)
        self.beta, self.include_query = float(beta), bool(include_query)
        if self.bg.shape != (A,) or self.ratio.shape != (A, A) or self.thresholds.ndim != 1:
            raise ValueError("bg must hold 28 weights, ratio 28 x 28 values, thresholds one row")
        if len(self.thresholds) > _lib.KS_PROFILE_MAX_THRESHOLDS:
            raise ValueError(f"{len(self.thresholds)} thresholds: at most {_lib.KS_PROFILE_MAX_THRESHOLDS}")
        if np.isnan(self.bg).any() or np.isnan(self.ratio).any() or np.isnan(self.thresholds).any() or self.beta != self.beta:
            raise ValueError("a NaN among bg, ratio, beta or the thresholds")
        if (self.bg < 0).any() or self.beta < 0:
            raise ValueError("a negative bg or beta")
        if not (np.diff(self.thresholds) > 0).all():
            raise ValueError("the thresholds do not ascend strictly")
        self.base = _int_in("base + 2^31", int(base) + 2 ** 31, 2 ** 32 - 1, "[0, 2^32): base is a 32-bit integer") - 2 ** 31

    def _opts(self):
        """(ks_profile_opts, the arrays its pointers read: keep them alive for the call)"""
        dp = C.POINTER(C.c_double)
        mp = self.matrix.ctypes.data_as(C.POINTER(C.c_int8)) if self.matrix is not None else None
        th = self.thresholds.ctypes.data_as(dp) if len(self.thresholds) else None
        return _lib.ks_profile_opts(mp, self.bg.ctypes.data_as(dp), self.ratio.ctypes.data_as(dp), self.beta, th, len(self.thresholds), self.base,
                                    _lib.KS_PROFILE_INCLUDE_QUERY if self.include_query else 0, 0), self


def profile_params(matrix, freq=None, beta: float = 10.0, include_query: bool = True) -> ProfileParams:
    """ProfileParams in the units of `matrix` (int8 [28, 28], None: +1 / -1).  freq: 28 background weights of which the 20
    standard classes count, renormalised (None: uniform over them); every other class is unmodelled and keeps the matrix's
    entries.  With lambda = karlin_ungapped(matrix, bg, bg): ratio = exp(lambda * matrix), base = min(matrix) - 8 and
    thresholds[k] = exp(lambda * (base + k + 0.5)) up to max(matrix) + 8 — a score is ln r / lambda rounded to the nearest
    integer, clamped to that range.  The device and the tests' host loop read these very tables: no libm shows in a result."""
    A = _lib.KS_RSCORE_ALPHABET
    m = _matrix28(matrix)
    if m is None:
        m = (2 * np.eye(A, dtype=np.int8) - 1).astype(np.int8)
    w = np.full(A, 1.0) if freq is None else np.ascontiguousarray(freq, dtype=np.float64)
    if w.shape != (A,) or np.isnan(w).any() or (w < 0).any():
        raise ValueError("freq must hold 28 weights >= 0")
    bg = np.zeros(A)
    bg[list(STANDARD_CLASSES)] = w[list(STANDARD_CLASSES)]
    if not bg.sum() > 0:
        raise ValueError("freq gives the 20 standard residue classes no weight")
    bg /= bg.sum()
    # lambda alone (ks_karlin_ungapped with K == NULL): the series for K does not settle for every matrix a profile can be made of
    L, lam, dp = _lib.load(), C.c_double(0), C.POINTER(C.c_double)
    st = L.ks_karlin_ungapped(m.ctypes.data_as(C.POINTER(C.c_int8)), bg.ctypes.data_as(dp), bg.ctypes.data_as(dp), C.byref(lam), None, None)
    if st != _lib.KS_OK:
        raise KmerseekError(st, "profile_params: " + (L.ks_karlin_last_error() or L.ks_status_string(st)).decode())
    lam = lam.value
    base = int(m.min()) - 8
    n_thr = min(int(m.max()) + 8 - base, _lib.KS_PROFILE_MAX_THRESHOLDS)
    thresholds = np.exp(lam * (base + np.arange(n_thr) + 0.5))
    return ProfileParams(m, bg, np.exp(lam * m.astype(np.float64)), beta, thresholds, base, include_query)


def search_opts(min_containment: float = 0.0, abund_stats: bool = False) -> Optional[_lib.ks_search_opts]:
    """The ks_search_opts of the keyword arguments, or None for the defaults (the plain entry points are called then)."""
    if not abund_stats and min_containment == 0.0:
        return None
    return _lib.ks_search_opts(_lib.KS_SEARCH_ABUND_STATS if abund_stats else 0, 0, float(min_containment))


def mask_opts(window: int = 12, k1: float = 2.2, k2: float = 2.5) -> _lib.ks_mask_opts:
    """The ks_mask_opts of a window length and two thresholds in BITS (millibits by round(1000 k)).  The window is always
    named — a window below 2 is refused here, 0 included, which in the C struct would stand for the default — so k1 = k2 = 0
    reaches the library as given: it masks exactly the windows of one residue class."""
    if _int_in("window", window, _lib.KS_MASK_MAX_WINDOW, f"[2, {_lib.KS_MASK_MAX_WINDOW}]") < 2:
        raise ValueError(f"window = {window} is not an integer in [2, {_lib.KS_MASK_MAX_WINDOW}]")
    return _lib.ks_mask_opts(int(window), _int_in("k1 in millibits", round(1000 * k1), 2 ** 32 - 1),
                             _int_in("k2 in millibits", round(1000 * k2), 2 ** 32 - 1))


BEST_RANK_BY = {"intersect": _lib.KS_BEST_INTERSECT, "target_containment": _lib.KS_BEST_TARGET_CONTAINMENT,
                "max_containment": _lib.KS_BEST_MAX_CONTAINMENT, "jaccard": _lib.KS_BEST_JACCARD, "score": _lib.KS_BEST_SCORE}
GREEDY_ASSIGN = {"first": _lib.KS_GREEDY_ASSIGN_FIRST, "best": _lib.KS_GREEDY_ASSIGN_BEST}


class _FollowDebugEnv:
    """Library proxy of a diagnostic context: re-reads the KS_DEBUG_* variables before every call (the library itself reads
    them only when a context is created).  The tests use it to force the rarely taken paths on one context."""

    def __init__(self, L, ctx):
        self._L, self._ctx = L, ctx

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if not name.startswith("ks_") or name in ("ks_ctx_create", "ks_ctx_destroy", "ks_ctx_reload_debug_env", "ks_last_error",
                                                    "ks_status_string"):
            return f

        def call(*a):
            if self._ctx._h:
                self._L.ks_ctx_reload_debug_env(self._ctx._h)
            return f(*a)
        return call


class Context:
    """One HIP device + stream + workspace (ks_ctx).  Not thread-safe: one per host thread.

    stream: None — the context creates a non-blocking stream of its own; a raw ``hipStream_t`` value (e.g.
    ``torch.cuda.current_stream().cuda_stream``) — the context launches there, so its work is ordered with the caller's.
    0 is what torch reports for the device's default (null) stream: it is passed on as ``hipStreamLegacy``, and
    ``Context.stream`` reports it as 0 again, so ``ctx.stream == torch.cuda.current_stream().cuda_stream`` holds."""

    _HIP_STREAM_LEGACY = 1  # hip_runtime_api.h: #define hipStreamLegacy ((hipStream_t)1)

    def __init__(self, device: int = 0, stream: Optional[int] = None, follow_debug_env: bool = False):
        self._L = _lib.load()
        self._h = None
        if follow_debug_env:
            self._L = _FollowDebugEnv(self._L, self)
        h = C.c_void_p()
        sp = None if stream is None else C.c_void_p(int(stream) if int(stream) != 0 else self._HIP_STREAM_LEGACY)
        st = self._L.ks_ctx_create(int(device), sp, C.byref(h))
        if st != _lib.KS_OK:
            raise KmerseekError(st, f"ks_ctx_create(device={device}) failed: {self._L.ks_status_string(st).decode()}"
                                    " — the HIP path has no CPU fallback")
        self._h = h
        self.device = device
        self._pinned, self._close_pending = 0, False

    def close(self):
        """Destroy the context (its pool, stream, pinned blocks).  While views of library-owned device arrays are alive
        (`_Owned.pin`: the world-size-1 hit exchange hands out torch views) the destruction waits for the last of them —
        a view must never outlive the memory it points into."""
        if getattr(self, "_pinned", 0) > 0:
            self._close_pending = True
            return
        if getattr(self, "_h", None):
            self._L.ks_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st: int):
        if st != _lib.KS_OK:
            msg = self._L.ks_last_error(self._h).decode() or self._L.ks_status_string(st).decode()
            raise KmerseekError(st, msg)

    @property
    def stream(self) -> int:
        v = int(self._L.ks_ctx_stream(self._h) or 0)
        return 0 if v == self._HIP_STREAM_LEGACY else v

    def synchronize(self):
        self._check(self._L.ks_ctx_synchronize(self._h))

    def to_device(self, a: np.ndarray) -> "DeviceBuffer":
        """Copy a host array into a plain device buffer (for the *_device entry points without torch)."""
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self._check(self._L.ks_dev_malloc(self._h, a.nbytes, C.byref(p)))
        buf = DeviceBuffer(self, p, a.nbytes)
        self._check(self._L.ks_dev_upload(self._h, p, _ptr(a), a.nbytes))
        return buf

    @contextlib.contextmanager
    def _uploaded(self, *arrays):
        """Host arrays on the device for the time of one call: yields their device pointers, in order; freed on the way out."""
        bufs = []
        try:
            for a in arrays:
                bufs.append(self.to_device(a))
            yield [b.ptr for b in bufs]
        finally:
            for b in bufs:
                b.free()

    @contextlib.contextmanager
    def _batches(self, q_res, q_off, t_res, t_off):
        """The query and target residue batches of a region pass on the device for one call: yields the eight arguments the
        *_device variants take for them (d_q_res, d_q_off, n_q, n_q_res, d_t_res, d_t_off, n_t, n_t_res)."""
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8); q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        t_res = np.ascontiguousarray(t_res, dtype=np.uint8); t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        with self._uploaded(q_res, q_off, t_res, t_off) as (d_q, d_qo, d_t, d_to):
            yield d_q, d_qo, len(q_off) - 1, len(q_res), d_t, d_to, len(t_off) - 1, len(t_res)

    def _device_empty(self, nbytes: int) -> "DeviceBuffer":
        p = C.c_void_p()
        self._check(self._L.ks_dev_malloc(self._h, int(nbytes), C.byref(p)))
        return DeviceBuffer(self, p, int(nbytes))

    def pinned_empty(self, n: int, dtype) -> np.ndarray:
        """Uninitialised numpy array of n items in pinned host memory (ks_host_alloc): copies between such an array and the
        device run as one DMA at link rate, where a pageable array is staged through pinned buffers by host threads.
        The memory is released when the array (and every view of it) is garbage-collected."""
        dt = np.dtype(dtype)
        nbytes = max(int(n) * dt.itemsize, 1)
        p = C.c_void_p()
        self._check(self._L.ks_host_alloc(self._h, nbytes, C.byref(p)))
        buf = (C.c_char * nbytes).from_address(p.value)
        buf._owner = _PinnedBlock(self, p)  # the ctypes view is the array's base: it keeps the block alive
        return np.frombuffer(buf, dtype=dt, count=int(n))

    def pool_stats(self) -> Dict[str, int]:
        v = [C.c_uint64(0) for _ in range(4)]
        self._check(self._L.ks_ctx_pool_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("blocks", "bytes_held", "bytes_in_use", "mallocs"), (int(x.value) for x in v)))

    def sketch_stats(self, paths: bool = False) -> Dict[str, int]:
        """Repeats this context needed so far (see ks_ctx_sketch_stats): results never depend on them, run time does.
        paths=True adds `planned_slots`, the shared-tile launches whose tiles took the start of their CSR slots from the tile
        plan instead of a look-back across tiles: a path taken, not a repeat, so it grows in normal operation."""
        v = (C.c_uint64 * 5)()
        self._check(self._L.ks_ctx_sketch_stats(self._h, C.byref(v)))
        out = {"ticket_fallbacks": int(v[0]), "uses_ticket": int(v[1]), "compact_fallbacks": int(v[2]), "cap_fallbacks": int(v[3])}
        if paths:
            out["planned_slots"] = int(v[4])
        return out

    def unpack_hits64_device(self, d_packed: int, n: int, qbits: int, tbits: int, d_qid: int, d_tid: int, d_isect: int, d_nw: int):
        """Transport words -> columns, all device pointers (ks_hits_unpack64_device): the receiving side of the exchange."""
        self._check(self._L.ks_hits_unpack64_device(self._h, C.c_void_p(d_packed), n, qbits, tbits, C.c_void_p(d_qid), C.c_void_p(d_tid),
                                                    C.c_void_p(d_isect), C.c_void_p(d_nw)))

    def merge_hits_by_qid_device(self, d_qid: int, d_tid: int, d_isect: int, d_nw: int, block_rows: Sequence[int], n_queries: int,
                                 o_qid: int, o_tid: int, o_isect: int, o_nw: int):
        """Rank blocks of a gathered index-sharded hit list -> one list ordered by (qid, tid), all device pointers
        (ks_hits_merge_by_qid_device: a counting merge instead of a sort)."""
        rows = (C.c_uint64 * len(block_rows))(*[int(x) for x in block_rows])
        self._check(self._L.ks_hits_merge_by_qid_device(self._h, C.c_void_p(d_qid), C.c_void_p(d_tid), C.c_void_p(d_isect), C.c_void_p(d_nw),
                                                        rows, len(block_rows), int(n_queries), C.c_void_p(o_qid), C.c_void_p(o_tid),
                                                        C.c_void_p(o_isect), C.c_void_p(o_nw)))

    def reload_debug_env(self):
        """Re-read the KS_DEBUG_* variables (diagnostics: the library reads them only when a context is created)."""
        self._check(self._L.ks_ctx_reload_debug_env(self._h))

    def search_stats(self, paths: bool = False) -> Dict[str, int]:
        """Repeats ks_search needed so far on this context (see ks_ctx_search_stats): `agg_overflows` counts the searches whose
        aggregate row pass gave up and resumed the sort.  paths=True adds `agg_used`, the searches whose rows that pass made, and
        `join_table`, the searches whose join ran the table kernel: paths taken, not repeats, so they grow in normal operation
        while every other counter here stands still."""
        v = (C.c_uint64 * 5)()
        self._check(self._L.ks_ctx_search_stats(self._h, C.byref(v)))
        out = {"join_retries": int(v[0]), "rows_ticket_fallbacks": int(v[1]), "agg_overflows": int(v[3])}
        if paths:
            out["agg_used"] = int(v[2])
            out["join_table"] = int(v[4])
        return out

    # ---- test hooks: the device-wide primitives on device pointers (ks_debug_scan ... ks_debug_msd_sort) ----
    def debug_scan(self, kind: int, d_in: int, d_out: int, n: int, d_total: int = 0):
        """kind 0: u32 -> u64 into d_out[0 .. n] (d_out[n] = total); kind 1: u32 -> u32 into d_out[0 .. n), total to d_total (0: none);
        kind 2: kind 0 for sums of 2^38 and more (never the one-launch path)."""
        self._check(self._L.ks_debug_scan(self._h, int(kind), C.c_void_p(d_in), C.c_void_p(d_out), int(n), C.c_void_p(d_total or None)))

    def debug_scan_seek(self, global_tile: int):
        self._check(self._L.ks_debug_scan_seek(self._h, int(global_tile) & 0xffffffff))

    def debug_scan_ticket(self) -> int:
        v = C.c_uint32(0)
        self._check(self._L.ks_debug_scan_ticket(self._h, C.byref(v)))
        return int(v.value)

    def debug_radix_sort(self, vbytes: int, d_keys: int, d_vals: int, n: int, shifts: Sequence[int], d_keys_out: int, d_vals_out: int,
                         pfx_k: int = 0, d_seg_len: int = 0, seg_cap: int = 0, seg_regions: int = 0, alias_in: bool = False):
        sh = (C.c_int * max(len(shifts), 1))(*[int(s) for s in shifts])
        self._check(self._L.ks_debug_radix_sort(self._h, int(vbytes), C.c_void_p(d_keys), C.c_void_p(d_vals or None), int(n), sh, len(shifts),
                                                int(pfx_k), C.c_void_p(d_seg_len or None), int(seg_cap), int(seg_regions), int(bool(alias_in)),
                                                C.c_void_p(d_keys_out), C.c_void_p(d_vals_out or None)))

    def debug_msd_sort(self, d_keys: int, n: int, lo_bit: int, nbits: int, seg_count: Optional[Sequence[int]] = None,
                       seg_cap: int = 0) -> Dict[str, int]:
        """The match sort in place on d_keys; returns {done, bits2, n_buckets, big} as the library reports them."""
        info = (C.c_uint32 * 4)()
        sc = None if seg_count is None else (C.c_uint32 * max(len(seg_count), 1))(*[int(c) for c in seg_count])
        self._check(self._L.ks_debug_msd_sort(self._h, C.c_void_p(d_keys), int(n), int(lo_bit), int(nbits), sc,
                                              0 if seg_count is None else len(seg_count), int(seg_cap), C.byref(info)))
        return dict(zip(("done", "bits2", "n_buckets", "big"), (int(x) for x in info)))

    # ---- sketch ----
    def sketch_batch(self, residues: np.ndarray, offsets: np.ndarray, ksize: int, scaled: int, moltype: str,
                     seed: int = SEED) -> "Sketches":
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_sketch_batch(self._h, _ptr(residues), _ptr(offsets), len(offsets) - 1, C.byref(p),
                                            C.byref(out)))
        return Sketches(self, out)

    def sketch_batch_device(self, d_residues: int, d_offsets: int, n_seqs: int, n_residues: int, ksize: int,
                            scaled: int, moltype: str, max_seq_len: int = 0, seed: int = SEED) -> "Sketches":
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_sketch_batch_device(self._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs,
                                                   n_residues, max_seq_len, C.byref(p), C.byref(out)))
        return Sketches(self, out)

    def sketch_queries_device(self, index: "Index", d_residues: int, d_offsets: int, n_seqs: int, n_residues: int,
                              max_seq_len: int = 0) -> "Sketches":
        """Sketch a query batch for an immediate search against `index` (also emits pre-partitioned postings)."""
        out = C.c_void_p()
        self._check(self._L.ks_sketch_queries_device(self._h, index._h, C.c_void_p(d_residues), C.c_void_p(d_offsets),
                                                     n_seqs, n_residues, max_seq_len, C.byref(out)))
        return Sketches(self, out)

    def sketch_search_device(self, index: "Index", d_residues: int, d_offsets: int, n_seqs: int, n_residues: int,
                             max_seq_len: int = 0, want_sketches: bool = True, *, min_containment: float = 0.0,
                             abund_stats: bool = False):
        """ks_sketch_search_device: sketch a query batch and search it against `index` in one call (two host waits instead
        of three).  Returns (Sketches or None, Hits); same results as sketch_queries_device + search.  The keywords are
        those of `search`."""
        sk, hits = C.c_void_p(), C.c_void_p()
        opts = search_opts(min_containment, abund_stats)
        if opts is None:
            st = self._L.ks_sketch_search_device(self._h, index._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs,
                                                 n_residues, max_seq_len, C.byref(sk) if want_sketches else None, C.byref(hits))
        else:
            st = self._L.ks_sketch_search_device_ex(self._h, index._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs,
                                                    n_residues, max_seq_len, C.byref(opts), C.byref(sk) if want_sketches else None,
                                                    C.byref(hits))
        self._check(st)
        return (Sketches(self, sk) if want_sketches else None), Hits(self, hits)

    def sketch_search(self, index: "Index", residues: np.ndarray, offsets: np.ndarray, want_sketches: bool = True, *,
                      min_containment: float = 0.0, abund_stats: bool = False):
        """ks_sketch_search: the same from host arrays (upload, sketch, search).  Returns (Sketches or None, Hits)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        sk, hits = C.c_void_p(), C.c_void_p()
        opts = search_opts(min_containment, abund_stats)
        if opts is None:
            st = self._L.ks_sketch_search(self._h, index._h, _ptr(residues), _ptr(offsets), len(offsets) - 1,
                                          C.byref(sk) if want_sketches else None, C.byref(hits))
        else:
            st = self._L.ks_sketch_search_ex(self._h, index._h, _ptr(residues), _ptr(offsets), len(offsets) - 1, C.byref(opts),
                                             C.byref(sk) if want_sketches else None, C.byref(hits))
        self._check(st)
        return (Sketches(self, sk) if want_sketches else None), Hits(self, hits)

    # ---- translated search: nucleotide input ----
    def translate6(self, nt: np.ndarray, offsets: np.ndarray) -> Tuple["DeviceBuffer", "DeviceBuffer", int]:
        """ks_translate6_device on a host batch of nucleotide records (the layout of `pack`): (frames, frame_offsets, n_residues)
        — two DeviceBuffers, the residues u8 of the 6 x n frames (record s: 6s + f forward, 6s + 3 + f reverse) and their u64
        offsets [6n + 1], the batch layout every *_device sketch entry reads — and the residue count.  Standard code; any byte
        but ACGT (after upper-casing) makes its codon X; stops are '*'."""
        nt = np.ascontiguousarray(nt, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, n_nt = len(offsets) - 1, int(offsets[-1])
        if nt.size != n_nt:
            raise ValueError(f"offsets end at {n_nt}, the batch holds {nt.size} bases")
        d_nt = self.to_device(nt if n_nt else np.zeros(16, np.uint8))
        d_off = self.to_device(offsets)
        frames = self._device_empty(int(self._L.ks_translate6_bound(n_nt)) + 16)  # (+ 16: the sketch tiles load whole 16-byte words)
        foff = self._device_empty(8 * (6 * n + 1))
        n_res = C.c_uint64(0)
        try:
            self._check(self._L.ks_translate6_device(self._h, d_nt._p, d_off._p, n, n_nt, frames._p, foff._p, C.byref(n_res)))
        finally:
            d_nt.free(); d_off.free()
        return frames, foff, int(n_res.value)

    def sketch_translated(self, nt: np.ndarray, offsets: np.ndarray, ksize: int, scaled: int, moltype: str,
                          seed: int = SEED) -> "Sketches":
        """ks_sketch_translated: protein / dayhoff / hp sketches of NUCLEOTIDE records — every record translated in six frames,
        its sketch the union of the six frame sketches (abundances summed).  ksize is the protein k."""
        nt = np.ascontiguousarray(nt, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_sketch_translated(self._h, _ptr(nt), _ptr(offsets), len(offsets) - 1, C.byref(p), C.byref(out)))
        return Sketches(self, out)

    def sketch_translated_device(self, d_nt: int, d_offsets: int, n_seqs: int, n_nt: int, ksize: int, scaled: int, moltype: str,
                                 max_seq_len: int = 0, seed: int = SEED) -> "Sketches":
        """The same with the batch resident on the device (raw pointers); max_seq_len: a bound on the longest record in BASES,
        or 0 to have it measured."""
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_sketch_translated_device(self._h, C.c_void_p(d_nt), C.c_void_p(d_offsets), n_seqs, n_nt, max_seq_len,
                                                        C.byref(p), C.byref(out)))
        return Sketches(self, out)

    # ---- low-complexity masking ----
    def mask_low_complexity(self, residues: np.ndarray, offsets: np.ndarray, window: int = 12, k1: float = 2.2, k2: float = 2.5) -> "Mask":
        """ks_mask_batch: the low-complexity mask of a host batch (the layout of `pack`) under this library's own integer rule
        (include/kmerseek_amd.h; the first stage of SEG, no parity claimed): windows of `window` residues with at most k1 bits of
        entropy trigger, neighbouring windows with at most k2 bits extend.  `Mask.to_host()` gives (mask u8, masked_counts u32)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        o = mask_opts(window, k1, k2)
        out = C.c_void_p()
        self._check(self._L.ks_mask_batch(self._h, _ptr(residues), _ptr(offsets), len(offsets) - 1, C.byref(o), C.byref(out)))
        return Mask(self, out)

    def mask_low_complexity_device(self, d_residues: int, d_offsets: int, n_seqs: int, n_residues: int, window: int = 12, k1: float = 2.2,
                                   k2: float = 2.5) -> "Mask":
        """The same with the batch resident on the device (raw pointers)."""
        o = mask_opts(window, k1, k2)
        out = C.c_void_p()
        self._check(self._L.ks_mask_device(self._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs, n_residues, C.byref(o), C.byref(out)))
        return Mask(self, out)

    def split_masked(self, mask: "Mask", residues: np.ndarray, offsets: np.ndarray, min_len: int = 1) -> "Segments":
        """ks_mask_split_device on a host batch: the unmasked stretches of at least min_len residues of every record, in order, as
        a residue batch of their own (`Segments`)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        with self._uploaded(residues if residues.size else np.zeros(16, np.uint8), offsets) as (d_res, d_off):
            return self.split_masked_device(mask, d_res, d_off, len(offsets) - 1, int(residues.size), min_len)

    def split_masked_device(self, mask: "Mask", d_residues: int, d_offsets: int, n_seqs: int, n_residues: int, min_len: int = 1) -> "Segments":
        out = C.c_void_p()
        self._check(self._L.ks_mask_split_device(self._h, mask._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs, n_residues,
                                                 _int_in("min_len", min_len, 2 ** 32 - 1), C.byref(out)))
        return Segments(self, out)

    def sketch_masked(self, residues: np.ndarray, offsets: np.ndarray, ksize: int, scaled: int, moltype: str, window: int = 12,
                      k1: float = 2.2, k2: float = 2.5, seed: int = SEED) -> "Sketches":
        """ks_sketch_masked: the sketches of the records with their low-complexity stretches left out — the hashes of exactly
        those windows that hold no masked residue, abundances counted over those windows.  A plain `Sketches` of len(offsets) - 1
        records; a record that is masked throughout has an empty sketch."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        p, o = make_params(ksize, scaled, moltype, seed), mask_opts(window, k1, k2)
        out = C.c_void_p()
        self._check(self._L.ks_sketch_masked(self._h, _ptr(residues), _ptr(offsets), len(offsets) - 1, C.byref(p), C.byref(o), C.byref(out)))
        return Sketches(self, out)

    def sketch_masked_device(self, d_residues: int, d_offsets: int, n_seqs: int, n_residues: int, ksize: int, scaled: int, moltype: str,
                             max_seq_len: int = 0, window: int = 12, k1: float = 2.2, k2: float = 2.5, seed: int = SEED) -> "Sketches":
        """The same with the batch resident on the device (raw pointers); max_seq_len as in sketch_batch_device."""
        p, o = make_params(ksize, scaled, moltype, seed), mask_opts(window, k1, k2)
        out = C.c_void_p()
        self._check(self._L.ks_sketch_masked_device(self._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs, n_residues, max_seq_len,
                                                    C.byref(p), C.byref(o), C.byref(out)))
        return Sketches(self, out)

    def kmer_positions_table_masked(self, residues: np.ndarray, offsets: np.ndarray, ksize: int, scaled: int, moltype: str, window: int = 12,
                                    k1: float = 2.2, k2: float = 2.5, seed: int = SEED) -> "KmerPositions":
        """ks_kmer_positions_masked_device on a host batch: the k-mer position table of the windows a masked sketch is made of,
        in the records' own numbering and coordinates (the input of `match_positions` beside masked sketches)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        with self._uploaded(residues if residues.size else np.zeros(16, np.uint8), offsets) as (d_res, d_off):
            return self.kmer_positions_table_masked_device(d_res, d_off, len(offsets) - 1, int(residues.size), ksize, scaled, moltype,
                                                           window, k1, k2, seed)

    def kmer_positions_table_masked_device(self, d_residues: int, d_offsets: int, n_seqs: int, n_residues: int, ksize: int, scaled: int,
                                           moltype: str, window: int = 12, k1: float = 2.2, k2: float = 2.5, seed: int = SEED) -> "KmerPositions":
        p, o = make_params(ksize, scaled, moltype, seed), mask_opts(window, k1, k2)
        out = C.c_void_p()
        self._check(self._L.ks_kmer_positions_masked_device(self._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs, n_residues,
                                                            C.byref(p), C.byref(o), C.byref(out)))
        return KmerPositions(self, out)

    def qfilter_stats(self) -> Dict[str, int]:
        """Query postings the filtered bucket scatters of this context read / dropped (see ks_ctx_qfilter_stats)."""
        v = (C.c_uint64 * 2)()
        self._check(self._L.ks_ctx_qfilter_stats(self._h, C.byref(v)))
        return {"seen": int(v[0]), "dropped": int(v[1])}

    def fused_stats(self) -> Dict[str, int]:
        """ks_sketch_search_device calls on this context: with the sketch read-back deferred / repeated the plain way / with
        their rows made by the aggregate pass (`aggregated`: the `agg_used` of search_stats(paths=True), counted per call here) /
        with their join run by the table kernel (`table_joined`: the `join_table` of search_stats(paths=True), likewise)."""
        v = (C.c_uint64 * 4)()
        self._check(self._L.ks_ctx_fused_stats(self._h, C.byref(v)))
        return {"deferred": int(v[0]), "redos": int(v[1]), "aggregated": int(v[2]), "table_joined": int(v[3])}

    def sketches_from_host(self, offsets: np.ndarray, hashes: np.ndarray, abunds: np.ndarray, ksize: int,
                           scaled: int, moltype: str, seed: int = SEED) -> "Sketches":
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        abunds = np.ascontiguousarray(abunds, dtype=np.uint32)
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_sketches_from_host(self._h, _ptr(offsets), _ptr(hashes), _ptr(abunds),
                                                  len(offsets) - 1, C.byref(p), C.byref(out)))
        return Sketches(self, out)

    def kmer_positions(self, residues: np.ndarray, offsets: np.ndarray, ksize: int, scaled: int, moltype: str,
                       seed: int = SEED) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(seq u32, start u32, hash u64) of every kept window, ordered by (seq, start)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_kmer_positions(self._h, _ptr(residues), _ptr(offsets), len(offsets) - 1, C.byref(p),
                                              C.byref(out)))
        try:
            n = int(self._L.ks_kmerpos_count(out))
            seq = np.zeros(n, np.uint32); start = np.zeros(n, np.uint32); h = np.zeros(n, np.uint64)
            self._check(self._L.ks_kmerpos_copy_to_host(self._h, out, _ptr(seq), _ptr(start), _ptr(h)))
        finally:
            self._L.ks_kmerpos_free(out)
        return seq, start, h

    def kmer_positions_device(self, d_residues: int, d_offsets: int, n_seqs: int, n_residues: int, ksize: int, scaled: int,
                              moltype: str, seed: int = SEED, fetch: bool = True):
        """Same from device-resident buffers; fetch=False returns only the number of kept windows (table stays on the GPU
        and is freed) — what bench / profiling runs use."""
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_kmer_positions_device(self._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs, n_residues,
                                                     C.byref(p), C.byref(out)))
        try:
            n = int(self._L.ks_kmerpos_count(out))
            if not fetch:
                return n
            seq = np.zeros(n, np.uint32); start = np.zeros(n, np.uint32); h = np.zeros(n, np.uint64)
            self._check(self._L.ks_kmerpos_copy_to_host(self._h, out, _ptr(seq), _ptr(start), _ptr(h)))
        finally:
            self._L.ks_kmerpos_free(out)
        return seq, start, h

    def kmer_positions_table(self, residues: np.ndarray, offsets: np.ndarray, ksize: int, scaled: int, moltype: str,
                             seed: int = SEED) -> "KmerPositions":
        """kmer_positions, with the table left on the device (the input of `match_positions`)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_kmer_positions(self._h, _ptr(residues), _ptr(offsets), len(offsets) - 1, C.byref(p),
                                              C.byref(out)))
        return KmerPositions(self, out)

    def kmer_positions_table_device(self, d_residues: int, d_offsets: int, n_seqs: int, n_residues: int, ksize: int, scaled: int,
                                    moltype: str, seed: int = SEED) -> "KmerPositions":
        """kmer_positions_device, with the table left on the device."""
        p = make_params(ksize, scaled, moltype, seed)
        out = C.c_void_p()
        self._check(self._L.ks_kmer_positions_device(self._h, C.c_void_p(d_residues), C.c_void_p(d_offsets), n_seqs, n_residues,
                                                     C.byref(p), C.byref(out)))
        return KmerPositions(self, out)

    def match_positions(self, q_pos: "KmerPositions", t_pos: "KmerPositions", hits: "Hits", max_pairs: int = 0) -> "MatchPositions":
        """ks_match_positions: per row of `hits` the (query start, target start) pairs of the windows that share a kept hash,
        ordered by (query start, target start), and the extents they span.  q_pos / t_pos: the k-mer position tables of the
        query batch and of the targets the hits were searched on (same parameters).  max_pairs > 0 refuses a larger join
        with KS_ERR_CAPACITY before the pairs are allocated (the message carries the count); 0: the library's own limit."""
        out = C.c_void_p()
        opts = _lib.ks_matchpos_opts(0, 0, int(max_pairs))
        self._check(self._L.ks_match_positions(self._h, q_pos._h, t_pos._h, hits._h, C.byref(opts), C.byref(out)))
        return MatchPositions(self, out)

    def match_regions(self, mp: "MatchPositions", max_gap: int = 0, min_kmers: int = 1) -> "Regions":
        """ks_match_regions: every hit row's pairs chained into maximal colinear regions — pairs of one diagonal (target start -
        query start) whose query starts, ascending, step by at most ksize + max_gap.  Per region q_start, t_start, length (the
        same on both sides), n_kmers and covered (residues under a shared window); inside a row ordered by (q_start, t_start).
        Regions with fewer than min_kmers pairs are dropped: a row may keep none."""
        for name, v in (("max_gap", max_gap), ("min_kmers", min_kmers)):
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError(f"{name} = {v} does not fit 32 bits")
        out = C.c_void_p()
        opts = _lib.ks_regions_opts(0, int(min_kmers), int(max_gap), 0)
        self._check(self._L.ks_match_regions(self._h, mp._h, C.byref(opts), C.byref(out)))
        return Regions(self, out)

    @staticmethod
    def _rscore_opts(matrix, extend: bool, x_drop: int):
        """(ks_rscore_opts, the int8 array its matrix pointer reads: keep it alive for the call)"""
        if not 0 <= int(x_drop) < 2 ** 32:
            raise ValueError(f"x_drop = {x_drop} does not fit 32 bits")
        m = _matrix28(matrix)
        mp = m.ctypes.data_as(C.POINTER(C.c_int8)) if m is not None else None
        return _lib.ks_rscore_opts(_lib.KS_RSCORE_EXTEND if extend else 0, int(x_drop), mp, 0), m

    def score_regions_device(self, regions: "Regions", hits: "Hits", d_q_res: int, d_q_off: int, n_q: int, n_q_res: int,
                             d_t_res: int, d_t_off: int, n_t: int, n_t_res: int, matrix=None, extend: bool = False,
                             x_drop: int = 0, profile: Optional["Profile"] = None) -> "RegionScores":
        """ks_regions_score from device-resident residue batches (raw pointers: residues u8, offsets u64[n + 1]): every region
        of `regions` — chained for the rows of `hits` — scored under `matrix` (int8 [28, 28], the query's residue class is the
        row: A..Z, '*', everything else; None: +1 / -1) and, with extend=True, extended without gaps to both sides under the
        X-drop rule.  Per region the (extended) q_start, t_start, length, the score (i64), identities and positives over the
        extended span and the identities of the seed region alone; include/kmerseek_amd.h has the definitions.
        profile= (a Profile of the query batch, exclusive with matrix=): ks_regions_score_profile, a pair scores the profile's
        row of the query residue's position."""
        _profile_or_matrix(profile, matrix)
        opts, keep = self._rscore_opts(matrix, extend, x_drop)
        out = C.c_void_p()
        batches = (C.c_void_p(d_q_res), C.c_void_p(d_q_off), int(n_q), int(n_q_res), C.c_void_p(d_t_res), C.c_void_p(d_t_off), int(n_t), int(n_t_res))
        if profile is not None:
            self._check(self._L.ks_regions_score_profile(self._h, regions._h, hits._h, *batches, profile._h, C.byref(opts), C.byref(out)))
        else:
            self._check(self._L.ks_regions_score(self._h, regions._h, hits._h, *batches, C.byref(opts), C.byref(out)))
        del keep
        return RegionScores(self, out)

    def score_regions(self, regions: "Regions", hits: "Hits", q_res: np.ndarray, q_off: np.ndarray, t_res: np.ndarray,
                      t_off: np.ndarray, matrix=None, extend: bool = False, x_drop: int = 0,
                      profile: Optional["Profile"] = None) -> "RegionScores":
        """score_regions_device from host arrays (the batches `hits` was searched on): uploaded, scored, released."""
        _profile_or_matrix(profile, matrix)
        self._rscore_opts(matrix, extend, x_drop)  # (refused before anything is uploaded)
        with self._batches(q_res, q_off, t_res, t_off) as b:
            return self.score_regions_device(regions, hits, *b, matrix=matrix, extend=extend, x_drop=x_drop, profile=profile)

    @staticmethod
    def _ralign_opts(matrix, band: int, gap_open: int, gap_extend: int, x_drop: int):
        """(ks_ralign_opts, the int8 array its matrix pointer reads: keep it alive for the call)"""
        words = [_int_in(name, v, top) for name, v, top in (
            ("band", band, _lib.KS_RALIGN_MAX_BAND), ("gap_open", gap_open, _lib.KS_RALIGN_MAX_GAP_COST),
            ("gap_extend", gap_extend, _lib.KS_RALIGN_MAX_GAP_COST), ("x_drop", x_drop, _lib.KS_RALIGN_MAX_X_DROP))]
        m = _matrix28(matrix)
        mp = m.ctypes.data_as(C.POINTER(C.c_int8)) if m is not None else None
        return _lib.ks_ralign_opts(mp, *words, 0), m

    def align_regions_device(self, regions: "Regions", hits: "Hits", d_q_res: int, d_q_off: int, n_q: int, n_q_res: int,
                             d_t_res: int, d_t_off: int, n_t: int, n_t_res: int, matrix=None, band: int = 16, gap_open: int = 11,
                             gap_extend: int = 1, x_drop: int = 30, profile: Optional["Profile"] = None) -> "RegionAlignments":
        """ks_regions_align from device-resident residue batches (raw pointers: residues u8, offsets u64[n + 1]): every region
        of `regions` — chained for the rows of `hits` — extended with gaps from the middle pair of its seed to both sides: a
        banded (|diagonal shift| <= band <= 31) affine-gap (a gap of L residues costs gap_open + L * gap_extend, each <= 255)
        dynamic program under `matrix` (as score_regions), stopped by a row-level X-drop (x_drop <= 2^20).  Per region the
        alignment's q_start, q_length, t_start, t_length, score (i64), identities, positives, gap_opens, gaps and aln_length;
        the path itself is trace_regions'.  include/kmerseek_amd.h has the definitions.
        profile= (a Profile of the query batch, exclusive with matrix=): ks_regions_align_profile; the result is profile-made
        (RegionAlignments.by_profile) and only trace_regions(..., profile=) walks its paths."""
        _profile_or_matrix(profile, matrix)
        opts, keep = self._ralign_opts(matrix, band, gap_open, gap_extend, x_drop)
        out = C.c_void_p()
        batches = (C.c_void_p(d_q_res), C.c_void_p(d_q_off), int(n_q), int(n_q_res), C.c_void_p(d_t_res), C.c_void_p(d_t_off), int(n_t), int(n_t_res))
        if profile is not None:
            self._check(self._L.ks_regions_align_profile(self._h, regions._h, hits._h, *batches, profile._h, C.byref(opts), C.byref(out)))
        else:
            self._check(self._L.ks_regions_align(self._h, regions._h, hits._h, *batches, C.byref(opts), C.byref(out)))
        del keep
        return RegionAlignments(self, out)

    def align_regions(self, regions: "Regions", hits: "Hits", q_res: np.ndarray, q_off: np.ndarray, t_res: np.ndarray,
                      t_off: np.ndarray, matrix=None, band: int = 16, gap_open: int = 11, gap_extend: int = 1,
                      x_drop: int = 30, profile: Optional["Profile"] = None) -> "RegionAlignments":
        """align_regions_device from host arrays (the batches `hits` was searched on): uploaded, aligned, released."""
        _profile_or_matrix(profile, matrix)
        self._ralign_opts(matrix, band, gap_open, gap_extend, x_drop)  # (refused before anything is uploaded)
        with self._batches(q_res, q_off, t_res, t_off) as b:
            return self.align_regions_device(regions, hits, *b, matrix=matrix, band=band, gap_open=gap_open, gap_extend=gap_extend, x_drop=x_drop,
                                             profile=profile)

    @staticmethod
    def _rtrace_opts(eqx: bool, max_scratch_bytes: int):
        return _lib.ks_rtrace_opts(_lib.KS_RTRACE_EQX if eqx else 0, 0, _int_in("max_scratch_bytes", max_scratch_bytes, 2 ** 64 - 1, "[0, 2^64)"))

    def trace_regions_device(self, regions: "Regions", hits: "Hits", d_q_res: int, d_q_off: int, n_q: int, n_q_res: int,
                             d_t_res: int, d_t_off: int, n_t: int, n_t_res: int, alignments: "RegionAlignments", eqx: bool = False,
                             max_scratch_bytes: int = 0, profile: Optional["Profile"] = None) -> "RegionCigars":
        """ks_regions_traceback from device-resident residue batches: the path of every alignment of `alignments` — made by
        align_regions from these regions, hits and batches, whose options it recorded — as a CIGAR with the query as the read:
        M (with eqx=True: = and X), I, D.  max_scratch_bytes bounds the direction scratch of one slice of regions (0: 1 GiB).
        include/kmerseek_amd.h has the definitions.  profile=: the Profile the alignments were made against
        (ks_regions_traceback_profile); alignments made under a matrix take none."""
        opts = self._rtrace_opts(eqx, max_scratch_bytes)
        out = C.c_void_p()
        batches = (C.c_void_p(d_q_res), C.c_void_p(d_q_off), int(n_q), int(n_q_res), C.c_void_p(d_t_res), C.c_void_p(d_t_off), int(n_t), int(n_t_res))
        if profile is not None:
            self._check(self._L.ks_regions_traceback_profile(self._h, regions._h, hits._h, *batches, alignments._h, _profile_or_matrix(profile, None)._h,
                                                             C.byref(opts), C.byref(out)))
        else:
            self._check(self._L.ks_regions_traceback(self._h, regions._h, hits._h, *batches, alignments._h, C.byref(opts), C.byref(out)))
        return RegionCigars(self, out)

    def trace_regions(self, regions: "Regions", hits: "Hits", q_res: np.ndarray, q_off: np.ndarray, t_res: np.ndarray,
                      t_off: np.ndarray, alignments: "RegionAlignments", eqx: bool = False,
                      max_scratch_bytes: int = 0, profile: Optional["Profile"] = None) -> "RegionCigars":
        """trace_regions_device from host arrays (the batches `alignments` was made on): uploaded, traced, released."""
        _profile_or_matrix(profile, None)
        self._rtrace_opts(eqx, max_scratch_bytes)  # (refused before anything is uploaded)
        with self._batches(q_res, q_off, t_res, t_off) as b:
            return self.trace_regions_device(regions, hits, *b, alignments, eqx=eqx, max_scratch_bytes=max_scratch_bytes, profile=profile)

    @staticmethod
    def _rcull_opts(overlap_pct: int, min_score, max_per_row: int):
        overlap_pct, max_per_row = _int_in("overlap_pct", overlap_pct, 100), _int_in("max_per_row", max_per_row, 2 ** 32 - 1)
        if min_score is not None and (isinstance(min_score, bool) or int(min_score) != min_score or not -2 ** 63 <= int(min_score) < 2 ** 63):
            raise ValueError(f"min_score = {min_score} is not a 64-bit integer")
        return _lib.ks_rcull_opts(overlap_pct, max_per_row, 0 if min_score is None else int(min_score),
                                  0 if min_score is None else _lib.KS_RCULL_MIN_SCORE, 0)

    def cull_regions_device(self, d_row_offsets: int, d_q_start: int, d_q_length: int, d_t_start: int, d_t_length: Optional[int],
                            d_score: int, n_rows: int, n_regions: int, overlap_pct: int = 100, min_score=None,
                            max_per_row: int = 0) -> "RegionCull":
        """ks_regions_cull_device from device-resident columns (raw pointers: row_offsets u64[n_rows + 1]; q_start, q_length,
        t_start, t_length u32 and score i64, each [n_regions]; d_t_length None or 0: the target lengths are the query lengths).
        Per hit row the regions are decided best score first (ties: the smaller index): one that a kept region of the row
        overlaps by at least overlap_pct percent of its own length on BOTH sequences is removed and names that region as its
        keeper; min_score (None: off) drops regions that score below it; max_per_row (0: no limit) bounds the kept regions of a
        row.  include/kmerseek_amd.h has the contract."""
        opts = self._rcull_opts(overlap_pct, min_score, max_per_row)
        out = C.c_void_p()
        ptrs = [C.c_void_p(int(p)) if p else None for p in (d_row_offsets, d_q_start, d_q_length, d_t_start, d_t_length, d_score)]
        self._check(self._L.ks_regions_cull_device(self._h, *ptrs, int(n_rows), int(n_regions), C.byref(opts), C.byref(out)))
        return RegionCull(self, out)

    def cull_regions(self, scored, overlap_pct: int = 100, min_score=None, max_per_row: int = 0) -> "RegionCull":
        """The cull of cull_regions_device on a RegionAlignments (ks_raligns_cull: the alignments' extents and scores) or a
        RegionScores (ks_rscores_cull: the extended regions, one length for both sides).  RegionCull.take then gives the
        Regions / RegionScores / RegionAlignments of the kept regions alone — what trace_regions should be given."""
        opts = self._rcull_opts(overlap_pct, min_score, max_per_row)
        if isinstance(scored, RegionAlignments):
            fn = self._L.ks_raligns_cull
        elif isinstance(scored, RegionScores):
            fn = self._L.ks_rscores_cull
        else:
            raise TypeError("cull_regions takes a RegionAlignments or a RegionScores")
        out = C.c_void_p()
        self._check(fn(self._h, scored._h, C.byref(opts), C.byref(out)))
        return RegionCull(self, out)

    @staticmethod
    def _rchain_opts(max_gap: int, max_overlap: int, link_cost: int, skew_cost: int, overlap_cost: int):
        words = [_int_in(name, v, top) for name, v, top in (
            ("max_gap", max_gap, 2 ** 32 - 1), ("max_overlap", max_overlap, 2 ** 32 - 1), ("link_cost", link_cost, 2 ** 30),
            ("skew_cost", skew_cost, 2 ** 16), ("overlap_cost", overlap_cost, 2 ** 16))]
        return _lib.ks_rchain_opts(*words, 0, (C.c_uint32 * 2)(0, 0))

    def chain_regions_device(self, d_row_offsets: int, d_q_start: int, d_q_length: int, d_t_start: int, d_t_length: Optional[int],
                             d_score: int, n_rows: int, n_regions: int, d_identities: Optional[int] = None,
                             d_aln_length: Optional[int] = None, max_gap: int = 0, max_overlap: int = 0, link_cost: int = 0,
                             skew_cost: int = 0, overlap_cost: int = 0) -> "RegionChain":
        """ks_regions_chain_device from device-resident columns (raw pointers: row_offsets u64[n_rows + 1]; q_start, q_length,
        t_start, t_length u32 and score i64, each [n_regions]; d_t_length None or 0: the target lengths are the query lengths;
        d_identities, d_aln_length: optional u32 columns that are summed over each chain).  Per hit row the best colinear chain:
        region b follows region a iff its starts and its ends lie strictly behind a's on both sequences, the two overlap by at
        most max_overlap positions on either and lie at most max_gap apart (0: no limit); a link costs link_cost + skew_cost *
        |dq - dt| + overlap_cost * overlap; a chain is worth its scores minus its links.  include/kmerseek_amd.h has the
        contract."""
        opts = self._rchain_opts(max_gap, max_overlap, link_cost, skew_cost, overlap_cost)
        out = C.c_void_p()
        ptrs = [C.c_void_p(int(p)) if p else None for p in (d_row_offsets, d_q_start, d_q_length, d_t_start, d_t_length, d_score,
                                                            d_identities, d_aln_length)]
        self._check(self._L.ks_regions_chain_device(self._h, *ptrs, int(n_rows), int(n_regions), C.byref(opts), C.byref(out)))
        return RegionChain(self, out)

    def chain_regions(self, scored, max_gap: int = 0, max_overlap: int = 0, link_cost: int = 0, skew_cost: int = 0,
                      overlap_cost: int = 0) -> "RegionChain":
        """The chain of chain_regions_device on a RegionAlignments (ks_raligns_chain: the alignments' extents and scores; their
        identities and aln_length are summed) or a RegionScores (ks_rscores_chain: one length for both sides and as
        aln_length).  The intended input is what a cull kept: chain_regions(cull.take(alignments))."""
        opts = self._rchain_opts(max_gap, max_overlap, link_cost, skew_cost, overlap_cost)
        if isinstance(scored, RegionAlignments):
            fn = self._L.ks_raligns_chain
        elif isinstance(scored, RegionScores):
            fn = self._L.ks_rscores_chain
        else:
            raise TypeError("chain_regions takes a RegionAlignments or a RegionScores")
        out = C.c_void_p()
        self._check(fn(self._h, scored._h, C.byref(opts), C.byref(out)))
        return RegionChain(self, out)

    # ---- translated search: frame hits per strand, chained in bases ----
    def fold_frames_device(self, frame_hits: "Hits", d_nt_offsets: int, n_records: int, d_row_offsets: int, d_q_start: int,
                           d_q_length: int, d_t_start: int, d_t_length: Optional[int], n_regions: int, d_score: Optional[int] = None,
                           d_identities: Optional[int] = None, d_aln_length: Optional[int] = None) -> "FrameFold":
        """ks_frames_fold_device from device-resident columns (raw pointers).  frame_hits: the hits of a search whose queries
        are the 6 x n frames of translate6; d_nt_offsets: the record offsets u64[n_records + 1] in bases; then the CSR of regions
        over those hit rows as chain_regions_device takes it (d_t_length None or 0: the target lengths are the query lengths)
        and the optional columns score i64, identities, aln_length u32, which the fold gathers.  The rows of one strand's three
        frames against one target become one row — FrameFold.hits, a Hits with qid = 2 * record + strand — and their regions
        move onto the strand's bases (s_start, nt_length; t_start3, t_length3 the target in the same unit): what chain_frames
        chains.  include/kmerseek_amd.h has the contract."""
        out, out_hits = C.c_void_p(), C.c_void_p()
        ptrs = [C.c_void_p(int(p)) if p else None for p in (d_row_offsets, d_q_start, d_q_length, d_t_start, d_t_length, d_score,
                                                            d_identities, d_aln_length)]
        self._check(self._L.ks_frames_fold_device(self._h, frame_hits._h, C.c_void_p(int(d_nt_offsets)), int(n_records), *ptrs,
                                                  int(n_regions), None, C.byref(out_hits), C.byref(out)))
        return FrameFold(self, out, Hits(self, out_hits))

    def fold_frames(self, frame_hits: "Hits", scored, nt_offsets: np.ndarray) -> "FrameFold":
        """The fold of fold_frames_device on a RegionScores (ks_rscores_fold_frames: the extended regions, one length for both
        sides and as aln_length) or a RegionAlignments (ks_raligns_fold_frames) made for the rows of frame_hits — typically what
        a cull kept, cull.take(...).  nt_offsets: the host offsets u64[n + 1] of the nucleotide records, uploaded for the call."""
        if isinstance(scored, RegionAlignments):
            fn = self._L.ks_raligns_fold_frames
        elif isinstance(scored, RegionScores):
            fn = self._L.ks_rscores_fold_frames
        else:
            raise TypeError("fold_frames takes a RegionAlignments or a RegionScores")
        nt_offsets = np.ascontiguousarray(nt_offsets, dtype=np.uint64)
        if nt_offsets.ndim != 1 or nt_offsets.size == 0:
            raise ValueError("nt_offsets must be a 1-d array of n + 1 offsets")
        out, out_hits = C.c_void_p(), C.c_void_p()
        with self._uploaded(nt_offsets) as (d_off,):
            self._check(fn(self._h, frame_hits._h, C.c_void_p(d_off), len(nt_offsets) - 1, scored._h, None, C.byref(out_hits), C.byref(out)))
        return FrameFold(self, out, Hits(self, out_hits))

    def chain_frames(self, fold: "FrameFold", max_gap: int = 0, max_overlap: int = 0, link_cost: int = 0, skew_cost: int = 0,
                     overlap_cost: int = 0) -> "RegionChain":
        """chain_regions_device on a fold's (row_offsets, s_start, nt_length, t_start3, t_length3, score, identities,
        aln_length): per folded row the best colinear chain of its regions on the strand's bases, across frames — the options
        are in bases.  The chain's rows are the folded rows (fold.hits) and its src_region indexes the fold's regions.  A fold
        made without a score column is refused."""
        p = dict(zip(fold._COLUMNS, fold.device_ptrs()))
        if not p["score"]:
            raise ValueError("chain_frames needs a fold with a score column")
        return self.chain_regions_device(p["row_offsets"], p["s_start"], p["nt_length"], p["t_start3"], p["t_length3"], p["score"],
                                         fold.n_rows, fold.n_regions, d_identities=p["identities"] or None,
                                         d_aln_length=p["aln_length"] or None, max_gap=max_gap, max_overlap=max_overlap,
                                         link_cost=link_cost, skew_cost=skew_cost, overlap_cost=overlap_cost)

    @staticmethod
    def _rstitch_opts(max_fill: int, eqx: bool, max_scratch_bytes: int):
        max_fill = _int_in("max_fill", max_fill, _lib.KS_RSTITCH_MAX_FILL)
        return _lib.ks_rstitch_opts(max_fill, _lib.KS_RSTITCH_EQX if eqx else 0, _int_in("max_scratch_bytes", max_scratch_bytes, 2 ** 64 - 1),
                                    (C.c_uint32 * 2)(0, 0))

    def stitch_chains_device(self, chain: "RegionChain", alignments: "RegionAlignments", cigars: "RegionCigars", hits: "Hits",
                             d_q_res: int, d_q_off: int, n_q: int, n_q_res: int, d_t_res: int, d_t_off: int, n_t: int, n_t_res: int,
                             max_fill: int = 0, eqx: bool = False, max_scratch_bytes: int = 0) -> "HitAlignments":
        """ks_regions_stitch from device-resident residue batches: the chain of every hit row made into ONE gapped alignment
        with one CIGAR.  `alignments` is what `chain` was computed from (chain_regions(cull.take(alignments))), `cigars` what
        trace_regions gave for exactly those alignments (with eqx=True here they must have been traced with eqx=True).  Between
        two consecutive members the overlap is trimmed off the later one, and the rectangle left between them is aligned
        globally (the alignments' matrix and gap costs) where its shorter side is at most 63 and its longer at most max_fill
        (0: 1024, at most 4096); a longer one stays an open I run beside a D run.  max_scratch_bytes bounds the direction
        scratch of one slice (0: 1 GiB).  include/kmerseek_amd.h has the contract."""
        opts = self._rstitch_opts(max_fill, eqx, max_scratch_bytes)
        out = C.c_void_p()
        self._check(self._L.ks_regions_stitch(self._h, chain._h, alignments._h, cigars._h, hits._h, C.c_void_p(d_q_res), C.c_void_p(d_q_off),
                                              int(n_q), int(n_q_res), C.c_void_p(d_t_res), C.c_void_p(d_t_off), int(n_t), int(n_t_res),
                                              C.byref(opts), C.byref(out)))
        return HitAlignments(self, out)

    def stitch_chains(self, chain: "RegionChain", alignments: "RegionAlignments", cigars: "RegionCigars", hits: "Hits",
                      q_res: np.ndarray, q_off: np.ndarray, t_res: np.ndarray, t_off: np.ndarray, max_fill: int = 0, eqx: bool = False,
                      max_scratch_bytes: int = 0) -> "HitAlignments":
        """stitch_chains_device from host arrays (the batches `alignments` was made on): uploaded, stitched, released."""
        self._rstitch_opts(max_fill, eqx, max_scratch_bytes)  # (refused before anything is uploaded)
        with self._batches(q_res, q_off, t_res, t_off) as b:
            return self.stitch_chains_device(chain, alignments, cigars, hits, *b, max_fill=max_fill, eqx=eqx, max_scratch_bytes=max_scratch_bytes)

    @staticmethod
    def _fstitch_opts(max_fill: int, eqx: bool, frameshift_cost: int, max_scratch_bytes: int):
        max_fill = _int_in("max_fill", max_fill, _lib.KS_RSTITCH_MAX_FILL)
        return _lib.ks_fstitch_opts(max_fill, _lib.KS_RSTITCH_EQX if eqx else 0, _int_in("frameshift_cost", frameshift_cost, _lib.KS_FSTITCH_MAX_COST),
                                    0, _int_in("max_scratch_bytes", max_scratch_bytes, 2 ** 64 - 1))

    def stitch_frames_device(self, fold: "FrameFold", chain: "RegionChain", alignments: "RegionAlignments", cigars: "RegionCigars",
                             d_f_res: int, d_f_off: int, n_f: int, n_f_res: int, d_t_res: int, d_t_off: int, n_t: int, n_t_res: int,
                             max_fill: int = 0, eqx: bool = False, frameshift_cost: int = 15, max_scratch_bytes: int = 0) -> "FrameAlignments":
        """ks_frames_stitch from device-resident residue batches: the chain of every folded row of a translated search made into
        ONE alignment of the strand's bases against the target protein — one CIGAR in codon columns, a frameshift as an N op of
        1 or 2 bases directly before the member behind it, paid with frameshift_cost in the re-computed score.  `fold` is
        fold_frames(frame_hits, alignments, ...) — its hits are the rows — `chain` chain_frames(fold), `alignments` the gapped
        alignments the fold was made of (cull.take(...)), `cigars` what trace_regions gave for exactly those (eqx=True here:
        traced with eqx=True).  d_f_res / d_f_off: the frame batch of translate6 (n_f = 6 x records), what align_regions took
        as queries; then the target batch.  max_fill, max_scratch_bytes as in stitch_chains_device.  A row whose chain lies in
        one frame gives what stitch_chains gives on that frame.  include/kmerseek_amd.h has the contract."""
        opts = self._fstitch_opts(max_fill, eqx, frameshift_cost, max_scratch_bytes)
        out = C.c_void_p()
        self._check(self._L.ks_frames_stitch(self._h, fold._h, fold.hits._h, chain._h, alignments._h, cigars._h, C.c_void_p(d_f_res),
                                             C.c_void_p(d_f_off), int(n_f), int(n_f_res), C.c_void_p(d_t_res), C.c_void_p(d_t_off), int(n_t),
                                             int(n_t_res), C.byref(opts), C.byref(out)))
        return FrameAlignments(self, out)

    def stitch_frames(self, fold: "FrameFold", chain: "RegionChain", alignments: "RegionAlignments", cigars: "RegionCigars",
                      frames: "DeviceBuffer", frame_offsets: "DeviceBuffer", n_frame_res: int, t_res: np.ndarray, t_off: np.ndarray,
                      max_fill: int = 0, eqx: bool = False, frameshift_cost: int = 15, max_scratch_bytes: int = 0) -> "FrameAlignments":
        """stitch_frames_device with the frame batch as translate6 returned it (frames, frame_offsets, n_frame_res: device
        buffers, 6 frames per record) and the target batch from host arrays, uploaded for the call."""
        self._fstitch_opts(max_fill, eqx, frameshift_cost, max_scratch_bytes)  # (refused before anything is uploaded)
        t_res = np.ascontiguousarray(t_res, dtype=np.uint8); t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        n_f = frame_offsets.nbytes // 8 - 1
        with self._uploaded(t_res if t_res.size else np.zeros(1, np.uint8), t_off) as (d_t, d_to):
            return self.stitch_frames_device(fold, chain, alignments, cigars, frames.ptr, frame_offsets.ptr, n_f, int(n_frame_res), d_t, d_to,
                                             len(t_off) - 1, int(t_res.size), max_fill=max_fill, eqx=eqx, frameshift_cost=frameshift_cost,
                                             max_scratch_bytes=max_scratch_bytes)

    def pileup_device(self, d_row_offsets: Optional[int], d_op_offsets: int, d_ops: int, n_rows: int, n_entries: int, n_ops: int,
                      d_start: int, d_other_start: Optional[int], d_row_mask: Optional[int], hits: "Hits", d_offsets: int, n_seqs: int,
                      n_res: int, side: str = "target", profile: bool = False, d_other_res: Optional[int] = None,
                      d_other_off: Optional[int] = None, n_other: int = 0, n_other_res: int = 0, d_weight: Optional[int] = None) -> "Pileup":
        """ks_pileup_device from raw device pointers: the entries (runs of CIGAR ops, each of a hit row of `hits`, with a start on
        the chosen side) piled up on the residues of that side's batch — per residue the depth, with profile=True also the 28
        counts of the residue classes aligned to it (the other batch and d_other_start are then needed), per sequence length,
        n_alignments, covered, max_depth, depth_sum, breadth and mean_depth.  d_row_offsets None: one entry per hit row;
        d_row_mask: u8 per hit row, the entries of a row with 0 are skipped.  d_weight: None, or u32 per entry (units of 2^-30,
        KS_WEIGHT_ONE is 1): ks_wpileup_device, which also sums the weights of the entries that place a residue
        (Pileup.weighted_to_host).  include/kmerseek_amd.h has the contract."""
        opts = _pileup_opts(side, profile)
        vp = lambda p: C.c_void_p(int(p)) if p else None
        out = C.c_void_p()
        if d_weight is not None:
            self._check(self._L.ks_wpileup_device(self._h, vp(d_row_offsets), vp(d_op_offsets), vp(d_ops), int(n_rows), int(n_entries),
                                                          int(n_ops), vp(d_start), vp(d_other_start), vp(d_row_mask), hits._h, vp(d_offsets),
                                                          int(n_seqs), int(n_res), vp(d_other_res), vp(d_other_off), int(n_other),
                                                          int(n_other_res), vp(d_weight), C.byref(opts), C.byref(out)))
            return Pileup(self, out)
        self._check(self._L.ks_pileup_device(self._h, vp(d_row_offsets), vp(d_op_offsets), vp(d_ops), int(n_rows), int(n_entries), int(n_ops),
                                             vp(d_start), vp(d_other_start), vp(d_row_mask), hits._h, vp(d_offsets), int(n_seqs), int(n_res),
                                             vp(d_other_res), vp(d_other_off), int(n_other), int(n_other_res), C.byref(opts), C.byref(out)))
        return Pileup(self, out)

    def pileup(self, aligned, hits: "Hits", side: str = "target", offsets=None, alignments: Optional["RegionAlignments"] = None,
               row_mask=None, profile: bool = False, other_res=None, other_off=None, weights=None) -> "Pileup":
        """The coverage of one batch by a RegionCigars (ks_cigars_pileup: every region is an entry; alignments= the
        RegionAlignments they were traced from, which hold the row CSR and the starts), a HitAlignments (ks_hitalns_pileup: one
        entry per hit row) or a FrameAlignments (ks_frames_pileup on fold.hits: side="target" only, no profile).
        side: "query" or "target", the batch the depth is counted on; offsets: its host offsets u64[n + 1], uploaded for the
        call.  row_mask: None or one truth value per hit row, the rows to take (a top-k selection).  profile=True also counts,
        per residue, the classes of the residues aligned to it: other_res / other_off are then the host arrays of the other
        batch.  weights: None, an EntryWeights (entry_weights) or a u32 array, one weight per entry in units of 2^-30: the
        weighted pileup, which makes every column alike and also sums the weights (Pileup.weighted_to_host); not for a
        FrameAlignments."""
        opts = _pileup_opts(side, profile)
        if weights is not None and isinstance(aligned, FrameAlignments):
            raise ValueError("pileup of a FrameAlignments: weights= is not built (ks_frames_pileup has no weighted form)")
        if weights is not None and not isinstance(weights, EntryWeights):
            weights = np.asarray(weights)
            if weights.dtype.kind not in "ui" or weights.ndim != 1 or (weights.size and (int(weights.min()) < 0 or int(weights.max()) > 0xffffffff)):
                raise ValueError("weights must be an EntryWeights or a 1-d array of u32 values, one weight per entry")
            weights = np.ascontiguousarray(weights, dtype=np.uint32)
        if isinstance(aligned, FrameAlignments):
            if side != "target":
                raise ValueError("pileup of a FrameAlignments: side=\"query\" is not built (depth in bases on a strand); side=\"target\" only")
            if profile:
                raise ValueError("pileup of a FrameAlignments: profile=True is not built (the query side is a strand's bases)")
        elif isinstance(aligned, RegionCigars):
            if alignments is None:
                raise TypeError("pileup of a RegionCigars needs alignments=, the RegionAlignments it was traced from")
        elif not isinstance(aligned, HitAlignments):
            raise TypeError("pileup takes a RegionCigars, a HitAlignments or a FrameAlignments")
        if offsets is None:
            raise TypeError("pileup needs offsets=, the offsets of the batch on the chosen side")
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offsets.ndim != 1 or offsets.size == 0:
            raise ValueError("offsets must be a 1-d array of n + 1 offsets")
        if profile and (other_res is None or other_off is None):
            raise ValueError("profile=True needs other_res and other_off, the batch on the other side")
        up = [offsets]
        if row_mask is not None:
            row_mask = np.ascontiguousarray(np.asarray(row_mask) != 0, dtype=np.uint8)
            if row_mask.shape != (hits.count,):
                raise ValueError(f"row_mask holds {row_mask.size} values for {hits.count} hit rows")
            up.append(row_mask if row_mask.size else np.zeros(1, np.uint8))
        if profile:
            other_res = np.ascontiguousarray(other_res, dtype=np.uint8); other_off = np.ascontiguousarray(other_off, dtype=np.uint64)
            up += [other_res if other_res.size else np.zeros(1, np.uint8), other_off]
        if isinstance(weights, np.ndarray):
            n_entries = aligned.n_regions if isinstance(aligned, RegionCigars) else aligned.n_rows
            if weights.size != n_entries:
                raise ValueError(f"weights holds {weights.size} values for {n_entries} entries")
            up.append(weights if weights.size else np.zeros(1, np.uint32))
        with self._uploaded(*up) as d:
            d_off, d = d[0], list(d[1:])
            d_mask = C.c_void_p(d.pop(0)) if row_mask is not None else None
            other = (C.c_void_p(d[0]), C.c_void_p(d[1]), len(other_off) - 1, int(other_res.size)) if profile else (None, None, 0, 0)
            side_batch = (C.c_void_p(d_off), len(offsets) - 1, int(offsets[-1]))
            out = C.c_void_p()
            if weights is not None:
                d_w = C.c_void_p(weights.weight_ptr if isinstance(weights, EntryWeights) else d[-1])
                if isinstance(aligned, RegionCigars):
                    st = self._L.ks_cigars_pileup_weighted(self._h, aligned._h, alignments._h, hits._h, d_mask, *side_batch, *other, d_w,
                                                           C.byref(opts), C.byref(out))
                else:
                    st = self._L.ks_hitalns_pileup_weighted(self._h, aligned._h, hits._h, d_mask, *side_batch, *other, d_w, C.byref(opts),
                                                            C.byref(out))
            elif isinstance(aligned, RegionCigars):
                st = self._L.ks_cigars_pileup(self._h, aligned._h, alignments._h, hits._h, d_mask, *side_batch, *other, C.byref(opts), C.byref(out))
            elif isinstance(aligned, HitAlignments):
                st = self._L.ks_hitalns_pileup(self._h, aligned._h, hits._h, d_mask, *side_batch, *other, C.byref(opts), C.byref(out))
            else:
                st = self._L.ks_frames_pileup(self._h, aligned._h, hits._h, d_mask, *side_batch, C.byref(opts), C.byref(out))
            self._check(st)
        return Pileup(self, out)

    def entry_weights_device(self, d_row_offsets: Optional[int], d_op_offsets: int, d_ops: int, n_rows: int, n_entries: int, n_ops: int,
                             d_start: int, d_other_start: int, d_row_mask: Optional[int], hits: "Hits", d_offsets: int, n_seqs: int,
                             n_res: int, d_other_res: int, d_other_off: int, n_other: int, n_other_res: int, d_counts: int,
                             side: str = "query", include_query: bool = False, d_res: Optional[int] = None) -> "EntryWeights":
        """ks_entry_weights_device from raw device pointers: one position-based (Henikoff) weight per entry, small where the
        entry agrees with many others — the arguments of pileup_device with profile=True, d_counts: the counts u32[n_res * 28]
        of that pileup of the same entries, mask and side, and with include_query=True d_res, the side's residues (the sequence
        the entries lie on is then one more member of its columns).  include/kmerseek_amd.h has the rule."""
        if side not in PILEUP_SIDES:
            raise ValueError(f"side = {side!r} is neither \"query\" nor \"target\"")
        if include_query and not d_res and n_res:
            raise ValueError("include_query=True needs d_res, the residues of the batch on the chosen side")
        vp = lambda p: C.c_void_p(int(p)) if p else None
        out = C.c_void_p()
        self._check(self._L.ks_entry_weights_device(self._h, vp(d_row_offsets), vp(d_op_offsets), vp(d_ops), int(n_rows), int(n_entries), int(n_ops),
                                                     vp(d_start), vp(d_other_start), vp(d_row_mask), hits._h, vp(d_res), vp(d_offsets), int(n_seqs),
                                                     int(n_res), vp(d_other_res), vp(d_other_off), int(n_other), int(n_other_res), vp(d_counts),
                                                     PILEUP_SIDES[side], _lib.KS_PWEIGHTS_INCLUDE_QUERY if include_query else 0, C.byref(out)))
        return EntryWeights(self, out)

    def entry_weights(self, aligned: "RegionCigars", hits: "Hits", pileup: "Pileup", side: str = "query", offsets=None,
                      alignments: Optional["RegionAlignments"] = None, row_mask=None, other_res=None, other_off=None,
                      include_query: bool = False, res=None) -> "EntryWeights":
        """One weight per region of a RegionCigars (ks_cigars_pileup_weights) from the Pileup made of them with profile=True on
        the same side and under the same row_mask: the arguments of pileup(), and with include_query=True res, the host
        residues of the side's batch.  Pass the result to pileup(..., weights=)."""
        if side not in PILEUP_SIDES:
            raise ValueError(f"side = {side!r} is neither \"query\" nor \"target\"")
        if not isinstance(aligned, RegionCigars):
            raise TypeError("entry_weights takes a RegionCigars (other entries: entry_weights_device)")
        if alignments is None:
            raise TypeError("entry_weights needs alignments=, the RegionAlignments the cigars were traced from")
        if not isinstance(pileup, Pileup):
            raise TypeError("entry_weights needs the Pileup made from the same entries with profile=True")
        if offsets is None or other_res is None or other_off is None:
            raise TypeError("entry_weights needs offsets=, other_res= and other_off=: the side's offsets and the other batch")
        if include_query and res is None:
            raise ValueError("include_query=True needs res=, the residues of the batch on the chosen side")
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offsets.ndim != 1 or offsets.size == 0:
            raise ValueError("offsets must be a 1-d array of n + 1 offsets")
        other_res = np.ascontiguousarray(other_res, dtype=np.uint8); other_off = np.ascontiguousarray(other_off, dtype=np.uint64)
        up = [offsets, other_res if other_res.size else np.zeros(1, np.uint8), other_off]
        if row_mask is not None:
            row_mask = np.ascontiguousarray(np.asarray(row_mask) != 0, dtype=np.uint8)
            if row_mask.shape != (hits.count,):
                raise ValueError(f"row_mask holds {row_mask.size} values for {hits.count} hit rows")
            up.append(row_mask if row_mask.size else np.zeros(1, np.uint8))
        if include_query:
            res = np.ascontiguousarray(res, dtype=np.uint8)
            if res.size != int(offsets[-1]):
                raise ValueError(f"res holds {res.size} residues, the offsets end at {int(offsets[-1])}")
            up.append(res if res.size else np.zeros(1, np.uint8))
        with self._uploaded(*up) as d:
            d = list(d)
            d_res = C.c_void_p(d.pop()) if include_query else None
            d_mask = C.c_void_p(d.pop()) if row_mask is not None else None
            out = C.c_void_p()
            self._check(self._L.ks_cigars_pileup_weights(self._h, aligned._h, alignments._h, pileup._h, hits._h, d_mask, d_res, C.c_void_p(d[0]),
                                                         len(offsets) - 1, int(offsets[-1]), C.c_void_p(d[1]), C.c_void_p(d[2]), len(other_off) - 1,
                                                         int(other_res.size), PILEUP_SIDES[side],
                                                         _lib.KS_PWEIGHTS_INCLUDE_QUERY if include_query else 0, C.byref(out)))
        return EntryWeights(self, out)

    def build_profile_device(self, d_counts: int, d_depth: int, d_q_res: int, d_q_off: int, n_q: int, n_q_res: int,
                             params: ProfileParams, d_wcounts: Optional[int] = None) -> "Profile":
        """ks_profile_build_device from raw device pointers: counts u32[n_q_res * 28] and depth u32[n_q_res] as a query-side
        Pileup with the profile holds them, and the query batch.  Per residue a row of 28 scores, a consensus byte and the
        observations behind the row; include/kmerseek_amd.h has the rule, params: ProfileParams (profile_params).  d_wcounts:
        None, or the weighted counts u64[n_q_res * 28] of a weighted pileup: ks_profile_build_weighted_device, whose
        frequencies are the weighted ones and whose evidence is the number of classes seen."""
        if not isinstance(params, ProfileParams):
            raise TypeError("params must be a ProfileParams (profile_params)")
        opts, keep = params._opts()
        out = C.c_void_p()
        if d_wcounts is not None:
            self._check(self._L.ks_profile_build_weighted_device(self._h, C.c_void_p(d_counts), C.c_void_p(d_wcounts), C.c_void_p(d_depth),
                                                                 C.c_void_p(d_q_res), C.c_void_p(d_q_off), int(n_q), int(n_q_res),
                                                                 C.byref(opts), C.byref(out)))
            del keep
            return Profile(self, out)
        self._check(self._L.ks_profile_build_device(self._h, C.c_void_p(d_counts), C.c_void_p(d_depth), C.c_void_p(d_q_res), C.c_void_p(d_q_off),
                                                    int(n_q), int(n_q_res), C.byref(opts), C.byref(out)))
        del keep
        return Profile(self, out)

    def build_profile(self, pileup, q_res: np.ndarray, q_off: np.ndarray, params: ProfileParams, weighted: bool = False) -> "Profile":
        """The Profile of the query batch (q_res, q_off: host arrays) from a Pileup made on its side with profile=True
        (ks_profile_build_pileup), or from host arrays (counts, depth) that stand for one.  weighted=True: the weighted build
        (ks_profile_build_weighted_pileup) from a Pileup made with weights=, or from host arrays (counts, wcounts, depth)."""
        if not isinstance(params, ProfileParams):
            raise TypeError("params must be a ProfileParams (profile_params)")
        if weighted and isinstance(pileup, Pileup) and pileup._h and not pileup.n_weighted and pileup.n_residues:
            raise ValueError("weighted=True needs a Pileup made with weights= (this one holds no weighted counts)")
        q_res = np.ascontiguousarray(q_res, dtype=np.uint8); q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        if isinstance(pileup, Pileup):
            opts, keep = params._opts()
            out = C.c_void_p()
            with self._uploaded(q_res, q_off) as (d_q, d_qo):
                fn = self._L.ks_profile_build_weighted_pileup if weighted else self._L.ks_profile_build_pileup
                self._check(fn(self._h, pileup._h, C.c_void_p(d_q), C.c_void_p(d_qo), len(q_off) - 1, len(q_res), C.byref(opts), C.byref(out)))
            del keep
            return Profile(self, out)
        if weighted:
            counts, wcounts, depth = pileup
            counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1); depth = np.ascontiguousarray(depth, dtype=np.uint32)
            wcounts = np.ascontiguousarray(wcounts, dtype=np.uint64).reshape(-1)
            if len(counts) != _lib.KS_RSCORE_ALPHABET * len(q_res) or len(wcounts) != len(counts) or len(depth) != len(q_res):
                raise ValueError("counts and wcounts must hold 28 entries and depth one per residue of the batch")
            with self._uploaded(counts, wcounts, depth, q_res, q_off) as (d_c, d_w, d_d, d_q, d_qo):
                return self.build_profile_device(d_c, d_d, d_q, d_qo, len(q_off) - 1, len(q_res), params, d_wcounts=d_w)
        counts, depth = pileup
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1); depth = np.ascontiguousarray(depth, dtype=np.uint32)
        if len(counts) != _lib.KS_RSCORE_ALPHABET * len(q_res) or len(depth) != len(q_res):
            raise ValueError("counts must hold 28 entries and depth one per residue of the batch")
        with self._uploaded(counts, depth, q_res, q_off) as (d_c, d_d, d_q, d_qo):
            return self.build_profile_device(d_c, d_d, d_q, d_qo, len(q_off) - 1, len(q_res), params)

    def profile_from_host(self, scores, n_seqs: int, matrix=None, consensus=None, n_obs=None) -> "Profile":
        """ks_profile_from_host: a Profile whose rows the caller brings — scores int8 [n_residues, 28] of a batch of n_seqs
        sequences; matrix: the fallback to record (None: +1 / -1)."""
        sc = np.ascontiguousarray(scores)
        if sc.dtype != np.int8 or sc.ndim != 2 or sc.shape[1] != _lib.KS_RSCORE_ALPHABET:
            raise ValueError("scores must be an int8 array of shape (n_residues, 28)")
        m = _matrix28(matrix)
        cons = None if consensus is None else np.ascontiguousarray(consensus, dtype=np.uint8)
        nobs = None if n_obs is None else np.ascontiguousarray(n_obs, dtype=np.uint32)
        if any(c is not None and c.shape != (len(sc),) for c in (cons, nobs)):
            raise ValueError("consensus and n_obs hold one entry per residue")
        out = C.c_void_p()
        self._check(self._L.ks_profile_from_host(self._h, _ptr(sc), _ptr(cons), _ptr(nobs), _int_in("n_seqs", n_seqs, 2 ** 32 - 1), len(sc), _ptr(m),
                                                 C.byref(out)))
        return Profile(self, out)

    def residue_composition_device(self, d_res: int, d_off: int, n_seqs: int, n_res: int) -> "Composition":
        """ks_residue_composition_device from a device-resident residue batch (raw pointers: residues u8, offsets
        u64[n_seqs + 1]): per sequence the count of each of the 28 residue classes of score_regions (A..Z, '*', everything else)
        and its length, and the class totals of the batch.  Build it once per database and reuse it."""
        out = C.c_void_p()
        self._check(self._L.ks_residue_composition_device(self._h, C.c_void_p(int(d_res)) if d_res else None, C.c_void_p(int(d_off)),
                                                          int(n_seqs), int(n_res), C.byref(out)))
        return Composition(self, out)

    def residue_composition(self, res: np.ndarray, off: np.ndarray) -> "Composition":
        """residue_composition_device from host arrays: uploaded, counted, released."""
        res = np.ascontiguousarray(res, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.uint64)
        with self._uploaded(res if len(res) else np.zeros(1, np.uint8), off) as (d_res, d_off):  # (an empty batch still has a buffer to point at)
            return self.residue_composition_device(d_res, d_off, len(off) - 1, len(res))

    @staticmethod
    def _astats_opts(matrix, params, background, composition: bool, pairwise: bool, allow_ungapped: bool, ratio, db_residues: int,
                     db_seqs: int, length_adjust: int):
        """(ks_astats_opts, the arrays its pointers read: keep them alive for the call)"""
        m = _matrix28(matrix)
        bg = None
        if background is not None:
            bg = np.ascontiguousarray(background, dtype=np.float64)
            if bg.shape != (_lib.KS_RSCORE_ALPHABET,):
                raise ValueError("background must hold 28 weights")
        lam, K = (0.0, 0.0) if params is None else (float(params[0]), float(params[1]))
        db_residues, db_seqs = _int_in("db_residues", db_residues, 2 ** 64 - 1), _int_in("db_seqs", db_seqs, 2 ** 64 - 1)
        length_adjust = _int_in("length_adjust", length_adjust, 2 ** 32 - 1)
        flags = ((0 if composition else _lib.KS_ASTATS_NO_COMPOSITION) | (_lib.KS_ASTATS_PAIRWISE if pairwise else 0)
                 | (_lib.KS_ASTATS_ALLOW_UNGAPPED if allow_ungapped else 0))
        opts = _lib.ks_astats_opts(flags, length_adjust, m.ctypes.data_as(C.POINTER(C.c_int8)) if m is not None else None, lam, K,
                                   bg.ctypes.data_as(C.POINTER(C.c_double)) if bg is not None else None, float(ratio[0]), float(ratio[1]),
                                   db_residues, db_seqs, 0)
        return opts, (m, bg)

    def alignment_stats_device(self, d_row_offsets: Optional[int], d_score: int, n_rows: int, n: int, hits: "Hits", q_comp: "Composition",
                               t_comp: Optional["Composition"], matrix=None, params=None, background=None, composition: bool = True,
                               pairwise: bool = False, ratio=(0.5, 1.0), db_residues: int = 0, db_seqs: int = 0,
                               length_adjust: int = 0) -> "AlignmentStats":
        """ks_scores_stats_device from device-resident columns (raw pointers: row_offsets u64[n_rows + 1] or None — one score per
        hit row —, score i64[n]): per entry a bit score and an E-value, per hit row the composition-based lambda ratio the scores
        were rescaled with.  params: (lambda, K) of the scoring system, typically the gapped ones of the matrix and its gap
        costs; None: the ungapped ones the library derives.  include/kmerseek_amd.h has the contract."""
        opts, keep = self._astats_opts(matrix, params, background, composition, pairwise, False, ratio, db_residues, db_seqs, length_adjust)
        out = C.c_void_p()
        self._check(self._L.ks_scores_stats_device(self._h, C.c_void_p(int(d_row_offsets)) if d_row_offsets else None,
                                                   C.c_void_p(int(d_score)) if d_score else None, int(n_rows), int(n), hits._h, q_comp._h,
                                                   None if t_comp is None else t_comp._h, C.byref(opts), C.byref(out)))
        del keep
        return AlignmentStats(self, out)

    def alignment_stats(self, scored, hits: "Hits", q_comp: "Composition", t_comp: Optional["Composition"], matrix=None, params=None,
                        background=None, composition: bool = True, pairwise: bool = False, allow_ungapped: bool = False,
                        ratio=(0.5, 1.0), db_residues: int = 0, db_seqs: int = 0, length_adjust: int = 0,
                        alignments: Optional["RegionAlignments"] = None) -> "AlignmentStats":
        """Bit scores and E-values of a RegionScores (ks_rscores_stats: ungapped scores), a RegionAlignments (ks_raligns_stats) or
        a HitAlignments (ks_hitalns_stats, one entry per hit row; `alignments`: the RegionAlignments it was stitched from, whose
        matrix is used).  The two gapped kinds need params=(lambda, K) — the gapped values that belong to the matrix and the gap
        costs — or allow_ungapped=True, which understates their E-values.  q_comp / t_comp: Context.residue_composition of the
        batches the hits were searched on; composition=False switches the per-pair rescaling off."""
        opts, keep = self._astats_opts(matrix, params, background, composition, pairwise, allow_ungapped, ratio, db_residues, db_seqs,
                                       length_adjust)
        tc = None if t_comp is None else t_comp._h
        out = C.c_void_p()
        if isinstance(scored, RegionScores):
            st = self._L.ks_rscores_stats(self._h, scored._h, hits._h, q_comp._h, tc, C.byref(opts), C.byref(out))
        elif isinstance(scored, RegionAlignments):
            st = self._L.ks_raligns_stats(self._h, scored._h, hits._h, q_comp._h, tc, C.byref(opts), C.byref(out))
        elif isinstance(scored, HitAlignments):
            if alignments is None:
                raise TypeError("alignment_stats of a HitAlignments needs alignments=, the RegionAlignments it was stitched from")
            st = self._L.ks_hitalns_stats(self._h, scored._h, alignments._h, hits._h, q_comp._h, tc, C.byref(opts), C.byref(out))
        else:
            raise TypeError("alignment_stats takes a RegionScores, a RegionAlignments or a HitAlignments")
        self._check(st)
        del keep
        return AlignmentStats(self, out)

    def significance(self, queries: "Sketches", targets: "Sketches", hits: "Hits", q_corpus: Optional["Corpus"] = None,
                     t_corpus: Optional["Corpus"] = None) -> "Significance":
        """ks_hits_significance: per row of `hits` the two f64 sums behind multisearch's prob_overlap and tf_idf_score, over the
        hashes the row's query and target share (include/kmerseek_amd.h has the definitions).  queries / targets: the sets the
        hits were searched on.  A corpus table that is not passed is built here (Sketches.corpus) and freed again — pass them
        when several hit lists share a set."""
        own = []
        try:
            if q_corpus is None:
                q_corpus = queries.corpus(); own.append(q_corpus)
            if t_corpus is None:
                t_corpus = targets.corpus(); own.append(t_corpus)
            out = C.c_void_p()
            opts = _lib.ks_signif_opts(0, 0)
            self._check(self._L.ks_hits_significance(self._h, queries._h, targets._h, q_corpus._h, t_corpus._h, hits._h, C.byref(opts),
                                                     C.byref(out)))
            return Significance(self, out)
        finally:
            for c in own:
                c.free()

    def best_hits(self, hits: "Hits", k: int, rank_by: str = "intersect", queries: Optional["Sketches"] = None,
                  targets: Optional["Sketches"] = None, score=None) -> "Hits":
        """ks_hits_best: the k best rows of every query of `hits`, still ordered by (qid, tid), with each kept row's rank
        inside its query and its row in `hits` (Hits.best_to_host).  rank_by: intersect | target_containment (needs
        `targets`) | max_containment | jaccard (need both sets) | score — `score` is a device column of hits.count f64, as a
        raw pointer or an object with data_ptr() (e.g. one of Significance.device_ptrs()); with `score` given and rank_by
        left at its default, rank_by becomes score.  Ties go to the smaller tid; NaN scores rank last."""
        if score is not None and rank_by == "intersect":
            rank_by = "score"
        if rank_by not in BEST_RANK_BY:
            raise ValueError(f"rank_by must be one of {', '.join(BEST_RANK_BY)}, not {rank_by!r}")
        if not 0 <= int(k) < 2 ** 32:
            raise ValueError(f"k = {k} does not fit 32 bits")
        d_score = None if score is None else C.c_void_p(int(score.data_ptr()) if hasattr(score, "data_ptr") else int(score))
        opts = _lib.ks_best_opts(BEST_RANK_BY[rank_by], int(k), 0, 0)
        out = C.c_void_p()
        self._check(self._L.ks_hits_best(self._h, hits._h, None if queries is None else queries._h,
                                         None if targets is None else targets._h, d_score, C.byref(opts), C.byref(out)))
        return Hits(self, out)

    def cluster(self, hits: "Hits", similarity: Optional[str] = None, threshold: float = 0.0, nodes: Optional["Sketches"] = None,
                score=None, n_nodes: int = 0) -> "Clusters":
        """ks_hits_cluster: the connected components of an all-vs-all hit list.  `hits` comes from searching one set against
        itself (any list in that id space: thresholded or best-hits output too); row (q, t) is an edge iff q != t and its
        score >= threshold.  similarity: the key names of best_hits — intersect | target_containment | max_containment |
        jaccard (these three need `nodes`, the sketch set) | score (`score`: a device column of hits.count f64, a raw pointer
        or an object with data_ptr()).  similarity left at None is jaccard, or score when a `score` column is given; an explicit
        key with a column it does not read is refused by the library.  Without `nodes` the node count comes from n_nodes.
        NaN scores never link."""
        if similarity is None:
            similarity = "jaccard" if score is None else "score"
        if similarity not in BEST_RANK_BY:
            raise ValueError(f"similarity must be one of {', '.join(BEST_RANK_BY)}, not {similarity!r}")
        if not 0 <= int(n_nodes) < 2 ** 32:
            raise ValueError(f"n_nodes = {n_nodes} does not fit 32 bits")
        d_score = None if score is None else C.c_void_p(int(score.data_ptr()) if hasattr(score, "data_ptr") else int(score))
        opts = _lib.ks_cluster_opts(BEST_RANK_BY[similarity], int(n_nodes), float(threshold), 0, 0)
        out = C.c_void_p()
        self._check(self._L.ks_hits_cluster(self._h, hits._h, None if nodes is None else nodes._h, d_score, C.byref(opts),
                                            C.byref(out)))
        return Clusters(self, out)

    def cluster_greedy(self, hits: "Hits", similarity: Optional[str] = None, threshold: float = 0.0, nodes: Optional["Sketches"] = None,
                       score=None, n_nodes: int = 0, assign: str = "first") -> "Clusters":
        """ks_hits_cluster_greedy: greedy representative clusters of an all-vs-all hit list (the clustering of CD-HIT and of
        the greedy modes of MMseqs2 / linclust).  Hits, edges, similarity, threshold, nodes, score and n_nodes are those of
        cluster().  The nodes are taken in priority order (with `nodes`: more distinct hashes first, ties to the smaller id;
        without: the smaller id first); a node with no representative among its neighbours of higher priority becomes one,
        every other node joins a neighbouring representative: assign="first" the one of highest priority, "best" the one at
        the other end of its passing row with the largest score (ties: the higher priority).  In the result a label is the
        representative's id; Clusters.n_rounds says how many rounds the pass took."""
        if similarity is None:
            similarity = "jaccard" if score is None else "score"
        if similarity not in BEST_RANK_BY:
            raise ValueError(f"similarity must be one of {', '.join(BEST_RANK_BY)}, not {similarity!r}")
        if assign not in GREEDY_ASSIGN:
            raise ValueError(f"assign must be one of {', '.join(GREEDY_ASSIGN)}, not {assign!r}")
        if not 0 <= int(n_nodes) < 2 ** 32:
            raise ValueError(f"n_nodes = {n_nodes} does not fit 32 bits")
        d_score = None if score is None else C.c_void_p(int(score.data_ptr()) if hasattr(score, "data_ptr") else int(score))
        opts = _lib.ks_greedy_opts(BEST_RANK_BY[similarity], int(n_nodes), float(threshold), GREEDY_ASSIGN[assign], 0)
        out = C.c_void_p()
        self._check(self._L.ks_hits_cluster_greedy(self._h, hits._h, None if nodes is None else nodes._h, d_score, C.byref(opts),
                                                   C.byref(out)))
        return Clusters(self, out)

    def gather(self, hits: "Hits", queries: "Sketches", targets: "Sketches", min_unique: int = 1, max_results: int = 0) -> "Hits":
        """ks_hits_gather: per query the greedy non-redundant targets.  Round after round the row of the query that covers the
        most hashes no earlier pick covered is kept (ties: the smaller tid) and its hashes are taken out; a query stops when the
        best remaining row would add fewer than min_unique new hashes (0 counts as 1) or after max_results rows (0: no limit).
        `hits` comes from any search of `queries` against an index of `targets` (thresholded and best-hits lists too).  The
        result is a Hits like that of best_hits — still in (qid, tid) order, with rank and src_row (Hits.best_to_host) — plus
        unique_intersect, remaining and unique_weighted per row (Hits.gather_to_host)."""
        for name, v in (("min_unique", min_unique), ("max_results", max_results)):
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError(f"{name} = {v} does not fit 32 bits")
        opts = _lib.ks_gather_opts(int(min_unique), int(max_results), 0, 0)
        out = C.c_void_p()
        self._check(self._L.ks_hits_gather(self._h, hits._h, queries._h, targets._h, C.byref(opts), C.byref(out)))
        return Hits(self, out)

    # ---- index / search ----
    def index_build(self, targets: "Sketches") -> "Index":
        out = C.c_void_p()
        self._check(self._L.ks_index_build(self._h, targets._h, C.byref(out)))
        return Index(self, out)

    def search(self, index: "Index", queries: "Sketches", *, min_containment: float = 0.0, abund_stats: bool = False) -> "Hits":
        """ks_search.  min_containment > 0 keeps the rows with intersect / (distinct query hashes) >= min_containment;
        abund_stats adds the per-row abundance statistics (Hits.abund_stats_to_host).  The defaults call ks_search itself."""
        out = C.c_void_p()
        opts = search_opts(min_containment, abund_stats)
        if opts is None:
            self._check(self._L.ks_search(self._h, index._h, queries._h, C.byref(out)))
        else:
            self._check(self._L.ks_search_ex(self._h, index._h, queries._h, C.byref(opts), C.byref(out)))
        return Hits(self, out)

    # ---- measurement ----
    def timing_enable(self, on=True):
        """on: False/0 off, True/1 every launch, 2 only the kernels that carry the bytes (low overhead)."""
        self._check(self._L.ks_timing_enable(self._h, int(on)))

    def timing_reset(self):
        self._check(self._L.ks_timing_reset(self._h))

    def device_rates(self) -> Dict[str, float]:
        """u64-multiply rate, device copy rate and nominal memory bandwidth of this context's GPU (bench.py prints them)."""
        v = [C.c_double(0) for _ in range(3)]
        self._check(self._L.ks_bench_device_rates(self._h, *[C.byref(x) for x in v]))
        return {"u64_gmul_per_s": v[0].value, "copy_gb_per_s": v[1].value, "nominal_gb_per_s": v[2].value}

    def gather_rates(self) -> Dict[str, float]:
        """Random 8-byte gathers per second from a 134 MB and from a 2 MB table (the ceiling of a table-lookup hash for hp)."""
        v = (C.c_double * 2)()
        self._check(self._L.ks_bench_gather_rates(self._h, C.byref(v)))
        return {"gathers_per_s_134mb": v[0], "gathers_per_s_2mb": v[1]}

    def timing(self) -> Dict[str, Tuple[int, float]]:
        """{kernel name: (launches, total ms)} from HIP events on the context's stream."""
        n = C.c_uint32(0)
        rows = (_lib.ks_kernel_time * 64)()
        self._check(self._L.ks_timing_get(self._h, rows, 64, C.byref(n)))
        return {rows[i].name.decode(): (int(rows[i].launches), float(rows[i].total_ms)) for i in range(min(n.value, 64))}


class _PinnedBlock:
    def __init__(self, ctx: "Context", ptr):
        self._ctx, self._p = ctx, ptr

    def __del__(self):
        try:
            if self._p is not None and self._ctx._h:
                self._ctx._L.ks_host_free(self._ctx._h, self._p)
        except Exception:
            pass
        self._p = None


class DeviceBuffer:
    def __init__(self, ctx: Context, ptr, nbytes: int):
        self._ctx, self._p, self.nbytes = ctx, ptr, nbytes

    @property
    def ptr(self) -> int:
        return int(self._p.value or 0)

    def to_host(self, dtype, count: Optional[int] = None) -> np.ndarray:
        """The first `count` items of `dtype` (default: the whole buffer) as a host array (ks_dev_download: ordered behind the
        work queued on the context's stream, returns when the copy is done)."""
        dt = np.dtype(dtype)
        n = self.nbytes // dt.itemsize if count is None else int(count)
        if n * dt.itemsize > self.nbytes:
            raise ValueError(f"{n} x {dt} does not fit a buffer of {self.nbytes} bytes")
        out = np.empty(n, dt)
        if n:
            self._ctx._check(self._ctx._L.ks_dev_download(self._ctx._h, _ptr(out), self._p, out.nbytes))
        return out

    def free(self):
        if self._p is not None and self._ctx._h:
            self._ctx._L.ks_dev_free(self._ctx._h, self._p)
        self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Owned:
    _free = None

    def __init__(self, ctx: Context, handle):
        self._ctx, self._h = ctx, handle
        self._pins, self._free_pending = 0, False

    def free(self):
        """Release the device object now — or, while views of its device arrays are alive (pin / unpin: the world-size-1
        hit exchange hands out torch views instead of copies), as soon as the last of them is gone."""
        if getattr(self, "_pins", 0) > 0:
            self._free_pending = True
            return
        if getattr(self, "_h", None) and self._ctx._h:
            getattr(self._ctx._L, self._free)(self._h)
        self._h = None

    def pin(self):
        self._pins += 1
        self._ctx._pinned += 1

    def unpin(self):
        self._pins -= 1
        self._ctx._pinned -= 1
        if self._pins == 0 and self._free_pending:
            self._free_pending = False
            self.free()
        if self._ctx._pinned == 0 and self._ctx._close_pending:
            self._ctx._close_pending = False
            self._ctx.close()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Sketches(_Owned):
    """Device-resident CSR of per-sequence sketches (ks_sketches)."""
    _free = "ks_sketches_free"

    @property
    def n_seqs(self) -> int:
        return int(self._ctx._L.ks_sketches_n_seqs(self._h))

    @property
    def n_hashes(self) -> int:
        return int(self._ctx._L.ks_sketches_n_hashes(self._h))

    @property
    def n_windows(self) -> int:
        return int(self._ctx._L.ks_sketches_n_windows(self._h))

    @property
    def has_postings(self) -> bool:
        return bool(self._ctx._L.ks_sketches_has_postings(self._h))

    @property
    def posting_bytes(self) -> int:
        """Bytes per partitioned query posting: 12, 10 (big fingerprint indexes at scaled = 1) or 0 (none attached)."""
        return (0, 12, 10)[int(self._ctx._L.ks_sketches_has_postings(self._h))]

    def device_ptrs(self) -> Tuple[int, int, int]:
        """Raw device pointers of the CSR (offsets u64[n_seqs + 1], hashes u64[n_hashes], abunds u32[n_hashes])."""
        L = self._ctx._L
        return tuple(int(f(self._h) or 0) for f in (L.ks_sketches_device_offsets, L.ks_sketches_device_hashes,
                                                    L.ks_sketches_device_abunds))

    def union(self) -> "Sketches":
        """Combined sketch: sorted unique hashes of all sequences with summed abundances (one sequence)."""
        out = C.c_void_p()
        self._ctx._check(self._ctx._L.ks_sketches_union(self._ctx._h, self._h, C.byref(out)))
        return Sketches(self._ctx, out)

    def union_groups(self, group_offsets) -> "Sketches":
        """ks_sketches_union_groups: sketch g of the result is the union of the sketches [group_offsets[g], group_offsets[g + 1])
        of this set, abundances summed per hash (saturating) — the proteins of a genome as one proteome sketch, the frames of a
        record as one.  group_offsets: n_groups + 1 ascending integers from 0 to n_seqs."""
        go = np.asarray(group_offsets)
        if go.ndim != 1 or go.size == 0 or (go.size and (go.min() < 0 or go.max() >= 2 ** 32)):
            raise ValueError("group_offsets must be a non-empty 1-d array of 32-bit offsets")
        go = np.ascontiguousarray(go, dtype=np.uint32)
        out = C.c_void_p()
        self._ctx._check(self._ctx._L.ks_sketches_union_groups(self._ctx._h, self._h, go.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                               len(go) - 1, C.byref(out)))
        return Sketches(self._ctx, out)

    def corpus(self) -> "Corpus":
        """Corpus table of the set (ks_corpus_build): per distinct hash its abundance sum (u64, no saturation) and the number
        of sketches that hold it, plus the set's total abundance — what `Context.significance` weighs shared hashes with."""
        out = C.c_void_p()
        self._ctx._check(self._ctx._L.ks_corpus_build(self._ctx._h, self._h, C.byref(out)))
        return Corpus(self._ctx, out)

    def to_host(self, pinned: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(offsets u64[n+1], hashes u64, abunds u32) on the host.  pinned=True returns arrays in pinned memory
        (Context.pinned_empty): one DMA at link rate instead of staged copies — what large sketch sets should use."""
        n, m = self.n_seqs, self.n_hashes
        if pinned:
            offs = self._ctx.pinned_empty(n + 1, np.uint64); hashes = self._ctx.pinned_empty(m, np.uint64)
            abunds = self._ctx.pinned_empty(m, np.uint32)
        else:
            offs = np.empty(n + 1, np.uint64); hashes = np.empty(m, np.uint64); abunds = np.empty(m, np.uint32)
        self._ctx._check(self._ctx._L.ks_sketches_copy_to_host(self._ctx._h, self._h, _ptr(offs), _ptr(hashes),
                                                               _ptr(abunds)))
        return offs, hashes, abunds


class KmerPositions(_Owned):
    """Device-resident (seq, start, hash) triples of the kept windows of a batch (ks_kmerpos), ordered by (seq, start)."""
    _free = "ks_kmerpos_free"

    @property
    def count(self) -> int:
        return int(self._ctx._L.ks_kmerpos_count(self._h))

    def to_host(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        n = self.count
        seq = np.zeros(n, np.uint32); start = np.zeros(n, np.uint32); h = np.zeros(n, np.uint64)
        self._ctx._check(self._ctx._L.ks_kmerpos_copy_to_host(self._ctx._h, self._h, _ptr(seq), _ptr(start), _ptr(h)))
        return seq, start, h


_DTYPE_NAMES = {"u1": "u8", "u4": "u32", "u8": "u64", "i8": "i64", "f8": "f64"}


def _with_doc(fn, doc):
    """A copy of the function `fn` that carries `doc`."""
    f = types.FunctionType(fn.__code__, fn.__globals__, fn.__name__, fn.__defaults__, fn.__closure__)
    f.__doc__, f.__annotations__, f.__qualname__ = doc, fn.__annotations__, fn.__qualname__
    return f


class _Columns(_Owned):
    """A device result object whose columns ONE table lists.  A subclass declares
        _PREFIX  the C prefix: ks_<prefix>_free, ks_<prefix>_copy_to_host, ks_<prefix>_device_<column>, ks_<prefix>_<count>;
        _COUNTS  {name of a count: its docstring or ""}: each becomes a read-only property over ks_<prefix>_<name>;
        _TABLE   one (column, dtype, count) per column in the order of ks_<prefix>_copy_to_host's parameters: dtype a numpy
                 code (u1, u4, u8, i8, f8), count an expression over the counts ("n_rows + 1"; a tuple gives a 2-d array).
    device_ptrs(), to_host(), _COLUMNS (the column names) and the count properties come from these; the docstrings of the two
    methods list the table."""
    _PREFIX, _COUNTS, _TABLE = None, {}, ()
    _VIEWS = {}  # {column: dtype}: a column whose bytes to_host() hands out under another dtype of the same size

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls._free = f"ks_{cls._PREFIX}_free"
        cls._COLUMNS = tuple(name for name, _, _ in cls._TABLE)
        for count, doc in cls._COUNTS.items():
            fn = f"ks_{cls._PREFIX}_{count}"
            setattr(cls, count, property(lambda self, fn=fn: int(getattr(self._ctx._L, fn)(self._h)), doc=doc or None))
        listing = ", ".join(f"{name} {_DTYPE_NAMES[dt]}[{n}]" for name, dt, n in cls._TABLE)
        cls.device_ptrs = _with_doc(_Columns.device_ptrs, f"Raw device pointers ({listing}).")
        cls.to_host = _with_doc(_Columns.to_host, f"The columns as numpy arrays ({listing}).")

    def device_ptrs(self) -> Tuple[int, ...]:
        L = self._ctx._L
        return tuple(int(getattr(L, f"ks_{self._PREFIX}_device_{c}")(self._h) or 0) for c in self._COLUMNS)

    def _copy_out(self, names) -> Tuple[np.ndarray, ...]:
        """The named columns as numpy arrays (ks_<prefix>_copy_to_host with NULL for every other column)."""
        counts = {c: getattr(self, c) for c in self._COUNTS}
        cols = [np.zeros(eval(n, {"__builtins__": {}}, counts), dt) if name in names else None for name, dt, n in self._TABLE]
        self._ctx._check(getattr(self._ctx._L, f"ks_{self._PREFIX}_copy_to_host")(self._ctx._h, self._h, *[_ptr(c) for c in cols]))
        return tuple(c.view(self._VIEWS[name]) if name in self._VIEWS else c for c, (name, _, _) in zip(cols, self._TABLE) if c is not None)

    def to_host(self) -> Tuple[np.ndarray, ...]:
        return self._copy_out(self._COLUMNS)


class Mask(_Columns):
    """Device-resident low-complexity mask of a residue batch (ks_mask): one byte per residue, 1 = masked, and per record its
    masked residues."""
    _PREFIX, _COUNTS = "mask", {"n_seqs": "", "n_residues": "", "n_masked": "masked residues of the whole batch"}
    _TABLE = (("mask", "u1", "n_residues"), ("masked_counts", "u4", "n_seqs"))


class Segments(_Columns):
    """Device-resident unmasked segments of a batch (ks_segments): per segment its record and its start in the record, the
    segments' residues as one batch (seg_offsets, residues) and per record the range of its segments (group_offsets)."""
    _PREFIX, _COUNTS = "segments", {"n_segs": "", "n_residues": "", "n_records": ""}
    _TABLE = (("seg_record", "u4", "n_segs"), ("seg_start", "u4", "n_segs"), ("seg_offsets", "u8", "n_segs + 1"),
              ("residues", "u1", "n_residues"), ("group_offsets", "u4", "n_records + 1"))


class MatchPositions(_Columns):
    """Device-resident CSR over hit rows (ks_matchpos): row r of the hits owns pairs [row_offsets[r], row_offsets[r + 1])."""
    _PREFIX, _COUNTS = "matchpos", {"n_rows": "", "n_pairs": ""}
    _TABLE = (("row_offsets", "u8", "n_rows + 1"), ("q_start", "u4", "n_pairs"), ("t_start", "u4", "n_pairs"),
              ("q_lo", "u4", "n_rows"), ("q_hi", "u4", "n_rows"), ("t_lo", "u4", "n_rows"), ("t_hi", "u4", "n_rows"))

    @property
    def n_slices(self) -> int:
        """Hit-row slices the call ran in (1 unless row index and starts do not fit one 64-bit key).  Diagnostic."""
        return int(self._ctx._L.ks_matchpos_n_slices(self._h))


class Regions(_Columns):
    """Device-resident CSR over hit rows (ks_regions): row r of the hits owns regions [row_offsets[r], row_offsets[r + 1])."""
    _PREFIX, _COUNTS = "regions", {"n_rows": "", "n_regions": ""}
    _TABLE = (("row_offsets", "u8", "n_rows + 1"),) + tuple((c, "u4", "n_regions") for c in ("q_start", "t_start", "length", "n_kmers", "covered"))

    @property
    def n_slices(self) -> int:
        """Hit-row slices the chaining ran in (1 unless row index, diagonal and start do not fit one 64-bit key).  Diagnostic."""
        return int(self._ctx._L.ks_regions_n_slices(self._h))


class RegionScores(_Columns):
    """Device-resident scores of the regions of a hit list (ks_rscores): the CSR of the Regions they were made from, per region
    the extended placement, the score, identities, positives and the identities of the seed region alone."""
    _PREFIX, _COUNTS = "rscores", {"n_rows": "", "n_regions": ""}
    _TABLE = (("row_offsets", "u8", "n_rows + 1"), ("q_start", "u4", "n_regions"), ("t_start", "u4", "n_regions"),
              ("length", "u4", "n_regions"), ("score", "i8", "n_regions"), ("identities", "u4", "n_regions"),
              ("positives", "u4", "n_regions"), ("core_identities", "u4", "n_regions"))


class RegionAlignments(_Columns):
    """Device-resident gapped alignments of the regions of a hit list (ks_raligns): the CSR of the Regions they were made from,
    per region the alignment's extents on both sequences, its score and its counts."""
    _PREFIX, _COUNTS = "raligns", {"n_rows": "", "n_regions": ""}
    _TABLE = (("row_offsets", "u8", "n_rows + 1"),) + tuple(
        (c, "i8" if c == "score" else "u4", "n_regions") for c in ("q_start", "q_length", "t_start", "t_length", "score", "identities",
                                                                    "positives", "gap_opens", "gaps", "aln_length"))


    @property
    def by_profile(self) -> bool:
        """Made against a Profile (align_regions(..., profile=)): trace_regions needs that profile, and the passes that read
        residues under a matrix (stitch, fold, alignment_stats, pileup) refuse the object."""
        return bool(self._ctx._L.ks_raligns_by_profile(self._h))


CIGAR_OPS = "MIDNSHP=X"  # the BAM op codes


def cigar_strings(op_offsets, ops) -> List[str]:
    """The CIGAR of every region as text ("35M2D17M1I40M") from RegionCigars.to_host(): an op is len << 4 | code."""
    offs = np.asarray(op_offsets).tolist()
    ops = np.asarray(ops).tolist()
    if any(v & 15 >= len(CIGAR_OPS) for v in ops):
        raise ValueError("an op code beyond the BAM codes")
    return ["".join(f"{v >> 4}{CIGAR_OPS[v & 15]}" for v in ops[offs[g]:offs[g + 1]]) for g in range(len(offs) - 1)]


class RegionCigars(_Columns):
    """Device-resident paths of the alignments of a hit list's regions (ks_cigars): a CSR over the regions in the order of the
    RegionAlignments they were traced from, region g owns ops [op_offsets[g], op_offsets[g + 1]), an op is len << 4 | BAM code."""
    _PREFIX, _COUNTS = "cigars", {
        "n_rows": "", "n_regions": "", "n_ops": "",
        "n_slices": "Slices of regions the traceback ran in (1 unless the directions did not fit max_scratch_bytes).  Diagnostic.",
        "scratch_bytes": "Direction scratch the traceback allocated.  Diagnostic."}
    _TABLE = (("op_offsets", "u8", "n_regions + 1"), ("ops", "u4", "n_ops"))

    def strings(self) -> List[str]:
        """The CIGAR of every region as text, e.g. "35M2D17M1I40M"."""
        return cigar_strings(*self.to_host())


class RegionCull(_Columns):
    """Device-resident result of Context.cull_regions (ks_rcull): a CSR of the kept regions over the input's hit rows — per
    kept region its input index (src_region), its rank inside the row (0: the best) and how many input regions it stands for
    (n_merged) — per input region its keeper (0xffffffff: dropped) and per hit row the score of its best kept region as f64
    (NaN: the row keeps none), a `score=` column for Context.best_hits."""
    _PREFIX, _COUNTS = "rcull", {"n_rows": "", "n_regions": "Regions of the input.", "n_kept": ""}
    _TABLE = (("row_offsets", "u8", "n_rows + 1"), ("src_region", "u4", "n_kept"), ("rank", "u4", "n_kept"), ("n_merged", "u4", "n_kept"),
              ("keeper", "u4", "n_regions"), ("row_best_score", "f8", "n_rows"))

    @property
    def row_best_score_ptr(self) -> int:
        """The device column row_best_score f64[n_rows]: pass it to Context.best_hits(score=...)."""
        return int(self._ctx._L.ks_rcull_device_row_best_score(self._h) or 0)

    def take(self, obj):
        """The Regions, RegionScores or RegionAlignments of the kept regions only (ks_*_take): every column gathered by
        src_region, the row offsets of this cull.  `obj` must hold the regions the cull was made of."""
        for cls in (Regions, RegionScores, RegionAlignments):
            if isinstance(obj, cls):
                out = C.c_void_p()
                self._ctx._check(getattr(self._ctx._L, f"ks_{cls._PREFIX}_take")(self._ctx._h, obj._h, self._h, C.byref(out)))
                return cls(self._ctx, out)
        raise TypeError("take() gathers a Regions, a RegionScores or a RegionAlignments")


class RegionChain(_Columns):
    """Device-resident result of Context.chain_regions (ks_rchain): a CSR of the members of each hit row's best colinear chain
    in chain order (src_region), per input region its best chain value and its predecessor (0xffffffff: none), and per hit row
    the chain's score, its span and its aligned lengths on both sequences, the sums of identities and aln_length over its
    members and the score as f64 (NaN: a row without regions), a `score=` column for Context.best_hits and the cluster passes.
    coverage() adds row_coverage, the share of the sequences the chain covers."""
    _PREFIX, _COUNTS = "rchain", {"n_rows": "", "n_regions": "Regions of the input.", "n_chained": ""}
    _TABLE = (("row_offsets", "u8", "n_rows + 1"), ("src_region", "u4", "n_chained"), ("best", "i8", "n_regions"), ("pred", "u4", "n_regions"),
              ("chain_score", "i8", "n_rows")) + \
        tuple((c, "u4", "n_rows") for c in ("q_start", "q_length", "t_start", "t_length", "q_aligned", "t_aligned")) + \
        (("identities", "u8", "n_rows"), ("aln_length", "u8", "n_rows"), ("row_chain_score", "f8", "n_rows"))
    _MODES = {"query": 0, "target": 1, "min": 2, "max": 3}

    @property
    def row_chain_score_ptr(self) -> int:
        """The device column row_chain_score f64[n_rows]: pass it to Context.best_hits(score=...) or a cluster pass."""
        return int(self._ctx._L.ks_rchain_device_row_chain_score(self._h) or 0)

    @property
    def row_coverage_ptr(self) -> int:
        """The device column row_coverage f64[n_rows]; 0 before coverage()."""
        return int(self._ctx._L.ks_rchain_device_row_coverage(self._h) or 0)

    def coverage(self, hits: "Hits", d_q_off: int, n_q: int, d_t_off: int, n_t: int, mode="min") -> int:
        """ks_rchain_coverage: fills the chain's device column row_coverage f64[n_rows] — per hit row q_aligned / len(query)
        (mode "query" or 0), t_aligned / len(target) ("target", 1), the smaller ("min", 2) or the larger ("max", 3) of the two;
        NaN for a row without a chain or a sequence of length 0 — and returns its device pointer, a `score=` column for
        Context.cluster / cluster_greedy.  d_q_off, d_t_off: device pointers of the u64 sequence offsets align_regions_device
        takes; hits: the hit list of the chained regions."""
        m = self._MODES.get(mode, mode)
        if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= 3:
            raise ValueError(f"mode = {mode!r} is not one of 'query', 'target', 'min', 'max' or 0 .. 3")
        self._ctx._check(self._ctx._L.ks_rchain_coverage(self._ctx._h, self._h, hits._h, C.c_void_p(int(d_q_off)), int(n_q),
                                                         C.c_void_p(int(d_t_off)), int(n_t), m))
        return self.row_coverage_ptr

    def coverage_from_host(self, hits: "Hits", q_off: np.ndarray, t_off: np.ndarray, mode="min") -> int:
        """coverage from host arrays of sequence offsets u64[n + 1] (those of the batches `hits` was searched on): uploaded
        for the call, as align_regions does."""
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64); t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        with self._ctx._uploaded(q_off, t_off) as (d_q, d_t):
            return self.coverage(hits, d_q, len(q_off) - 1, d_t, len(t_off) - 1, mode=mode)

    def coverage_to_host(self) -> np.ndarray:
        """row_coverage f64[n_rows] of the last coverage call."""
        out = np.zeros(self.n_rows, np.float64)
        self._ctx._check(self._ctx._L.ks_rchain_coverage_to_host(self._ctx._h, self._h, _ptr(out)))
        return out


class FrameFold(_Columns):
    """Device-resident result of Context.fold_frames (ks_ffold): the frame rows of a translated search folded into one row per
    (record, strand, target) — `hits`, a Hits with qid = 2 * record + strand, is the folded hit list — and their regions on the
    strand's bases.  Per folded row src_row (the input rows of its three frames, 0xffffffff: none) and row_offsets, the CSR of
    its regions (frame 0's, then frame 1's, then frame 2's); per region the input region, its frame 0 .. 5, nt_length, s_start
    (in the strand's own orientation: what chain_frames chains on), nt_start (on the record as given), t_start3 / t_length3
    (the target in bases) and the gathered score, identities and aln_length.  A fold made without one of the last three has no
    such column: its device pointer is 0 and to_host() leaves zeros (has_score, has_identities, has_aln_length tell)."""
    _PREFIX, _COUNTS = "ffold", {"n_rows": "Folded rows.", "n_regions": "", "n_src_rows": "Hit rows of the input."}
    _TABLE = (("src_row", "u4", "3 * n_rows"), ("row_offsets", "u8", "n_rows + 1"), ("src_region", "u4", "n_regions"), ("frame", "u1", "n_regions")) + \
        tuple((c, "u4", "n_regions") for c in ("nt_length", "s_start", "nt_start", "t_start3", "t_length3")) + \
        (("score", "i8", "n_regions"), ("identities", "u4", "n_regions"), ("aln_length", "u4", "n_regions"))

    def __init__(self, ctx: "Context", handle, hits: "Hits"):
        super().__init__(ctx, handle)
        self.hits = hits

    @property
    def has_score(self) -> bool:
        return bool(self._ctx._L.ks_ffold_device_score(self._h))

    @property
    def has_identities(self) -> bool:
        return bool(self._ctx._L.ks_ffold_device_identities(self._h))

    @property
    def has_aln_length(self) -> bool:
        return bool(self._ctx._L.ks_ffold_device_aln_length(self._h))

    def free(self):
        """Releases the fold and its folded hit list."""
        hits = getattr(self, "hits", None)
        if hits is not None:
            hits.free()
        super().free()


class _StitchedRows:
    """What the two stitched results share beside a table (HitAlignments, FrameAlignments): the diagnostic counts, the
    row_score column alone and the CIGARs alone.  A subclass declares _DOCS: the docstrings of row_score_ptr and of strings."""
    _COUNTS = {"n_rows": "", "n_ops": "",
               "n_slices": "Slices of chain members the fills ran in (1 unless the directions did not fit max_scratch_bytes).  Diagnostic.",
               "scratch_bytes": "Direction scratch the call allocated.  Diagnostic."}

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        fn = f"ks_{cls._PREFIX}_device_row_score"
        cls.row_score_ptr = property(lambda self: int(getattr(self._ctx._L, fn)(self._h) or 0), doc=cls._DOCS[0])
        cls.strings = _with_doc(_StitchedRows.strings, cls._DOCS[1])

    def ops_to_host(self) -> Tuple[np.ndarray, np.ndarray]:
        """(op_offsets u64[n_rows + 1], ops u32[n_ops]) alone."""
        return self._copy_out(("op_offsets", "ops"))

    def strings(self) -> List[str]:
        return cigar_strings(*self.ops_to_host())


class HitAlignments(_StitchedRows, _Columns):
    """Device-resident result of Context.stitch_chains (ks_hitalns): per hit row ONE gapped alignment — the members of the
    row's chain with the links between them filled — as a CSR of BAM-encoded ops (row r owns ops [op_offsets[r],
    op_offsets[r + 1]), an op is len << 4 | code) and the columns of that alignment: its span on both sequences, score (i64),
    identities, positives, gap_opens, gaps, aln_length, the chain members, filled and open links and trimmed columns behind it,
    and the score as f64 (NaN: a row without a chain), a `score=` column for Context.best_hits and the cluster passes."""
    _PREFIX = "hitalns"
    _TABLE = (("op_offsets", "u8", "n_rows + 1"), ("ops", "u4", "n_ops")) + tuple(
        (c, {"score": "i8", "row_score": "f8"}.get(c, "u4"), "n_rows") for c in (
            "q_start", "q_length", "t_start", "t_length", "score", "identities", "positives", "gap_opens", "gaps", "aln_length",
            "n_members", "n_filled", "n_open", "n_trimmed", "row_score"))
    _DOCS = ("The device column row_score f64[n_rows]: pass it to Context.best_hits(score=...) or a cluster pass.",
             'The CIGAR of every hit row as text, e.g. "60M40I60M"; "" for a row without a chain.')


class FrameAlignments(_StitchedRows, _Columns):
    """Device-resident result of Context.stitch_frames (ks_framealns): per folded row of a translated search ONE alignment of
    the strand's bases against the target protein, as a CSR of BAM-encoded ops in codon columns (row r owns ops
    [op_offsets[r], op_offsets[r + 1]), an op is len << 4 | code; M, = and X a codon against a residue, I a codon alone, D a
    residue alone, N a frameshift of 1 or 2 skipped bases) and the columns of that alignment: its span in strand bases (s_start,
    nt_length), nt_start on the record as given, its span on the target, score (i64: pairs minus gaps minus frameshift_cost per
    N), identities, positives, gap_opens, gaps, aln_length (N not counted), the chain members, filled and open links, trimmed
    columns and frameshifts behind it, and the score as f64 (NaN: a row without a chain), a `score=` column for
    Context.best_hits(fold.hits, ...)."""
    _PREFIX = "framealns"
    _TABLE = (("op_offsets", "u8", "n_rows + 1"), ("ops", "u4", "n_ops")) + tuple(
        (c, {"score": "i8", "row_score": "f8"}.get(c, "u4"), "n_rows") for c in (
            "s_start", "nt_length", "nt_start", "t_start", "t_length", "score", "identities", "positives", "gap_opens", "gaps", "aln_length",
            "n_members", "n_filled", "n_open", "n_trimmed", "n_frameshifts", "row_score"))
    _DOCS = ("The device column row_score f64[n_rows]: pass it to Context.best_hits(fold.hits, score=...).",
             'The CIGAR of every folded row as text, e.g. "41M1N59M"; "" for a row without a chain.')


class Pileup(_Columns):
    """Device-resident result of Context.pileup (ks_pileup): the alignments of a hit list piled up on the residues of one
    batch.  Per residue of the batch (batch coordinates offsets[seq] + position) depth, the pair columns that place it, and —
    with profile=True, else an empty column — counts, 28 per residue: those columns by the class of the residue aligned to it
    (reshape(-1, 28); the classes of Composition).  Per sequence length, n_alignments (entries with a pair column on it),
    covered (positions with depth > 0), max_depth, depth_sum, breadth = covered / length and mean_depth = depth_sum / length
    (NaN for an empty sequence)."""
    _PREFIX = "pileup"
    _COUNTS = {"n_seqs": "", "n_residues": "", "n_profile": "Entries of counts: 28 x n_residues with the profile, else 0."}
    _TABLE = (("depth", "u4", "n_residues"), ("counts", "u4", "n_profile")) + tuple(
        (c, {"depth_sum": "u8", "breadth": "f8", "mean_depth": "f8"}.get(c, "u4"), "n_seqs") for c in (
            "length", "n_alignments", "covered", "max_depth", "depth_sum", "breadth", "mean_depth"))

    @property
    def depth_ptr(self) -> int:
        """The device column depth u32[n_residues]."""
        return int(self._ctx._L.ks_pileup_device_depth(self._h) or 0)

    @property
    def n_weighted(self) -> int:
        """Entries of wdepth: n_residues for a pileup made with weights, else 0."""
        return int(self._ctx._L.ks_wpileup_n_weighted(self._h))

    @property
    def wdepth_ptr(self) -> int:
        """The device column wdepth u64[n_weighted]; 0 without weights."""
        return int(self._ctx._L.ks_wpileup_device_wdepth(self._h) or 0)

    @property
    def wcounts_ptr(self) -> int:
        """The device column wcounts u64[n_weighted * 28] (with the profile); 0 without weights."""
        return int(self._ctx._L.ks_wpileup_device_wcounts(self._h) or 0)

    def weighted_to_host(self) -> Tuple[np.ndarray, np.ndarray]:
        """(wdepth u64[n_weighted], wcounts u64[28 * n_weighted with the profile, else 0]) of a pileup made with weights: per
        residue the weights of the entries that place it, summed, and the same by the class of the residue aligned to it."""
        wdepth = np.zeros(self.n_weighted, np.uint64)
        wcounts = np.zeros(self.n_profile if self.n_weighted else 0, np.uint64)
        self._ctx._check(self._ctx._L.ks_wpileup_copy_to_host(self._ctx._h, self._h, _ptr(wdepth), _ptr(wcounts)))
        return wdepth, wcounts


class EntryWeights(_Columns):
    """Device-resident result of Context.entry_weights (ks_pweights): per entry of a pileup its weight u32 in units of 2^-30
    (KS_WEIGHT_ONE is 1; 0 for an entry that was not taken) and n_cols, its pair columns."""
    _PREFIX, _COUNTS = "pweights", {"n_entries": ""}
    _TABLE = (("weight", "u4", "n_entries"), ("n_cols", "u4", "n_entries"))

    @property
    def weight_ptr(self) -> int:
        """The device column weight u32[n_entries]: pass it to Context.pileup_device(d_weight=)."""
        return int(self._ctx._L.ks_pweights_device_weight(self._h) or 0)


class Profile(_Columns):
    """Device-resident position-specific scores of a query batch (ks_profile, Context.build_profile): per residue of the batch
    (batch coordinates offsets[seq] + position) a row of 28 scores (reshape(-1, 28); the classes of Composition), the
    consensus byte and n_obs, the observations behind the row (0: the row is the fallback matrix's).  The C ABI hands the
    scores out as bytes; to_host() gives them as the int8 they are."""
    _PREFIX = "profile"
    _COUNTS = {"n_seqs": "", "n_residues": "", "n_scores": "Entries of scores: 28 x n_residues."}
    _TABLE = (("scores", "u1", "n_scores"), ("consensus", "u1", "n_residues"), ("n_obs", "u4", "n_residues"))
    _VIEWS = {"scores": np.int8}

    @property
    def scores_ptr(self) -> int:
        """The device column scores i8[n_residues * 28]."""
        return int(self._ctx._L.ks_profile_device_scores(self._h) or 0)

    def consensus_strings(self, offsets) -> List[str]:
        """The consensus of every sequence of the batch as text (offsets: the batch's, n_seqs + 1)."""
        offs = [int(v) for v in np.asarray(offsets).tolist()]
        if len(offs) != self.n_seqs + 1 or (offs and offs[-1] != self.n_residues):
            raise ValueError(f"the profile is of {self.n_seqs} sequences and {self.n_residues} residues: offsets of another batch")
        text = self._copy_out(("consensus",))[0].tobytes().decode("latin-1")
        return [text[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


class Composition(_Columns):
    """Device-resident residue composition of a batch (ks_rcomp): counts u32[n_seqs, 28] over the residue classes of
    score_regions, length u32[n_seqs] and the class totals u64[28] of the batch."""
    _PREFIX, _COUNTS = "rcomp", {"n_seqs": "", "n_residues": ""}
    _TABLE = (("counts", "u4", "n_seqs, 28"), ("totals", "u8", "28"), ("length", "u4", "n_seqs"))


class AlignmentStats(_Columns):
    """Device-resident result of Context.alignment_stats (ks_astats): per hit row status u8 (0 regular, 1 fallback, 2 no
    composition asked for), x f64 (e^-lambda of the pair), lambda_ratio f64, row_bit_score and row_evalue f64 (the row's best;
    NaN for a row without entries); per entry bit_score and evalue f64."""
    _PREFIX = "astats"
    _COUNTS = {"n_rows": "", "n_entries": "", "n_fallback": "Hit rows whose composition gave no lambda of their own (ratio 1)."}
    _TABLE = (("status", "u1", "n_rows"), ("x", "f8", "n_rows"), ("lambda_ratio", "f8", "n_rows"), ("bit_score", "f8", "n_entries"),
              ("evalue", "f8", "n_entries"), ("row_bit_score", "f8", "n_rows"), ("row_evalue", "f8", "n_rows"))

    @property
    def lambda_std(self) -> float:
        return float(self._ctx._L.ks_astats_lambda_std(self._h))

    @property
    def lambda_used(self) -> float:
        return float(self._ctx._L.ks_astats_lambda_used(self._h))

    @property
    def K_used(self) -> float:
        return float(self._ctx._L.ks_astats_k_used(self._h))

    @property
    def params_source(self) -> int:
        """0: lambda and K were computed (ungapped), 1: the caller's."""
        return int(self._ctx._L.ks_astats_params_source(self._h))

    @property
    def row_bit_score_ptr(self) -> int:
        """The device column row_bit_score f64[n_rows]: pass it to Context.best_hits(score=...) or a cluster pass."""
        return int(self._ctx._L.ks_astats_device_row_bit_score(self._h) or 0)

    @property
    def row_evalue_ptr(self) -> int:
        """The device column row_evalue f64[n_rows]."""
        return int(self._ctx._L.ks_astats_device_row_evalue(self._h) or 0)


class Clusters(_Columns):
    """Device-resident clusters of a hit list (ks_clusters): per node its label and cluster_id, the clusters as a CSR (offsets,
    members) and a representative per cluster.  From cluster(): connected components, the label is the smallest id of the
    cluster and orders the clusters.  From cluster_greedy(): the label is the representative's id and orders the clusters."""
    _PREFIX = "clusters"
    _COUNTS = {"n_nodes": "", "n_clusters": "", "n_edges": "Rows that passed the threshold: self rows and both directions counted as they occur.",
               "largest": "", "n_rounds": "Rounds a cluster_greedy() result took (a diagnostic: it may depend on the schedule); 0 for cluster()."}
    _TABLE = (("label", "u4", "n_nodes"), ("cluster_id", "u4", "n_nodes"), ("offsets", "u8", "n_clusters + 1"), ("members", "u4", "n_nodes"),
              ("representative", "u4", "n_clusters"))


class Corpus(_Owned):
    """Device-resident corpus table of a sketch set (ks_corpus): distinct hashes ascending, abundance sums, document frequencies."""
    _free = "ks_corpus_free"

    @property
    def n_hashes(self) -> int:
        return int(self._ctx._L.ks_corpus_n_hashes(self._h))

    @property
    def n_docs(self) -> int:
        """Sketches of the set, empty ones included."""
        return int(self._ctx._L.ks_corpus_n_docs(self._h))

    @property
    def total_abund(self) -> int:
        return int(self._ctx._L.ks_corpus_total_abund(self._h))

    def to_host(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(hashes u64, abund_sum u64, doc_freq u32), n_hashes entries each."""
        n = self.n_hashes
        h = np.zeros(n, np.uint64); a = np.zeros(n, np.uint64); d = np.zeros(n, np.uint32)
        self._ctx._check(self._ctx._L.ks_corpus_copy_to_host(self._ctx._h, self._h, _ptr(h), _ptr(a), _ptr(d)))
        return h, a, d


class Significance(_Columns):
    """Device-resident f64 columns over hit rows (ks_signif): prob_overlap and tf_idf, row r belongs to row r of the hits."""
    _PREFIX, _COUNTS = "signif", {"n_rows": ""}
    _TABLE = (("prob_overlap", "f8", "n_rows"), ("tf_idf", "f8", "n_rows"))

    @property
    def prob_overlap_ptr(self) -> int:
        """Device pointer of the prob_overlap column (`Context.best_hits(score=...)`)."""
        return self.device_ptrs()[0]

    @property
    def tf_idf_ptr(self) -> int:
        """Device pointer of the tf_idf column (`Context.best_hits(score=...)`)."""
        return self.device_ptrs()[1]


class Index(_Owned):
    _free = "ks_index_free"

    @property
    def n_targets(self) -> int:
        return int(self._ctx._L.ks_index_n_targets(self._h))

    @property
    def n_postings(self) -> int:
        return int(self._ctx._L.ks_index_n_postings(self._h))


class Hits(_Owned):
    _free = "ks_hits_free"

    @property
    def count(self) -> int:
        return int(self._ctx._L.ks_hits_count(self._h))

    @property
    def n_pair_instances(self) -> int:
        return int(self._ctx._L.ks_hits_n_pair_instances(self._h))

    @property
    def partition_path(self) -> int:
        """0 sketch regions == buckets, 1 regions + bucket scatter, 2 regions + dense pass, 3 dense from the CSR."""
        return int(self._ctx._L.ks_hits_partition_path(self._h))

    @property
    def bucket_posting_bytes(self) -> int:
        """Bytes per query posting inside the join buckets (12 / 10 / 9; 0 = no bucket scatter ran)."""
        return int(self._ctx._L.ks_hits_bucket_posting_bytes(self._h))

    def device_ptrs(self) -> Tuple[int, int, int, int]:
        """Raw device pointers of the COO columns (qid u32, tid u32, intersect u32, n_weighted u64), `count` entries each."""
        L = self._ctx._L
        return tuple(int(f(self._h) or 0) for f in (L.ks_hits_device_qid, L.ks_hits_device_tid, L.ks_hits_device_intersect,
                                                    L.ks_hits_device_n_weighted))

    def copy_to_device(self, d_qid: int, d_tid: int, d_isect: int, d_nw: int, qid_base: int = 0, tid_base: int = 0):
        """D2D copy of the columns into caller-owned device buffers (ids shifted to global numbering); asynchronous on the
        context's stream.  This is how a shard's hits enter the send block of an all-gather (kmerseek_amd/dist.py)."""
        self._ctx._check(self._ctx._L.ks_hits_copy_to_device(self._ctx._h, self._h, qid_base, tid_base, C.c_void_p(d_qid),
                                                             C.c_void_p(d_tid), C.c_void_p(d_isect), C.c_void_p(d_nw)))

    def pack64_to_device(self, d_packed: int, d_esc_row: int, d_esc_isect: int, d_esc_nw: int, d_n_esc: int, esc_cap: int,
                         qbits: int, tbits: int, qid_base: int = 0, tid_base: int = 0):
        """Rows as 64-bit transport words (ks_hits_pack64_to_device) into caller-owned device buffers: 8 instead of 20
        bytes per row for the all-gather of a multi-GPU search; rows with wide values go to the escape list."""
        self._ctx._check(self._ctx._L.ks_hits_pack64_to_device(self._ctx._h, self._h, qid_base, tid_base, qbits, tbits,
                                                               C.c_void_p(d_packed), C.c_void_p(d_esc_row), C.c_void_p(d_esc_isect),
                                                               C.c_void_p(d_esc_nw), C.c_void_p(d_n_esc), esc_cap))

    def to_host(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        n = self.count
        qid = np.zeros(n, np.uint32); tid = np.zeros(n, np.uint32)
        isect = np.zeros(n, np.uint32); nw = np.zeros(n, np.uint64)
        self._ctx._check(self._ctx._L.ks_hits_copy_to_host(self._ctx._h, self._h, _ptr(qid), _ptr(tid), _ptr(isect),
                                                           _ptr(nw)))
        return qid, tid, isect, nw

    @property
    def has_abund_stats(self) -> bool:
        return bool(self._ctx._L.ks_hits_has_abund_stats(self._h))

    def abund_stats_to_host(self) -> Tuple[np.ndarray, np.ndarray]:
        """(median2 u64, ss f64) per row of a search with abund_stats=True: 2 x the median and the sum of squared deviations
        from the mean of the shared target abundances (median = median2 / 2, std = sqrt(ss / intersect))."""
        n = self.count
        median2 = np.zeros(n, np.uint64); ss = np.zeros(n, np.float64)
        self._ctx._check(self._ctx._L.ks_hits_copy_abund_stats_to_host(self._ctx._h, self._h, _ptr(median2), _ptr(ss)))
        return median2, ss

    def best_to_host(self) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        """(rank u32, src_row u32) per row of a `Context.best_hits` result: the row's rank inside its query (0 = best) and its
        row in the hit list it was chosen from.  None for hits that did not come from best_hits."""
        if not self._ctx._L.ks_hits_device_rank(self._h):
            return None
        n = self.count
        rank = np.zeros(n, np.uint32); src = np.zeros(n, np.uint32)
        self._ctx._check(self._ctx._L.ks_hits_copy_best_to_host(self._ctx._h, self._h, _ptr(rank), _ptr(src)))
        return rank, src

    def gather_to_host(self) -> Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
        """(unique_intersect u32, remaining u32, unique_weighted u64) per row of a `Context.gather` result: the hashes the row
        newly covered, the query's hashes still uncovered after it, and the query's abundances summed over the newly covered
        ones.  None for hits that did not come from gather."""
        if not self._ctx._L.ks_hits_device_unique_intersect(self._h):
            return None
        n = self.count
        uniq = np.zeros(n, np.uint32); rem = np.zeros(n, np.uint32); uw = np.zeros(n, np.uint64)
        self._ctx._check(self._ctx._L.ks_hits_copy_gather_to_host(self._ctx._h, self._h, _ptr(uniq), _ptr(rem), _ptr(uw)))
        return uniq, rem, uw
