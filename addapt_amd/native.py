"""ctypes binding of the engine's C ABI (include/addapt_gpu.h).

This is the Python face of the product: it loads the in-tree
``addapt_amd/_lib/libaddapt_gpu.so`` (built by ``__graft_entry__.build()``)
and fails loudly when it is missing -- there is no CPU fallback.
"""
import collections
import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADX_LIB") or os.path.join(HERE, "_lib", "libaddapt_gpu.so")
DEFAULT_PARAMS = os.path.join(HERE, "data", "rna_turner2004_addapt.par")

ABI_VERSION = 4   # include/addapt_gpu.h ADX_ABI_VERSION (v4 renumbered the motif modes)
OK, EINVAL, EHIP, ECONSTRAINT, EPARAM, ENOMEM, EMOVE, ESTATE, ENODEV, EUNSUPPORTED = range(10)
APO, HOLO = 0, 1
THERMO_FIXED, THERMO_ANNEAL, THERMO_AUTO = 0, 1, 2
MOTIF_AUTO, MOTIF_ADD, MOTIF_REPLACE = 0, 1, 2   # include/addapt_gpu.h; AUTO is the default
FOLD_PF, FOLD_MFE = 0, 1
TERM_MACROSTATE, TERM_PAIR = 0, 1
OUTCOMES = ["REJECT", "ACCEPT_WORSENED", "ACCEPT_UNCHANGED", "ACCEPT_IMPROVED"]


class AdxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("adx status %d: %s" % (status, msg))
        self.status = status


class Term(C.Structure):
    _fields_ = [("condition", C.c_int), ("macrostate", C.c_int), ("favorable", C.c_int),
                ("weight", C.c_double), ("kind", C.c_int), ("pair_i", C.c_int), ("pair_j", C.c_int)]


class Thermostat(C.Structure):
    _fields_ = [("kind", C.c_int), ("t_fixed", C.c_double), ("t_hi", C.c_double),
                ("t_lo", C.c_double), ("cycle_len", C.c_int), ("target_rate", C.c_double),
                ("period", C.c_int), ("t_init", C.c_double)]


class ContextDesc(C.Structure):
    _fields_ = [("before", C.c_char_p), ("after", C.c_char_p)]


class RunDesc(C.Structure):
    _fields_ = [("params", C.c_void_p), ("sequence", C.c_char_p), ("n_macrostates", C.c_int),
                ("macrostates", C.POINTER(C.c_char_p)), ("n_terms", C.c_int),
                ("terms", C.POINTER(Term)), ("aptamer_seq", C.c_char_p),
                ("aptamer_fold", C.c_char_p), ("aptamer_energy_kcal", C.c_double),
                ("motif_mode", C.c_int), ("n_contexts", C.c_int),
                ("contexts", C.POINTER(ContextDesc)), ("thermostat", Thermostat),
                ("device", C.c_int), ("fold_mode", C.c_int)]


class Info(C.Structure):
    _fields_ = [("length", C.c_int), ("n_variants", C.c_int), ("n_terms", C.c_int),
                ("n_mutable", C.c_int), ("max_walkers", C.c_int), ("scale_per_nt", C.c_double)]


class EnsembleStats(C.Structure):
    _fields_ = [("mea", C.c_double), ("centroid_dist", C.c_double), ("diversity", C.c_double)]


class Trace(C.Structure):
    _fields_ = [("position", C.POINTER(C.c_int32)), ("base", C.c_char_p),
                ("outcome", C.POINTER(C.c_int32)), ("temperature", C.POINTER(C.c_double)),
                ("proposed_score", C.POINTER(C.c_double)), ("current_score", C.POINTER(C.c_double)),
                ("random_threshold", C.POINTER(C.c_double)), ("term_values", C.POINTER(C.c_double))]


# Every symbol include/addapt_gpu.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "adx_last_error", "adx_abi_version", "adx_params_load", "adx_params_free", "adx_kT",
    "adx_eval_structure", "adx_fold_create", "adx_fold_add_motif", "adx_fold_add_constraint",
    "adx_fold_pf", "adx_fold_mfe", "adx_fold_bpp", "adx_fold_free", "adx_ctx_create", "adx_ctx_destroy",
    "adx_ctx_info", "adx_walkers_init", "adx_run_steps", "adx_last_kernel_ms", "adx_last_score_kernel_ms",
    "adx_last_kernel_split_ms",
    "adx_last_kernel_names",
    "adx_walkers_download", "adx_score_batch", "adx_variant_desc", "adx_walkers_export",
    "adx_walkers_import", "adx_walkers_import_after", "adx_walkers_export_on", "adx_set_temperature", "adx_bppm_batch",
    "adx_walkers_rescore",
    "adx_fold_mfe_structure", "adx_mfe_structure_batch", "adx_walkers_mfe_structures",
    "adx_fold_subopt_structures", "adx_subopt_structures_batch", "adx_walkers_subopt_structures", "adx_last_subopt_ms",
    "adx_fold_sample_structures", "adx_sample_structures_batch", "adx_walkers_sample_structures",
    "adx_last_sample_ms",
    "adx_fold_eval_structures", "adx_eval_structures_batch", "adx_walkers_eval_structures", "adx_last_eval_ms",
    "adx_fold_unpaired_probs", "adx_unpaired_probs_batch", "adx_walkers_unpaired_probs", "adx_last_unpaired_ms",
    "adx_fold_ensemble_structures", "adx_ensemble_structures_batch", "adx_walkers_ensemble_structures",
    "adx_last_ensemble_ms",
    "adx_pick_scores", "adx_record_begin", "adx_record_end", "adx_record_picks", "adx_last_pick_ms",
    "adx_autocorr_codes", "adx_record_autocorr", "adx_last_autocorr_ms", "adx_autocorr_time",
    "adx_select_designs", "adx_record_designs", "adx_last_design_ms",
]

_lib = None


def lib():
    """Load the HIP engine; raise if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("addapt_amd native engine not built: %s missing "
                              "(run __graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        # a stale build (or an ADX_LIB ablation library) of another ABI would
        # silently swap enum meanings (v4: motif AUTO = 0, ADD = 1, REPLACE = 2)
        got = L.adx_abi_version()
        if got != ABI_VERSION:
            raise ImportError("%s has ABI version %d, this binding needs %d (rebuild: "
                              "__graft_entry__.build())" % (LIB_PATH, got, ABI_VERSION))
        L.adx_last_error.restype = C.c_char_p
        L.adx_kT.restype = C.c_double
        L.adx_params_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.adx_params_free.argtypes = [C.c_void_p]
        L.adx_eval_structure.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_double)]
        L.adx_fold_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.adx_fold_add_motif.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_double]
        L.adx_fold_add_constraint.argtypes = [C.c_void_p, C.c_char_p]
        L.adx_fold_pf.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.adx_fold_mfe.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.adx_fold_mfe_structure.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_float)]
        L.adx_mfe_structure_batch.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p,
                                              C.POINTER(C.c_float)]
        L.adx_walkers_mfe_structures.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_float)]
        subopt_out = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_char_p, C.POINTER(C.c_float),
                      C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.adx_fold_subopt_structures.argtypes = [C.c_void_p, C.c_double, C.c_int] + subopt_out
        L.adx_subopt_structures_batch.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_int] + subopt_out
        L.adx_walkers_subopt_structures.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int] + subopt_out
        L.adx_last_subopt_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.adx_fold_sample_structures.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_char_p, C.POINTER(C.c_float)]
        L.adx_sample_structures_batch.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_uint64,
                                                  C.c_char_p, C.POINTER(C.c_float)]
        L.adx_walkers_sample_structures.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_char_p,
                                                    C.POINTER(C.c_float)]
        L.adx_last_sample_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.adx_fold_eval_structures.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        L.adx_eval_structures_batch.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p,
                                                C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        L.adx_walkers_eval_structures.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        L.adx_last_eval_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        unpaired_out = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                        C.POINTER(C.c_float)]
        L.adx_fold_unpaired_probs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                              C.POINTER(C.c_float)]
        L.adx_unpaired_probs_batch.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int] + unpaired_out
        L.adx_walkers_unpaired_probs.argtypes = [C.c_void_p, C.c_int] + unpaired_out
        L.adx_last_unpaired_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.adx_fold_ensemble_structures.argtypes = [C.c_void_p, C.c_double, C.c_char_p, C.c_char_p,
                                                   C.POINTER(EnsembleStats)]
        L.adx_ensemble_structures_batch.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_double,
                                                    C.c_char_p, C.c_char_p, C.POINTER(EnsembleStats),
                                                    C.POINTER(C.c_double)]
        L.adx_walkers_ensemble_structures.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_char_p, C.c_char_p,
                                                      C.POINTER(EnsembleStats), C.POINTER(C.c_double)]
        L.adx_last_ensemble_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.adx_fold_bpp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.adx_fold_free.argtypes = [C.c_void_p]
        L.adx_ctx_create.argtypes = [C.POINTER(RunDesc), C.POINTER(C.c_void_p)]
        L.adx_ctx_destroy.argtypes = [C.c_void_p]
        L.adx_ctx_info.argtypes = [C.c_void_p, C.POINTER(Info)]
        L.adx_walkers_init.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_uint32)]
        L.adx_run_steps.argtypes = [C.c_void_p, C.c_int, C.POINTER(Trace)]
        L.adx_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.adx_last_score_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.adx_last_kernel_split_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.adx_last_kernel_names.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        L.adx_walkers_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.adx_walkers_import.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.adx_walkers_import_after.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.adx_walkers_export_on.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.adx_set_temperature.argtypes = [C.c_void_p, C.c_double]
        L.adx_walkers_download.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double),
                                           C.POINTER(C.c_int64)]
        L.adx_score_batch.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_float)]
        L.adx_walkers_rescore.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.adx_bppm_batch.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                     C.POINTER(C.c_double)]
        L.adx_variant_desc.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.adx_pick_scores.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int32)]
        L.adx_record_begin.argtypes = [C.c_void_p, C.c_int]
        L.adx_record_end.argtypes = [C.c_void_p]
        L.adx_record_picks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_double), C.c_char_p, C.POINTER(C.c_int64)]
        L.adx_last_pick_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.adx_autocorr_codes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.adx_record_autocorr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_ubyte),
                                          C.POINTER(C.c_int)]
        L.adx_last_autocorr_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.adx_autocorr_time.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int64, C.c_int64, C.c_double,
                                        C.POINTER(C.c_int)]
        L.adx_select_designs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_double), C.c_int, C.c_int,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.adx_record_designs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_char_p,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64)]
        L.adx_last_design_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib = L
    return _lib


def _check(status):
    if status != OK:
        raise AdxError(status, lib().adx_last_error().decode())


def _b(s):
    return s.encode() if isinstance(s, str) else s


# status bits of the eval-structures calls (include/addapt_gpu.h ADX_EVAL_*)
EVAL_MALFORMED, EVAL_HAIRPIN, EVAL_EXCLUDED, EVAL_BIGLOOP = 1, 2, 4, 8


def _eval_structures(n_seqs, n_per, L, structures, with_probs, call):
    """The three outputs of an eval-structures call as (n_seqs, n_per) arrays; probs None without with_probs."""
    flat = [_b(s) for s in structures]
    if any(len(s) != L for s in flat):
        raise ValueError("every structure must have the folded length %d" % L)
    buf = b"".join(flat)
    n = n_seqs * n_per
    e = np.zeros(n, np.float64)
    p = np.zeros(n, np.float64) if with_probs else None
    st = np.zeros(n, np.uint8)
    _check(call(buf, e.ctypes.data_as(C.POINTER(C.c_double)),
                p.ctypes.data_as(C.POINTER(C.c_double)) if with_probs else None,
                st.ctypes.data_as(C.POINTER(C.c_uint8))))
    shape = (n_seqs, n_per)
    return e.reshape(shape), p.reshape(shape) if with_probs else None, st.reshape(shape)


def _unpaired(W, L, max_len, regions, call):
    """(profile (W, max_len, L) or None, region probabilities (W, n_regions) or None, float32
    energies) of an unpaired-probs call; regions: (first, length) pairs, first 0-based."""
    reg = np.ascontiguousarray(regions if regions is not None else [], np.int32).reshape(-1, 2)
    R = len(reg)
    prof = np.zeros((W, max(max_len, 0), L), np.float64) if max_len != 0 else None
    rp = np.zeros((W, R), np.float64) if regions is not None else None
    e = np.zeros(max(W, 1), np.float32)
    dp = C.POINTER(C.c_double)
    _check(call(max_len, R, reg.ctypes.data_as(C.POINTER(C.c_int)) if R else None,
                prof.ctypes.data_as(dp) if prof is not None else None,
                rp.ctypes.data_as(dp) if rp is not None else None, e.ctypes.data_as(C.POINTER(C.c_float))))
    return prof, rp, e[:W]


def kT():
    return lib().adx_kT()


def theo_energy(kd_uM=0.32):
    """kT * ln(Kd / 1 M) -- the bonus scoring.cc:91-99 passes to vrna_sc_add_hi_motif."""
    return kT() * math.log(kd_uM / 1e6)


def pick_scores(scores, window, cap=None, device=0):
    """The peaks of trajectories given as a (steps, trajectories) float64 array
    (adx_pick_scores): a list per trajectory of its picked steps, ascending, or
    None for a trajectory with a non-finite score.  Each trajectory's threshold
    is its 75th percentile; picks are at least `window` steps apart.  cap: the
    per-trajectory capacity passed down (default: the least that always fits)."""
    sc = np.ascontiguousarray(scores, np.float64)
    if sc.ndim != 2:
        raise ValueError("pick_scores: scores must be (steps, trajectories)")
    S, W = sc.shape
    if cap is None:
        cap = -(-S // window) if window >= 1 else 1
    n = np.zeros(max(W, 1), np.int32)
    st = np.zeros(max(W * cap, 1), np.int32)
    _check(lib().adx_pick_scores(device, W, S, sc.ctypes.data_as(C.POINTER(C.c_double)), window, cap,
                                 n.ctypes.data_as(C.POINTER(C.c_int)), st.ctypes.data_as(C.POINTER(C.c_int32))))
    st = st[:W * cap].reshape(W, cap)
    return [None if n[w] < 0 else [int(x) for x in st[w, :n[w]]] for w in range(W)]


def autocorr_codes(codes, max_lag, device=0):
    """(pos_matches, traj_matches) of trajectories given as a (steps, trajectories,
    positions) uint8 array of base codes 1..4 (adx_autocorr_codes): for each lag
    k in 0..max_lag the number of steps i < steps - k with codes[i + k] == codes[i],
    as int64 arrays (positions, max_lag + 1) summed over the trajectories and
    (trajectories, max_lag + 1) summed over the positions.  Dividing by
    trajectories * (steps - k), or positions * (steps - k), gives the autocorrelation."""
    cd = np.ascontiguousarray(codes, np.uint8)
    if cd.ndim != 3:
        raise ValueError("autocorr_codes: codes must be (steps, trajectories, positions)")
    S, W, P = cd.shape
    pm = np.zeros((max(P, 1), max(max_lag, 0) + 1), np.int64)
    tm = np.zeros((max(W, 1), max(max_lag, 0) + 1), np.int64)
    _check(lib().adx_autocorr_codes(device, W, S, P, cd.ctypes.data_as(C.POINTER(C.c_uint8)), max_lag,
                                    pm.ctypes.data_as(C.POINTER(C.c_int64)), tm.ctypes.data_as(C.POINTER(C.c_int64))))
    return pm, tm


def autocorr_time(matches, n_series, kept_steps, baseline):
    """The correlation time of a pooled curve of match counts for the lags
    0..len(matches) - 1 (adx_autocorr_time; host arithmetic): the least lag
    k >= 1 at which matches[k] / (n_series * (kept_steps - k)) - baseline has
    fallen to (1 - baseline) / e; -1 if none has, 0 if baseline >= 1."""
    m = np.ascontiguousarray(matches, np.int64)
    tau = C.c_int()
    _check(lib().adx_autocorr_time(m.ctypes.data_as(C.POINTER(C.c_int64)), len(m) - 1, n_series, kept_steps,
                                   baseline, C.byref(tau)))
    return tau.value


def select_designs(seqs, scores, radius, max_designs=None, device=0, with_hist=True):
    """Distinct designs among scored sequences by greedy Hamming selection
    (adx_select_designs).  seqs: strings of one length over ACGU / acgu, or an
    (entries, length) array of such characters (uint8 or S1); scores: a float per
    entry.  Best score first (ties: the lower index; non-finite scores take no
    part), an entry leads a new design iff no earlier leader is within `radius`
    mutations of it, else it joins the lowest-numbered leader within `radius`; at
    most max_designs designs (default: as many as entries).  A dict: leaders
    (entry index per design) and sizes (entries covered), int32 of n_designs;
    member_of (entries,) int32, -1 for none; pair_hist (length + 1,) int64, the
    unordered pairs of finite-score entries per distance (None without with_hist)."""
    if isinstance(seqs, np.ndarray) and seqs.ndim == 2:
        ch = np.ascontiguousarray(seqs).view(np.uint8)
        M, N = ch.shape
        buf = ch.tobytes()
    else:
        seqs = [_b(s) for s in seqs]
        M, N = len(seqs), (len(seqs[0]) if seqs else 0)
        if any(len(s) != N for s in seqs):
            raise ValueError("select_designs: sequences of different lengths")
        buf = b"".join(seqs)
    sc = np.ascontiguousarray(scores, np.float64).reshape(-1)
    if len(sc) != M:
        raise ValueError("select_designs: %d scores for %d sequences" % (len(sc), M))
    if max_designs is None:
        max_designs = max(M, 1)
    K = max(max_designs, 1)
    n = C.c_int()
    lead, size = np.zeros(K, np.int32), np.zeros(K, np.int32)
    member = np.zeros(max(M, 1), np.int32)
    hist = np.zeros(max(N, 0) + 1, np.int64) if with_hist else None
    i32 = C.POINTER(C.c_int32)
    _check(lib().adx_select_designs(device, M, N, buf, sc.ctypes.data_as(C.POINTER(C.c_double)), radius, max_designs,
                                    C.byref(n), lead.ctypes.data_as(i32), size.ctypes.data_as(i32),
                                    member.ctypes.data_as(i32),
                                    hist.ctypes.data_as(C.POINTER(C.c_int64)) if with_hist else None))
    return dict(leaders=lead[:n.value].copy(), sizes=size[:n.value].copy(), member_of=member[:M], pair_hist=hist)


class Params:
    def __init__(self, path=DEFAULT_PARAMS):
        self.ptr = C.c_void_p()
        _check(lib().adx_params_load(_b(path), C.byref(self.ptr)))

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.adx_params_free(self.ptr)
            self.ptr = None

    def eval_structure(self, seq, structure):
        e = C.c_double()
        _check(lib().adx_eval_structure(self.ptr, _b(seq), _b(structure), C.byref(e)))
        return e.value


Subopt = collections.namedtuple("Subopt", "mfe n_pairs_within structures energies seeds pair_energy")


def _subopt(W, L, K, with_pair_energy, call, row=None):
    """One Subopt per sequence from a *_subopt_structures call: mfe (kcal/mol, +inf when the
    constraint admits nothing), the number of pairs within delta, the n_found structures,
    their float32 energies and 1-based seed pairs, and (on request) the (L, L) float32
    energies of the best structure through every pair (+inf: none).  row: bytes per
    structure in the call's buffer (the fold layer terminates each)."""
    row = row or L
    K = max(K, 0)
    nf, nw = np.zeros(W, np.int32), np.zeros(W, np.int32)
    mfe, e = np.zeros(W, np.float32), np.zeros(W * K, np.float32)
    seeds = np.zeros(W * K * 2, np.int32)
    pe = np.zeros(W * L * L if with_pair_energy else 0, np.float32)
    buf = C.create_string_buffer(W * K * row + 1)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    _check(call(nf.ctypes.data_as(ip), nw.ctypes.data_as(ip), mfe.ctypes.data_as(fp), buf, e.ctypes.data_as(fp),
                seeds.ctypes.data_as(ip), pe.ctypes.data_as(fp) if with_pair_energy else None))
    raw = buf.raw
    out = []
    for w in range(W):
        n = int(nf[w])
        sts = [raw[(w * K + k) * row:(w * K + k) * row + L].decode() for k in range(n)]
        out.append(Subopt(float(mfe[w]), int(nw[w]), sts, e[w * K:w * K + n].copy(),
                          [tuple(int(x) for x in seeds[2 * (w * K + k):2 * (w * K + k) + 2]) for k in range(n)],
                          pe[w * L * L:(w + 1) * L * L].reshape(L, L).copy() if with_pair_energy else None))
    return out


_params = None


def default_params():
    global _params
    if _params is None:
        _params = Params()
    return _params


class Fold:
    """Per-fold layer: the six ViennaRNA calls of scoring.cc, one-to-one."""

    def __init__(self, seq, with_bppm=False, params=None, device=0):
        self.params = params or default_params()
        self.N = len(seq)
        self.ptr = C.c_void_p()
        _check(lib().adx_fold_create(self.params.ptr, _b(seq), int(with_bppm), device,
                                     C.byref(self.ptr)))

    def add_motif(self, seq, fold, energy):
        _check(lib().adx_fold_add_motif(self.ptr, _b(seq), _b(fold), energy))

    def add_constraint(self, db):
        _check(lib().adx_fold_add_constraint(self.ptr, _b(db)))

    def pf(self):
        g = C.c_float()
        _check(lib().adx_fold_pf(self.ptr, C.byref(g)))
        return g.value

    def mfe(self):
        g = C.c_float()
        _check(lib().adx_fold_mfe(self.ptr, C.byref(g)))
        return g.value

    def mfe_structure(self):
        """(energy kcal/mol, dot-bracket) of one minimum-free-energy structure."""
        g = C.c_float()
        buf = C.create_string_buffer(self.N + 1)
        _check(lib().adx_fold_mfe_structure(self.ptr, buf, C.byref(g)))
        return g.value, buf.value.decode()

    def subopt_structures(self, delta=3.0, max_structs=32, with_pair_energy=False):
        """Zuker suboptimal structures (RNAsubopt --zuker): a Subopt of the structures
        within `delta` kcal/mol of the MFE, at most one per base pair and `max_structs`
        in all, motif and constraint honoured."""
        return _subopt(1, self.N, max_structs, with_pair_energy,
                       lambda *out: lib().adx_fold_subopt_structures(self.ptr, delta, max_structs, *out), self.N + 1)[0]

    def sample_structures(self, n, seed=0):
        """(ensemble energy kcal/mol, n dot-bracket strings drawn from the ensemble)."""
        g = C.c_float()
        buf = C.create_string_buffer(max(0, n) * self.N + 1)
        _check(lib().adx_fold_sample_structures(self.ptr, n, seed, buf, C.byref(g)))
        raw = buf.raw[:n * self.N].decode()
        return g.value, [raw[k * self.N:(k + 1) * self.N] for k in range(n)]

    def eval_structures(self, structures, convention="pf", with_probs=False):
        """(energies kcal/mol, probabilities or None, status bytes) of the given dot-bracket
        strings on this sequence, motif and constraint honoured: RNAeval on the GPU.
        convention "pf" (E = -kT ln of the ensemble's weight) or "mfe" (the MFE folds'
        integer arithmetic); with_probs ("pf" only): exp(-(E - G) / kT).  status 0 = a
        member of the ensemble, else EVAL_* bits."""
        n = len(structures)
        conv = {"pf": 0, "mfe": 1}[convention]
        e, p, st = _eval_structures(1, n, self.N, structures, with_probs,
                                    lambda s, en, pr, sb: lib().adx_fold_eval_structures(self.ptr, conv, n, s, en, pr, sb))
        return e[0], p[0] if with_probs else None, st[0]

    def unpaired_probs(self, max_len, pair_probs=False):
        """(P_u (max_len, N), pair probabilities (N, N) or None, ensemble energy kcal/mol), float64:
        RNAplfold -u's accessibility.  P_u[u - 1, i - 1] is the probability that the u bases
        from i (1-based) on are all unpaired, motif and constraint honoured; 0 past N - u and
        where the constraint forces a base of the window to pair, NaN everywhere when the
        constraint admits no structure."""
        ml = max(max_len, 0)
        p = np.zeros((ml, self.N), np.float64)
        pp = np.zeros((self.N, self.N), np.float64) if pair_probs else None
        g = C.c_float()
        dp = C.POINTER(C.c_double)
        _check(lib().adx_fold_unpaired_probs(self.ptr, max_len, p.ctypes.data_as(dp),
                                             pp.ctypes.data_as(dp) if pair_probs else None, C.byref(g)))
        return p, pp, g.value

    def ensemble_structures(self, gamma=1.0):
        """(centroid, MEA structure, EnsembleStats) of the ensemble: RNAfold -p --MEA's
        lines after the MFE one.  The statistics are NaN when the constraint admits nothing."""
        cen, mea = C.create_string_buffer(self.N + 1), C.create_string_buffer(self.N + 1)
        st = EnsembleStats()
        _check(lib().adx_fold_ensemble_structures(self.ptr, gamma, cen, mea, C.byref(st)))
        return cen.value.decode(), mea.value.decode(), st

    def bpp(self, i, j):
        p = C.c_double()
        _check(lib().adx_fold_bpp(self.ptr, i, j, C.byref(p)))
        return p.value

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.adx_fold_free(self.ptr)
            self.ptr = None


def make_thermostat(kind="fixed", t=1.0, t_hi=1.0, t_lo=0.0, cycle_len=1, rate=0.5, period=100,
                    t0=1.0):
    th = Thermostat()
    th.kind = {"fixed": THERMO_FIXED, "annealing": THERMO_ANNEAL, "auto": THERMO_AUTO}[kind]
    th.t_fixed, th.t_hi, th.t_lo, th.cycle_len = t, t_hi, t_lo, cycle_len
    th.target_rate, th.period, th.t_init = rate, period, t0
    return th


class Engine:
    """Batched Monte Carlo context (adx_ctx_*).

    terms: list of (condition 'apo'|'holo', target, favorable bool, weight); target is a
    macrostate index (MacrostateProbTerm) or ("pair", i, j) (base-pair probability term,
    0-based device positions)
    aptamer: None or (seq, fold, energy_kcal); contexts: list of (before, after).
    fold_mode: "pf" (ensembles, vrna_pf) or "mfe" (minimum free energies, ADX_FOLD_MFE).
    """

    def __init__(self, sequence, macrostates, terms, aptamer=None, thermostat=None, contexts=None,
                 motif_mode=MOTIF_AUTO, params=None, device=0, fold_mode="pf"):
        self.params = params or default_params()
        self.N = len(sequence)
        d = RunDesc()
        d.params = self.params.ptr
        d.sequence = _b(sequence)
        self._ms = (C.c_char_p * max(1, len(macrostates)))(*[_b(m) for m in macrostates])
        d.n_macrostates = len(macrostates)
        d.macrostates = self._ms
        self._terms = (Term * max(1, len(terms)))()
        for k, (cond, mi, fav, w) in enumerate(terms):
            c = HOLO if cond in ("holo", HOLO) else APO
            if isinstance(mi, tuple):
                self._terms[k] = Term(c, 0, int(bool(fav)), w, TERM_PAIR, mi[1], mi[2])
            else:
                self._terms[k] = Term(c, mi, int(bool(fav)), w, TERM_MACROSTATE, 0, 0)
        d.n_terms = len(terms)
        d.terms = self._terms
        if aptamer is not None:
            d.aptamer_seq, d.aptamer_fold, d.aptamer_energy_kcal = _b(aptamer[0]), _b(aptamer[1]), aptamer[2]
        d.motif_mode = motif_mode
        ctx = contexts or []
        self._ctx = (ContextDesc * max(1, len(ctx)))()
        for k, (b, a) in enumerate(ctx):
            self._ctx[k] = ContextDesc(_b(b), _b(a))
        d.n_contexts = len(ctx)
        d.contexts = self._ctx
        self._ctx_lens = [(len(b), len(a)) for b, a in ctx]
        d.thermostat = thermostat if thermostat is not None else make_thermostat()
        d.device = device
        d.fold_mode = {"pf": FOLD_PF, "mfe": FOLD_MFE}[fold_mode]
        self.fold_mode = fold_mode
        self._desc = d
        self.ptr = C.c_void_p()
        _check(lib().adx_ctx_create(C.byref(d), C.byref(self.ptr)))
        self.info = Info()
        _check(lib().adx_ctx_info(self.ptr, C.byref(self.info)))
        self.n_terms_total = len(terms) * max(1, len(ctx))
        self.W = 0
        self._rec_rows = None   # steps in the pick record (None: no record)

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.adx_ctx_destroy(self.ptr)
            self.ptr = None

    def variant(self, v):
        c, cond, m = C.c_int(), C.c_int(), C.c_int()
        _check(lib().adx_variant_desc(self.ptr, v, C.byref(c), C.byref(cond), C.byref(m)))
        return c.value, cond.value, m.value

    def score_batch(self, seqs):
        W = len(seqs)
        buf = b"".join(_b(s) for s in seqs)
        sc = np.zeros(W, np.float64)
        tv = np.zeros(W * max(1, self.n_terms_total), np.float64)
        dg = np.zeros(W * self.info.n_variants, np.float32)
        _check(lib().adx_score_batch(self.ptr, W, buf, sc.ctypes.data_as(C.POINTER(C.c_double)),
                                     tv.ctypes.data_as(C.POINTER(C.c_double)),
                                     dg.ctypes.data_as(C.POINTER(C.c_float))))
        return sc, tv.reshape(W, -1)[:, :self.n_terms_total], dg.reshape(W, -1)

    def bppm_batch(self, seqs, condition="apo", context=0):
        """(W, L, L) base-pair probability matrices of the (context, condition) fold."""
        W = len(seqs)
        buf = b"".join(_b(s) for s in seqs)
        c = HOLO if condition in ("holo", HOLO) else APO
        L = self.N
        if self._ctx_lens:
            L += sum(self._ctx_lens[context])
        out = np.zeros(W * L * L, np.float64)
        _check(lib().adx_bppm_batch(self.ptr, W, buf, c, context,
                                    out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(W, L, L)

    def _variant_length(self, v):
        """Folded (context-padded) length of variant v (a bad index is the engine's to report)."""
        if not 0 <= v < self.info.n_variants:
            return self.N
        ctx = self.variant(v)[0]
        return self.N + (sum(self._ctx_lens[ctx]) if ctx >= 0 else 0)

    def _structures(self, W, L, call):
        buf = C.create_string_buffer(W * L + 1)
        e = np.zeros(W, np.float32)
        _check(call(buf, e.ctypes.data_as(C.POINTER(C.c_float))))
        raw = buf.raw[:W * L].decode()
        return [raw[w * L:(w + 1) * L] for w in range(W)], e

    def mfe_structures(self, seqs, variant):
        """(dot-bracket strings, float32 energies) of the MFE structures of `seqs`
        in fold variant `variant` (fold_mode="mfe" engines)."""
        W = len(seqs)
        seqbuf = b"".join(_b(s) for s in seqs)
        return self._structures(W, self._variant_length(variant), lambda st, e: lib().adx_mfe_structure_batch(
            self.ptr, W, seqbuf, variant, st, e))

    def walker_structures(self, variant):
        """The same for the walkers' current sequences."""
        return self._structures(self.W, self._variant_length(variant), lambda st, e: lib().adx_walkers_mfe_structures(
            self.ptr, variant, st, e))

    def subopt_structures(self, seqs, variant, delta=3.0, max_structs=32, with_pair_energy=False):
        """One Subopt per sequence: the Zuker suboptimal structures of `seqs` in fold
        variant `variant` within `delta` kcal/mol of each MFE (fold_mode="mfe" engines)."""
        W = len(seqs)
        seqbuf = b"".join(_b(s) for s in seqs)
        return _subopt(W, self._variant_length(variant), max_structs, with_pair_energy,
                       lambda *out: lib().adx_subopt_structures_batch(self.ptr, W, seqbuf, variant, delta, max_structs,
                                                                      *out))

    def walker_subopt_structures(self, variant, delta=3.0, max_structs=32, with_pair_energy=False):
        """The same for the walkers' current sequences."""
        return _subopt(max(self.W, 0), self._variant_length(variant), max_structs, with_pair_energy,
                       lambda *out: lib().adx_walkers_subopt_structures(self.ptr, variant, delta, max_structs, *out))

    def last_subopt_ms(self):
        """(fill ms, selection ms) of the last subopt_structures / walker_subopt_structures call, from HIP events."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_subopt_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _samples(self, W, L, n, call):
        buf = C.create_string_buffer(W * max(0, n) * L + 1)
        e = np.zeros(W, np.float32)
        _check(call(buf, e.ctypes.data_as(C.POINTER(C.c_float))))
        raw = buf.raw[:W * n * L].decode()
        return [[raw[(w * n + k) * L:(w * n + k + 1) * L] for k in range(n)] for w in range(W)], e

    def sample_structures(self, seqs, variant, n_samples, seed=0):
        """(W lists of n_samples dot-bracket strings drawn from the ensembles of
        `seqs` in fold variant `variant`, float32 ensemble energies); fold_mode="pf"
        engines.  Sample k of sequence w depends on (seed, w, k) alone."""
        W = len(seqs)
        seqbuf = b"".join(_b(s) for s in seqs)
        return self._samples(W, self._variant_length(variant), n_samples,
                             lambda st, e: lib().adx_sample_structures_batch(self.ptr, W, seqbuf, variant, n_samples,
                                                                             seed, st, e))

    def walker_samples(self, variant, n_samples, seed=0):
        """The same for the walkers' current sequences."""
        return self._samples(self.W, self._variant_length(variant), n_samples,
                             lambda st, e: lib().adx_walkers_sample_structures(self.ptr, variant, n_samples, seed,
                                                                               st, e))

    def last_sample_ms(self):
        """(fill ms, sampling ms) of the last sample_structures / walker_samples call, from HIP events."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_sample_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def eval_structures(self, seqs, variant, structures, with_probs=False):
        """(energies, probabilities or None, status bytes), each (W, n), of structures[w][k] on
        seqs[w] in fold variant `variant`, in the convention of the engine's fold mode
        (with_probs: fold_mode="pf" engines).  structures: W lists of n dot-bracket strings
        of the variant's folded length, as sample_structures returns them."""
        W, n = len(seqs), len(structures[0]) if structures else 0
        if len(structures) != W or any(len(row) != n for row in structures):
            raise ValueError("structures must be one list of equal length per sequence")
        seqbuf = b"".join(_b(s) for s in seqs)
        return _eval_structures(W, n, self._variant_length(variant), [s for row in structures for s in row], with_probs,
                                lambda s, e, p, st: lib().adx_eval_structures_batch(self.ptr, W, seqbuf, variant, n, s,
                                                                                    e, p, st))

    def walker_eval_structures(self, variant, structures, with_probs=False):
        """The same (W, n) arrays for one list of n target structures on every walker's
        current sequence, read on the device."""
        n = len(structures)
        return _eval_structures(max(self.W, 0), n, self._variant_length(variant), structures, with_probs,
                                lambda s, e, p, st: lib().adx_walkers_eval_structures(self.ptr, variant, n, s, e, p, st))

    def last_eval_ms(self):
        """(fill ms, eval ms) of the last eval_structures / walker_eval_structures call, from HIP events."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_eval_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def unpaired_probs(self, seqs, variant, max_len=0, regions=None):
        """(profile (W, max_len, L) or None when max_len is 0, region probabilities (W, n) or
        None, float32 ensemble energies) of `seqs` in fold variant `variant` (fold_mode="pf"
        engines): the probability that a window is all unpaired, float64.  profile[w, u - 1, i]
        is the window of u bases from 0-based i on; regions are (first, length) pairs, first
        0-based, both in the variant's folded (context-padded) coordinates."""
        W = len(seqs)
        seqbuf = b"".join(_b(s) for s in seqs)
        return _unpaired(W, self._variant_length(variant), max_len, regions,
                         lambda *a: lib().adx_unpaired_probs_batch(self.ptr, W, seqbuf, variant, *a))

    def walker_unpaired_probs(self, variant, max_len=0, regions=None):
        """The same for the walkers' current sequences, read on the device."""
        return _unpaired(max(self.W, 0), self._variant_length(variant), max_len, regions,
                         lambda *a: lib().adx_walkers_unpaired_probs(self.ptr, variant, *a))

    def last_unpaired_ms(self):
        """(fill ms, outside ms) of the last unpaired_probs / walker_unpaired_probs call, from HIP events."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_unpaired_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _ensemble(self, W, condition, context, with_probs, call):
        L = self.N + (sum(self._ctx_lens[context]) if self._ctx_lens and 0 <= context < len(self._ctx_lens) else 0)
        cen, mea = C.create_string_buffer(W * L + 1), C.create_string_buffer(W * L + 1)
        st = np.zeros((W, 3), np.float64)
        P = np.zeros(W * L * L if with_probs else 0, np.float64)
        c = HOLO if condition in ("holo", HOLO) else APO
        _check(call(c, cen, mea, st.ctypes.data_as(C.POINTER(EnsembleStats)),
                    P.ctypes.data_as(C.POINTER(C.c_double)) if with_probs else None))
        cen, mea = cen.raw[:W * L].decode(), mea.raw[:W * L].decode()
        out = ([cen[w * L:(w + 1) * L] for w in range(W)], [mea[w * L:(w + 1) * L] for w in range(W)], st)
        return out + (P.reshape(W, L, L),) if with_probs else out

    def ensemble_structures(self, seqs, condition="apo", context=0, gamma=1.0, with_probs=False):
        """(centroids, MEA structures, stats) of `seqs` in the unconstrained
        (context, condition) fold, as bppm_batch addresses it: W dot-bracket strings
        each and a (W, 3) float64 array of (mea, centroid_dist, diversity).
        with_probs appends the (W, L, L) matrices the structures were computed from.
        fold_mode="pf" engines."""
        W = len(seqs)
        seqbuf = b"".join(_b(s) for s in seqs)
        return self._ensemble(W, condition, context, with_probs,
                              lambda c, cen, mea, st, P: lib().adx_ensemble_structures_batch(
                                  self.ptr, W, seqbuf, c, context, gamma, cen, mea, st, P))

    def walker_ensemble_structures(self, condition="apo", context=0, gamma=1.0, with_probs=False):
        """The same for the walkers' current sequences."""
        return self._ensemble(self.W, condition, context, with_probs,
                              lambda c, cen, mea, st, P: lib().adx_walkers_ensemble_structures(
                                  self.ptr, c, context, gamma, cen, mea, st, P))

    def last_ensemble_ms(self):
        """(outside-pass ms, structure-kernel ms) of the last ensemble_structures /
        walker_ensemble_structures call, from HIP events."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_ensemble_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def walkers_init(self, seeds, seqs=None):
        W = len(seeds)
        sd = (C.c_uint32 * W)(*seeds)
        buf = b"".join(_b(s) for s in seqs) if seqs is not None else None
        _check(lib().adx_walkers_init(self.ptr, W, buf, sd))
        self.W = W

    def run_steps(self, steps, trace=False):
        tr = None
        out = None
        if trace:
            R = steps * self.W
            out = dict(position=np.zeros(R, np.int32), outcome=np.zeros(R, np.int32),
                       temperature=np.zeros(R), proposed_score=np.zeros(R), current_score=np.zeros(R),
                       random_threshold=np.zeros(R), term_values=np.zeros(R * max(1, self.n_terms_total)))
            base = C.create_string_buffer(R + 1)
            tr = Trace(out["position"].ctypes.data_as(C.POINTER(C.c_int32)), C.cast(base, C.c_char_p),
                       out["outcome"].ctypes.data_as(C.POINTER(C.c_int32)),
                       out["temperature"].ctypes.data_as(C.POINTER(C.c_double)),
                       out["proposed_score"].ctypes.data_as(C.POINTER(C.c_double)),
                       out["current_score"].ctypes.data_as(C.POINTER(C.c_double)),
                       out["random_threshold"].ctypes.data_as(C.POINTER(C.c_double)),
                       out["term_values"].ctypes.data_as(C.POINTER(C.c_double)))
        _check(lib().adx_run_steps(self.ptr, steps, C.byref(tr) if tr is not None else None))
        if self._rec_rows is not None:
            self._rec_rows += max(0, steps)
        if trace:
            out["base"] = base.raw[:steps * self.W].decode()
            for k in ("position", "outcome", "temperature", "proposed_score", "current_score",
                      "random_threshold"):
                out[k] = out[k].reshape(steps, self.W)
            out["term_values"] = out["term_values"].reshape(steps, self.W, -1)[:, :, :self.n_terms_total]
        return out

    def record(self, max_steps):
        """Start the pick record (adx_record_begin): the following run_steps calls,
        up to max_steps steps in all, keep each step's score and move on the device."""
        _check(lib().adx_record_begin(self.ptr, max_steps))
        self._rec_rows = 0

    def record_end(self):
        _check(lib().adx_record_end(self.ptr))
        self._rec_rows = None

    def picks(self, window, cap=None):
        """(picks, base_counts) of the steps recorded so far (adx_record_picks):
        per walker a list of (step, score, sequence) in ascending step order (None
        for a walker whose recorded scores are not all finite), step being the
        engine's global 0-based step index; base_counts is the (N, 4) int64
        histogram of A, C, G, U over all walkers' picked sequences."""
        W, N = self.W, self.N
        if cap is None:
            cap = max(1, -(-(self._rec_rows or 0) // window)) if window >= 1 else 1
        n = np.zeros(max(W, 1), np.int32)
        st = np.zeros(max(W * cap, 1), np.int64)
        sc = np.zeros(max(W * cap, 1), np.float64)
        buf = C.create_string_buffer(W * cap * N + 1)
        cnt = np.zeros((N, 4), np.int64)
        _check(lib().adx_record_picks(self.ptr, window, cap, n.ctypes.data_as(C.POINTER(C.c_int)),
                                      st.ctypes.data_as(C.POINTER(C.c_int64)), sc.ctypes.data_as(C.POINTER(C.c_double)),
                                      buf, cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        raw = buf.raw
        out = []
        for w in range(W):
            if n[w] < 0:
                out.append(None)
                continue
            out.append([(int(st[w * cap + k]), float(sc[w * cap + k]),
                         raw[(w * cap + k) * N:(w * cap + k + 1) * N].decode()) for k in range(n[w])])
        return out, cnt

    def autocorr(self, max_lag, discard=0):
        """The per-position autocorrelation of the steps recorded so far, the first
        `discard` dropped (adx_record_autocorr).  A dict: pos_matches (N, max_lag + 1)
        and walker_matches (W, max_lag + 1), int64 match counts summed over the
        walkers and over the changeable positions; base_counts (N, 4) and
        outcome_counts (W, 4) over the kept steps; changeable (N,) bool; kept_steps;
        baseline, the chance that two independent draws at a changeable position
        match; pooled, the autocorrelation over all walkers and changeable positions
        per lag; tau, its correlation time (adx_autocorr_time), in steps."""
        W, N, L = self.W, self.N, max(max_lag, 0) + 1
        pm, wm = np.zeros((N, L), np.int64), np.zeros((max(W, 1), L), np.int64)
        bc, oc = np.zeros((N, 4), np.int64), np.zeros((max(W, 1), 4), np.int64)
        ch = np.zeros(N, np.uint8)
        nch = C.c_int()
        i64 = C.POINTER(C.c_int64)
        _check(lib().adx_record_autocorr(self.ptr, max_lag, discard, pm.ctypes.data_as(i64), wm.ctypes.data_as(i64),
                                         bc.ctypes.data_as(i64), oc.ctypes.data_as(i64),
                                         ch.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(nch)))
        kept = (self._rec_rows or 0) - discard
        ch = ch.astype(bool)
        pooled_m = pm[ch].sum(axis=0)
        if nch.value > 0:
            f = bc[ch] / float(W * kept)
            baseline = float((f * f).sum(axis=1).mean())
            tau = autocorr_time(pooled_m, W * nch.value, kept, baseline)
            pooled = pooled_m / (float(W * nch.value) * (kept - np.arange(L)))
        else:   # nothing can change
            baseline, tau, pooled = 1.0, 0, np.ones(L)
        return dict(pos_matches=pm, walker_matches=wm[:W], base_counts=bc, outcome_counts=oc[:W], changeable=ch,
                    kept_steps=kept, baseline=baseline, pooled=pooled, tau=tau)

    def designs(self, window, radius, max_designs=100):
        """(designs, pair_hist, n_picks): the distinct designs among the picks of the
        steps recorded so far (adx_record_designs).  The entries are what
        picks(window) returns, walker-major; best score first, a pick leads a new
        design iff no earlier leader is within `radius` mutations of it.  Each design
        is (walker, step, score, sequence, size, n_walkers) of its leader, size the
        picks it covers and n_walkers the distinct walkers among them; pair_hist is
        the (N + 1,) int64 count of pick pairs per distance, n_picks the entries."""
        N, K = self.N, max(max_designs, 1)
        n, total = C.c_int(), C.c_int64()
        wk, sz, nw = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
        st, sc = np.zeros(K, np.int64), np.zeros(K, np.float64)
        buf = C.create_string_buffer(K * N + 1)
        hist = np.zeros(N + 1, np.int64)
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        _check(lib().adx_record_designs(self.ptr, window, radius, max_designs, C.byref(n), wk.ctypes.data_as(i32),
                                        st.ctypes.data_as(i64), sc.ctypes.data_as(C.POINTER(C.c_double)), buf,
                                        sz.ctypes.data_as(i32), nw.ctypes.data_as(i32), C.byref(total),
                                        hist.ctypes.data_as(i64)))
        raw = buf.raw
        out = [(int(wk[d]), int(st[d]), float(sc[d]), raw[d * N:(d + 1) * N].decode(), int(sz[d]), int(nw[d]))
               for d in range(n.value)]
        return out, hist, total.value

    def last_design_ms(self):
        """(selection ms, all-pairs histogram ms) of the last designs() call, from HIP events."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_design_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_autocorr_ms(self):
        """(plane packing ms, lag kernel ms) of the last autocorr() call, from HIP events."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_autocorr_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_pick_ms(self):
        """(picking kernels ms, replay kernel ms) of the last picks() call, from HIP events."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_pick_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_kernel_ms(self):
        ms = C.c_double()
        _check(lib().adx_last_kernel_ms(self.ptr, C.byref(ms)))
        return ms.value

    def export_walkers(self, dev_seqs_ptr, dev_scores_ptr, on_stream=None):
        """Device-to-device copy of the walkers' sequence codes (W*N uint8) and
        scores (W float64) into caller-owned device buffers (raw pointers).
        `on_stream` (a raw HIP stream handle, e.g.
        torch.cuda.current_stream().cuda_stream -- 0 is the null stream) orders
        the copy between that stream's earlier and later work without a host
        synchronisation; None: synchronous."""
        if on_stream is None:
            _check(lib().adx_walkers_export(self.ptr, C.c_void_p(dev_seqs_ptr), C.c_void_p(dev_scores_ptr)))
        else:
            _check(lib().adx_walkers_export_on(self.ptr, C.c_void_p(dev_seqs_ptr), C.c_void_p(dev_scores_ptr),
                                               C.c_void_p(int(on_stream))))

    def import_walkers(self, dev_seqs_ptr, dev_scores_ptr, after_stream=None):
        """Copy configurations back in; `after_stream` (a raw HIP stream handle;
        0 is the null stream, not "none") orders the copy after the work queued
        there, and that stream's later work after the copy, without a host
        synchronisation; None: the synchronous import."""
        if after_stream is None:
            _check(lib().adx_walkers_import(self.ptr, C.c_void_p(dev_seqs_ptr), C.c_void_p(dev_scores_ptr)))
        else:
            _check(lib().adx_walkers_import_after(self.ptr, C.c_void_p(dev_seqs_ptr),
                                                  C.c_void_p(dev_scores_ptr), C.c_void_p(int(after_stream))))

    def set_temperature(self, t):
        _check(lib().adx_set_temperature(self.ptr, float(t)))

    def last_score_kernel_ms(self):
        """(average score-kernel launch ms, launches) of the last run_steps."""
        ms, n = C.c_double(), C.c_int()
        _check(lib().adx_last_score_kernel_ms(self.ptr, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_kernel_split_ms(self):
        """(average inside-fold ms, average outside-pass ms) per step of the last run_steps."""
        a, b = C.c_double(), C.c_double()
        _check(lib().adx_last_kernel_split_ms(self.ptr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_kernel_names(self):
        """(fold kernel(s), outside pass or "") the last run_steps launched."""
        a, b = C.create_string_buffer(256), C.create_string_buffer(256)
        _check(lib().adx_last_kernel_names(self.ptr, a, 256, b, 256))
        return a.value.decode(), b.value.decode()

    def rescore(self):
        """(scores, term values) of every walker's current configuration folded
        from scratch by the MC step's own kernels (adx_walkers_rescore); the
        stored scores are not touched."""
        W = self.W
        sc = np.zeros(W, np.float64)
        tv = np.zeros(W * max(1, self.n_terms_total), np.float64)
        _check(lib().adx_walkers_rescore(self.ptr, sc.ctypes.data_as(C.POINTER(C.c_double)),
                                         tv.ctypes.data_as(C.POINTER(C.c_double))))
        return sc, tv.reshape(W, -1)[:, :self.n_terms_total]

    def download(self):
        W = self.W
        buf = C.create_string_buffer(W * self.N + 1)
        sc = np.zeros(W, np.float64)
        cnt = np.zeros(W * 4, np.int64)
        _check(lib().adx_walkers_download(self.ptr, buf, sc.ctypes.data_as(C.POINTER(C.c_double)),
                                          cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        raw = buf.raw[:W * self.N].decode()
        seqs = [raw[w * self.N:(w + 1) * self.N] for w in range(W)]
        return seqs, sc, cnt.reshape(W, 4)
