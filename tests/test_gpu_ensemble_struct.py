"""Centroid and MEA structures from pair probabilities on the GPU
(ensemble_struct.hip) through the per-fold call, the batched context call and
the current walkers.

Every returned (centroid, mea, stats) is checked against ensemble_check.py's
restatement of the definitions ON THE MATRIX THE SAME CALL USED (read back
through adx_fold_bpp, or returned with with_probs): the comparisons with 1/2
and 0 are then exact, and the values differ only by summation order, within
    TOL = 8 L^2 max(1, 2 gamma) 2^-53
(each value is a sum of at most L terms of size at most max(1, 2 gamma), the
terms' own error is at most L ulps).  Structures are compared through their
expected accuracy, not character by character: ties may fall differently.  The
matrices themselves are held to the oracle's within the project's 2e-4.
"""
import ctypes as C
import math
import random

import numpy as np
import pytest

from addapt_amd import workloads
from ensemble_check import Mea, centroid, centroid_dist, diversity, expected_accuracy, pairs_of, tol
from structure_check import cons, rand_seq
from test_oracle_enum import SEQS

pytestmark = pytest.mark.gpu

BPP_TOL = 2e-4
APT = workloads.THEO_SEQ
GAMMAS = (0.5, 1.0, 4.0)


def check_structures(cen, mea, stats, P, gamma):
    """The structure check of one sequence; P: (L, L) array from the same call."""
    L = len(P)
    P = np.asarray(P).tolist()
    t = tol(L, gamma)
    assert all(P[i][i] == 0.0 for i in range(L)) and all(P[i][j] == P[j][i] for i in range(L) for j in range(i))
    cp, mp = pairs_of(cen), pairs_of(mea)
    assert len(cen) == L and len(mea) == L and cp is not None and mp is not None, (cen, mea)
    assert all(P[i][j] > 0.0 for i, j in mp)
    assert cp == [(i, j) for i in range(L) for j in range(i + 1, L) if P[i][j] > 0.5]
    assert cen == centroid(P)[1]
    T = Mea(P, gamma)
    ea = expected_accuracy(mp, P, gamma)
    print("L %d gamma %g: mea %.17g ref %.17g EA %.17g dist %.17g ref %.17g div %.17g ref %.17g tol %.3g" % (
        L, gamma, stats[0], T.mea, ea, stats[1], centroid_dist(P, cp), stats[2], diversity(P), t))
    assert abs(ea - T.mea) <= t and abs(stats[0] - T.mea) <= t
    assert abs(stats[1] - centroid_dist(P, cp)) <= t
    assert abs(stats[2] - diversity(P)) <= t


# ------------------------------------------------------------------ 1. the per-fold call
def _fold(native, seq, cst=None, motif=False):
    f = native.Fold(seq)
    if motif:
        f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    if cst:
        f.add_constraint(cst)
    return f


def _fold_matrix(f):
    """The compound's probabilities, pair by pair through adx_fold_bpp."""
    P = np.zeros((f.N, f.N))
    for i in range(f.N):
        for j in range(i + 1, f.N):
            P[i, j] = P[j, i] = f.bpp(i + 1, j + 1)
    return P


def _fold_cases():
    rng = random.Random(53)
    out = [(s, None, False) for s in ("G", "GCGC", "GAAAC", "GGAAAACC")]
    out += [(s, None, False) for s in SEQS]
    out += [(s, cons(rng, s), False) for s in SEQS[:4]]
    for n in (64, 65, 100):
        s = rand_seq(rng, n)
        out += [(s, None, False), (s, cons(rng, s), False)]
    withm = rand_seq(rng, 12) + APT + rand_seq(rng, 17)
    out += [(withm, None, True), (withm, cons(rng, withm[:12]) + "." * (len(withm) - 12), True)]
    return out


@pytest.mark.parametrize("seq,cst,motif", _fold_cases())
def test_fold_ensemble_structures(native, seq, cst, motif):
    for gamma in GAMMAS:
        f = _fold(native, seq, cst, motif)
        cen, mea, st = f.ensemble_structures(gamma)
        check_structures(cen, mea, (st.mea, st.centroid_dist, st.diversity), _fold_matrix(f), gamma)


def test_fold_by_product_is_adx_fold_bpp(native, oracle):
    """The probabilities the call leaves behind are the ones a fresh compound computes, and the oracle's."""
    rng = random.Random(5)
    seq = rand_seq(rng, 40)
    a, b = _fold(native, seq), _fold(native, seq)
    a.ensemble_structures()
    Pa, Pb = _fold_matrix(a), _fold_matrix(b)
    assert Pa.tobytes() == Pb.tobytes()
    assert np.abs(Pa - oracle.bppm(seq, None, None)[1]).max() <= BPP_TOL


def test_fold_empty_ensemble(native):
    f = _fold(native, "AAAAAAAAAA", "(........)")
    cen, mea, st = f.ensemble_structures()
    assert cen == mea == "." * 10
    assert math.isnan(st.mea) and math.isnan(st.centroid_dist) and math.isnan(st.diversity)
    assert f.bpp(1, 10) == 0.0


# ------------------------------------------------------------------ 2. the batch call
def _engine(native, tmpl, macro, terms, thermostat=None, contexts=None, fold_mode="pf"):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    return native.Engine(tmpl, macro, terms, aptamer=apt, contexts=contexts, fold_mode=fold_mode,
                         thermostat=thermostat or native.make_thermostat("fixed", t=1.0))


_ORACLE_P = {}


def _oracle_matrix(oracle, seq, holo):
    """oracle.bppm, computed once per (sequence, condition) and left unchanged."""
    if (seq, holo) not in _ORACLE_P:
        m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus()) if holo else None
        _ORACLE_P[seq, holo] = oracle.bppm(seq, None, m)[1]
    return _ORACLE_P[seq, holo]


def _check_batch(native, oracle, N, condition, gamma, contexts=None, context=0):
    tmpl, active = workloads.synthetic(N)
    eng = _engine(native, tmpl, [active], workloads.default_objective(), contexts=contexts)
    seqs = workloads.walker_sequences(tmpl, [active], 7)
    cen, mea, st, P = eng.ensemble_structures(seqs, condition, context, gamma, with_probs=True)
    b, a = contexts[context] if contexts else ("", "")
    assert P.shape == (7, N + len(b) + len(a), N + len(b) + len(a)) and st.shape == (7, 3)
    for w in range(7):
        full = (b + seqs[w] + a).upper()
        assert np.abs(P[w] - _oracle_matrix(oracle, full, condition == "holo")).max() <= BPP_TOL, (N, w)
        check_structures(cen[w], mea[w], st[w], P[w], gamma)
    assert any("(" in s for s in cen) and any("(" in s for s in mea)
    # the same call without the matrices, and the matrices alone
    cen2, mea2, st2 = eng.ensemble_structures(seqs, condition, context, gamma)
    assert (cen2, mea2) == (cen, mea) and st2.tobytes() == st.tobytes()
    assert eng.bppm_batch(seqs, condition, context).tobytes() == P.tobytes()


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("condition", ["apo", "holo"])
@pytest.mark.parametrize("N", [60, 100, 150])   # 150: the outside pass's global-scratch path
def test_batch_ensemble_structures(native, oracle, N, condition, gamma):
    _check_batch(native, oracle, N, condition, gamma)


def test_batch_contexts(native, oracle):
    """A context-padded fold: L = N + 7 and N + 4."""
    ctx = [("GGAC", "UUA"), ("", "CCCA")]
    _check_batch(native, oracle, 60, "holo", 1.0, contexts=ctx, context=0)
    _check_batch(native, oracle, 60, "apo", 1.0, contexts=ctx, context=1)


# ------------------------------------------------------------------ 3. a stable hairpin
def test_stable_hairpin_centroid_mea_mfe_agree(native, oracle):
    """GGGGCGCGAAAGCGCCCC: by oracle.bppm every pair of its MFE structure has
    p >= 0.976 and no other pair has p >= 1.1e-4, so the matrix's 2e-4 bound
    cannot flip a comparison with 1/2 or the MEA's choice at gamma = 1."""
    seq = "GGGGCGCGAAAGCGCCCC"
    _, P = oracle.bppm(seq, None, None)
    _, ref = oracle.mfe(seq)
    pairs = set(pairs_of(ref))
    assert ref == "(((((((....)))))))"
    assert min(P[i, j] for i, j in pairs) >= 0.9
    assert max(P[i, j] for i in range(18) for j in range(i + 1, 18) if (i, j) not in pairs) < 0.1
    f = _fold(native, seq)
    cen, mea, st = f.ensemble_structures(1.0)
    assert cen == mea == f.mfe_structure()[1] == ref
    assert st.centroid_dist < 0.5 and st.diversity < 1.0


# ------------------------------------------------------------------ 4. chunks, determinism
def test_launch_chunks_do_not_show(native):
    """800 sequences of 150 nt: each takes a 150 x 150 matrix and two triangular
    tables of doubles, 361 200 B, so 743 fit the 256 MiB bound of one launch and
    the call is split; its first 70 rows equal a 70-sequence call, which is one launch."""
    tmpl, active = workloads.synthetic(150)
    eng = _engine(native, tmpl, [active], workloads.default_objective())
    seqs = workloads.walker_sequences(tmpl, [active], 800)
    each = (150 * 150 + 2 * (150 * 151 // 2)) * 8
    assert 800 * each > 256 << 20 > 70 * each
    cen, mea, st = eng.ensemble_structures(seqs)
    cen70, mea70, st70 = eng.ensemble_structures(seqs[:70])
    assert cen[:70] == cen70 and mea[:70] == mea70 and st[:70].tobytes() == st70.tobytes()
    cl, ml, sl = eng.ensemble_structures(seqs[799:])   # the second launch's rows are filled too
    assert (cen[799], mea[799]) == (cl[0], ml[0]) and st[799].tobytes() == sl[0].tobytes()
    assert "(" in mea[799] and np.isfinite(st).all()


def test_deterministic(native):
    tmpl, active = workloads.synthetic(100)
    eng = _engine(native, tmpl, [active], workloads.default_objective())
    seqs = workloads.walker_sequences(tmpl, [active], 9)
    a = eng.ensemble_structures(seqs, "holo", 0, 1.0, with_probs=True)
    b = eng.ensemble_structures(seqs, "holo", 0, 1.0, with_probs=True)
    assert a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    f = _fold(native, seqs[0].upper())
    x, y = f.ensemble_structures(), f.ensemble_structures()
    assert x[:2] == y[:2] and bytes(x[2]) == bytes(y[2])
    bm, sm = eng.last_ensemble_ms()
    assert bm > 0.0 and sm > 0.0


# ------------------------------------------------------------------ 5. current walkers
def test_walkers_and_untouched_state(native):
    tmpl, active = workloads.synthetic(60)
    terms = workloads.default_objective()
    W = 70
    seqs = workloads.walker_sequences(tmpl, [active], W)

    def engine():
        th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
        eng = _engine(native, tmpl, [active], terms, thermostat=th)
        eng.walkers_init(list(range(W)), seqs)
        eng.run_steps(5)
        return eng

    eng, plain = engine(), engine()
    cur = eng.download()[0]
    assert cur != seqs   # the walkers moved
    for cond in ("apo", "holo"):
        a = eng.walker_ensemble_structures(cond, 0, 1.0, with_probs=True)
        b = eng.ensemble_structures(cur, cond, 0, 1.0, with_probs=True)
        assert a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes(), cond
    x, y = eng.run_steps(5, trace=True), plain.run_steps(5, trace=True)
    assert x["base"] == y["base"]
    for k in ("position", "outcome", "temperature", "proposed_score", "current_score", "random_threshold",
              "term_values"):
        assert x[k].tobytes() == y[k].tobytes(), k
    fa, fb = eng.download(), plain.download()
    assert fa[0] == fb[0] and fa[1].tobytes() == fb[1].tobytes() and (fa[2] == fb[2]).all()


# ------------------------------------------------------------------ 6. errors
def test_errors(native):
    tmpl, active = workloads.synthetic(60)
    terms = workloads.default_objective()
    seqs = workloads.walker_sequences(tmpl, [active], 2)
    mfe = _engine(native, tmpl, [active], terms, fold_mode="mfe")
    with pytest.raises(native.AdxError) as ei:
        mfe.ensemble_structures(seqs)
    assert ei.value.status == native.EUNSUPPORTED
    mfe.walkers_init([0, 1], seqs)
    with pytest.raises(native.AdxError) as ei:
        mfe.walker_ensemble_structures()
    assert ei.value.status == native.EUNSUPPORTED
    eng = _engine(native, tmpl, [active], terms)
    for gamma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(native.AdxError) as ei:
            eng.ensemble_structures(seqs, gamma=gamma)
        assert ei.value.status == native.EINVAL
        with pytest.raises(native.AdxError) as ei:
            _fold(native, "GGGAAACCC").ensemble_structures(gamma)
        assert ei.value.status == native.EINVAL
    for context in (1, -1):   # an engine without contexts folds context 0 alone
        with pytest.raises(native.AdxError) as ei:
            _engine(native, tmpl, [active], terms, contexts=[("GG", "")]).ensemble_structures(seqs, context=context)
        assert ei.value.status == native.EINVAL
    with pytest.raises(native.AdxError) as ei:
        eng.walker_ensemble_structures()
    assert ei.value.status == native.ESTATE
    # a length whose pair probabilities the outside pass cannot do
    t153, a153 = workloads.synthetic(153)
    with pytest.raises(native.AdxError) as ei:
        _engine(native, t153, [a153], terms).ensemble_structures(workloads.walker_sequences(t153, [a153], 1))
    assert ei.value.status == native.EUNSUPPORTED
    assert "base-pair probabilities of length 153 do not fit one CU's LDS yet" in str(ei.value)
    with pytest.raises(native.AdxError) as ei:
        _fold(native, t153.upper()).ensemble_structures()
    assert ei.value.status == native.EUNSUPPORTED
    # the raw library: null pointers
    L = native.lib()
    buf = b"".join(s.encode() for s in seqs)
    cen, st = C.create_string_buffer(2 * 60 + 1), (native.EnsembleStats * 2)()
    assert L.adx_ensemble_structures_batch(None, 2, buf, 0, 0, 1.0, cen, None, st, None) == native.EINVAL
    assert L.adx_ensemble_structures_batch(eng.ptr, 2, None, 0, 0, 1.0, cen, None, st, None) == native.EINVAL
    assert L.adx_ensemble_structures_batch(eng.ptr, 0, buf, 0, 0, 1.0, cen, None, st, None) == native.EINVAL
    assert L.adx_ensemble_structures_batch(eng.ptr, 2, buf, 0, 0, 1.0, None, None, None, None) == native.EINVAL
    assert L.adx_ensemble_structures_batch(eng.ptr, 2, buf, 0, 0, 1.0, cen, None, None, None) == 0   # one output is enough
    assert "(" in cen.raw.decode()
    assert L.adx_walkers_ensemble_structures(None, 0, 0, 1.0, cen, None, st, None) == native.EINVAL
    assert L.adx_fold_ensemble_structures(None, 1.0, cen, None, None) == native.EINVAL
    f = _fold(native, "GGGAAACCC")
    assert L.adx_fold_ensemble_structures(f.ptr, 1.0, None, None, None) == native.EINVAL
    assert L.adx_last_ensemble_ms(eng.ptr, None, None) == native.EINVAL
    assert L.adx_last_ensemble_ms(None, None, None) == native.EINVAL
