"""Unpaired-region probabilities on the GPU (pf_access.hip) through the per-fold call,
the batched context call and the current walkers.

P_u(i, j) is held to unpaired_check.brute, the ratio of two of the CPU oracle's
partition functions, within 2e-4 absolute: the bound test_gpu_bppm.py holds pair
probabilities to, which follows from the project's 1e-4 kcal/mol PF bound on both
energies.  Each test prints the largest deviation it saw.  Pinned structures, short
sequences, infeasible constraints and forced bases give exact answers; the identities
at 100 nt need no reference fold; equal inputs give equal bytes.
"""
import ctypes as C
import math
import random

import numpy as np
import pytest

import loop_zoo as Z
import unpaired_check as uc
from addapt_amd import workloads
from structure_check import cons, rand_seq

pytestmark = pytest.mark.gpu

TOL = 2e-4
APT = workloads.THEO_SEQ
CONTEXTS = [("GGAC", "UUA"), ("", "CCCA")]


def _motif(oracle):
    return oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())


def _fold(native, seq, cst=None, motif=False):
    f = native.Fold(seq)
    if motif:
        f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    if cst:
        f.add_constraint(cst)
    return f


def _engine(native, tmpl, macro, terms, thermostat=None, contexts=None, fold_mode="pf"):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    return native.Engine(tmpl, macro, terms, aptamer=apt, contexts=contexts, fold_mode=fold_mode,
                         thermostat=thermostat or native.make_thermostat("fixed", t=1.0))


def _synthetic(native, N, **kw):
    tmpl, active = workloads.synthetic(N)
    return _engine(native, tmpl, [active], workloads.default_objective(), **kw), tmpl, active


def _against_brute(native, oracle, seq, cst, max_len, motif=False):
    got, _, e = _fold(native, seq, cst, motif).unpaired_probs(max_len)
    m = _motif(oracle) if motif else None
    ref = uc.brute(oracle, seq, cst, max_len, m)
    assert got.shape == ref.shape and got.dtype == np.float64
    dev = np.abs(got - ref).max()
    print("largest deviation from brute, %d nt, max_len %d: %.3g" % (len(seq), max_len, dev))
    assert dev <= TOL, (seq, cst, dev)
    assert abs(e - oracle.pf_energy(seq, cst, m)) <= 1e-4
    return got


# ------------------------------------------------------------------ 1. against brute
def _all_window_cases():
    rng = random.Random(41)
    return list(uc.ENUM_CASES) + [(rand_seq(rng, 23), None), (rand_seq(rng, 30), None)]


@pytest.mark.parametrize("seq,cst", _all_window_cases())
def test_every_window_of_short_folds(native, oracle, seq, cst):
    n = len(seq)
    got = _against_brute(native, oracle, seq, cst, n)
    # the windows at i = 1 and at j = L, and the open chain's probability
    g = oracle.pf_energy(seq, cst)
    open_chain = 0.0 if cst and any(c in uc.FORCED for c in cst) else math.exp(g / oracle.KT_KCAL)
    assert abs(got[n - 1, 0] - open_chain) <= TOL
    for u in range(1, n + 1):
        assert (got[u - 1, n - u + 1:] == 0.0).all()   # columns past L - u


def _len6_cases():
    rng = random.Random(31)
    out = []
    for n in (37, 64, 65):
        seq = rand_seq(rng, n)
        out += [(seq, None), (seq, cons(rng, seq))]
    return out


@pytest.mark.parametrize("seq,cst", _len6_cases())
def test_windows_up_to_six(native, oracle, seq, cst):
    got = _against_brute(native, oracle, seq, cst, 6)
    for i, c in enumerate(cst or ""):   # a window over a forced base is exactly 0
        if c in uc.FORCED:
            for u in range(1, 7):
                assert (got[u - 1, max(0, i - u + 1):i + 1] == 0.0).all()


def test_windows_up_to_three_at_100(native, oracle):
    _against_brute(native, oracle, rand_seq(random.Random(100), 100), None, 3)


def test_regions_at_150(native, oracle):
    """40 fixed random windows of one 150-nt sequence, through the region form."""
    eng, tmpl, active = _synthetic(native, 150)
    seq = workloads.walker_sequences(tmpl, [active], 1)[0]
    free = [v for v in range(eng.info.n_variants) if eng.variant(v)[1:] == (0, -1)][0]
    rng = random.Random(150)
    regions = []
    for _ in range(40):
        ln = rng.randrange(1, 25)
        regions.append((rng.randrange(0, 150 - ln + 1), ln))
    prof, rp, e = eng.unpaired_probs([seq], free, regions=regions)
    assert prof is None and rp.shape == (1, 40)
    g = oracle.pf_energy(seq.upper())
    ref = [uc.window(oracle, seq.upper(), None, a + 1, a + ln, None, g) for a, ln in regions]
    dev = np.abs(rp[0] - ref).max()
    print("largest deviation from brute, 150 nt regions: %.3g" % dev)
    assert dev <= TOL and abs(e[0] - g) <= 1e-4


@pytest.mark.parametrize("holo", [False, True])
def test_motif_apo_and_holo(native, oracle, holo):
    """Windows up to 6 everywhere: inside the motif's dots, across its closing pair and outside it."""
    rng = random.Random(31)
    seq = rand_seq(rng, 12) + APT + rand_seq(rng, 17)
    got = _against_brute(native, oracle, seq, None, 6, motif=holo)
    o = seq.index(APT)
    dots = [k for k, c in enumerate(workloads.THEO_FOLD) if c == "."]
    assert got[0, o + dots[0]] > 0.0 and o > 0 and o + len(APT) < len(seq)


def test_context_padded_variants(native, oracle):
    """L > N: every kind of variant of a synthetic(60) engine in two contexts, in the
    folded coordinates: windows up to 2 everywhere and regions across the context's seams."""
    eng, tmpl, active = _synthetic(native, 60, contexts=CONTEXTS)
    seq = workloads.walker_sequences(tmpl, [active], 1)[0]
    m = _motif(oracle)
    kinds, worst = set(), 0.0
    for v in range(eng.info.n_variants):
        c, cond, mac = eng.variant(v)
        b, a = CONTEXTS[c]
        full = (b + seq + a).upper()
        L = len(full)
        cst = "." * len(b) + active + "." * len(a) if mac >= 0 else None
        regions = [(0, 9), (max(len(b) - 2, 0), 5), (L - len(a) - 3, 6), (L - 12, 12), (20, 31)]
        prof, rp, e = eng.unpaired_probs([seq], v, max_len=2, regions=regions)
        assert prof.shape == (1, 2, L) and rp.shape == (1, len(regions))
        mm = m if cond == 1 else None
        g = oracle.pf_energy(full, cst, mm)
        ref = uc.brute(oracle, full, cst, 2, mm)
        rref = [uc.window(oracle, full, cst, s + 1, s + ln, mm, g) for s, ln in regions]
        worst = max(worst, np.abs(prof[0] - ref).max(), np.abs(rp[0] - rref).max())
        assert abs(e[0] - g) <= 1e-4
        kinds.add((cond, mac >= 0))
    print("largest deviation from brute, context-padded variants: %.3g" % worst)
    assert worst <= TOL
    assert kinds == {(0, False), (0, True), (1, False), (1, True)}


# ------------------------------------------------------------------ 2. deterministic facts
def test_pinned_structures(native):
    for name, seq, st in uc.zoo(wide=True):
        n = len(seq)
        got, pp, e = _fold(native, seq, uc.pin(st)).unpaired_probs(n, pair_probs=True)
        dots = uc.dots_table(st, n)
        assert math.isfinite(e), name
        assert got[dots == 1].min() >= 1 - 1e-9, name
        assert got[dots == 0].max() <= 1e-12, name
        pt = Z.pair_table(st)
        want = np.zeros((n, n))
        for k, p in enumerate(pt):
            if p >= 0:
                want[k, p] = 1.0
        assert np.abs(pp - want).max() <= 1e-9, name


def test_tiny_infeasible_and_forced(native):
    for seq in ("ACG", "ACGU"):
        n = len(seq)
        got, pp, e = _fold(native, seq).unpaired_probs(n, pair_probs=True)
        assert e == 0.0 and (pp == 0.0).all()
        for u in range(1, n + 1):
            assert (got[u - 1, :n - u + 1] == 1.0).all() and (got[u - 1, n - u + 1:] == 0.0).all()
    got, pp, e = _fold(native, "AAAAAAAAAA", "(........)").unpaired_probs(10, pair_probs=True)
    assert np.isnan(pp).all() and math.isinf(e) and e > 0
    for u in range(1, 11):   # every window; the columns past L - u stay 0
        assert np.isnan(got[u - 1, :10 - u + 1]).all() and (got[u - 1, 10 - u + 1:] == 0.0).all()
    seq, cst = "GGGUGAAAACUAGUGAAAGCCC", "(...|...........|....)"
    got, _, _ = _fold(native, seq, cst).unpaired_probs(22)
    for k in (0, 4, 16, 21):
        for u in range(1, 23):
            for i in range(max(0, k - u + 1), min(k, 22 - u) + 1):
                assert got[u - 1, i] == 0.0
    assert got[0, 1] > 0.0


# ------------------------------------------------------------------ 3. identities at 100 nt
def test_identities_at_100(native, oracle):
    seq = rand_seq(random.Random(7), 100)
    got, pp, _ = _fold(native, seq).unpaired_probs(30, pair_probs=True)
    _, P = oracle.bppm(seq)
    d1 = np.abs(got[0] - (1.0 - P.sum(axis=1))).max()
    d2 = np.abs(pp - P).max()
    print("100 nt: length-1 row vs 1 - sum bppm %.3g, pair_probs vs bppm %.3g" % (d1, d2))
    assert d1 <= TOL and d2 <= TOL
    assert (pp == pp.T).all()
    assert np.abs(got[0] + pp.sum(axis=1) - 1.0).max() <= 1e-12
    for u in range(1, 30):   # a longer window is no likelier than either of its parts
        n = 100 - u
        assert (got[u, :n] <= np.minimum(got[u - 1, :n], got[u - 1, 1:n + 1]) + 1e-12).all()


# ------------------------------------------------------------------ 4. same bytes
def test_repeats_fold_batch_and_regions(native):
    eng, tmpl, active = _synthetic(native, 100)
    seqs = workloads.walker_sequences(tmpl, [active], 5)
    regions = [(0, 1), (10, 7), (40, 30), (0, 100), (99, 1), (60, 40)]
    for v in range(eng.info.n_variants):
        a, ra, ea = eng.unpaired_probs(seqs, v, max_len=40, regions=regions)
        b, rb, eb = eng.unpaired_probs(seqs, v, max_len=40, regions=regions)
        assert a.tobytes() == b.tobytes() and ra.tobytes() == rb.tobytes() and ea.tobytes() == eb.tobytes()
        _, rc, _ = eng.unpaired_probs(seqs, v, regions=regions)   # regions alone, max_len 0
        assert rc.tobytes() == ra.tobytes()
        for k, (s, ln) in enumerate(regions):   # a region is the profile's entry
            if ln <= 40:
                assert ra[:, k].tobytes() == np.ascontiguousarray(a[:, ln - 1, s]).tobytes()
        assert (ra[:, 3] <= ra[:, 5]).all()
    # the per-fold call folds under its own pf scale: the same numbers to the rounding of
    # the FP32 factors (a relative 6e-8 each), not the same bytes
    free = [v for v in range(eng.info.n_variants) if eng.variant(v)[1:] == (0, -1)][0]
    a, _, ea = eng.unpaired_probs(seqs[:1], free, max_len=40)
    f = _fold(native, seqs[0].upper())
    g, _, eg = f.unpaired_probs(40)
    g2, _, _ = f.unpaired_probs(40)
    assert g.tobytes() == g2.tobytes()
    assert np.abs(a[0] - g).max() <= 1e-6 and abs(ea[0] - eg) <= 1e-4


def test_launch_chunks_do_not_show(native):
    """400 sequences of 150 nt: their slices alone (0.70 MB each) pass the 256 MiB bound of
    one launch, so the call is split; its first 20 rows equal a 20-sequence call, which is
    one launch, and the last row is its own one-sequence call's."""
    eng, tmpl, active = _synthetic(native, 150)
    seqs = workloads.walker_sequences(tmpl, [active], 400)
    slice_bytes = (6 * (146 * 147 // 2) + 150 * 150 + 152) * 8
    regions = [(0, 150), (30, 20), (149, 1), (75, 4)]
    assert 400 * slice_bytes > 256 << 20 > 20 * (slice_bytes + 8 * len(regions))
    _, big, eb = eng.unpaired_probs(seqs, 0, regions=regions)
    _, small, es = eng.unpaired_probs(seqs[:20], 0, regions=regions)
    assert big[:20].tobytes() == small.tobytes() and eb[:20].tobytes() == es.tobytes()
    _, last, el = eng.unpaired_probs(seqs[399:], 0, regions=regions)
    assert big[399].tobytes() == last[0].tobytes() and eb[399] == el[0]
    assert (big[399] > 0.0).all() and (big[399] < 1.0).all()


def test_walkers_and_untouched_state(native):
    tmpl, active = workloads.synthetic(60)
    terms = workloads.default_objective()
    W = 70
    seqs = workloads.walker_sequences(tmpl, [active], W)
    regions = [(3, 8), (20, 20), (59, 1)]

    def engine():
        th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
        eng = _engine(native, tmpl, [active], terms, thermostat=th)
        eng.walkers_init(list(range(W)), seqs)
        eng.run_steps(5)
        return eng

    eng, plain = engine(), engine()
    cur = eng.download()[0]
    assert cur != seqs   # the walkers moved
    for v in range(eng.info.n_variants):
        p, r, e = eng.walker_unpaired_probs(v, max_len=5, regions=regions)
        p2, r2, e2 = eng.unpaired_probs(cur, v, max_len=5, regions=regions)
        assert p.shape == (W, 5, 60) and r.shape == (W, 3)
        assert p.tobytes() == p2.tobytes() and r.tobytes() == r2.tobytes() and e.tobytes() == e2.tobytes(), v
        none, r3, _ = eng.walker_unpaired_probs(v, regions=regions)
        assert none is None and r3.tobytes() == r.tobytes()
    fill_ms, outside_ms = eng.last_unpaired_ms()
    assert fill_ms > 0.0 and outside_ms > 0.0
    a, b = eng.run_steps(5, trace=True), plain.run_steps(5, trace=True)
    assert a["base"] == b["base"]
    for k in ("position", "outcome", "temperature", "proposed_score", "current_score", "random_threshold",
              "term_values"):
        assert a[k].tobytes() == b[k].tobytes(), k
    fa, fb = eng.download(), plain.download()
    assert fa[0] == fb[0] and fa[1].tobytes() == fb[1].tobytes() and (fa[2] == fb[2]).all()


# ------------------------------------------------------------------ 5. errors
def _status(native, call, *args, **kw):
    with pytest.raises(native.AdxError) as ei:
        call(*args, **kw)
    return ei.value.status


def test_errors(native):
    tmpl, active = workloads.synthetic(60)
    terms = workloads.default_objective()
    seqs = workloads.walker_sequences(tmpl, [active], 2)
    mfe = _engine(native, tmpl, [active], terms, fold_mode="mfe")
    assert _status(native, mfe.unpaired_probs, seqs, 0, max_len=4) == native.EUNSUPPORTED
    mfe.walkers_init([0, 1], seqs)
    assert _status(native, mfe.walker_unpaired_probs, 0, max_len=4) == native.EUNSUPPORTED
    eng = _engine(native, tmpl, [active], terms)
    for v in (-1, eng.info.n_variants):
        assert _status(native, eng.unpaired_probs, seqs, v, max_len=4) == native.EINVAL
    for ml in (-1, 61):
        assert _status(native, eng.unpaired_probs, seqs, 0, max_len=ml) == native.EINVAL
        assert _status(native, eng.unpaired_probs, seqs, 0, max_len=ml, regions=[(0, 4)]) == native.EINVAL
    assert _status(native, eng.unpaired_probs, seqs, 0) == native.EINVAL              # nothing asked for
    assert _status(native, eng.unpaired_probs, seqs, 0, regions=[]) == native.EINVAL
    for bad in ((-1, 4), (0, 0), (0, -2), (60, 1), (57, 4), (0, 61)):
        assert _status(native, eng.unpaired_probs, seqs, 0, regions=[(0, 4), bad]) == native.EINVAL, bad
    assert eng.unpaired_probs(seqs, 0, max_len=60, regions=[(0, 60), (59, 1)])[0].shape == (2, 60, 60)
    assert _status(native, eng.walker_unpaired_probs, 0, max_len=4) == native.ESTATE
    eng.walkers_init([0, 1], seqs)
    for v in (-1, eng.info.n_variants):
        assert _status(native, eng.walker_unpaired_probs, v, max_len=4) == native.EINVAL
    assert _status(native, eng.walker_unpaired_probs, 0) == native.EINVAL
    assert _status(native, eng.walker_unpaired_probs, 0, regions=[(60, 1)]) == native.EINVAL
    f = _fold(native, "GGGAAACCC")
    for ml in (0, -1, 10):
        assert _status(native, f.unpaired_probs, ml) == native.EINVAL
    L = native.lib()
    buf = b"".join(s.encode() for s in seqs)
    out = np.zeros(2 * 4 * 60)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    reg = np.array([0, 4], np.int32)
    pr = reg.ctypes.data_as(C.POINTER(C.c_int))
    assert L.adx_fold_unpaired_probs(None, 1, po, None, None) == native.EINVAL
    assert L.adx_fold_unpaired_probs(f.ptr, 1, None, None, None) == native.EINVAL
    assert L.adx_unpaired_probs_batch(None, 2, buf, 0, 4, 0, None, po, None, None) == native.EINVAL
    assert L.adx_unpaired_probs_batch(eng.ptr, 2, None, 0, 4, 0, None, po, None, None) == native.EINVAL
    assert L.adx_unpaired_probs_batch(eng.ptr, 0, buf, 0, 4, 0, None, po, None, None) == native.EINVAL
    assert L.adx_unpaired_probs_batch(eng.ptr, 2, buf, 0, 4, 0, None, None, None, None) == native.EINVAL
    assert L.adx_unpaired_probs_batch(eng.ptr, 2, buf, 0, 0, 1, None, None, po, None) == native.EINVAL   # regions NULL
    assert L.adx_unpaired_probs_batch(eng.ptr, 2, buf, 0, 0, 1, pr, None, po, None) == 0
    assert L.adx_walkers_unpaired_probs(None, 0, 4, 0, None, po, None, None) == native.EINVAL
    assert L.adx_walkers_unpaired_probs(eng.ptr, 0, 4, 0, None, None, None, None) == native.EINVAL
    assert L.adx_walkers_unpaired_probs(eng.ptr, 0, 4, 0, None, po, None, None) == 0
    assert L.adx_last_unpaired_ms(eng.ptr, None, None) == native.EINVAL
    assert L.adx_last_unpaired_ms(None, None, None) == native.EINVAL
