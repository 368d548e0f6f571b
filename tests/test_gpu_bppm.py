"""GPU parity of the outside pass / base-pair probabilities (SURVEY.md §8 A16,
configs 3-4): RnaFold::base_pair_prob (scoring.cc:37-51) through adx_fold_bpp,
adx_bppm_batch and the ADX_TERM_PAIR score term, against the oracle's FP64
adjoint sweep (oracle/fold.c orc_bppm).

Tolerances: FP32 inside + outside with per-nucleotide scaling vs FP64:
|P_gpu - P_oracle| <= 2e-4 absolute per pair (whole matrices); score terms
within the bound 1e-4 kcal/mol per fold induces (tests/parity_bounds.py:
a pair probability is a ratio of two ensembles like a macrostate's); MC
trajectories bit-exact with the oracle forced through Metropolis near-ties
(|crit - u| <= 1e-6).

Whole matrices under hard constraints (every constraint character, the motif
with a constraint, lengths on both sides of bppm_kernel's layouts) also hold
the derived bound on ln P from pair_probe.REL_FLOOR up and are exactly 0 where
the oracle is; measured there: max |dP| and worst |d ln P| 6.2e-6.
"""
import math
import random

import numpy as np
import pytest

from addapt_amd import workloads
from pair_probe import REL_FLOOR, can_pair
from parity_bounds import close_score, close_term, score_bound
from structure_check import cons, pin

pytestmark = pytest.mark.gpu

P_TOL = 2e-4


def rand_seq(rng, n):
    return "".join(rng.choice("ACGU") for _ in range(n))


def test_fold_bpp_matches_oracle(native, oracle):
    rng = random.Random(23)
    cases = [("GGGGAAACCCC", None), ("ACGUGAAAACGU", "((((....))))"), (workloads.THEO_SEQ, None)]
    for n in (20, 45, 80, 100, 150):
        for _ in range(2):
            cases.append((rand_seq(rng, n), None))
    cases.append((cases[-3][0], "." * 10 + "x" * 5 + "." * 85))
    for seq, cst in cases:
        f = native.Fold(seq)
        if cst:
            f.add_constraint(cst)
        _, ref = oracle.bppm(seq, cst)
        n = len(seq)
        got = np.array([[f.bpp(i + 1, j + 1) for j in range(n)] for i in range(n)])
        assert np.abs(got - ref).max() <= P_TOL, (seq, cst, np.abs(got - ref).max())


def test_fold_bpp_motif(native, oracle):
    apt, fold = workloads.THEO_SEQ, workloads.THEO_FOLD
    e = oracle.theo_bonus()
    for seq in (apt, "GGGA" + apt + "UCCC"):
        f = native.Fold(seq)
        f.add_motif(apt, fold, e)
        _, ref = oracle.bppm(seq, None, oracle.make_motif(apt, fold, e))
        n = len(seq)
        got = np.array([[f.bpp(i + 1, j + 1) for j in range(n)] for i in range(n)])
        assert np.abs(got - ref).max() <= P_TOL, (seq, np.abs(got - ref).max())


def _objective(N):
    # config 3: default objective + apo/holo base-pair probability terms
    return workloads.default_objective() + [("apo", ("pair", 0, N - 1), False, 1.0),
                                            ("holo", ("pair", 0, N - 1), True, 1.0)]


def _engine(native, tmpl, macro, terms, thermostat=None, contexts=None):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    return native.Engine(tmpl, macro, terms, aptamer=apt, contexts=contexts,
                         thermostat=thermostat or native.make_thermostat("fixed", t=1.0))


def _oracle_sf(oracle, terms, contexts=None):
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    return oracle.ScoreFunction(terms, aptamer=m, contexts=contexts)


@pytest.mark.parametrize("N", [60, 100, 150])
def test_bppm_batch(native, oracle, N):
    tmpl, active = workloads.synthetic(N)
    eng = _engine(native, tmpl, [active], _objective(N))
    seqs = workloads.walker_sequences(tmpl, [active], 6)
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    for cond in ("apo", "holo"):
        got = eng.bppm_batch(seqs, cond)
        for w in range(6):
            _, ref = oracle.bppm(seqs[w].upper(), None, m if cond == "holo" else None)
            err = np.abs(got[w] - ref).max()
            assert err <= P_TOL, (N, cond, w, err)


def _close_terms(tv, tref, terms):
    return all(close_term(a, b, terms[k % len(terms)][2]) for k, (a, b) in enumerate(zip(tv, tref)))


@pytest.mark.parametrize("N", [60, 100, 150])
def test_score_with_pair_terms(native, oracle, N):
    tmpl, active = workloads.synthetic(N)
    terms = _objective(N)
    eng = _engine(native, tmpl, [active], terms)
    seqs = workloads.walker_sequences(tmpl, [active], 12)
    sc, tv, _ = eng.score_batch(seqs)
    sf = _oracle_sf(oracle, terms)
    for w in range(12):
        ref, tref = sf.score(seqs[w], [active])
        assert _close_terms(tv[w], tref, terms), (w, list(tv[w]), tref)
        assert close_score(sc[w], ref, tref, terms), (w, sc[w], ref)


def test_pair_terms_with_contexts(native, oracle):
    tmpl, active = workloads.synthetic(60)
    terms = [("apo", ("pair", 2, 57), True, 1.0), ("holo", ("pair", 0, 59), False, 0.5),
             ("holo", 0, True, 1.0)]
    ctx = [("GGAC", "UUA"), ("", "CCCA")]
    eng = _engine(native, tmpl, [active], terms, contexts=ctx)
    seqs = workloads.walker_sequences(tmpl, [active], 4)
    sc, tv, _ = eng.score_batch(seqs)
    sf = _oracle_sf(oracle, terms, contexts=ctx)
    for w in range(4):
        ref, tref = sf.score(seqs[w], [active])
        assert _close_terms(tv[w], tref, terms), (w, list(tv[w]), tref)
        assert close_score(sc[w], ref, tref, terms), (w, sc[w], ref)


def test_mc_trajectory_with_pair_terms(native, oracle):
    tmpl, active = workloads.synthetic(60)
    terms = _objective(60)
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
    eng = _engine(native, tmpl, [active], terms, thermostat=th)
    seeds = [0, 1, 2, 3]
    seqs = workloads.walker_sequences(tmpl, [active], len(seeds))
    therm_o = oracle.thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
    steps = 25
    eng.walkers_init(seeds, seqs)
    tr = eng.run_steps(steps, trace=True)
    final, scores, counters = eng.download()
    sf = _oracle_sf(oracle, terms)
    for w, seed in enumerate(seeds):
        forced = [int(x) for x in tr["outcome"][:, w]]
        ref = oracle.mc_run(sf, seqs[w], [active], therm_o, seed, steps, forced=forced, tie_eps=1e-6)
        assert ref["rc"] == 0
        assert list(tr["position"][:, w]) == ref["pos"], w
        assert tr["base"][w::len(seeds)] == ref["base"], w
        assert list(tr["outcome"][:, w]) == ref["outcome"], w
        assert final[w].upper() == ref["seq"].upper(), w
        assert list(counters[w]) == ref["counters"]


@pytest.mark.parametrize("N,motif_pairs", [(60, False), (80, True), (100, False), (110, False), (150, False),
                                           (150, True), ("longest", False)])
def test_mc_pair_terms_proposed_scores(native, oracle, N, motif_pairs):
    """Configs 3 / 4 shape: inside folds first (N <= 100: pf_cells_kernel,
    else pf_ring_kernel), the outside pass on the proposal's stored inside tables
    (N <= 100: outside_cells_kernel; N > 100: outside_ring_kernel on the ring
    kernel's diagonal-major slot), then the scores.  Every
    scored proposal's score matches the oracle's from-scratch score of that
    proposal (within the derived bound).  motif_pairs: pair terms inside the
    ligand motif (credited from the motif's closing cell in the holo fold).
    "longest": the longest template a pair-term context accepts (<= 190)."""
    if N == "longest":
        for N in range(190, 149, -1):
            try:
                _engine(native, workloads.synthetic(N)[0], [workloads.synthetic(N)[1]], _objective(N))
                break
            except native.AdxError as e:
                assert e.status == native.EUNSUPPORTED, e
    tmpl, active = workloads.synthetic(N)
    terms = _objective(N)
    if motif_pairs:
        o = (N - 27) // 2   # the aptamer's site in the synthetic template
        terms = workloads.default_objective() + [("holo", ("pair", o + 4, o + 22), True, 1.0),
                                                ("apo", ("pair", o, o + 26), False, 0.5),
                                                ("holo", ("pair", o + 7, o + 16), True, 0.25)]
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
    eng = _engine(native, tmpl, [active], terms, thermostat=th)
    seeds = [21, 22, 23]
    seqs = workloads.walker_sequences(tmpl, [active], 64)
    eng.walkers_init(seeds + list(range(100, 161)), seqs)
    steps = 10
    tr = eng.run_steps(steps, trace=True)
    _, _, counters = eng.download()
    assert (counters.sum(axis=1) == steps).all()
    sf = _oracle_sf(oracle, terms)
    therm_o = oracle.thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
    for w, seed in enumerate(seeds):
        forced = [int(x) for x in tr["outcome"][:, w]]
        ref = oracle.mc_run(sf, seqs[w], [active], therm_o, seed, steps, forced=forced, tie_eps=1e-6)
        assert ref["rc"] == 0
        assert list(tr["position"][:, w]) == ref["pos"], w
        for s in range(steps):
            if ref["outcome"][s] != 2:
                a, b = tr["proposed_score"][s, w], ref["proposed_score"][s]
                assert close_score(a, b, tr["term_values"][s, w], terms), (N, w, s, a, b)


@pytest.mark.parametrize("N", [100, 150])
def test_mc_pair_terms_full_size(native, oracle, N):
    """Configs 3 / 4 at their per-GPU size (4096 walkers; N = 100: pf_cells +
    outside_cells, N = 150: pf_ring + outside_ring): counters sum to the steps,
    and sampled walkers' final scores (pair probabilities included) equal the
    oracle's from-scratch scores of their final sequences."""
    tmpl, active = workloads.synthetic(N)
    terms = _objective(N)
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=300)
    eng = _engine(native, tmpl, [active], terms, thermostat=th)
    W = 4096
    seqs = workloads.walker_sequences(tmpl, [active], W)
    eng.walkers_init(list(range(W)), seqs)
    eng.run_steps(2)
    final, scores, counters = eng.download()
    assert (counters.sum(axis=1) == 2).all()
    inside, outside = eng.last_kernel_names()
    assert (inside.startswith("pf_cells_kernel") and outside == "outside_cells_kernel") if N <= 100 else \
        (inside.startswith("pf_ring_kernel") and outside == "outside_ring_kernel"), (inside, outside)
    sf = _oracle_sf(oracle, terms)
    for w in list(range(0, W, 683)) + [W - 1]:
        ref, tref = sf.score(final[w], [active])
        assert close_score(scores[w], ref, tref, terms), (N, w, scores[w], ref)


# ------------------------------------------------------------------ whole matrices under hard constraints
CST_LENGTHS = (20, 45, 64, 65, 100, 101, 128, 150, 152)
CST_KINDS = ("cons", "pair", "xrun", "|", "<", ">", "pin")


def _bpp_matrix(native, seq, cst=None, motif=None):
    f = native.Fold(seq)
    if motif:
        f.add_motif(*motif)
    if cst:
        f.add_constraint(cst)
    n = len(seq)
    return np.array([[f.bpp(i + 1, j + 1) for j in range(n)] for i in range(n)])


def _assert_matrix(got, ref, where):
    """|dP| <= P_TOL everywhere, the derived bound on ln P from REL_FLOOR up,
    exactly 0 where the oracle is exactly 0."""
    err = np.abs(got - ref)
    assert err.max() <= P_TOL, where + (float(err.max()),)
    assert not got[ref == 0.0].any(), where + (np.argwhere((ref == 0.0) & (got != 0.0))[:4].tolist(),)
    worst = 0.0
    for i, j in np.argwhere(ref >= REL_FLOOR):
        a = math.log(got[i, j]) if got[i, j] > 0.0 else -math.inf
        b = math.log(ref[i, j])
        assert close_term(a, b, True), where + ((int(i), int(j)), got[i, j], ref[i, j], abs(a - b))
        worst = max(worst, abs(a - b))
    print("CST", where, "max|dP| %.3e worst|dlnP| %.3e over %d" % (err.max(), worst, (ref >= REL_FLOOR).sum()))


def _side_position(seq, P0, side):
    """The position whose unconstrained pairing probability is nearest 0.5 among
    those that can pair on `side` ("<": a partner before it, ">": after it, "|": either)."""
    U = np.triu(P0, 1)                             # [i][j], i < j
    up, down = U.sum(axis=0), U.sum(axis=1)
    can = {"<": up > 0.0, ">": down > 0.0, "|": (up + down) > 0.0}[side]
    tot = np.where(can, up + down, np.inf)
    return int(np.argmin(np.abs(tot - 0.5)))


def _constraint(oracle, rng, seq, kind):
    n = len(seq)
    if kind == "cons":
        return cons(rng, seq)
    if kind == "pair":      # one enforced pair of span >= n / 2 where the bases pair
        i, j = rng.choice([(i, j) for i in range(n) for j in range(i + (n + 1) // 2, n) if can_pair(seq, i, j)])
        return "." * i + "(" + "." * (j - i - 1) + ")" + "." * (n - j - 1)
    if kind == "xrun":
        a = rng.randrange(0, n - 9)
        return "." * a + "x" * 10 + "." * (n - a - 10)
    if kind == "pin":
        return pin(oracle.mfe(seq)[1])
    k = _side_position(seq, oracle.bppm(seq)[1], kind)
    return "." * k + kind + "." * (n - k - 1)


def _cst_sequence(oracle, N):
    """A random sequence of length N whose MFE structure has a pair (to pin)."""
    rng = random.Random(7000 + N)
    while True:
        seq = rand_seq(rng, N)
        if "(" in oracle.mfe(seq)[1]:
            return seq


@pytest.mark.parametrize("kind", CST_KINDS)
@pytest.mark.parametrize("N", CST_LENGTHS)
def test_fold_bpp_constrained(native, oracle, N, kind):
    """bppm_kernel under every hard-constraint character, at the lengths on both
    sides of its layouts (64 / 65, 100 / 101, the global-scratch layout from 114)."""
    seq = _cst_sequence(oracle, N)
    rng = random.Random(N * 31 + CST_KINDS.index(kind))
    cst = _constraint(oracle, rng, seq, kind)
    assert len(cst) == N
    _, ref = oracle.bppm(seq, cst)
    assert ref.any(), (N, kind, cst)                # the constraint admits structures
    got = _bpp_matrix(native, seq, cst)
    _assert_matrix(got, ref, (N, kind, cst))
    if kind in "|<>":
        k = cst.index(kind)
        up, down = got[:k, k].sum(), got[k, k + 1:].sum()
        assert abs(up + down - 1.0) <= N * P_TOL, (N, kind, k, up, down)
        if kind == "<":
            assert down == 0.0 and ref[k, k + 1:].sum() == 0.0, (N, k, down)
        if kind == ">":
            assert up == 0.0 and ref[:k, k].sum() == 0.0, (N, k, up)
    if kind == "pin":
        s = oracle.mfe(seq)[1]
        assert "(" in s
        st, paired = [], np.zeros((N, N), bool)
        for k, c in enumerate(s):
            if c == "(":
                st.append(k)
            elif c == ")":
                paired[st.pop(), k] = True
        up = np.triu(np.ones((N, N), bool), 1)
        assert (got[paired] >= 1.0 - P_TOL).all() and (got[up & ~paired] <= P_TOL).all(), (N, s)


@pytest.mark.parametrize("tail", [17, 111])
def test_fold_bpp_constrained_motif(native, oracle, tail):
    """A constraint on the flanks together with the ligand motif (56 and 150 nt)."""
    rng = random.Random(9000 + tail)
    apt, fold = workloads.THEO_SEQ, workloads.THEO_FOLD
    left, right = rand_seq(rng, 12), rand_seq(rng, tail)
    seq = left + apt + right
    cst = cons(rng, left) + "." * len(apt) + cons(rng, right)
    assert set(cst) > {"."}
    e = oracle.theo_bonus()
    _, ref = oracle.bppm(seq, cst, oracle.make_motif(apt, fold, e))
    _, bare = oracle.bppm(seq, cst)
    assert ref.max() > 0.5 and np.abs(ref - bare).max() > 0.01     # the motif matters here
    got = _bpp_matrix(native, seq, cst, (apt, fold, e))
    _assert_matrix(got, ref, (len(seq), "motif", cst))


def test_fold_bpp_infeasible_101(native, oracle):
    """An enforced pair of bases that cannot pair: nothing is admissible, every probability is 0."""
    rng = random.Random(101)
    seq = "A" + rand_seq(rng, 99) + "A"
    cst = "(" + "." * 99 + ")"
    _, ref = oracle.bppm(seq, cst)
    assert not ref.any()
    got = _bpp_matrix(native, seq, cst)
    assert not got.any(), np.argwhere(got != 0.0)[:4].tolist()
