"""GPU parity of pf_ring_kernel (pf_ring.hip): partition functions of folds
longer than pf_cells_kernel covers (101 <= N <= 150; BASELINE config 4's
N = 150), one workgroup per variant with qb in a ring of diagonals and the
exterior sums read back from the walker's table slot.

Bar (north_star): fold free energies within 1e-4 kcal/mol of the FP64 oracle,
MC trajectories (positions, bases, outcomes, counters) identical, incremental
refolds bit-identical to from-scratch folds."""
import math
import random

import numpy as np
import pytest

from addapt_amd import workloads
from parity_bounds import close_score, close_term, score_bound

pytestmark = pytest.mark.gpu

DG_TOL = 1e-4


def rand_seq(rng, n):
    return "".join(rng.choice("ACGU") for _ in range(n))


def rand_constraint(rng, n, p_x=0.1, n_pairs=2):
    c = ["."] * n
    for _ in range(n_pairs):
        i = rng.randrange(0, n - 8)
        j = rng.randrange(i + 5, n)
        if all(ch == "." for ch in c[i:j + 1]):
            c[i], c[j] = "(", ")"
    for k in range(n):
        if c[k] == "." and rng.random() < p_x:
            c[k] = rng.choice("x|<>") if rng.random() < 0.2 else "x"
    return "".join(c)


def _motif(oracle):
    return oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())


def test_ring_fold_layer(native, oracle):
    """Single folds (adx_fold_pf: stateless, qb scratch) at ring lengths, with
    random hard constraints and the ligand motif."""
    rng = random.Random(101)
    apt, fold = workloads.THEO_SEQ, workloads.THEO_FOLD
    e = oracle.theo_bonus()
    for n in (101, 117, 128, 150):
        for _ in range(2):
            s = rand_seq(rng, n)
            for cst in (None, rand_constraint(rng, n)):
                f = native.Fold(s)
                if cst:
                    f.add_constraint(cst)
                g = f.pf()
                ref = np.float32(oracle.pf_energy(s, cst))
                if math.isinf(ref):
                    assert math.isinf(g) and g > 0, (n, cst, g)
                else:
                    assert abs(g - ref) <= DG_TOL, (n, s, cst, g, float(ref))
        s = rand_seq(rng, (n - 27) // 2) + apt
        s = s + rand_seq(rng, n - len(s))
        f = native.Fold(s)
        f.add_motif(apt, fold, e)
        g = f.pf()
        ref = oracle.pf_energy(s, None, oracle.make_motif(apt, fold, e))
        assert abs(g - np.float32(ref)) <= DG_TOL, (n, g, ref)


def _mid_pair(n):
    """An enforced pair of span 5 in the middle, the rest free."""
    a = n // 2 - 2
    return "." * (a - 1) + "(....)" + "." * (n - a - 5)


def _mid_run(n, ch, k=10):
    """Constraint character ch on k positions in the middle, the rest free."""
    a = (n - k) // 2
    return "." * a + ch * k + "." * (n - a - k)


@pytest.mark.parametrize("seq,cst", [("GUGC" * 34, None), ("GUGC" * 37 + "GU", None), ("GUGC" * 34, _mid_run(136, "x")),
                                     ("GUGC" * 37 + "GU", _mid_pair(150))],
                         ids=["n136", "n150", "n136-x", "n150-pair"])
def test_ring_fold_layer_dense_diagonals(native, oracle, seq, cst):
    """G on every odd position, U or C on every even one: every cell of every
    odd diagonal is pairable, so D = 7, the first diagonal with B records, holds
    129 of them at 136 nt: one cell in pf_ring_kernel's third lane-set (150 nt: the
    last length).  'x' on ten middle positions forbids their pairs and leaves
    the unpaired runs up / dn whole: the unmasked shapes with `constrained` set.
    The enforced pair cuts the runs, so the cells around it get the record's
    masked bit and their B batches take the masked (MK) shapes, on diagonals
    that keep more than 128 records (150 nt: D = 7 has 131 pairable cells, one
    masked; D = 9 has 129, three masked)."""
    f = native.Fold(seq)
    if cst:
        f.add_constraint(cst)
    g = f.pf()
    ref = np.float32(oracle.pf_energy(seq, cst))
    assert abs(g - ref) <= DG_TOL, (seq, cst, g, float(ref))


@pytest.mark.parametrize("N", [101, 150])
def test_ring_score_batch(native, oracle, N):
    tmpl, active = workloads.synthetic(N)
    terms = workloads.default_objective()
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    eng = native.Engine(tmpl, [active], terms, aptamer=apt)
    seqs = workloads.walker_sequences(tmpl, [active], 12)
    sc, tv, dg = eng.score_batch(seqs)
    m = _motif(oracle)
    for v in range(eng.info.n_variants):
        _, cond, mac = eng.variant(v)
        for w in range(0, 12, 4):
            ref = oracle.pf_energy(seqs[w], active if mac >= 0 else None, m if cond == 1 else None)
            assert abs(dg[w, v] - np.float32(ref)) <= DG_TOL, (N, v, w, dg[w, v], ref)
    sf = oracle.ScoreFunction(terms, aptamer=m)
    for w in range(12):
        ref, tref = sf.score(seqs[w], [active])
        assert close_score(sc[w], ref, tref, terms), (w, sc[w], ref, score_bound(tref, terms))


def _replay(native, oracle, N, seeds, steps, contexts=None, macro_extra=None):
    tmpl, active = workloads.synthetic(N)
    macro = [active] + ([macro_extra] if macro_extra else [])
    terms = workloads.default_objective() + ([("apo", 1, True, 2.0)] if macro_extra else [])
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
    eng = native.Engine(tmpl, macro, terms, aptamer=apt, contexts=contexts, thermostat=th)
    seqs = workloads.walker_sequences(tmpl, macro, len(seeds))
    eng.walkers_init(seeds, seqs)
    tr = eng.run_steps(steps, trace=True)
    final, scores, counters = eng.download()
    sf = oracle.ScoreFunction(terms, aptamer=_motif(oracle), contexts=contexts)
    therm_o = oracle.thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
    for w, seed in enumerate(seeds):
        forced = [int(x) for x in tr["outcome"][:, w]]
        ref = oracle.mc_run(sf, seqs[w], macro, therm_o, seed, steps, forced=forced, tie_eps=1e-6)
        assert ref["rc"] == 0
        assert list(tr["position"][:, w]) == ref["pos"], w
        assert tr["base"][w::len(seeds)] == ref["base"], w
        assert list(tr["outcome"][:, w]) == ref["outcome"], w
        for s in range(steps):
            if ref["outcome"][s] != 2:
                a, b = tr["proposed_score"][s, w], ref["proposed_score"][s]
                assert close_score(a, b, tr["term_values"][s, w], terms), (N, w, s, a, b)
        assert final[w].upper() == ref["seq"].upper(), w
        fref, ftv = sf.score(ref["seq"], macro)
        assert close_score(scores[w], ref["score"], ftv, terms), (N, w, scores[w], ref["score"])
        assert list(counters[w]) == ref["counters"]


def test_ring_trajectory_n150(native, oracle):
    """Incremental refolds at config 4's length against the oracle's full folds."""
    _replay(native, oracle, 150, [31, 32, 33, 34], 25)


def test_ring_trajectory_contexts(native, oracle):
    """Contexts push the folded length into the ring range (96 + up to 9 nt) and
    shift the changed positions; a second macrostate adds a constrained group."""
    ctx = [("GGACA", "UUAC"), ("", "CCCAGU"), ("AUAUAUA", "")]
    N = 96
    other = "." * 8 + "(" + "." * 16 + ")" + "." * (N - 26)   # mutable positions (the aptamer is frozen)
    _replay(native, oracle, N, [41, 42, 43], 20, contexts=ctx, macro_extra=other)


def test_ring_trajectory_short_variants(native, oracle):
    """A context mix whose folded lengths straddle the ring threshold (96 and
    102 nt): the context takes the ring kernel for every variant, including
    the ones shorter than 101 nt (pf_ring_lds is chosen once per context)."""
    _replay(native, oracle, 96, [51, 52, 53], 20, contexts=[("", ""), ("AAAAAA", "")])


def _longest_context(native):
    """The longest synthetic template a context accepts (the ring kernels take
    up to RG_NMAX = 190 nt; the context also sizes the stateless score
    kernel's LDS layout, api_problem.hpp check_lds, which ends lower)."""
    terms = workloads.default_objective()
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    for N in range(190, 149, -1):
        tmpl, active = workloads.synthetic(N)
        try:
            return N, native.Engine(tmpl, [active], terms, aptamer=apt)
        except native.AdxError as e:
            assert e.status == native.EUNSUPPORTED, e
    raise AssertionError("no context above 150 nt")


def test_ring_long_score_and_trajectory(native, oracle):
    """At the longest length a context accepts (>= 150): ensemble energies of
    every variant vs the FP64 oracle, then a short trajectory replay."""
    N, eng = _longest_context(native)
    tmpl, active = workloads.synthetic(N)
    terms = workloads.default_objective()
    seqs = workloads.walker_sequences(tmpl, [active], 4)
    sc, tv, dg = eng.score_batch(seqs)
    m = _motif(oracle)
    for v in range(eng.info.n_variants):
        _, cond, mac = eng.variant(v)
        for w in range(0, 4, 2):
            ref = oracle.pf_energy(seqs[w], active if mac >= 0 else None, m if cond == 1 else None)
            assert abs(dg[w, v] - np.float32(ref)) <= DG_TOL, (N, v, w, dg[w, v], ref)
    _replay(native, oracle, N, [61, 62], 12)


def test_ring_incremental_consistency(native):
    """512 walkers x 40 steps at N = 150: every stored score equals a
    from-scratch score of the final sequence bit for bit."""
    tmpl, active = workloads.synthetic(150)
    terms = workloads.default_objective()
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=300)
    eng = native.Engine(tmpl, [active], terms, aptamer=apt, thermostat=th)
    W = 512
    seqs = workloads.walker_sequences(tmpl, [active], W)
    eng.walkers_init(list(range(W)), seqs)
    eng.run_steps(40)
    final, scores, counters = eng.download()
    assert (counters.sum(axis=1) == 40).all()
    assert "pf_ring_kernel" in eng.last_kernel_names()[0]
    sc, _, _ = eng.score_batch(final)
    bad = np.nonzero(scores != sc)[0]
    assert bad.size == 0, [(int(w), scores[w], sc[w]) for w in bad[:8]]
    fresh, _ = eng.rescore()   # the step's own kernels from scratch
    assert (fresh == scores).all()
