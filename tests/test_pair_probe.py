"""pair_probe.py on the CPU oracle alone: the pairs pair_sets() chooses cover
what test_gpu_outside_pairs.py claims to check, check_terms() fails on an error
just past the bound, and the replayer reproduces the oracle's trajectories.

The coverage counts are conditions, not measurements: a later edit of the
selection that thins them fails here.  Where they come from (oracle, k_sets = 3,
per_set = 62): the anchors have 55 (syn60 holo, the tightest) to 367 pairs with
P >= 1e-3 and 203 to 2636 with P >= 1e-6; the dense anchors have 128 (100 nt)
and 823 (150 nt) pairs with P >= 1e-6 at compacted rank >= 64, and 34 (150 nt)
and 50 (152 nt) at rank >= 128.
"""
import math

import pytest

import pair_probe
from addapt_amd import workloads
from pair_probe import REL_FLOOR
from parity_bounds import E_TERM

K_SETS, PER_SET = 3, 62

CASES = [(name, seq, cond, dense) for name, seq, conds, dense in pair_probe.anchors() for cond in conds]


def _matrix(oracle, seq, cond):
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    return oracle.bppm(seq, None, m if cond == "holo" else None)[1]


@pytest.mark.parametrize("name,seq,cond,dense", CASES, ids=["%s-%s" % (c[0], c[2]) for c in CASES])
def test_pair_sets_coverage(oracle, name, seq, cond, dense):
    P = _matrix(oracle, seq, cond)
    sets = pair_probe.pair_sets(seq, P, K_SETS, PER_SET)
    assert len(sets) == K_SETS and all(len(s) <= PER_SET for s in sets)
    chosen = [c for s in sets for c in s]
    assert len(set(chosen)) == len(chosen)
    assert all(0 <= i < j < len(seq) for i, j in chosen)
    cov = pair_probe.coverage(seq, P, sets)
    print(name, cond, cov)
    assert cov["p1e3"] >= 50, cov
    assert cov["p1e6"] >= 120, cov
    assert cov["empty_bands"] == [], cov
    assert cov["zeros"] >= 3, cov
    for i, j in pair_probe.zero_pairs(seq):
        assert P[i][j] == 0.0 and (i, j) in chosen
    assert any(not pair_probe.can_pair(seq, i, j) for i, j in chosen)
    assert {1, 3} <= {j - i for i, j in chosen}
    if dense:
        assert cov["rank64"] >= 16, cov
        if len(seq) >= 150:
            assert cov["rank128"] >= 8, cov
    # every set holds some of each kind
    for s in sets:
        c1 = pair_probe.coverage(seq, P, [s])
        assert c1["p1e3"] >= 50 // K_SETS and c1["zeros"] >= 1, c1
        if dense:
            assert c1["rank64"] >= 16 // K_SETS, c1


def test_rank_is_the_compacted_index():
    seq = "GAUC" * 3
    # diagonal 5: cells (i, i + 5), pairable where the bases pair
    cells = [i for i in range(len(seq) - 5) if pair_probe.can_pair(seq, i, i + 5)]
    for r, i in enumerate(cells):
        assert pair_probe.rank(seq, i, i + 5) == r
    dense = "GUGC" * 38
    assert max(pair_probe.rank(dense, i, i + 5) for i in range(len(dense) - 5)) >= 64


def _terms_of(P, pairs, favourable):
    return [(math.log(P[i][j]) if P[i][j] > 0.0 else -math.inf) if f else math.log1p(-P[i][j])
            for (i, j), f in zip(pairs, favourable)]


def test_check_terms(oracle):
    seq = pair_probe.synthetic_anchor(60)
    P = _matrix(oracle, seq, "apo")
    pairs = pair_probe.pair_sets(seq, P, 1, 40)[0]
    fav = [k % 5 != 2 for k in range(len(pairs))]
    # and one pair below the floor of the relative bound
    pairs.append(next((i, j) for i in range(60) for j in range(i + 4, 60) if 0.0 < P[i][j] < REL_FLOOR))
    fav.append(True)
    tv = _terms_of(P, pairs, fav)
    n_rel, n_abs, n_zero, worst = pair_probe.check_terms(tv, P, pairs, fav)
    assert n_zero == 3 and n_rel > 20 and n_abs == len(pairs) - 3 and worst == 0.0
    # one matrix entry 3e-4 relative off: 3e-4 on ln P is inside E_TERM (3.25e-4), so
    # what catches it is the absolute bound, on a pair with P > 2/3
    k = next(k for k, (i, j) in enumerate(pairs) if fav[k] and P[i][j] > 0.7)
    Q = P.copy()
    Q[pairs[k]] *= 1.0 - 3e-4
    with pytest.raises(AssertionError, match="absolute"):
        pair_probe.check_terms(_terms_of(Q, pairs, fav), P, pairs, fav)
    # the relative bound: 0.9 of it passes, 1.1 fails where the absolute bound is far
    k = next(k for k, (i, j) in enumerate(pairs) if fav[k] and 1e-5 <= P[i][j] <= 1e-2)
    ok = list(tv)
    ok[k] += 0.9 * E_TERM
    assert pair_probe.check_terms(ok, P, pairs, fav)[3] == pytest.approx(0.9 * E_TERM)
    bad = list(tv)
    bad[k] -= 1.1 * E_TERM
    with pytest.raises(AssertionError, match="relative"):
        pair_probe.check_terms(bad, P, pairs, fav)
    # the absolute bound catches what the relative one does not look at
    unf = next(k for k in range(len(pairs)) if not fav[k] and 0.0 < P[pairs[k]] < 0.5)
    bad = list(tv)
    bad[unf] = math.log1p(-(P[pairs[unf]] + 3e-4))
    with pytest.raises(AssertionError, match="absolute"):
        pair_probe.check_terms(bad, P, pairs, fav)
    small = len(pairs) - 1
    bad = list(tv)
    bad[small] = math.log(P[pairs[small]] + 3e-4)
    with pytest.raises(AssertionError, match="absolute"):
        pair_probe.check_terms(bad, P, pairs, fav)
    bad[small] = -math.inf                    # underflow to 0 below the floor is inside the absolute bound
    pair_probe.check_terms(bad, P, pairs, fav)
    # exact zeros admit nothing else
    z = next(k for k, (i, j) in enumerate(pairs) if P[i][j] == 0.0)
    bad = list(tv)
    bad[z] = math.log(1e-30) if fav[z] else -1e-30
    with pytest.raises(AssertionError, match="exact zero"):
        pair_probe.check_terms(bad, P, pairs, fav)


def test_replay_reproduces_mc_run(oracle):
    tmpl, active = workloads.synthetic(60)
    seq = workloads.walker_sequences(tmpl, [active], 1)[0]
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    pair_terms = [("apo", ("pair", 0, 59), True, 1.0), ("holo", ("pair", 3, 56), False, 1.0)]
    for macro, start, terms in (([active], seq, workloads.default_objective()), (["." * 60], seq.upper(), pair_terms)):
        sf = oracle.ScoreFunction(terms, aptamer=m)
        ref = oracle.mc_run(sf, start, macro, oracle.thermostat("fixed", t=0.5), 5, 40, want_seqs=True)
        assert ref["rc"] == 0
        steps = list(pair_probe.replay(oracle, start, macro, ref["pos"], ref["base"], ref["outcome"]))
        assert [cur for _, _, _, cur in steps] == ref["seqs"]
        assert steps[-1][3] == ref["seq"]
        seen = {o for _, _, o, _ in steps}                # rejections and acceptances both replayed
        assert oracle.REJECT in seen and seen & {oracle.ACCEPT_WORSENED, oracle.ACCEPT_IMPROVED}, seen
        for s, prop, out, cur in steps:
            if out == oracle.ACCEPT_UNCHANGED:
                assert prop == (ref["seqs"][s - 1] if s else start)
