"""The sampling yardstick (sample_check.py) on the CPU oracle alone: exact
multinomial draws from the enumerated Boltzmann distribution stay within the
bound, a biased sampler does not, and the pair helpers read structures right."""
import numpy as np
import pytest

from sample_check import bound, distribution, frequency_violations, pair_frequencies, pair_violations, within
from test_oracle_enum import SEQS

CASES = [(s, None) for s in SEQS] + [("ACGUGAAAACGU", "xxxx........"), ("GCGCUUCGGCGC", "..|........."),
                                     ("GGACUUCGGUCC", "(..........)"), ("GCGCUUCGGCGC", "....xxxx....")]
S = 20000


def _draw(rng, dist, weights=None):
    names = sorted(dist)
    p = np.array([dist[s] for s in names]) if weights is None else weights
    counts = rng.multinomial(S, p / p.sum())
    return [s for s, n in zip(names, counts) for _ in range(n)], names


@pytest.mark.parametrize("seq,cst", CASES)
def test_exact_draws_stay_within_the_bound(oracle, seq, cst):
    dist, _ = distribution(oracle, seq, cst)
    assert abs(sum(dist.values()) - 1.0) < 1e-12
    for seed in range(50):
        samples, _ = _draw(np.random.default_rng(seed), dist)
        assert frequency_violations(samples, dist) == ([], []), (seq, cst, seed)


def test_biased_draws_do_not(oracle):
    """A sampler at twice the temperature (every weight to the power 1/2) is caught."""
    caught = 0
    for seq, cst in CASES[:4]:
        dist, _ = distribution(oracle, seq, cst)
        names = sorted(dist)
        w = np.array([dist[s] for s in names]) ** 0.5
        samples, _ = _draw(np.random.default_rng(1), dist, w)
        foreign, off = frequency_violations(samples, dist)
        assert foreign == []
        caught += bool(off)
    assert caught == 4
    dist, _ = distribution(oracle, "GGGAAACCC")
    assert frequency_violations(["...(....)"], dist)[0] == ["...(....)"]   # not a structure of the 9-mer


def test_bound_and_pairs():
    assert bound(0.0, 100) == pytest.approx(0.06) and bound(1.0, 100) == pytest.approx(0.06)
    assert bound(0.5, 10000) == pytest.approx(6 * 0.005 + 6e-4)
    assert bound(-1e-17, 100) == bound(0.0, 100) and bound(1.0 + 1e-12, 100) == bound(1.0, 100)
    assert within(0.53, 0.5, 10000) and not within(0.54, 0.5, 10000)
    seq = "GGGAAACCC"
    f, bad = pair_frequencies(["(((...)))", "((.....))", ".........", "(((...)))"], seq)
    assert bad == [] and f[0, 8] == 0.75 and f[2, 6] == 0.5 and f[1, 7] == 0.75 and f.sum() == 2.0
    _, bad = pair_frequencies(["(((..))).", "...(....)", ")(......."], seq)
    assert sorted(bad) == sorted(["(((..))).", "...(....)", ")(......."])   # hairpin of 2, an A-C pair, unbalanced
    P = np.zeros((9, 9))
    P[0, 8] = 0.75
    v = pair_violations(f, P, 4)
    assert v == []   # S = 4: the floor 6 / S covers everything
    v = pair_violations(f, P, 4000)
    assert sorted((i, j) for i, j, _, _ in v) == [(1, 7), (2, 6)]
