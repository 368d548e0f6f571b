"""The yardstick of the unpaired-region tests (unpaired_check.py) on the CPU oracle
alone: the ratio of two constrained partition functions is the enumerated
ensemble's probability that the window is all dots, and its length-1 row is
1 - sum_j of the oracle's pair probabilities."""
import random

import numpy as np
import pytest

import loop_zoo as Z
import sample_check as sc
import structure_check as stc
import unpaired_check as uc

BOUND = 1e-9


@pytest.mark.parametrize("seq,cst", uc.ENUM_CASES)
def test_brute_is_the_enumerated_probability(oracle, seq, cst):
    n = len(seq)
    dist, _ = sc.distribution(oracle, seq, cst)
    ref = uc.enumerated(dist, n, n)
    got = uc.brute(oracle, seq, cst, n)
    dev = np.abs(got - ref).max()
    print("enumeration vs constrained folds, %d nt: %.3g" % (n, dev))
    assert dev <= BOUND
    if cst:   # a window over a base the constraint forces to pair is 0, not a fold
        for i, c in enumerate(cst):
            if c in uc.FORCED:
                assert got[0, i] == 0.0


def _row1_cases(oracle):
    rng = random.Random(11)
    out = []
    for n in (40, 60):
        seq = "".join(rng.choice("ACGU") for _ in range(n))
        out.append((seq, None, None))
        out.append((seq, stc.cons(rng, seq), None))
    theo = oracle.make_motif(Z.THEO_SEQ, Z.THEO_FOLD, oracle.theo_bonus())
    out.append(("GCCACUGGGAA" + Z.THEO_SEQ + "GUAGCGUCACUG", None, theo))
    return out


def test_length_one_row_is_one_minus_the_pair_probabilities(oracle):
    for seq, cst, motif in _row1_cases(oracle):
        _, P = oracle.bppm(seq, cst, motif)
        got = uc.brute(oracle, seq, cst, 1, motif)[0]
        dev = np.abs(got - (1.0 - P.sum(axis=1))).max()
        print("length-1 row vs bppm, %d nt, %s: %.3g" % (len(seq), cst, dev))
        assert dev <= BOUND


def test_merge_and_tables():
    assert uc.merge(None, 2, 3, 5) == ".xx.."
    assert uc.merge("(...)", 2, 3, 5) == "(xx.)"
    assert uc.merge("(...)", 1, 2, 5) is None and uc.merge(".|...", 2, 2, 5) is None
    t = uc.enumerated({"..(...)": 0.25, ".......": 0.75}, 7, 3)
    assert t[0].tolist() == [1.0, 1.0, 0.75, 1.0, 1.0, 1.0, 0.75]
    assert t[2].tolist() == [0.75, 0.75, 0.75, 1.0, 0.75, 0.0, 0.0]
    assert uc.dots_table("..(...)", 3)[2].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert uc.pin("..(...)") == "xx(xxx)"
    for _, seq, st in uc.zoo(True):
        assert len(seq) == len(st) and Z.pair_table(st) is not None
