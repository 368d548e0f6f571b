"""The MFE structure yardstick (structure_check.py) on the CPU oracle's own
structures: a right structure passes, one with a pair removed does not."""
import random

import pytest

from structure_check import check, cons, pin, rand_seq, same_energy, satisfies


def _cases():
    rng = random.Random(41)
    out = []
    for n in (20, 37, 64, 100):
        for _ in range(3):
            s = rand_seq(rng, n)
            out.append((s, None))
            out.append((s, cons(rng, s)))
    return out


def test_oracle_structures_pass(oracle):
    for seq, cst in _cases():
        e, s = oracle.mfe(seq, cst)
        assert same_energy(e, oracle.mfe_energy(seq, cst)), (seq, cst)
        check(oracle, seq, s, e, cst)


def test_altered_structure_fails(oracle):
    tried = 0
    for seq, cst in _cases():
        e, s = oracle.mfe(seq, cst)
        if "(" not in s or e >= 0:
            continue
        # drop the innermost pair of the first hairpin: a stack or loop closing is lost
        b = s.index(")")
        a = s.rindex("(", 0, b)
        t = s[:a] + "." + s[a + 1:b] + "." + s[b + 1:]
        assert satisfies(t, None)
        if satisfies(t, cst) and same_energy(oracle.mfe_energy(seq, pin(t)), e):
            continue   # a co-optimal neighbour is a right answer too
        with pytest.raises(AssertionError):
            check(oracle, seq, t, e, cst)
        tried += 1
    assert tried >= 10


def test_satisfies():
    assert satisfies("((..))", "(....)")
    assert satisfies("((..))", None)
    assert not satisfies("((..))", "(...).")
    assert not satisfies("((..))", ".x....")
    assert not satisfies("((..)", None)
    assert not satisfies(")(..()", None)
    assert pin("(.)") == "(x)"
