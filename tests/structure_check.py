"""Yardstick of the MFE structure tests (test_structure_check.py pins it on the
CPU oracle; test_gpu_mfe_structure.py and test_host_mfe_structure_gpu.py apply
it to the engine).

A returned structure s with energy e for (seq, constraint cst, motif m) is
right when

    oracle.mfe_energy(seq, pin(s), m) == e == oracle.mfe_energy(seq, cst, m)

and satisfies(s, cst): pinning s as an all-'x' / '()' constraint leaves exactly
that structure admissible, so the oracle prices it (motif included), and it
must cost the optimum.  Co-optimal structures pass, which holo folds need: the
oracle has no holo traceback to compare strings with.
"""
import math

import numpy as np

PAIRS = {"AU", "UA", "GC", "CG", "GU", "UG"}


def pin(s):
    return s.replace(".", "x")


def pair_table(s):
    """{i: j, j: i} of a dot-bracket string, or None when it is not balanced."""
    st, pt = [], {}
    for k, c in enumerate(s):
        if c == "(":
            st.append(k)
        elif c == ")":
            if not st:
                return None
            a = st.pop()
            pt[a], pt[k] = k, a
    return None if st else pt


def satisfies(s, cst):
    """s is balanced, holds every ( ) pair of cst and leaves every x of cst unpaired."""
    pt = pair_table(s)
    if pt is None or any(c not in ".()" for c in s):
        return False
    if cst is None:
        return True
    if len(cst) != len(s):
        return False
    want = pair_table(cst)
    if want is None:
        return False
    if any(pt.get(a) != b for a, b in want.items()):
        return False
    return all(s[k] == "." for k, c in enumerate(cst) if c == "x")


def same_energy(a, b):
    """float32 equality, +inf included."""
    a, b = np.float32(a), np.float32(b)
    if math.isinf(b):
        return bool(math.isinf(a) and a > 0 and b > 0)
    return bool(a == b)


def check(oracle, seq, s, e, cst=None, motif=None):
    """Assert the energy identity and the constraint for a returned (s, e)."""
    ref = oracle.mfe_energy(seq, cst, motif)
    assert same_energy(e, ref), (seq, cst, s, e, ref)
    assert len(s) == len(seq), (seq, s)
    if math.isinf(ref):
        assert s == "." * len(seq), (seq, cst, s)
        return
    assert satisfies(s, cst), (seq, cst, s)
    priced = oracle.mfe_energy(seq, pin(s), motif)
    assert same_energy(priced, e), (seq, cst, s, e, priced)


def rand_seq(rng, n):
    return "".join(rng.choice("ACGU") for _ in range(n))


def cons(rng, seq, p_x=0.1, n_pairs=2):
    """A random constraint of x marks and up to n_pairs enforced pairs, placed
    only where the bases can pair."""
    n = len(seq)
    c = ["."] * n
    if n >= 9:
        for _ in range(n_pairs):
            for _try in range(50):
                i = rng.randrange(0, n - 8)
                j = rng.randrange(i + 5, n)
                if seq[i] + seq[j] in PAIRS and all(ch == "." for ch in c[i:j + 1]):
                    c[i], c[j] = "(", ")"
                    break
    for k in range(n):
        if c[k] == "." and rng.random() < p_x:
            c[k] = "x"
    return "".join(c)
