"""Yardstick of the ensemble-sampling tests (test_sample_check.py pins it on
the CPU oracle alone; test_gpu_pf_sample.py and test_host_pf_sample_gpu.py
apply it to the engine).

An event of reference probability p observed with frequency f over S samples
passes when

    |f - p| <= 6 sqrt(p (1 - p) / S) + 6 / S

six binomial standard deviations, plus a floor that covers the Poisson regime
p S <~ 1 where a single count is many "sigmas".  The sampler is deterministic
under a fixed seed, so a pass does not flake.
"""
import collections
import math

import numpy as np

from test_oracle_enum import KT, structures

PAIRS = {"AU", "UA", "GC", "CG", "GU", "UG"}


def bound(p, S):
    p = min(1.0, max(0.0, float(p)))   # an oracle probability may leave [0, 1] by rounding
    return 6.0 * math.sqrt(p * (1.0 - p) / S) + 6.0 / S


def within(f, p, S):
    return abs(f - p) <= bound(p, S)


def distribution(oracle, seq, cst=None):
    """{structure: exp(-E/kT)/Z} over every structure the constraint admits."""
    w = {}
    for s in structures(seq, cst):
        e = oracle.eval_structure(seq, s)
        if e < 1e6:
            w[s] = math.exp(-e / KT)
    Z = sum(w.values())
    return {s: x / Z for s, x in w.items()}, Z


def frequency_violations(samples, dist):
    """The samples outside the enumerated set, and the structures whose frequency
    misses the bound, as (structure, frequency, probability)."""
    S = len(samples)
    cnt = collections.Counter(samples)
    foreign = sorted(s for s in cnt if s not in dist)
    off = [(s, cnt[s] / S, p) for s, p in dist.items() if not within(cnt[s] / S, p, S)]
    return foreign, off


def pair_table(s):
    st, pt = [], {}
    for k, c in enumerate(s):
        if c == "(":
            st.append(k)
        elif c == ")":
            if not st:
                return None
            a = st.pop()
            pt[a] = k
    return None if st else pt


def pair_frequencies(samples, seq):
    """(L x L upper-triangular pair frequencies, the samples that are not valid
    structures of seq: unbalanced, a non-canonical pair or a hairpin below 3)."""
    L = len(seq)
    f = np.zeros((L, L))
    bad = []
    for s, n in collections.Counter(samples).items():
        pt = pair_table(s) if len(s) == L and set(s) <= set(".()") else None
        if pt is None or any(seq[a] + seq[b] not in PAIRS or b - a < 4 for a, b in pt.items()):
            bad.append(s)
            continue
        for a, b in pt.items():
            f[a, b] += n
    return f / len(samples), bad


def pair_violations(f, P, S):
    """The pairs (i, j, frequency, probability), i < j, whose frequency misses the bound."""
    L = f.shape[0]
    return [(i, j, f[i, j], P[i, j]) for i in range(L) for j in range(i + 1, L) if not within(f[i, j], P[i, j], S)]
