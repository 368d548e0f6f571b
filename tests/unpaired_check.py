"""What the unpaired-region calls must return, from the CPU oracle alone;
test_unpaired_check.py pins it on the enumerated ensemble, test_pf_access_core.py
(the per-lane code on the host) and test_gpu_unpaired.py (the kernel) apply it.

P_u(i, j) is the ratio of two partition functions: the fold's own, and the fold
whose constraint has 'x' over i..j,

    P_u(i, j) = exp(-(G_x - G) / kT),   G = oracle.pf_energy(seq, cst, motif)

0 where the constraint forces a base of the window to pair."""
import math

import numpy as np

import loop_zoo as Z

FORCED = "|<>()"

# the enumeration cases: (sequence, constraint or None)
ENUM_CASES = [
    ("GGGUGAAAGCUAGCGAAAGUCC", None),
    ("GGGUGAAAACUAGUGAAAGCCC", "(...|...........|....)"),
    ("GCGCUUCGGCGC", "....xxxx...."),
    ("GGACUUCGGUCCAAGGACUUCG", None),
]


def merge(cst, i, j, n):
    """The constraint with 'x' over i..j (1-based, inclusive), or None where it forces a base of the window to pair."""
    cst = cst or "." * n
    if any(c in FORCED for c in cst[i - 1:j]):
        return None
    return cst[:i - 1] + "x" * (j - i + 1) + cst[j:]


def window(oracle, seq, cst, i, j, motif=None, g=None):
    """P_u(i, j), 1-based inclusive; g: the fold's own energy when the caller has it.  NaN: the constraint admits nothing."""
    g = oracle.pf_energy(seq, cst, motif) if g is None else g
    if math.isinf(g) or math.isnan(g):
        return float("nan")
    m = merge(cst, i, j, len(seq))
    if m is None:
        return 0.0
    gx = oracle.pf_energy(seq, m, motif)
    return 0.0 if math.isinf(gx) else math.exp(-(gx - g) / oracle.KT_KCAL)


def brute(oracle, seq, cst, max_len, motif=None):
    """[max_len][L]: row u-1, column i-1 holds the window of length u starting at i; columns past L-u are 0."""
    n = len(seq)
    g = oracle.pf_energy(seq, cst, motif)
    out = np.zeros((max_len, n))
    for u in range(1, max_len + 1):
        for i in range(1, n - u + 2):
            out[u - 1, i - 1] = window(oracle, seq, cst, i, i + u - 1, motif, g)
    return out


def enumerated(dist, n, max_len):
    """The same table from sample_check.distribution's {structure: probability}."""
    out = np.zeros((max_len, n))
    for s, p in dist.items():
        run = 0   # the run of dots ending at k
        for k, c in enumerate(s):
            run = run + 1 if c == "." else 0
            for u in range(1, min(run, max_len) + 1):
                out[u - 1, k - u + 1] += p
    return out


def dots_table(st, max_len):
    """1 where the window is all dots in st, else 0, in brute's layout."""
    n = len(st)
    out = np.zeros((max_len, n))
    for u in range(1, max_len + 1):
        for i in range(0, n - u + 1):
            out[u - 1, i] = 1.0 if st[i:i + u] == "." * u else 0.0
    return out


def pin(st):
    """A constraint that admits st alone: its pairs enforced, every other base 'x'."""
    return st.replace(".", "x")


def zoo(wide=False):
    """(name, sequence, structure): the loop kinds a window can lie in, built by
    loop_zoo and pinned one structure at a time; wide: a 30-unpaired interior loop too."""
    core = Z.hairpin(4)
    sts = [
        ("hairpin", Z.pad(Z.hairpin(5), 15, 2)),
        ("bulge5", Z.chain([(2, 0)], core)),
        ("bulge3", Z.pad(Z.chain([(0, 1)], core), 18, 0)),
        ("int11", Z.chain([(1, 1)], core)),
        ("int15", Z.chain([(15, 15)], core)),
        ("multi", Z.multiloop(2, 3)),                                  # a leading, a middle and a trailing run
        ("multi3", Z.pad(Z.multiloop(3, 1, Z.chain([(2, 3)], core)), 70, 1)),
        ("ends", Z.pad(Z.hairpin(3) + ".." + Z.hairpin(6), 28, 2)),    # exterior runs at both ends and between
    ]
    if wide:
        sts.append(("int30", Z.pad(Z.chain([(17, 13)], core), 50, 2)))
    return [(name, Z.default_seq(st), st) for name, st in sts]
