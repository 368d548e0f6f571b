"""A refold's finalize runs only the rows it rewrites (mfe_pair.hip, role F).

The multiloop table of the MFE fold is, for every cell where the split exists,

    qm(i, j) = min(split(i, j), U(i, j)),
    split(i, j) = min over k of qm(i, k - 1) + qm1(k, j),
    U(i, j) = min(qm1(i, j), [up_i >= 1] U(i + 1, j) + MLbase)

(oracle/fold.c orc_mfe_energy's fML; U is the unpaired-prefix part, kept as a
column recursion as in tests/test_qm_recursion.py).  The pair kernel used to
run every row of a span only to carry U down to the rows a refold rewrites.
It now starts the recursion one row above them, at a ghost row r*, from the
restored, final qm(r*, j) in place of U(r*, j): whatever qm(r*, j) holds beyond
U(r*, j) is a split of (r*, j), and that split plus the MLbase of the unpaired
rows below r* is a split of the row that takes it (same right part, the left
part qm one row longer).  This checks the identity cell by cell in exact
integer arithmetic (CPU, no GPU)."""
import numpy as np
import pytest

INF = 1 << 40   # impossible; sums stay exact Python integers
N = 40


def run_lengths(unp):
    """up[i] = number of consecutive positions i, i+1, ... that may stay unpaired."""
    n = len(unp)
    up = np.zeros(n + 1, dtype=np.int64)
    for i in range(n - 1, -1, -1):
        up[i] = up[i + 1] + 1 if unp[i] else 0
    return up[:n]


def add(a, b):
    return INF if a >= INF or b >= INF else a + b


def split(qm, qm1, i, j):
    """min over the split points k: both parts span at least 4."""
    best = INF
    for k in range(i + 5, j - 3):
        best = min(best, add(qm[i][k - 1], qm1[k][j]))
    return best


def fold_all_rows(qm1, up, mlbase):
    """qm and U with every row of every span computed (the recursion as stated)."""
    qm = [[INF] * (N + 2) for _ in range(N + 2)]
    U = [[INF] * (N + 2) for _ in range(N + 2)]
    for s in range(4, N):
        for i in range(1, N - s + 1):
            j = i + s
            u = qm1[i][j]
            if up[i] >= 1 and s - 1 >= 4:
                u = min(u, add(U[i + 1][j], mlbase))
            U[i][j] = u
            qm[i][j] = min(split(qm, qm1, i, j), u)
    return qm, U


def fold_window(qm1, up, mlbase, ref, rstar):
    """Rows >= rstar keep the restored qm (ref); rows below are recomputed with U
    started at the ghost row rstar from qm(rstar, j), where the span has that row."""
    qm = [[INF] * (N + 2) for _ in range(N + 2)]
    U = [[INF] * (N + 2) for _ in range(N + 2)]
    for s in range(4, N):
        rows = N - s
        for i in range(min(rows, rstar), 0, -1):
            j = i + s
            if i >= rstar:          # the ghost: no cell written, its qm stands in for U
                qm[i][j] = U[i][j] = ref[i][j]
                continue
            u = qm1[i][j]
            if up[i] >= 1 and s - 1 >= 4:
                u = min(u, add(U[i + 1][j], mlbase))
            U[i][j] = u
            qm[i][j] = min(split(qm, qm1, i, j), u)
        for i in range(rstar + 1, rows + 1):   # restored rows above the ghost (split's left parts never read them)
            qm[i][i + s] = ref[i][i + s]
    return qm, U


def tables(seed):
    rng = np.random.default_rng(seed)
    unp = rng.random(N + 2) > (0.0 if seed == 0 else 0.25)   # seed 0: unconstrained
    up = run_lengths(unp)
    q = rng.integers(-300, 900, size=(N + 2, N + 2))
    imp = rng.random((N + 2, N + 2)) < 0.5                   # half the entries impossible
    qm1 = [[INF if imp[i, j] else int(q[i, j]) for j in range(N + 2)] for i in range(N + 2)]
    return qm1, up


# r* = 36 is the last row of the shortest span (N - 4) and the last row of span
# N - r* for every smaller r*; 37 and 45 lie beyond every span (no ghost at all)
@pytest.mark.parametrize("rstar", [3, 7, 15, 28, 36, 37, 45])
@pytest.mark.parametrize("mlbase", [0, 7, 39])
def test_ghost_row_qm_equals_all_rows(rstar, mlbase):
    lower = 0   # cells where the ghost's qm is below the U it replaces
    for seed in range(8):
        qm1, up = tables(seed)
        ref, Uref = fold_all_rows(qm1, up, mlbase)
        got, Ugot = fold_window(qm1, up, mlbase, ref, rstar)
        for s in range(4, N):
            for i in range(1, N - s + 1):
                assert got[i][i + s] == ref[i][i + s], (seed, rstar, mlbase, i, i + s)
            if rstar <= N - s:
                lower += ref[rstar][rstar + s] < Uref[rstar][rstar + s]
    if rstar <= N - 9:   # spans with a split have the row: the replacement is not trivially U itself
        assert lower > 0
