"""The centroid / MEA kernel's per-lane code (addapt_amd/csrc/ensemble_struct_core.hpp)
without a GPU: a stand-alone program built against the header runs the
column pass, the centroid scan, the fill and the traceback lane by lane in the
kernel's order on matrices read from stdin, and is held to ensemble_check.py's
restatement of the definitions.  The program is built once more with the
address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded).

On the same doubles the program's table is the restatement's bit for bit (no
multiply feeds an add, and pu is summed in ascending j on both sides), so mea
and every traceback winner are compared exactly; the two statistics are summed
by columns in the program and by rows here and are held to tol()."""
import math
import os
import random
import subprocess

import pytest

from ensemble_check import Mea, centroid, centroid_dist, diversity, expected_accuracy, pairs_of, tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "ensemble_struct_core_probe.cc")
GAMMAS = (0.5, 1.0, 4.0)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    out = str(tmp_path_factory.mktemp("ensemble_struct_core") / "probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", out, SRC], check=True)
    return out


def _run(exe, cases):
    """cases: (P, gamma).  Per case (centroid, mea structure, (mea, dist, diversity), [(i, j, win)])."""
    lines = [str(len(cases))]
    for P, g in cases:
        lines.append("%d %r" % (len(P), g))
        lines += [" ".join(repr(x) for x in row) for row in P]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    out, res, at = r.stdout.split("\n"), [], 0
    for _ in cases:
        n = int(out[at + 3])
        pops = [tuple(int(x) for x in l.split()) for l in out[at + 4:at + 4 + n]]
        res.append((out[at], out[at + 1], tuple(float(x) for x in out[at + 2].split()), pops))
        at += 4 + n
    return res


def _check(P, g, got):
    """Every property of one finite case."""
    cen, mea_db, (mea, dist, div), pops = got
    L, t = len(P), tol(len(P), g)
    ref_pairs, ref_cen = centroid(P)
    assert cen == ref_cen
    assert abs(dist - centroid_dist(P, ref_pairs)) <= t and abs(div - diversity(P)) <= t
    T = Mea(P, g)
    assert mea == T.mea
    pairs = pairs_of(mea_db)
    assert pairs is not None and len(mea_db) == L and all(P[i][j] > 0.0 for i, j in pairs)
    assert abs(expected_accuracy(pairs, P, g) - T.mea) <= t
    # the traceback: every interval's winner is the smallest candidate that attains the cell
    assert 1 <= len(pops) <= L
    marked = []
    for i, j, win in pops:
        assert win == min(c for c, v in T.candidates(i, j) if v == T.at(i, j)), (i, j, win)
        if win > 0:
            marked.append((i + win - 1, j))
    assert sorted(marked) == pairs


# ------------------------------------------------------------------ exact ensembles
def _structures(L, i=0):
    """Every nested structure on positions i .. L-1 (hairpins of >= 1 base), as pair tuples."""
    if i >= L:
        yield ()
        return
    yield from _structures(L, i + 1)
    for j in range(i + 2, L):
        for inner in _structures(j, i + 1):
            for rest in _structures(L, j + 1):
                yield ((i, j),) + inner + rest


def _ensemble(L, rng):
    """Random Boltzmann weights on every structure: (structures, P)."""
    S = list(_structures(L))
    w = [rng.random() ** 4 for _ in S]
    Z = math.fsum(w)
    P = [[0.0] * L for _ in range(L)]
    for s, x in zip(S, w):
        for i, j in s:
            P[i][j] += x / Z
    for i in range(L):
        for j in range(i):
            P[i][j] = P[j][i]
    return S, P


@pytest.mark.parametrize("L", [1, 4, 5, 8, 11])
def test_enumerated_ensembles(exe, L):
    rng = random.Random(100 + L)
    ens = [_ensemble(L, rng) for _ in range(3)]
    cases = [(P, g) for _, P in ens for g in GAMMAS]
    for (P, g), got, S in zip(cases, _run(exe, cases), [S for S, _ in ens for _ in GAMMAS]):
        _check(P, g, got)
        best = max(expected_accuracy(s, P, g) for s in S)   # every structure over pairs with P > 0 is in S
        assert abs(got[2][0] - best) <= tol(L, g), (L, g)
        # exact probabilities never conflict above 1/2: nothing was filtered
        assert pairs_of(got[0]) == [(i, j) for i in range(L) for j in range(i + 1, L) if P[i][j] > 0.5]


# ------------------------------------------------------------------ random sparse matrices
def _sparse(L, rng, step=None):
    """Symmetric, zero diagonal, about 4 entries per row plus a helix above 1/2;
    step quantises the values so that candidates tie."""
    P = [[0.0] * L for _ in range(L)]

    def put(i, j, x):
        if step:
            x = max(step, round(x / step) * step)
        P[i][j] = P[j][i] = x

    for _ in range(2 * L):
        i, j = sorted(rng.sample(range(L), 2))
        if j - i >= 2:
            put(i, j, rng.random() * 0.3)
    a, b = L // 5, L - 1 - L // 7
    for k in range(min(6, (b - a - 3) // 2)):
        put(a + k, b - k, 0.55 + 0.4 * rng.random())
    return P


@pytest.mark.parametrize("L", [63, 64, 65, 255])
def test_random_sparse_matrices(exe, L):
    rng = random.Random(L)
    cases = [(_sparse(L, rng), 1.0), (_sparse(L, rng), 0.5), (_sparse(L, rng, step=0.125), 4.0),
             (_sparse(L, rng, step=0.25), 1.0)]
    for (P, g), got in zip(cases, _run(exe, cases)):
        _check(P, g, got)
        assert "(" in got[0] and "(" in got[1]


def test_ties_take_the_smallest_index(exe):
    """pu = 1/2 everywhere a pair of weight 1 competes with two unpaired bases: all tie."""
    L = 12
    P = [[0.0] * L for _ in range(L)]
    for i, j in ((0, 11), (1, 10), (2, 6), (7, 9)):
        P[i][j] = P[j][i] = 0.5
    got = _run(exe, [(P, 1.0)])[0]
    _check(P, 1.0, got)
    assert got[1] == "." * L and got[2][0] == L - 4.0   # candidate 0, "j unpaired", is the smallest


# ------------------------------------------------------------------ the filter and the edges
def test_conflicting_entries_above_one_half(exe):
    L = 10
    P = [[0.0] * L for _ in range(L)]
    for i, j, x in ((1, 6, 0.7), (3, 8, 0.8), (1, 9, 0.6), (2, 5, 0.9)):   # (3, 8) crosses, (1, 9) shares a base
        P[i][j] = P[j][i] = x
    got = _run(exe, [(P, 1.0)])[0]
    assert got[0] == ".((..))..."
    assert pairs_of(got[0]) == [(1, 6), (2, 5)]
    _check(P, 1.0, got)
    assert abs(got[2][1] - (0.3 + 0.1 + 0.8 + 0.6)) <= tol(L, 1.0)


def test_nan_terminates_with_nan_statistics(exe):
    for L, at in ((9, (2, 7)), (64, (0, 63)), (255, (100, 101))):
        rng = random.Random(L)
        P = _sparse(L, rng)
        P[at[0]][at[1]] = P[at[1]][at[0]] = float("nan")
        for bad in (P, [[float("inf") if x != x else x for x in row] for row in P]):
            cen, mea_db, stats, pops = _run(exe, [(bad, 1.0)])[0]
            assert all(math.isnan(x) for x in stats)
            assert len(pops) <= 2 * L and len(cen) == L and len(mea_db) == L
            assert pairs_of(cen) is not None


def test_all_zero_matrix(exe):
    for L in (1, 2, 64, 255):
        P = [[0.0] * L for _ in range(L)]
        cen, mea_db, stats, pops = _run(exe, [(P, 1.0)])[0]
        assert cen == mea_db == "." * L and stats == (float(L), 0.0, 0.0)
        assert pops == [(0, j, 0) for j in range(L - 1, -1, -1)]
