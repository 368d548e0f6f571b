"""Which pairs to request from the MC step's outside kernels, and how their
term values are judged (test_pair_probe.py pins this module on the CPU oracle;
test_gpu_outside_pairs.py applies it to the engine).

outside_cells_kernel and outside_ring_kernel return only the pairs the
objective names, at most OX_MAXP = 64 a fold.  pair_sets() spends that budget
on the pairs at which a wrong kernel shows: the probable ones (the relative
bound binds there), two of every band of 8 spans (every interior-loop size
block and multiloop split reaches some of them), the pairs a diagonal's
second and third lane-set finalize (compacted rank >= 64, >= 128), and a few
cells that must stay exactly zero.

check_terms() holds a term value against the oracle's FP64 matrix with the
project's own numbers: parity_bounds.close_term (|d ln P| <= 2 * 1e-4 / kT)
from REL_FLOOR up, test_gpu_bppm.py's absolute 2e-4 everywhere, equality at
exact zeros.
"""
import math

from addapt_amd import workloads
from parity_bounds import close_term

REL_FLOOR = 1e-6      # the relative bound holds from this oracle probability up
P_TOL = 2e-4          # test_gpu_bppm.py: |P_gpu - P_oracle| per pair
BAND = 8              # spans per band
SPAN_MIN = 4          # the shortest span that can pair (3 unpaired bases)
RANK_SETS = ((64, 24), (128, 12))   # (compacted rank from, pairs to take): lane-sets 2 and 3
OX_MAXP = 64          # addapt_amd/csrc/outside_common.hpp
MAX_TERMS = 64        # addapt_amd/csrc/dev_types.hpp

CANONICAL = {"AU", "UA", "GC", "CG", "GU", "UG"}

SYNTHETIC_N = (60, 100, 101, 150, 152)
DENSE = ("GUGC" * 25, "GUGC" * 37 + "GU", "GUGC" * 38)


def synthetic_anchor(N):
    tmpl, active = workloads.synthetic(N)
    return workloads.walker_sequences(tmpl, [active], 1)[0].upper()


def anchors():
    """[(name, sequence, conditions, dense)]"""
    out = [("syn%d" % N, synthetic_anchor(N), ("apo", "holo"), False) for N in SYNTHETIC_N]
    out += [("dense%d" % len(s), s, ("apo",), True) for s in DENSE]
    return out


def can_pair(seq, i, j):
    return seq[i] + seq[j] in CANONICAL


def rank(seq, i, j):
    """Rank of cell (i, j) among the cells of its diagonal that have a pair
    type, in ascending i: its index in the outside kernels' cl list."""
    d = j - i
    return sum(1 for a in range(i) if can_pair(seq, a, a + d))


def bands(N):
    """[(first span, last span)] of the bands of BAND spans from SPAN_MIN to N - 1."""
    return [(lo, min(lo + BAND - 1, N - 1)) for lo in range(SPAN_MIN, N, BAND)]


def _by_probability(P, cells):
    return sorted(cells, key=lambda c: (-P[c[0]][c[1]], c))


def zero_pairs(seq):
    """Cells whose probability is exactly 0 whatever else the sequence holds: one
    pair of bases without a pair type, one of span 1 and one of span 3."""
    N = len(seq)
    non = next((i, j) for i in range(N // 4, N) for j in range(i + 10, N) if not can_pair(seq, i, j))
    return [non, (N // 2, N // 2 + 1), (N // 3, N // 3 + 3)]


def pair_sets(seq, P, k_sets, per_set):
    """k_sets lists of at most per_set pairs (i < j, 0-based) of `seq`, chosen
    from its oracle matrix P: the most probable pairs, then per band of 8 spans
    the (up to two) most probable not yet chosen with P >= REL_FLOOR, the most
    probable of compacted rank >= 64 and >= 128 (only a dense anchor has them),
    and zero_pairs().  The reserved kinds are taken after the most probable ones
    but budgeted before them; the chosen pairs are dealt to the sets in turn, so
    every set holds some of each kind."""
    N = len(seq)
    budget = k_sets * per_set
    cells = [(i, j) for i in range(N) for j in range(i + 1, N)]
    zeros = zero_pairs(seq)
    n_rank = sum(q for _, q in RANK_SETS)
    n_top = budget - 2 * len(bands(N)) - n_rank - len(zeros)
    live = _by_probability(P, [c for c in cells if P[c[0]][c[1]] > 0.0])
    chosen = live[:max(0, n_top)]
    seen = set(chosen)

    def take(cands, n):
        got = [c for c in cands if c not in seen][:n]
        chosen.extend(got)
        seen.update(got)

    floor = [c for c in live if P[c[0]][c[1]] >= REL_FLOOR]
    for lo, hi in bands(N):
        take([c for c in floor if lo <= c[1] - c[0] <= hi], 2)
    for r0, q in RANK_SETS:
        take([c for c in floor if rank(seq, *c) >= r0], q)
    take(zeros, len(zeros))
    take(live, budget - len(chosen))        # what the reserved kinds left unused
    return [chosen[k::k_sets][:per_set] for k in range(k_sets)]


def coverage(seq, P, sets):
    """The counts test_pair_probe.py holds pair_sets() to."""
    chosen = [c for s in sets for c in s]
    p = {c: P[c[0]][c[1]] for c in chosen}
    floor = [c for c in chosen if p[c] >= REL_FLOOR]
    ranks = {c: rank(seq, *c) for c in floor}
    return dict(
        n=len(chosen),
        p1e3=sum(1 for c in chosen if p[c] >= 1e-3),
        p1e6=len(floor),
        empty_bands=[b for b in bands(len(seq)) if not any(b[0] <= c[1] - c[0] <= b[1] for c in floor)],
        rank64=sum(1 for c in floor if ranks[c] >= 64),
        rank128=sum(1 for c in floor if ranks[c] >= 128),
        zeros=sum(1 for c in chosen if p[c] == 0.0))


def check_terms(tv, P, pairs, favourable, where=""):
    """Assert the term values tv[k] of pairs[k] = (i, j) (favourable[k]: ln P,
    else ln(1 - P)) against the oracle matrix P.  Returns (terms under the
    relative bound, terms under the absolute bound, exact zeros, worst
    |d ln P| among the first)."""
    n_rel = n_abs = n_zero = 0
    worst = 0.0
    for k, (i, j) in enumerate(pairs):
        p, fav, got = float(P[i][j]), bool(favourable[k]), float(tv[k])
        at = (where, k, (i, j), "favourable" if fav else "unfavourable", got, p)
        if p == 0.0:
            assert got == (-math.inf if fav else 0.0), ("exact zero",) + at
            n_zero += 1
            continue
        gp = math.exp(got) if fav else 1.0 - math.exp(got)
        assert abs(gp - p) <= P_TOL, ("absolute",) + at
        n_abs += 1
        if fav and p >= REL_FLOOR:
            assert close_term(got, math.log(p), True), ("relative", abs(got - math.log(p))) + at
            worst = max(worst, abs(got - math.log(p)))
            n_rel += 1
    return n_rel, n_abs, n_zero, worst


def replay(oracle, start, macrostates, position, base, outcome):
    """Yield (step, proposal, outcome, sequence after the step) of one walker's
    trace (position[s], base[s], outcome[s] per step): the proposal is the
    oracle's move on the current sequence, which advances when the step was
    accepted with a changed sequence (outcomes 1 and 3)."""
    cur = start
    for s in range(len(outcome)):
        rc, prop = oracle.mutate_recursively(cur, macrostates, int(position[s]), base[s])
        assert rc == 0, (s, rc)
        if int(outcome[s]) in (oracle.ACCEPT_WORSENED, oracle.ACCEPT_IMPROVED):
            cur = prop
        yield s, prop, int(outcome[s]), cur
