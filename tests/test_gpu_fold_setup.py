"""The per-fold setup every fold kernel shares (addapt_amd/csrc/fold_setup_core.hpp: the
sequence in its context, the wrap, the motif sites) on every kernel route, with the
motif site at the very ends of the fold.

Templates: the aptamer (lower case: fixed) as the first 27 bases, or as the last 27, of a
raw length of 33 (101 on the ring routes, the shortest length those kernels take), in the
contexts ("", "") and ("GGA", "UCC"): the site starts at folded position 1, or ends at
folded N, in the first context and sits inside in the second; the mutable bases are the
other end, so the MC steps change the first or the last base.  Macrostates: free; 'x' on
two bases outside the aptamer; 'x' on the motif's first unpaired base; '|' on that base.
An 'x' on a base the motif leaves unpaired does not remove the site (the base stays
unpaired: oracle/fold.c motif_at, tests/test_fold_setup_core.py); the '|' does, so the
holo and apo energies of that macrostate coincide.  Every term is favourable (the free
macrostate has probability 1).

Per case one engine and 4 walkers: score_batch against oracle.ScoreFunction (PF within
parity_bounds, MFE to 1e-12 relative as test_gpu_parity.py / test_gpu_mfe.py), then 3 hot
MC steps (every finite proposal is accepted, so the downloaded scores are the refold
path's) and each walker's score against the oracle's score of its downloaded sequence.
The route's kernel names must be test_gpu_dispatch.py's.  On the short templates the
energies of mfe_structure_batch / sample_structures_batch equal score_batch's of the same
variant (MFE: equal; PF: within DG_TOL).

What the "last" template found: on the routes that recompute every cell's inner-pair code but
restore the cells outside a refold's band from the stored tables (mfe_cells_kernel, the rows
kernels) a change of base 1 left qbm of the cells (i, N) with the old code's mismatch (the code
reads the wrapped S[N + 1] = S[1]); the score was off by 1.6 (MFE -26.8367 against -25.2141).  A
proposal that changes an end base folds from scratch now (mc_step.hip propose_walker)."""
import math
import random

import numpy as np
import pytest

import test_gpu_dispatch as dispatch
from addapt_amd import workloads
from parity_bounds import DG_TOL, close_score, close_term

pytestmark = pytest.mark.gpu

APT = workloads.THEO_SEQ.lower()
CONTEXTS = [("", ""), ("GGA", "UCC")]
T_HOT = 1e9
FIRST_UNPAIRED = workloads.THEO_FOLD.index(".")


def template(where, n):
    """(template, macrostates, motif offset) with the aptamer first or last in n raw bases"""
    rng = random.Random(n * 7 + len(where))
    rest = "".join(rng.choice("ACGU") for _ in range(n - len(APT)))
    tmpl, o = (APT + rest, 0) if where == "first" else (rest + APT, n - len(APT))
    out = (o + len(APT), o + len(APT) + 1) if where == "first" else (o - 1, o - 2)

    def mark(c, *pos):
        m = ["."] * n
        for p in pos:
            m[p] = c
        return "".join(m)

    return tmpl, ["." * n, mark("x", *out), mark("x", o + FIRST_UNPAIRED), mark("|", o + FIRST_UNPAIRED)], o


def objective(macros, pair, o):
    terms = [(cond, k, True, 1.0) for k in range(len(macros)) for cond in ("apo", "holo")]
    if pair:   # the motif's outer pair
        terms.append(("holo", ("pair", o, o + len(APT) - 1), True, 1.0))
    return terms


def _names(fold, pair, env, n):
    """test_gpu_dispatch.py's strings for the route (its rows at 100 / 101 nt)"""
    for f, p, N, e, inside, outside in dispatch.CASES:
        if (f, p, e) == (fold, pair, env) and N == (100 if n <= 100 else 101):
            return inside, outside
    raise KeyError((fold, pair, env, n))


# (fold mode, pair terms, raw length, environment)
ROUTES = [
    ("mfe", 0, 33, {}),
    ("mfe", 0, 33, {"ADX_MFE_PAIR": "0"}),
    ("mfe", 0, 33, {"ADX_MFE_KERNEL": "rows"}),
    ("mfe", 0, 33, {"ADX_NO_MFE16": "1"}),
    ("pf", 0, 33, {}),
    ("pf", 0, 33, {"ADX_PF_KERNEL": "rows"}),
    ("pf", 0, 101, {}),
    ("pf", 1, 33, {}),
    ("pf", 1, 33, {"ADX_OUTSIDE_KERNEL": "bppm"}),
    ("pf", 1, 101, {}),
]
CASES = [r + (where,) for r in ROUTES for where in ("first", "last")]


def _id(c):
    return "%s-%s-%d%s-%s" % (c[0], "pair" if c[1] else "nopair", c[2],
                              "".join("-%s=%s" % kv for kv in sorted(c[3].items())), c[4])


def test_route_names_are_the_dispatch_table_s():
    assert _names("mfe", 0, {}, 33) == (dispatch.MFE_PAIR, "")
    assert _names("mfe", 0, {"ADX_MFE_PAIR": "0"}, 33) == (dispatch.MFE_CELLS, "")
    assert _names("mfe", 0, {"ADX_MFE_KERNEL": "rows"}, 33) == (dispatch.ROWS16, "")
    assert _names("pf", 0, {}, 33) == (dispatch.CELLS, "")
    assert _names("pf", 0, {}, 101) == (dispatch.RING, "")
    assert _names("pf", 1, {}, 33) == (dispatch.CELLS, "outside_cells_kernel")
    assert _names("pf", 1, {}, 101) == (dispatch.RING, "outside_ring_kernel")


_refs = {}


def _ref(oracle, fold, pair, n, where, seq):
    """the oracle's (score, term values) of one sequence of a case's objective: computed once, never written to"""
    key = (fold, pair, n, where, seq.upper())
    if key not in _refs:
        tmpl, macros, o = template(where, n)
        m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
        sf = oracle.ScoreFunction(objective(macros, pair, o), aptamer=m, contexts=CONTEXTS, mode=fold)
        sc, tv = sf.score(seq, macros)
        _refs[key] = (sc, tuple(tv))
    return _refs[key]


def _close_mfe(a, b):
    if math.isinf(b) or math.isnan(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


def _check(fold, terms, sc, tv, ref, tref, where):
    print("FOLD_SETUP", where, "score", sc, "oracle", ref)
    assert math.isfinite(ref), where
    if fold == "mfe":
        assert _close_mfe(sc, ref), (where, sc, ref)
        for k, (a, b) in enumerate(zip(tv, tref)):
            assert _close_mfe(a, b), (where, k, a, b)
    else:
        assert close_score(sc, ref, tref, terms), (where, sc, ref)
        for k, (a, b) in enumerate(zip(tv, tref)):
            assert close_term(a, b, terms[k % len(terms)][2]), (where, k, a, b)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_setup_on_every_route(native, oracle, monkeypatch, case):
    fold, pair, n, env, where = case
    for k in dispatch.ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tmpl, macros, o = template(where, n)
    terms = objective(macros, pair, o)
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    eng = native.Engine(tmpl, macros, terms, aptamer=apt, contexts=CONTEXTS, fold_mode=fold,
                        thermostat=native.make_thermostat("fixed", t=T_HOT))
    seqs = workloads.walker_sequences(tmpl, macros, 4)
    # 1. from scratch
    sc, tv, dg = eng.score_batch(seqs)
    for w in range(4):
        ref, tref = _ref(oracle, fold, pair, n, where, seqs[w])
        _check(fold, terms, sc[w], tv[w], ref, tref, (_id(case), "batch", w))
    # 2. after three accepted moves of the other end: the refold path
    eng.walkers_init([1, 2, 3, 4], seqs)
    eng.run_steps(3)
    assert tuple(eng.last_kernel_names()) == _names(fold, pair, env, n)
    final, scores, _ = eng.download()
    assert any(f.upper() != s.upper() for f, s in zip(final, seqs))
    for w in range(4):   # every figure before the first assertion
        print("FOLD_SETUP", _id(case), "walker", w, "first base changed", final[w][0].upper() != seqs[w][0].upper(),
              "last base changed", final[w][-1].upper() != seqs[w][-1].upper(), "score", scores[w], "oracle",
              _ref(oracle, fold, pair, n, where, final[w])[0])
    for w in range(4):
        assert final[w][o:o + len(APT)] == APT
        ref, tref = _ref(oracle, fold, pair, n, where, final[w])
        _check(fold, terms, scores[w], tref, ref, tref, (_id(case), "steps", w))
    # 3. the structure kernels fold the same variants to the same energies
    if n == 33:
        for v in range(eng.info.n_variants):
            if fold == "mfe":
                _, e = eng.mfe_structures(seqs, v)
                assert e.tobytes() == np.ascontiguousarray(dg[:, v]).tobytes(), (v, e, dg[:, v])
            else:
                _, e = eng.sample_structures(seqs, v, 1, seed=v)
                for w in range(4):
                    assert math.isfinite(dg[w, v]) and abs(e[w] - dg[w, v]) <= DG_TOL, (v, w, e[w], dg[w, v])
