"""The MC step's refolds on the templates of step_zoo.py, on every kernel route of
test_gpu_fold_setup.py: a motif site that vanishes and comes back between the stored tables
and the proposal (flicker), four-base moves over a hull of 10 (chain), hot runs (every finite
proposal accepted) and runs at T = 1.0 (rejections: the next refold starts from the current
slot, not from the rejected proposal's), lengths 33 and 40 (101 on the ring routes).

Per case one engine and one traced run of 32 walkers x 40 steps (step_zoo.W, STEPS, SEEDS):

  1. every scored proposal and every current score of the trace equals, bit for bit, the score
     a second engine of the same description gives the replayed sequence from scratch
     (walkers_init folds with the step's own kernels): 1280 proposals a run, the rejected and
     the overwritten ones included ("Step zoo")
  2. the final state: stored scores == rescore(), downloaded sequences == the replay's, frozen
     bases unchanged, enforced partners complementary
  3. 8 walkers (4 at 101 nt) replayed by the oracle with the outcomes forced at near-ties:
     positions, bases, outcomes and thresholds exact, proposed scores to 1e-12 relative (MFE)
     or within parity_bounds.close_score (PF)
  4. the coverage conditions of test_step_zoo.py, recomputed from the engine's own trace

and further: the moves the reference refuses (stuck: EMOVE, the walker and the text, the
counters of the stopped and of the other walkers), and 700 annealing steps of flicker(33)
against the oracle, past the third twist of the move stream and the second of the
acceptance stream.

Every route is bit-identical in 1.: no route is compared through parity_bounds there.

chain_in is chain(41): at n = 40 the four-base move's hull starts at raw position 0, and a
proposal that changes an end base folds from scratch (mc_step.hip propose_walker); one frozen
base first, the same moves refold incrementally, as they do at 101 nt.

What 3. found: the engine summed a score flat over contexts x terms, the reference sums each
context's terms and then the contexts (scoring.cc evaluate / evaluate_terms).  The last bit
differs, and when a move leaves an MFE score where it was (whole-dcal energies: other terms,
the same total) it decides between ACCEPT_IMPROVED and ACCEPT_WORSENED: flicker hot and chain
at T = 1 each had one walker's counters off by one.  Fixed in combine.hpp (ContextSum),
dispatch.hip combine_kernel and fold_rows.hip combine_score; a single context sums as before.

Measured on an MI355X, oracle included: the module's 62 cases take 25 s; a 33 / 40 / 41-nt case
0.1 to 0.35 s, a 101-nt case 1.4 to 2.4 s (the slowest: pf, pair term, flicker, T = 1), the
700-step runs 0.6 and 0.8 s.
"""
import math

import numpy as np
import pytest

import step_zoo as Z
import test_gpu_dispatch as dispatch
from parity_bounds import close_score
from test_gpu_fold_setup import ROUTES, _names
from test_setup_core import MOVE_TEXT

pytestmark = pytest.mark.gpu

# chain_in is chain one base in (step_zoo.py): at 101 nt chain itself is
CASES = [(r, name, T) for r in ROUTES for name in ("flicker", "chain", "chain_in")[:3 if r[2] <= 100 else 2]
         for T in (Z.T_HOT, Z.T_COLD)]
ORACLE_WALKERS = {False: [0, 1, 6, 11, 16, 21, 26, 31], True: [0, 1, 12, 27]}   # ring lengths: 4


def _id(c):
    (fold, pair, rn, env), name, T = c
    return "%s-%s-%d%s-%s-T%g" % (fold, "pair" if pair else "nopair", rn,
                                  "".join("-%s=%s" % kv for kv in sorted(env.items())), name, T)


def _set_env(monkeypatch, env):
    for k in dispatch.ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _engine(native, tmpl, macros, terms, fold, thermostat):
    apt = (Z.APT, Z.THEO_FOLD, native.theo_energy())
    return native.Engine(tmpl, macros, terms, aptamer=apt, contexts=Z.CONTEXTS, fold_mode=fold, thermostat=thermostat)


def _same(a, b):
    """float64 ==, and NaN for NaN"""
    return a == b or (math.isnan(a) and math.isnan(b))


def _close_mfe(a, b):
    if math.isinf(b) or math.isnan(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


def _accepted(outcome):
    return outcome in (Z.ACCEPT_WORSENED, Z.ACCEPT_IMPROVED)


def _against_oracle(oracle, tr, W, walkers, refs, fold, terms, final, counters, where):
    """3.: positions, bases, outcomes, thresholds exact; proposed scores within the project's bounds"""
    for w, ref in zip(walkers, refs):
        assert ref["rc"] == 0, (where, w)
        assert list(tr["position"][:, w]) == ref["pos"], (where, w)
        assert tr["base"][w::W] == ref["base"], (where, w)
        assert list(tr["outcome"][:, w]) == ref["outcome"], (where, w)
        for s in range(len(ref["pos"])):
            if ref["outcome"][s] != Z.ACCEPT_UNCHANGED:
                a, b = tr["proposed_score"][s, w], ref["proposed_score"][s]
                ok = _close_mfe(a, b) if fold == "mfe" else close_score(a, b, tr["term_values"][s, w], terms)
                assert ok, (where, w, s, a, b)
                assert tr["random_threshold"][s, w] == ref["random_threshold"][s], (where, w, s)
        assert final[w].upper() == ref["seq"].upper(), (where, w)
        assert list(counters[w]) == ref["counters"], (where, w)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_proposal_on_every_route(native, oracle, monkeypatch, case):
    (fold, pair, rn, env), name, T = case
    _set_env(monkeypatch, env)
    ring = rn > 100
    n = Z.RING_LENGTH if ring else Z.LENGTH[name]
    W, S = Z.W, Z.STEPS
    tmpl, macros, o = Z.TEMPLATES[name](n)
    terms = Z.objective(len(macros), pair, o)
    eng = _engine(native, tmpl, macros, terms, fold, native.make_thermostat("fixed", t=T))
    seqs = Z.starts(name, n)
    eng.walkers_init(Z.SEEDS, seqs)
    tr = eng.run_steps(S, trace=True)
    names = tuple(eng.last_kernel_names())
    final, scores, counters = eng.download()
    fresh, _ = eng.rescore()
    out = tr["outcome"]
    rep = [Z.replay(tmpl, macros, seqs[w], tr["position"][:, w], tr["base"][w::W], out[:, w]) for w in range(W)]
    c = Z.census(tmpl, macros, o, seqs, tr["position"], tr["base"], out)
    # 1. from scratch, on a second engine: the proposals of step s, then the sequences after its decisions
    eng2 = _engine(native, tmpl, macros, terms, fold, native.make_thermostat("fixed", t=T))
    bad = []
    for s in range(S):
        props = [rep[w][0][s][1] for w in range(W)]
        after = [rep[w][0][s][1] if _accepted(out[s, w]) else rep[w][0][s][0] for w in range(W)]
        eng2.walkers_init([0] * (2 * W), props + after)
        _, ref, _ = eng2.download()
        for w in range(W):
            cur, prop = rep[w][0][s]
            diff = [i for i in range(n) if cur[i] != prop[i]]
            what = (s, w, int(out[s, w]), diff, "motif %d->%d" % (Z.has_motif(cur, o), Z.has_motif(prop, o)))
            if out[s, w] != Z.ACCEPT_UNCHANGED and not _same(tr["proposed_score"][s, w], ref[w]):
                bad.append(("proposed",) + what + (tr["proposed_score"][s, w], ref[w]))
            if not _same(tr["current_score"][s, w], ref[W + w]):
                bad.append(("current",) + what + (tr["current_score"][s, w], ref[W + w]))
    # every figure before the first assertion
    print("STEP_ZOO", _id(case), Z.census_line(c), "| scores off", len(bad), "the first", bad[:6],
          "| non-finite proposals", int((~np.isfinite(tr["proposed_score"][out != Z.ACCEPT_UNCHANGED])).sum()))
    assert names == _names(fold, pair, env, n)
    assert not bad, "%d scores differ from a from-scratch fold, the first: %r" % (len(bad), bad[:6])
    # 2. the final state
    assert all(_same(a, b) for a, b in zip(scores, fresh)), [(w, scores[w], fresh[w]) for w in range(W)
                                                              if not _same(scores[w], fresh[w])]
    assert all(_same(a, b) for a, b in zip(scores, tr["current_score"][S - 1]))
    assert (counters.sum(axis=1) == S).all()
    for w in range(W):
        assert final[w].upper() == rep[w][1].upper(), w
        assert all(final[w][i] == ch for i, ch in enumerate(tmpl) if ch.islower()), (w, final[w])
        for m in macros:
            stk = []
            for i, ch in enumerate(m):
                if ch == "(":
                    stk.append(i)
                elif ch == ")":
                    assert final[w][i].upper() == Z.workloads.COMP[final[w][stk.pop()].upper()], (w, m, i, final[w])
    # 3. the oracle
    walkers = ORACLE_WALKERS[ring]
    sf, _ = Z.score_function(oracle, len(macros), pair, o, fold)
    refs = Z.oracle_runs(oracle, sf, macros, oracle.thermostat("fixed", t=T), [Z.SEEDS[w] for w in walkers],
                         [seqs[w] for w in walkers], S, forced=[[int(x) for x in out[:, w]] for w in walkers],
                         tie_eps=1e-12 if fold == "mfe" else 1e-6)
    _against_oracle(oracle, tr, W, walkers, refs, fold, terms, final, counters, _id(case))
    # 4. the run covered what it is here for
    assert sum(c["outcomes"]) == W * S
    Z.check_coverage(name, T, c)


@pytest.mark.parametrize("fold", ["mfe", "pf"])
@pytest.mark.parametrize("code", [2, 3])
def test_refused_moves(native, oracle, monkeypatch, fold, code):
    """clo_err -> st.err -> ADX_EMOVE: the run reports the lowest-index walker that drew a refused
    move, with the reference's text; that walker stopped counting at its refused step (the
    reference's exception leaves the earlier steps counted; accept_walker and propose_walker
    return early on err), the walkers that drew none ran on.  The first STUCK_CLEAN steps, which
    no walker's move stream refuses, raise nothing and are the oracle's."""
    _set_env(monkeypatch, {})
    n, S = Z.STUCK_N, Z.STUCK_STEPS
    tmpl, macros, o, with_terms, _ = Z.stuck(n, code)
    terms = Z.objective(len(with_terms), 0, o)
    seeds, seqs = Z.STUCK_SEEDS[code], Z.stuck_starts(n, code, 8)
    W = len(seeds)
    sf, _ = Z.score_function(oracle, len(with_terms), 0, o, fold)
    th = oracle.thermostat("fixed", t=Z.T_COLD)
    eng = _engine(native, tmpl, macros, terms, fold, native.make_thermostat("fixed", t=Z.T_COLD))
    # the clean run
    eng.walkers_init(seeds, seqs)
    tr = eng.run_steps(Z.STUCK_CLEAN, trace=True)
    final, _, counters = eng.download()
    refs = Z.oracle_runs(oracle, sf, macros, th, seeds, seqs, Z.STUCK_CLEAN,
                         forced=[[int(x) for x in tr["outcome"][:, w]] for w in range(W)],
                         tie_eps=1e-12 if fold == "mfe" else 1e-6)
    _against_oracle(oracle, tr, W, list(range(W)), refs, fold, terms, final, counters, ("stuck", code, fold))
    # the run that stops
    refs = Z.oracle_runs(oracle, sf, macros, th, seeds, seqs, S)
    failed = [w for w in range(W) if refs[w]["rc"] != 0]
    assert failed and failed[0] > 0 and [refs[w]["rc"] for w in failed] == [code] * len(failed)
    eng.walkers_init(seeds, seqs)
    with pytest.raises(native.AdxError) as ei:
        eng.run_steps(S)
    _, _, counters = eng.download()
    print("STEP_ZOO stuck", code, fold, str(ei.value), "| steps counted", [int(x) for x in counters.sum(axis=1)],
          "oracle", [sum(r["counters"]) for r in refs])
    assert ei.value.status == native.EMOVE
    assert str(ei.value) == "adx status %d: walker %d: %s" % (native.EMOVE, failed[0], MOVE_TEXT[code])
    for w in range(W):
        first = Z.STUCK_FIRST[code][w]
        assert counters[w].sum() == sum(refs[w]["counters"]) == (S if first is None else first), (w, counters[w])
    assert sum(f is None for f in Z.STUCK_FIRST[code]) == 2


TWIST_STEPS, TWIST_W, TWIST_CYCLE = 700, 4, 100


@pytest.mark.parametrize("fold", ["mfe", "pf"])
def test_past_the_second_twist(native, oracle, monkeypatch, fold):
    """The walkers' MT19937 streams past their later twists (MtView stages a window of the state
    and writes the whole state back when it twists): the move stream draws two words a step and
    twists at steps 0, 312 and 624, the acceptance stream two words a scored step and twists again
    at each walker's own 313th scored step.  700 annealing steps (5 -> 0, cycle 100) of 4 walkers on
    flicker(33): positions, bases, outcomes, thresholds and proposed scores of every step are the
    oracle's."""
    _set_env(monkeypatch, {})
    n, S, W = Z.LENGTH["flicker"], TWIST_STEPS, TWIST_W
    tmpl, macros, o = Z.flicker(n)
    terms = Z.objective(len(macros), 0, o)
    eng = _engine(native, tmpl, macros, terms, fold,
                  native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=TWIST_CYCLE))
    seeds, seqs = Z.SEEDS[:W], Z.starts("flicker", n, W)
    eng.walkers_init(seeds, seqs)
    tr = eng.run_steps(S, trace=True)
    final, _, counters = eng.download()
    scored = (tr["outcome"] != Z.ACCEPT_UNCHANGED).sum(axis=0)
    print("STEP_ZOO twist", fold, "scored proposals per walker", [int(x) for x in scored])
    assert (scored > 312).all(), scored
    sf, _ = Z.score_function(oracle, len(macros), 0, o, fold)
    refs = Z.oracle_runs(oracle, sf, macros, oracle.thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=TWIST_CYCLE),
                         seeds, seqs, S, forced=[[int(x) for x in tr["outcome"][:, w]] for w in range(W)],
                         tie_eps=1e-12 if fold == "mfe" else 1e-6)
    _against_oracle(oracle, tr, W, list(range(W)), refs, fold, terms, final, counters, ("twist", fold))
