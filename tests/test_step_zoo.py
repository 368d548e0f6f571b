"""The fixtures of step_zoo.py on the CPU: the templates are what their descriptions say, the
replay reproduces the oracle's trajectories step for step, and the runs test_gpu_step_zoo.py
makes (32 walkers x 40 steps, seeds 0..31, fixed T = 1e9 and T = 1.0) meet the coverage
conditions on the oracle alone -- a GPU test that covered nothing would pass for nothing.

The oracle's counts at n = 33 (flicker) / 40 (chain) / 41 (chain_in), 1280 steps a run; the
engine's traces gave the same counts on every route.  gone / back: scored proposals that
remove / restore the motif; wide: moves of >= 3 bases; outcomes: rejected, accepted worse,
unchanged (not scored), accepted better; then: rejections that a scored proposal of the same
walker follows directly.  The minimums (step_zoo.check_coverage) are asserted, not the counts:

  run                        gone back wide  outcomes              then
  flicker  mfe       T 1e9     30   23    0  [0, 602, 327, 351]       0
  flicker  mfe       T 1       98   39    0  [473, 303, 329, 175]   345
  flicker  pf        T 1e9     30   23    0  [0, 486, 327, 467]       0
  flicker  pf        T 1      146   23    0  [537, 170, 332, 241]   386
  flicker  pf, pair  T 1e9     61   36    0  [172, 438, 329, 341]   127
  flicker  pf, pair  T 1      252   22    0  [588, 193, 336, 163]   417
  chain    mfe       T 1e9      0    0  156  [0, 524, 325, 431]       0
  chain    mfe       T 1        0    0  160  [637, 124, 351, 168]   450
  chain    pf        T 1e9      0    0  156  [0, 493, 325, 462]       0
  chain    pf        T 1        0    0  157  [653, 73, 342, 212]    474
  chain    pf, pair  T 1e9      0    0  156  [0, 497, 325, 458]       0
  chain    pf, pair  T 1        0    0  157  [653, 72, 342, 213]    474
  chain_in mfe       T 1e9      0    0  156  [0, 525, 325, 430]       0
  chain_in mfe       T 1        0    0  162  [660, 113, 335, 172]   477
  chain_in pf        T 1e9      0    0  156  [0, 491, 325, 464]       0
  chain_in pf        T 1        0    0  162  [661, 60, 340, 219]    477
  chain_in pf, pair  T 1e9      0    0  156  [0, 488, 325, 467]       0
  chain_in pf, pair  T 1        0    0  162  [661, 62, 338, 219]    476

With the pair term on the motif's outer pair a proposal whose outer bases cannot pair scores
-inf and is rejected at any temperature: the 172 rejections of the hot flicker run.  Every
mutable position of chain and chain_in is scored 69 to 105 times a run.

Not guarded here: the 101-nt runs of the two ring routes (the same mutable set and move
stream, other frozen bases, so other decisions at T = 1).  The oracle takes 20 s a run there;
test_gpu_step_zoo.py asserts the same minimums on the engine's own trace, which the oracle's
replay of 4 walkers ties to the reference.  The engine's counts at 101 nt: flicker pf T 1
gone 28 back 19, rejected 348, accepted 616; flicker pf, pair T 1 gone 307 back 16, rejected
668, accepted 285; chain T 1 wide 173, rejected 710, accepted 257.
"""
import math

import pytest

import step_zoo as Z

RUNS = [(name, fold, pair, T) for name in ("flicker", "chain", "chain_in") for fold, pair in (("mfe", 0), ("pf", 0), ("pf", 1))
        for T in (Z.T_HOT, Z.T_COLD)]


def _id(r):
    return "%s-%s%s-T%g" % (r[0], r[1], "-pair" if r[2] else "", r[3])


def _run(oracle, tmpl, macros, sf, seqs, seeds, steps, T):
    return Z.oracle_runs(oracle, sf, macros, oracle.thermostat("fixed", t=T), seeds, seqs, steps)


def test_templates_are_as_described():
    for n in (Z.LENGTH["flicker"], Z.RING_LENGTH):
        tmpl, macros, o = Z.flicker(n)
        assert len(tmpl) == n and all(len(m) == n for m in macros) and Z.has_motif(tmpl, o)
        assert [i for i, c in enumerate(tmpl) if c.isupper()] == [0, 2, o, o + 2, o + 8, n - 1]
        assert Z.mutable(tmpl, macros) == [0, 2, o, o + 2, o + 8]
        assert macros == ["x" + "." * (n - 2) + "x", "(" + "." * (n - 2) + ")"]
        assert Z.THEO_FOLD[0] == "(" and Z.THEO_FOLD[2] == "." and Z.THEO_FOLD[8] == "("
        assert Z.THEO_FOLD.index(")") > 8 and Z.THEO_FOLD[26] == ")"
        seqs = Z.starts("flicker", n)
        assert [Z.has_motif(s, o) for s in seqs] == [w % 4 == 0 for w in range(Z.W)]
        assert all(sum(a != b for a, b in zip(s, tmpl)) <= 4 for s in seqs)   # 0, n - 1, 2 and one motif base
    for n in (Z.LENGTH["chain"], Z.LENGTH["chain_in"], Z.RING_LENGTH):
        tmpl, macros, o = Z.chain(n)
        a = n - 40
        assert len(tmpl) == n and o == n - 27 and tmpl[o:] == Z.APT.lower()
        assert [i for i, c in enumerate(tmpl) if c.isupper()] == list(range(a, a + 13))
        assert Z.mutable(tmpl, macros) == [a + k for k in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12)]
    assert Z.chain(40)[1] == ["((......))" + "." * 30, ".(.......)" + "." * 30]


def test_chain_moves_four_bases(oracle):
    for n in (Z.LENGTH["chain"], Z.LENGTH["chain_in"], Z.RING_LENGTH):
        tmpl, macros, _ = Z.chain(n)
        a = n - 40
        for s in Z.starts("chain", n, 4):
            for k in range(13):
                base = "ACGU"[("ACGU".index(s[a + k]) + 1) % 4]
                rc, prop = oracle.mutate_recursively(s, macros, a + k, base)
                changed = [i - a for i in range(n) if prop[i] != s[i]]
                assert rc == 0 and changed == ([0, 1, 8, 9] if k in (0, 1, 8, 9) else [k]), (n, k, changed)


@pytest.mark.parametrize("name", ["flicker", "chain", "chain_in"])
def test_replay_reproduces_the_oracle(oracle, name):
    n = Z.LENGTH[name]
    tmpl, macros, o = Z.TEMPLATES[name](n)
    sf, _ = Z.score_function(oracle, len(macros), 0, o, "mfe")
    seqs = Z.starts(name, n, 6)
    for w, ref in enumerate(_run(oracle, tmpl, macros, sf, seqs, Z.SEEDS[:6], Z.STEPS, Z.T_COLD)):
        assert ref["rc"] == 0
        steps, final = Z.replay(tmpl, macros, seqs[w], ref["pos"], ref["base"], ref["outcome"])
        after = [prop if out in (Z.ACCEPT_WORSENED, Z.ACCEPT_IMPROVED) else cur
                 for (cur, prop), out in zip(steps, ref["outcome"])]
        assert after == ref["seqs"] and final == ref["seq"], w
        assert [cur for cur, _ in steps] == [seqs[w]] + ref["seqs"][:-1], w


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_the_gpu_runs_cover_what_they_claim(oracle, run):
    name, fold, pair, T = run
    n = Z.LENGTH[name]
    tmpl, macros, o = Z.TEMPLATES[name](n)
    sf, _ = Z.score_function(oracle, len(macros), pair, o, fold)
    seqs = Z.starts(name, n)
    refs = _run(oracle, tmpl, macros, sf, seqs, Z.SEEDS, Z.STEPS, T)
    assert all(r["rc"] == 0 for r in refs)
    c = Z.census(tmpl, macros, o, seqs, [[r["pos"][s] for r in refs] for s in range(Z.STEPS)],
                 [[r["base"][s] for r in refs] for s in range(Z.STEPS)],
                 [[r["outcome"][s] for r in refs] for s in range(Z.STEPS)])
    print("STEP_ZOO", _id(run), Z.census_line(c))
    assert sum(c["outcomes"]) == Z.W * Z.STEPS
    Z.check_coverage(name, T, c)


@pytest.mark.parametrize("code", [2, 3])
def test_stuck_runs_stop_where_the_move_stream_says(oracle, code):
    """Which walker stops at which step (STUCK_FIRST), with the reference's error; the walkers
    that never draw the refused move run all 40 steps, and the first STUCK_CLEAN steps are clean."""
    n = Z.STUCK_N
    tmpl, macros, o, with_terms, fatal = Z.stuck(n, code)
    seeds, seqs = Z.STUCK_SEEDS[code], Z.stuck_starts(n, code, 8)
    assert [Z.first_fatal_pick(tmpl, macros, fatal, sd, Z.STUCK_STEPS) for sd in seeds] == Z.STUCK_FIRST[code]
    for p in Z.mutable(tmpl, macros):
        rc, _ = oracle.mutate_recursively(seqs[0], macros, p, "A")
        assert rc == (code if p in fatal else 0), (p, rc)
    sf, _ = Z.score_function(oracle, len(with_terms), 0, o, "mfe")
    for steps in (Z.STUCK_STEPS, Z.STUCK_CLEAN):
        refs = _run(oracle, tmpl, macros, sf, seqs, seeds, steps, Z.T_COLD)
        for w, r in enumerate(refs):
            first = Z.STUCK_FIRST[code][w]
            stops = first is not None and first < steps
            assert r["rc"] == (code if stops else 0), (w, r["rc"])
            assert sum(r["counters"]) == (first if stops else steps), (w, r["counters"])
            assert math.isfinite(r["score"]), (w, r["score"])
    assert min(f for f in Z.STUCK_FIRST[code] if f is not None) >= Z.STUCK_CLEAN
    assert Z.STUCK_FIRST[code][0] is None and Z.STUCK_FIRST[code][1] > Z.STUCK_FIRST[code][2]
