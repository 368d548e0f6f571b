"""Templates that take the MC step off the synthetic layout, and what a run on them covered.

workloads.synthetic(N) has one macrostate, the aptamer frozen in the middle and an enforced
helix at the two ends; every stepped GPU test but test_gpu_fold_setup.py folds it.  The
templates here (all in CONTEXTS, every macrostate with an apo and a holo term):

  flicker(n)  the aptamer in the middle, frozen but for motif indices 0 (the 5' base of the
              outer pair), 2 (unpaired) and 8 (a base of an inner pair); raw positions 0 and 2
              mutable too, and n - 1 through the second macrostate's pair (0, n - 1).  The
              motif site, found by sequence match in every fold, vanishes and comes back
              between the stored tables and the proposal.
  chain(n)    the aptamer frozen at the 3' end, the 13 bases before it mutable, n - 40 frozen
              bases before those.  Macrostate A enforces (0, 9) and (1, 8), B enforces (1, 9)
              (positions counted from the first mutable base): a move at 0 or 1 changes
              {0, 1, 8, 9}, a hull of 10 with unchanged bases inside it.  At n = 40 the hull
              starts at raw position 0 and a proposal that changes an end base folds from
              scratch (mc_step.hip propose_walker); "chain_in" is chain(41), one frozen base
              first, where the same moves refold incrementally, as they do at 101.
  stuck(n, code)   chain with a move the reference refuses: code 2, one more pair in A from
              mutable base 10 to the aptamer's frozen last base; code 3, a second pair (4, 8)
              in B and a third macrostate with (0, 4): 0-9-1-8-4-0 is an odd cycle.  No
              sequence pairs along an odd cycle, so the third macrostate carries no term.

replay() rebuilds every step's current sequence and proposal from a trace with
oracle.mutate_recursively; census() counts what the scored proposals of a run covered.
test_step_zoo.py holds the runs' parameters to the coverage conditions on the oracle alone,
test_gpu_step_zoo.py runs them on the engine."""
import os
import random
from concurrent.futures import ThreadPoolExecutor

from addapt_amd import workloads

APT = workloads.THEO_SEQ
THEO_FOLD = workloads.THEO_FOLD
CONTEXTS = [("", ""), ("GGA", "UCC")]
FLICKER_MOTIF_UP = (0, 2, 8)
CHAIN_UP = 13            # mutable bases before the aptamer
REJECT, ACCEPT_WORSENED, ACCEPT_UNCHANGED, ACCEPT_IMPROVED = range(4)

# the runs of the two test modules
W, STEPS = 32, 40
SEEDS = list(range(W))
T_HOT, T_COLD = 1e9, 1.0
LENGTH = {"flicker": 33, "chain": 40, "chain_in": 41}
RING_LENGTH = 101

# stuck: 8 walkers at n = 40; the seeds are chosen from the move stream alone (first_fatal_pick)
# so that walkers 0 and 4 never draw a refused move in 40 steps (one seed in 45 does with code 2,
# one in 7500 with code 3), walker 1 draws its first at STUCK_FIRST[code][1], later than walker 2,
# and no walker draws one in the first STUCK_CLEAN steps
STUCK_N, STUCK_STEPS = 40, 40
STUCK_SEEDS = {2: [33, 25, 5, 0, 45, 3, 4, 9], 3: [1453, 484, 6, 3, 21307, 569, 4, 5]}
STUCK_FIRST = {2: [None, 37, 6, 10, None, 25, 10, 25], 3: [None, 26, 3, 6, None, 26, 7, 9]}
STUCK_CLEAN = 3


def _frozen(rng, k):
    return [rng.choice("acgu") for _ in range(k)]


def _mark(n, pairs, other=()):
    m = ["."] * n
    for i, j in pairs:
        m[i], m[j] = "(", ")"
    for p in other:
        m[p] = "x"
    return "".join(m)


def flicker(n):
    """(template, macrostates, motif offset)"""
    o = (n - len(APT)) // 2
    assert o >= 3 and n - 1 >= o + len(APT)
    s = _frozen(random.Random(3300 + n), n)
    for k, c in enumerate(APT):
        s[o + k] = c if k in FLICKER_MOTIF_UP else c.lower()
    s[0], s[2] = s[0].upper(), s[2].upper()
    s[n - 1] = workloads.COMP[s[0]]
    return "".join(s), [_mark(n, [], (0, n - 1)), _mark(n, [(0, n - 1)])], o


def _chain_template(n):
    lead = n - CHAIN_UP - len(APT)
    assert lead >= 0
    rng = random.Random(4000 + n)
    s = _frozen(rng, lead) + [c.upper() for c in _frozen(rng, CHAIN_UP)] + list(APT.lower())
    s[lead + 9] = workloads.COMP[s[lead]]
    s[lead + 1], s[lead + 8] = s[lead], s[lead + 9]
    return s, lead


def chain(n):
    """(template, macrostates, motif offset)"""
    s, a = _chain_template(n)
    return "".join(s), [_mark(n, [(a, a + 9), (a + 1, a + 8)]), _mark(n, [(a + 1, a + 9)])], n - len(APT)


def stuck(n, code):
    """(template, macrostates, motif offset, macrostates that carry terms, refused raw positions)"""
    s, a = _chain_template(n)
    if code == 2:   # 10 pairs with the aptamer's last base, c: G in every start (stuck_starts)
        s[a + 10] = "G"
        macros = [_mark(n, [(a, a + 9), (a + 1, a + 8), (a + 10, n - 1)]), _mark(n, [(a + 1, a + 9)])]
        return "".join(s), macros, n - len(APT), [0, 1], [a + 10]
    assert code == 3
    s[a + 4] = s[a]
    macros = [_mark(n, [(a, a + 9), (a + 1, a + 8)]), _mark(n, [(a + 1, a + 9), (a + 4, a + 8)]),
              _mark(n, [(a, a + 4)])]
    return "".join(s), macros, n - len(APT), [0, 1], [a, a + 1]


def stuck_starts(n, code, count):
    """Starts that every macrostate with a term can fold: the chain's, with the base the refused
    move would change left as the template has it.  The chain's macrostates, not stuck's:
    walker_sequences writes complements on every partner, and stuck's extra pairs would have it
    overwrite the frozen base (code 2) or contradict itself along the odd cycle (code 3)."""
    tmpl = stuck(n, code)[0]
    a = n - CHAIN_UP - len(APT)
    out = []
    for s in workloads.walker_sequences(tmpl, chain(n)[1], count):
        s = list(s)
        if code == 2:
            s[a + 10] = "G"
        else:
            s[a + 4] = s[a]
        out.append("".join(s))
    return out


def objective(n_macros, pair, o):
    """apo and holo of every macrostate, favourable; with pair terms one holo term on the motif's outer pair"""
    terms = [(cond, k, True, 1.0) for k in range(n_macros) for cond in ("apo", "holo")]
    if pair:
        terms.append(("holo", ("pair", o, o + len(APT) - 1), True, 1.0))
    return terms


def score_function(oracle, n_macros, pair, o, fold):
    """(the oracle's ScoreFunction of objective(), the terms)"""
    terms = objective(n_macros, pair, o)
    m = oracle.make_motif(APT, THEO_FOLD, oracle.theo_bonus())
    return oracle.ScoreFunction(terms, aptamer=m, contexts=CONTEXTS, mode=fold), terms


def oracle_runs(oracle, sf, macros, therm, seeds, seqs, steps, forced=None, tie_eps=0.0):
    """oracle.mc_run of every walker (want_seqs; forced[w]: the outcomes to take at near-ties), a few
    at a time: the library call releases the interpreter lock"""
    def one(w):
        return oracle.mc_run(sf, seqs[w], macros, therm, seeds[w], steps, forced=forced[w] if forced else None,
                             tie_eps=tie_eps, want_seqs=True)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(one, range(len(seeds))))


def starts(name, n, count=W):
    """chain: workloads.walker_sequences.  flicker: every fourth walker starts from the template
    (the motif present), the others from workloads.walker_sequences with two of the motif's three
    mutable bases put back, so that the motif is one move away.  With fully random motif bases
    and half the walkers on the template, the 101-nt run with a pair term at T = 1.0 proposed
    the motif's return 9 times in 1280 steps, with any frozen bases: there a walker that has lost
    the motif moves little, and one that has it back keeps it."""
    tmpl, macros, o = TEMPLATES[name](n)
    seqs = workloads.walker_sequences(tmpl, macros, count)
    if name != "flicker":
        return seqs
    for w in range(count):
        s, off = list(seqs[w]), FLICKER_MOTIF_UP[(w // 4) % 3]
        for k in FLICKER_MOTIF_UP:
            if k != off:
                s[o + k] = APT[k]
            elif s[o + k] == APT[k]:
                s[o + k] = "ACGU"[("ACGU".index(APT[k]) + 1 + w % 3) % 4]
        seqs[w] = tmpl if w % 4 == 0 else "".join(s)
    return seqs


TEMPLATES = {"flicker": flicker, "chain": chain, "chain_in": chain}


def mutable(template, macrostates):
    """The positions a move can pick (can_be_freely_mutated)"""
    return [i for i, c in enumerate(template) if c.isupper() and all(m[i] != ")" for m in macrostates)]


def first_fatal_pick(template, macrostates, fatal, seed, steps):
    """The first step at which stream A of `seed` picks a position of `fatal`, or None: the move
    stream's draws do not depend on a score"""
    mut = mutable(template, macrostates)
    g = workloads.MT19937(seed)
    for s in range(steps):
        pos = mut[g.uniform_int(0, len(mut) - 1)]
        g.uniform_int(0, 3)
        if pos in fatal:
            return s
    return None


def has_motif(seq, o):
    return seq[o:o + len(APT)].upper() == APT


def replay(template, macrostates, seq0, positions, bases, outcomes):
    """(steps, final): per step the walker's (current sequence, proposal) before the decision,
    rebuilt from its trace with oracle.mutate_recursively; final: the sequence after the last"""
    from oracle import oracle as O

    assert len(seq0) == len(template) and [c.isupper() for c in seq0] == [c.isupper() for c in template]
    cur, out = seq0, []
    for pos, base, outcome in zip(positions, bases, outcomes):
        rc, prop = O.mutate_recursively(cur, macrostates, int(pos), base)
        assert rc == 0, (pos, base, rc)
        assert (prop == cur) == (outcome == ACCEPT_UNCHANGED), (cur, prop, outcome)
        out.append((cur, prop))
        if outcome in (ACCEPT_WORSENED, ACCEPT_IMPROVED):
            cur = prop
    return out, cur


def census(template, macrostates, o, seqs0, positions, bases, outcomes):
    """What the scored proposals (outcome not ACCEPT_UNCHANGED) of a run covered.  positions and
    outcomes are indexed [step][walker], bases [step * W + walker] or [step][walker], as the
    engine's trace.  A dict: gone / back (the motif present in the current sequence and absent
    in the proposal, and the reverse), wide (moves of >= 3 changed bases), outcomes (4 counts),
    scored (per mutable position), rej_then_scored (rejections that a scored proposal of the
    same walker follows directly), unscored_positions."""
    nw, ns = len(seqs0), len(positions)
    c = dict(gone=0, back=0, wide=0, outcomes=[0, 0, 0, 0], scored={p: 0 for p in mutable(template, macrostates)},
             rej_then_scored=0)
    for w in range(nw):
        pos = [int(positions[s][w]) for s in range(ns)]
        out = [int(outcomes[s][w]) for s in range(ns)]
        bs = [bases[s * nw + w] if isinstance(bases, str) else bases[s][w] for s in range(ns)]
        steps, _ = replay(template, macrostates, seqs0[w], pos, bs, out)
        for s, (cur, prop) in enumerate(steps):
            c["outcomes"][out[s]] += 1
            if out[s] == ACCEPT_UNCHANGED:
                continue
            c["scored"][pos[s]] += 1
            c["gone"] += has_motif(cur, o) and not has_motif(prop, o)
            c["back"] += has_motif(prop, o) and not has_motif(cur, o)
            c["wide"] += sum(a != b for a, b in zip(cur, prop)) >= 3
            c["rej_then_scored"] += s > 0 and out[s - 1] == REJECT
    c["unscored_positions"] = sorted(p for p, k in c["scored"].items() if k == 0)
    return c


def check_coverage(name, temperature, c):
    """The coverage conditions of a W x STEPS run (the minimums leave the oracle's counts,
    test_step_zoo.py's docstring, a factor of two)"""
    if name == "flicker":
        assert c["gone"] >= 10 and c["back"] >= 10, c
    if name in ("chain", "chain_in"):
        assert c["wide"] >= 50 and not c["unscored_positions"], c
    if temperature == T_COLD:
        acc = c["outcomes"][ACCEPT_WORSENED] + c["outcomes"][ACCEPT_IMPROVED]
        assert c["outcomes"][REJECT] >= 100 and acc >= 100 and c["rej_then_scored"] >= 50, c


def census_line(c):
    return "gone %d back %d wide %d outcomes %s rejected-then-scored %d scored per position %s" % (
        c["gone"], c["back"], c["wide"], c["outcomes"], c["rej_then_scored"], sorted(c["scored"].items()))
