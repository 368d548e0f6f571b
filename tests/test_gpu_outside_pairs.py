"""The MC step's outside kernels (outside_cells_kernel, outside_ring_kernel) and
their fallbacks at interior pairs, against the oracle's FP64 matrices.

The step kernels return only the pairs the objective names, so each engine here
names up to 62 of them (pair_probe.pair_sets: the probable pairs, two per band of
8 spans, compacted ranks >= 64 and >= 128 on the dense anchors, exact zeros) and
three engines cover an anchor's 186 chosen pairs.  Per engine, 4 walkers (the
anchor and 1, 2, 5 point mutations of it):

  1. from scratch: rescore() (the step's own inside + outside kernels) and
     score_batch() (bppm_kernel, verified on whole matrices by test_gpu_bppm.py)
     against oracle.bppm of each walker's sequence; a failure reports both, so
     it says which kernel is off;
  2. on stored tables: 8 (at most 16) hot MC steps; every scored proposal's term
     values against oracle.bppm of the replayed proposal, and the final
     sequences against the replay.

The bounds are pair_probe.check_terms': parity_bounds.close_term from
REL_FLOOR = 1e-6 up, |dP| <= 2e-4 everywhere, equality at exact zeros.

Measured on an MI355X: worst |d ln P| among the terms with oracle P >= 1e-6
(bound 3.245e-4), the step's kernels (from scratch and on stored tables) |
bppm_kernel (from scratch), REL_FLOOR as set:

    syn60  9.9e-07 | 5.0e-06    syn150   1.6e-06 | 5.6e-06    dense150 2.6e-06 | 1.9e-06
    syn100 1.8e-06 | 3.6e-06    syn152   2.0e-06 | 2.5e-06    dense152 2.3e-06 | 2.1e-06
    syn101 1.7e-06 | 5.4e-06    dense100 1.4e-06 | 1.7e-06    overrides, contexts <= 6.3e-06

What these checks found: a change of the first or the last base left the cells
that read it as their wrapped dangle unrefolded (test_end_base_changes); every
value of that walker's outside pass was off by up to 60 % until later moves
happened to refold those cells.
"""
import random

import numpy as np
import pytest

import pair_probe
from addapt_amd import workloads
from pair_probe import MAX_TERMS, OX_MAXP, check_terms
from parity_bounds import close_term

pytestmark = pytest.mark.gpu

K_SETS, PER_SET = 3, 62
T_HOT = 1e9           # exp(dS / T_HOT) is 1 to 1e-6 for any finite dS: every finite proposal is accepted
SEEDS = [11, 12, 13, 14]
MUTATIONS = (0, 1, 2, 5)
ENV_VARS = ("ADX_MFE_KERNEL", "ADX_MFE_PAIR", "ADX_PF_KERNEL", "ADX_OUTSIDE_KERNEL", "ADX_NO_MFE16")

CELLS = "pf_cells_kernel (scores combined in step_tail_kernel)"
RING = "pf_ring_kernel (scores combined in step_tail_kernel)"
ROWS2 = "score_kernel<768, 2, SumProd>"
ROWS1 = "score_kernel<768, 1, SumProd>"

ANCHORS = {name: (seq, conds, dense) for name, seq, conds, dense in pair_probe.anchors()}

_matrices = {}


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for k in ENV_VARS:
        monkeypatch.delenv(k, raising=False)


def _matrix(oracle, seq, cond):
    """oracle.bppm of (seq, condition), computed once a session and never written to."""
    key = (seq, cond)
    if key not in _matrices:
        m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
        P = oracle.bppm(seq, None, m if cond == "holo" else None)[1]
        P.setflags(write=False)
        _matrices[key] = P
    return _matrices[key]


def _walkers(anchor):
    """The anchor and copies of it with 1, 2 and 5 point mutations."""
    rng = random.Random(len(anchor) * 1009 + sum(map(ord, anchor[:16])))
    out = []
    for n in MUTATIONS:
        s = list(anchor)
        for p in rng.sample(range(len(s)), n):
            s[p] = rng.choice([b for b in "ACGU" if b != s[p]])
        out.append("".join(s))
    return out


def _engine(native, tmpl, terms, contexts=None):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    return native.Engine(tmpl, ["." * len(tmpl)], terms, aptamer=apt, contexts=contexts,
                         thermostat=native.make_thermostat("fixed", t=T_HOT))


def _pair_terms(pairs, cond, unfavourable=()):
    return [(cond, ("pair", i, j), k not in unfavourable, 1.0) for k, (i, j) in enumerate(pairs)]


def _check_sequence(oracle, tv, seq, terms, contexts, where):
    """check_terms of one sequence's flat contexts x terms values; a macrostate
    term ("." * N: the whole ensemble) is ln 1.  Returns check_terms' counts summed."""
    tot = np.zeros(4)
    nt = len(terms)
    for c, (before, after) in enumerate(contexts or [("", "")]):
        padded = before + seq + after
        for cond in ("apo", "holo"):
            ks = [k for k, t in enumerate(terms) if t[0] == cond and isinstance(t[1], tuple)]
            if not ks:
                continue
            r = check_terms([tv[c * nt + k] for k in ks], _matrix(oracle, padded, cond),
                            [(terms[k][1][1] + len(before), terms[k][1][2] + len(before)) for k in ks],
                            [terms[k][2] for k in ks], where + (c, cond))
            tot[:3] += r[:3]
            tot[3] = max(tot[3], r[3])
        for k, t in enumerate(terms):
            if not isinstance(t[1], tuple):
                assert t[2] and close_term(tv[c * nt + k], 0.0, True), (where, c, k, tv[c * nt + k])
    return tot


def _fmt(tot):
    return "rel %d abs %d zero %d worst|dlnP| %.3e" % (tot[0], tot[1], tot[2], tot[3])


def _probe(native, oracle, name, seq, terms, expect, contexts=None, seeds=SEEDS, must_change=()):
    """Checks 1 and 2 of the module docstring on one engine; expect: the kernel
    names, or a predicate on them; must_change: positions that scored proposals
    of the run have to change (the seeds were chosen for it)."""
    assert len(terms) <= MAX_TERMS
    eng = _engine(native, seq, terms, contexts)
    seqs = _walkers(seq)
    eng.walkers_init(seeds, seqs)
    # 1. from scratch: the step's kernels and bppm_kernel on the same sequences
    _, tv_step = eng.rescore()
    _, tv_bppm, _ = eng.score_batch(seqs)
    failures, report = [], {}
    for kernel, tv in (("step", tv_step), ("bppm_kernel", tv_bppm)):
        tot = np.zeros(4)
        for w in range(len(seqs)):
            try:
                r = _check_sequence(oracle, tv[w], seqs[w], terms, contexts, (name, kernel, "walker", w))
                tot[:3] += r[:3]
                tot[3] = max(tot[3], r[3])
            except AssertionError as e:
                failures.append(str(e))
        report[kernel] = tot
        print("PROBE %s scratch %s %s" % (name, kernel, _fmt(tot)))
    assert not failures, "\n".join(failures)
    # 2. on stored tables: hot steps, every scored proposal against the oracle
    macro = ["." * len(seq)]
    accepted = [0] * len(seqs)
    changed = set()
    tot = np.zeros(4)
    cur = list(seqs)
    W = len(seqs)
    for first in (0, 8):                    # 8 steps, and 8 more where a walker has had too few accepted
        tr = eng.run_steps(8, trace=True)
        for w in range(W):
            for s, prop, out, after in pair_probe.replay(oracle, cur[w], macro, tr["position"][:, w],
                                                         tr["base"][w::W], tr["outcome"][:, w]):
                if out == oracle.ACCEPT_UNCHANGED:
                    continue
                r = _check_sequence(oracle, tr["term_values"][s, w], prop, terms, contexts,
                                    (name, "step", "walker", w, "step", first + s))
                tot[:3] += r[:3]
                tot[3] = max(tot[3], r[3])
                accepted[w] += out != oracle.REJECT
                changed.add(int(tr["position"][s, w]))
            cur[w] = after
        if min(accepted) >= 3:
            break
    print("PROBE %s stored step %s accepted %s" % (name, _fmt(tot), accepted))
    final, _, _ = eng.download()
    assert [f.upper() for f in final] == cur
    assert min(accepted) >= 3, accepted
    assert changed >= set(must_change), (sorted(changed), must_change)
    names = tuple(eng.last_kernel_names())
    assert expect(names) if callable(expect) else names == expect, names
    return report


def _default_names(N):
    return (CELLS, "outside_cells_kernel") if N <= 100 else (RING, "outside_ring_kernel")


CASES = [(name, cond, k) for name, (seq, conds, dense) in ANCHORS.items() for cond in conds for k in range(K_SETS)]


@pytest.mark.parametrize("name,cond,k", CASES, ids=["%s-%s-set%d" % c for c in CASES])
def test_step_kernels_at_interior_pairs(native, oracle, name, cond, k):
    """The product's shape: favourable pair terms plus the two macrostate terms."""
    seq, _, dense = ANCHORS[name]
    P = _matrix(oracle, seq, cond)
    pairs = pair_probe.pair_sets(seq, P, K_SETS, PER_SET)[k]
    cov = pair_probe.coverage(seq, P, [pairs])
    print("PROBE %s-%s-set%d chosen %s" % (name, cond, k, cov))
    if dense:       # the lane-sets past the first are among the pairs checked
        assert cov["rank64"] >= 16 // K_SETS and (len(seq) < 150 or cov["rank128"] >= 8 // K_SETS), cov
    terms = _pair_terms(pairs, cond) + [("apo", 0, True, 1.0), ("holo", 0, True, 1.0)]
    _probe(native, oracle, "%s-%s-set%d" % (name, cond, k), seq, terms, _default_names(len(seq)))


VARIANTS = [(name, conds[-1]) for name, (seq, conds, dense) in ANCHORS.items()]


@pytest.mark.parametrize("name,cond", VARIANTS, ids=["%s-%s" % c for c in VARIANTS])
def test_step_kernels_pair_terms_only(native, oracle, name, cond):
    """Pair terms alone (no macrostate fold beside the outside variant), a few of
    them unfavourable: every sixth, and the span-1 cell, whose ln(1 - 0) is 0."""
    seq, _, _ = ANCHORS[name]
    pairs = pair_probe.pair_sets(seq, _matrix(oracle, seq, cond), K_SETS, PER_SET)[1]
    unf = {k for k, (i, j) in enumerate(pairs) if k % 6 == 4 or j - i == 1}
    _probe(native, oracle, "%s-%s-pairs-only" % (name, cond), seq, _pair_terms(pairs, cond, unf),
           _default_names(len(seq)))


# seeds whose first six steps change the first base (walkers 0, 1) and the last (2, 3)
END_BASES = [
    (60, [9, 1, 56, 31], {}, (CELLS, "outside_cells_kernel")),
    (101, [14, 1, 204, 84], {}, (RING, "outside_ring_kernel")),
    (105, [14, 1, 204, 50], {"ADX_PF_KERNEL": "rows"}, (ROWS2, "outside_cells_kernel")),
]


@pytest.mark.parametrize("N,seeds,env,expect", END_BASES, ids=["%d%s" % (c[0], "-rows" if c[2] else "") for c in END_BASES])
def test_end_base_changes(native, oracle, monkeypatch, N, seeds, env, expect):
    """A change of the first or the last base: the cells (i, N) and (1, j) read
    it as their wrapped dangle (S[N + 1] = S[1], S[0] = S[N]).  The folds never
    use those cells' qm1, so an incremental refold that skipped them kept every
    energy right, and only the outside pass on the stored tables showed it (such a
    proposal folds from scratch now, mc_step.hip propose_walker)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seq = pair_probe.synthetic_anchor(N)
    pairs = pair_probe.pair_sets(seq, _matrix(oracle, seq, "apo"), K_SETS, PER_SET)[0]
    terms = _pair_terms(pairs, "apo") + [("apo", 0, True, 1.0), ("holo", 0, True, 1.0)]
    _probe(native, oracle, "ends-%d" % N, seq, terms, expect, seeds=seeds, must_change=(0, N - 1))


CONTEXTS = [("GGACA", "UUAC"), ("", "CCCAGU")]


def _context_terms(oracle, seq, n, cond):
    """n pair terms of one condition (contexts x terms pairs are requested), chosen
    on the bare sequence's matrix."""
    pairs = pair_probe.pair_sets(seq, _matrix(oracle, seq, cond), 1, n)[0]
    assert len(pairs) == n
    return _pair_terms(pairs, cond)


def test_contexts_at_the_pair_limit(native, oracle):
    """96 nt in two contexts (105 and 102 nt folded: the ring kernels), 32 pair
    terms = 64 requested pairs, exactly OX_MAXP."""
    seq = pair_probe.synthetic_anchor(96)
    terms = _context_terms(oracle, seq, 32, "holo")
    assert len(terms) * len(CONTEXTS) == OX_MAXP
    _probe(native, oracle, "ctx96-64pairs", seq, terms, (RING, "outside_ring_kernel"), CONTEXTS)


def test_contexts_past_the_pair_limit(native, oracle):
    """33 pair terms = 66 requested pairs: outside_ring_lds / outside_cells_lds
    return 0, the context falls back to the rows fold and bppm_kernel on its tables."""
    seq = pair_probe.synthetic_anchor(96)
    terms = _context_terms(oracle, seq, 33, "holo")
    assert len(terms) * len(CONTEXTS) > OX_MAXP
    _probe(native, oracle, "ctx96-66pairs", seq, terms, lambda names: names[1].startswith("bppm_kernel"), CONTEXTS)


@pytest.mark.parametrize("contexts,expect", [
    # 66 pairs: pf_ring_layout (dispatch.hip) needs outside_ring_lds > 0, which n_pairs > OX_MAXP
    # denies, so the context takes the rows layout; 152 nt folded: one fold per workgroup, and
    # outside tables in global scratch (GOUT)
    ([("G", "C"), ("", "AU")], (ROWS1, "bppm_kernel<1024, GOUT>")),
    # 33 pairs: the ring layout
    ([("G", "C")], (RING, "outside_ring_kernel")),
], ids=["66pairs", "33pairs"])
def test_contexts_at_150(native, oracle, contexts, expect):
    seq = pair_probe.synthetic_anchor(150)
    terms = _context_terms(oracle, seq, 33, "apo")
    _probe(native, oracle, "ctx150-%dpairs" % (33 * len(contexts)), seq, terms, expect, contexts)


# the rows of test_gpu_dispatch.py's table (pf, one pair term) for these overrides
OVERRIDES = [
    (100, "apo", {"ADX_OUTSIDE_KERNEL": "bppm"}, (CELLS, "bppm_kernel<512>")),
    (100, "holo", {"ADX_PF_KERNEL": "rows"}, (ROWS2, "outside_cells_kernel")),
    (105, "apo", {"ADX_PF_KERNEL": "rows"}, (ROWS2, "outside_cells_kernel")),
    (108, "holo", {"ADX_PF_KERNEL": "rows"}, (ROWS2, "bppm_kernel<512>")),
    (114, "apo", {"ADX_PF_KERNEL": "rows"}, (ROWS1, "bppm_kernel<1024, GOUT>")),
    (150, "holo", {"ADX_PF_KERNEL": "rows"}, (ROWS1, "bppm_kernel<1024, GOUT>")),
]


@pytest.mark.parametrize("N,cond,env,expect", OVERRIDES,
                         ids=["%d-%s" % (c[0], "-".join("%s=%s" % kv for kv in c[2].items())) for c in OVERRIDES])
def test_overrides_at_interior_pairs(native, oracle, monkeypatch, N, cond, env, expect):
    """The override and fallback paths of the step's outside pass: outside_cells
    on the rows kernel's slot layout, bppm_kernel reusing the stored tables, and
    its global-scratch layout from 114 nt."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seq = pair_probe.synthetic_anchor(N)
    pairs = pair_probe.pair_sets(seq, _matrix(oracle, seq, cond), K_SETS, PER_SET)[0]
    terms = _pair_terms(pairs, cond) + [("apo", 0, True, 1.0), ("holo", 0, True, 1.0)]
    _probe(native, oracle, "override-%d-%s" % (N, cond), seq, terms, expect)


# the lengths around which the longest diagonal (span 4, N - 4 cells) takes one more lane-set:
# 64 -> 65 cells in outside_cells_kernel (one -> two), 128 -> 129 in outside_ring_kernel (two -> three)
LANE_SET_BOUNDARIES = [(N, cond) for N in (68, 69, 132, 133) for cond in ("apo", "holo")]


@pytest.mark.parametrize("N,cond", LANE_SET_BOUNDARIES, ids=["%d-%s" % c for c in LANE_SET_BOUNDARIES])
def test_lane_set_boundaries(native, oracle, N, cond):
    """The lane-set count of the records, the finalize and the exterior adjoint, and
    the form of the finalize's sums over the multiloop parts, change with the
    diagonal's cell count at exactly these lengths."""
    seq = pair_probe.synthetic_anchor(N)
    pairs = pair_probe.pair_sets(seq, _matrix(oracle, seq, cond), K_SETS, PER_SET)[0]
    terms = _pair_terms(pairs, cond) + [("apo", 0, True, 1.0), ("holo", 0, True, 1.0)]
    _probe(native, oracle, "lanesets-%d-%s" % (N, cond), seq, terms, _default_names(N))
