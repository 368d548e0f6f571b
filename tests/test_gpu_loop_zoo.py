"""Every loop shape and every energy-table entry on each fold kernel, by pinned
structures (loop_zoo.py): a constraint of enforced pairs and 'x' admits one
structure, so the constrained fold's answer is that structure's loop-energy sum
and a kernel that mishandles one of its loops is wrong, with no minimum or
average to hide it.  test_loop_zoo.py checks the fixtures on the CPU.

  a. shapes per inside kernel: one engine per zoo structure (pinned macrostate,
     apo + holo terms), score_batch of 8 randomised sequences; the constrained
     variants against the oracle's fold of (sequence, pinned), the unconstrained
     ones of the same launch against its free fold
  b. table entries per inside kernel: the same on the enumerated batches of
     table_batches(), padded to the kernel's length
  c. off the step: traceback, samples, pair probabilities, centroid and MEA
     structure of every zoo structure, through Fold and the engine's batch calls
  d. incremental refolds across a 22-nt loop side, a 12-nt bulge and a 3-branch
     multiloop: hot trajectories replayed against the oracle

MFE energies are compared bit for bit as float32, ensemble energies within
1e-4 kcal/mol.  Every case asserts the kernel names the dispatcher reports.
The zoo is cut into bands of BAND structures, one parametrised case each.

A PF context holds scaled FP32 tables on one scale, calibrated on its template,
and they reach about 54 kcal/mol to either side of it; a pinned structure of weak
pairs lies up to 80 kcal/mol above the free ensemble of its own sequence.  The PF
cases therefore calibrate each context on a helix of known energy and fold a
batch in as many contexts as it spans windows (_pf_groups); the MFE cases fold
each batch in one context.  Beyond the window the PF step kernels are off by
1e-3 kcal/mol and more and then return +inf: the smallest such case is kept as a
strict xfail (test_pf_step_kernels_beyond_the_reach_of_their_scale; DESIGN.md,
parity).

What these checks found: adx_fold_pf, adx_fold_bpp and
adx_fold_ensemble_structures took a constrained ensemble of positive energy for
an empty one (test_fold_pf_positive_energy_is_not_an_empty_ensemble, fixed), and
the reach limit above (open).

Per-case times measured on an MI355X, oracle included (an engine is created,
scored and stepped once in about 10 ms): a. 0.2 to 1.6 s a band (pf_ring at 150 the
slowest); b. chunks of CHUNK sequences, every variant of every sequence compared:
the whole module, 223 cases, takes 72 s; c. 0.1 to 0.8 s a band; d. 0.3 to 2.3 s
(mfe at 150).
"""
import math

import numpy as np
import pytest

import loop_zoo as Z
from addapt_amd import workloads
from parity_bounds import close_score

pytestmark = pytest.mark.gpu

DG_TOL = 1e-4
BPP_TOL = 2e-4        # pair_probe's bound on |dP|
PF_REACH = 50.0       # kcal/mol from a PF context's scale that a test asks of its FP32 tables (_pf_groups)
T_HOT = 1e9           # exp(dS / T_HOT) is 1 to 1e-6 for any finite dS: every finite proposal is accepted
BAND = 25             # zoo structures per parametrised case
N_SEQ = 8
N_SAMPLES = 32
ENV_VARS = ("ADX_MFE_KERNEL", "ADX_MFE_PAIR", "ADX_PF_KERNEL", "ADX_OUTSIDE_KERNEL", "ADX_NO_MFE16")

# the dispatcher's names, as test_gpu_dispatch.py records them
CELLS = "pf_cells_kernel (scores combined in step_tail_kernel)"
RING = "pf_ring_kernel (scores combined in step_tail_kernel)"
MFE_PAIR = "mfe_pair_kernel + score_kernel<MinPlus> (FP32 fallback launch); scores combined in step_tail_kernel"
MFE_CELLS = "mfe_cells_kernel + score_kernel<MinPlus> (FP32 fallback launch); scores combined in step_tail_kernel"
ROWS16 = "score_kernel<512, 1, MinPlus16> + score_kernel<MinPlus> (FP32 fallback launch)"

# id -> (fold mode, length, environment, inside kernel)
KERNELS = {
    "mfe_pair-100": ("mfe", 100, {}, MFE_PAIR),
    "mfe_cells-100": ("mfe", 100, {"ADX_MFE_PAIR": "0"}, MFE_CELLS),
    "mfe_cells-150": ("mfe", 150, {}, MFE_CELLS),
    "mfe_rows16-100": ("mfe", 100, {"ADX_MFE_KERNEL": "rows"}, ROWS16),
    "mfe_fp32-100": ("mfe", 100, {"ADX_NO_MFE16": "1"}, "score_kernel<768, 2, MinPlus>"),
    "pf_cells-100": ("pf", 100, {}, CELLS),
    "pf_ring-150": ("pf", 150, {}, RING),
    "pf_rows-100": ("pf", 100, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 2, SumProd>"),
    "pf_rows-150": ("pf", 150, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 1, SumProd>"),
}

_refs = {}


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for k in ENV_VARS:
        monkeypatch.delenv(k, raising=False)


def _motif(oracle):
    return oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())


def _ref(oracle, fold, seq, cst, holo):
    """The oracle's fold energy, computed once a session.  A sequence without the
    aptamer's bases has no motif site, so its holo fold is its apo fold."""
    holo = holo and Z.THEO_SEQ in seq
    key = (fold, seq, cst, holo)
    if key not in _refs:
        f = oracle.mfe_energy if fold == "mfe" else oracle.pf_energy
        _refs[key] = f(seq, cst, _motif(oracle) if holo else None)
    return _refs[key]


def _same(g, ref):
    ref = np.float32(ref)
    if math.isinf(ref):
        return math.isinf(g) and g > 0
    return np.float32(g) == ref


def _agrees(fold, g, ref):
    if fold == "mfe":
        return _same(g, ref)
    ref = np.float32(ref)
    if math.isinf(ref):
        return math.isinf(g) and g > 0
    return abs(g - ref) <= DG_TOL


def _engine(native, tmpl, st, fold, t=1.0):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    return native.Engine(tmpl, [Z.pinned(st)], workloads.default_objective(), aptamer=apt, fold_mode=fold,
                         thermostat=native.make_thermostat("fixed", t=t))


def _anchor(oracle, L, target):
    """(template, its ensemble energy): a G.C helix in poly-A of L nt whose ensemble
    energy is the nearest to target kcal/mol.  A PF context scales its FP32 tables
    by exp(g0 / kT) per nucleotide, g0 = min(-0.05, the template's ensemble energy
    / L) (api_problem.hpp calibrate)."""
    if L not in _anchors:
        helices = ["G" * k + "AAAA" + "C" * k + "A" * (L - 2 * k - 4) for k in range(0, 31)]
        _anchors[L] = [(oracle.pf_energy(s), s) for s in helices]
    g, s = min(_anchors[L], key=lambda a: abs(a[0] - target))
    return s, g


_anchors = {}


def _pf_groups(oracle, st, seqs):
    """seqs in groups that one PF context can hold, as (template, indices).  Scaled
    FP32 tables hold energies up to 53.9 kcal/mol above the context's scale L * g0
    (2^-126 = exp(-87.3), kT = 0.616) and 54.6 below it (2^128), partial sums
    included; a pinned structure of weak pairs lies up to 80 kcal/mol above its own
    sequence's free ensemble, and an enumerated batch spans more than one window.
    So the sequences are binned by the highest energy among the pinned structure
    and the parts it encloses, 10 kcal/mol a bin, and each bin's context is
    calibrated on a helix 35 kcal/mol below the bin's floor (at most -0.05 * L):
    every member then lies 35 to PF_REACH above the scale, and its free ensemble
    at most PF_REACH below it, or the fixture is at fault."""
    L, bins = len(st), {}
    top = [max(oracle.eval_structure(s, t) for s, t in Z.enclosed(v, st)) for v in seqs]
    for w, e in enumerate(top):
        bins.setdefault(math.floor(e / 10.0), []).append(w)
    out = []
    for b, ws in sorted(bins.items()):
        tmpl, g = _anchor(oracle, L, min(10.0 * b - 35.0, -0.05 * L))
        scale = min(g, -0.05 * L)
        for w in ws:
            assert top[w] - scale <= PF_REACH, ("fixture out of the FP32 range", seqs[w], st, top[w], scale)
            assert scale - _ref(oracle, "pf", seqs[w], None, False) <= PF_REACH, \
                ("fixture out of the FP32 range", seqs[w], scale)
        out.append((tmpl, ws))
    return out


def _check_batch(native, oracle, fold, st, seqs, inside, where):
    """One engine for the structure, one score_batch of seqs (PF: of each group of
    _pf_groups): every variant's energy of every sequence against the oracle; then
    one MC step of two walkers, for the names of the kernels this context
    dispatches to."""
    groups = [(seqs[0], list(range(len(seqs))))] if fold == "mfe" else _pf_groups(oracle, st, seqs)
    for tmpl, ws in groups:
        _check_group(native, oracle, fold, st, tmpl, [seqs[w] for w in ws], inside, where)


def _check_group(native, oracle, fold, st, tmpl, seqs, inside, where):
    eng = _engine(native, tmpl, st, fold)
    assert eng.info.n_variants == 4
    _, _, dg = eng.score_batch(seqs)
    cst = Z.pinned(st)
    bad = []
    for v in range(eng.info.n_variants):
        _, cond, mac = eng.variant(v)
        for w, s in enumerate(seqs):
            ref = _ref(oracle, fold, s, cst if mac >= 0 else None, cond == 1)
            if mac >= 0:
                assert math.isfinite(ref), (where, s)
            if not _agrees(fold, dg[w, v], ref):
                bad.append((where, st, s, "holo" if cond == 1 else "apo", "pinned" if mac >= 0 else "free",
                            float(dg[w, v]), float(ref)))
    assert not bad, "%d energies off, the first: %r" % (len(bad), bad[:4])
    # adx_last_kernel_names reports run_steps' launches only.  score_batch and the step choose their
    # kernel in the same place (dispatch.hip inside_choice, with energies requested in both), so the
    # step's names are score_batch's as long as that stays one function
    eng.walkers_init([1, 2], (seqs + seqs)[:2])
    eng.run_steps(1)
    assert tuple(eng.last_kernel_names()) == (inside, ""), where


def _bands(L):
    n = len(Z.shape_zoo(L))
    return [(a, min(a + BAND, n)) for a in range(0, n, BAND)]


SHAPE_CASES = [(k, a, b) for k, (_, L, _, _) in KERNELS.items() for a, b in _bands(L)]


@pytest.mark.parametrize("kernel,a,b", SHAPE_CASES, ids=["%s-zoo%d:%d" % c for c in SHAPE_CASES])
def test_shapes_per_inside_kernel(native, oracle, monkeypatch, kernel, a, b):
    fold, L, env, inside = KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    zoo, var = Z.shape_zoo(L), Z.zoo_variants(L, N_SEQ)
    for n in range(a, b):
        _check_batch(native, oracle, fold, zoo[n][1], var[n], inside, (kernel, n))


CHUNK = 128           # sequences of a table batch per parametrised case (the oracle's free folds set the time)
TABLE_CASES = [(k, n, a) for k in KERNELS for n, (_, _, seqs) in enumerate(Z.table_batches())
               for a in range(0, len(seqs), CHUNK)]


@pytest.mark.parametrize("kernel,n,a", TABLE_CASES,
                         ids=["%s-%s-%d" % (k, Z.table_batches()[n][0], a) for k, n, a in TABLE_CASES])
def test_table_entries_per_inside_kernel(native, oracle, monkeypatch, kernel, n, a):
    """CHUNK sequences of one enumerated batch in one engine and one score_batch (the
    batches' coverage as a whole: test_loop_zoo.py)."""
    fold, L, env, inside = KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name, st, seqs = Z.fitted_batches(L)[n]
    assert len(st) == L
    _check_batch(native, oracle, fold, st, seqs[a:a + CHUNK], inside, (kernel, name, a))


# ------------------------------------------------------------------ c. off the step
def _fold(native, seq, st, with_bppm=False):
    f = native.Fold(seq, with_bppm=with_bppm)
    if Z.theo_offset(seq, st) >= 0:
        f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    f.add_constraint(Z.pinned(st))
    return f


def _non_pairs(st):
    """One pair of positions per loop that st does not pair: the closing base with
    the first inner pair's 3' base, the two ends of a hairpin's loop, the first
    and the last base for the exterior loop."""
    pt, out = Z.pair_table(st), []
    for lp in Z.loops(st):
        if lp["kind"] == "exterior":
            i, j = 0, len(st) - 1
        elif lp["kind"] == "hairpin":
            i, j = lp["closing"][0] + 1, lp["closing"][1] - 1
        else:
            i, j = lp["closing"][0], lp["branches"][0][1]
        if pt[i] != j and i < j:
            out.append((i, j))
    return out


def _check_off_step_fold(native, oracle, seq, st):
    holo = Z.theo_offset(seq, st) >= 0
    cst = Z.pinned(st)
    e, got = _fold(native, seq, st).mfe_structure()
    assert got == st and _same(e, _ref(oracle, "mfe", seq, cst, holo)), (seq, st, got, e)
    g_ref = _ref(oracle, "pf", seq, cst, holo)
    g, samples = _fold(native, seq, st).sample_structures(N_SAMPLES, seed=20161015)
    assert samples == [st] * N_SAMPLES and abs(g - np.float32(g_ref)) <= DG_TOL, (seq, st, g, g_ref)
    f = _fold(native, seq, st, with_bppm=True)
    assert abs(f.pf() - np.float32(g_ref)) <= DG_TOL, (seq, st, f.pf(), g_ref)
    cen, mea, _ = f.ensemble_structures()
    assert cen == st and mea == st, (seq, st, cen, mea)
    for i, j in enumerate(Z.pair_table(st)):
        if j > i:
            assert abs(f.bpp(i + 1, j + 1) - 1.0) <= BPP_TOL, (seq, st, i, j, f.bpp(i + 1, j + 1))
    for i, j in _non_pairs(st):
        assert f.bpp(i + 1, j + 1) == 0.0, (seq, st, i, j, f.bpp(i + 1, j + 1))


OFF_STEP_CASES = [(L, a, b) for L in (100, 150) for a, b in _bands(L)]


@pytest.mark.parametrize("L,a,b", OFF_STEP_CASES, ids=["%d-zoo%d:%d" % c for c in OFF_STEP_CASES])
def test_off_the_step_fold(native, oracle, L, a, b):
    """adx_fold_*: the traceback returns S with the oracle's energy, all 32 samples
    are S, P is 1 on S's pairs and exactly 0 on a non-pair per loop, the centroid
    and the MEA structure are S."""
    for seq, st in Z.shape_zoo(L)[a:b]:
        _check_off_step_fold(native, oracle, seq, st)


@pytest.mark.parametrize("L,a,b", OFF_STEP_CASES, ids=["%d-zoo%d:%d" % c for c in OFF_STEP_CASES])
def test_off_the_step_engine(native, oracle, L, a, b):
    """The engine's batch calls on the constrained variants: mfe_structures and
    sample_structures of the zoo's sequence and three randomised ones.  (The
    engine's ensemble_structures addresses the unconstrained folds only.)"""
    zoo, var = Z.shape_zoo(L), Z.zoo_variants(L, N_SEQ)
    for n in range(a, b):
        seq, st = zoo[n]
        seqs, cst = [seq] + var[n][:3], Z.pinned(st)
        mfe, pf = _engine(native, seq, st, "mfe"), _engine(native, seq, st, "pf")
        for v in range(mfe.info.n_variants):
            _, cond, mac = mfe.variant(v)
            if mac < 0:
                continue
            got, e = mfe.mfe_structures(seqs, v)
            assert got == [st] * len(seqs), (n, v, got)
            for w, s in enumerate(seqs):
                assert _same(e[w], _ref(oracle, "mfe", s, cst, cond == 1)), (n, v, s, e[w])
            assert pf.variant(v) == mfe.variant(v)
            got, g = pf.sample_structures(seqs, v, N_SAMPLES, seed=7 + n)
            for w, s in enumerate(seqs):
                assert got[w] == [st] * N_SAMPLES, (n, v, s)
                assert abs(g[w] - np.float32(_ref(oracle, "pf", s, cst, cond == 1))) <= DG_TOL, (n, v, s, g[w])


@pytest.mark.parametrize("N,k", [(150, 5), (100, 7)])
def test_fold_pf_positive_energy_is_not_an_empty_ensemble(native, oracle, N, k):
    """The bug the zoo's 150-nt structures above 19 kcal/mol showed, at its
    smallest: k forced U.G triloops in poly-A (28.8 kcal/mol at 150 nt, 40.4 at
    100).  adx_fold_pf's first fold runs on an assumed scale of -0.30 kcal/mol per
    nucleotide; an ensemble more than 63.6 kcal/mol above N * -0.30 is below FP32
    there (exp(-103)), and its Z = 0 was taken for an empty ensemble: pf() gave
    +inf, ensemble_structures() all dots, bpp() 0.  fold_one now folds such a case
    once more on the mildest scale, -0.05 per nucleotide, which reaches 53.9
    kcal/mol above N * -0.05."""
    seq, st = "UUUUG" * k + "A" * (N - 5 * k), "(...)" * k + "." * (N - 5 * k)
    ref = oracle.pf_energy(seq, Z.pinned(st))
    assert 63.6 - 0.30 * N < ref < 53.9 - 0.05 * N      # where the bug was, and within the mild scale's reach
    f = native.Fold(seq, with_bppm=True)
    f.add_constraint(Z.pinned(st))
    assert abs(f.pf() - np.float32(ref)) <= DG_TOL, (f.pf(), ref)
    cen, mea, _ = f.ensemble_structures()
    assert cen == st and mea == st, (cen, mea)
    for p in range(k):
        assert abs(f.bpp(5 * p + 1, 5 * p + 5) - 1.0) <= BPP_TOL
    assert f.bpp(1, 10) == 0.0


REACH_KERNELS = ["pf_cells-100", "pf_ring-150", "pf_rows-100", "pf_rows-150"]


@pytest.mark.xfail(strict=True, reason="12 forced U.G triloops in poly-A, pinned, 100 and 150 nt: expected 69.4 kcal/mol "
                   "(oracle), observed +inf for the apo and the holo pinned variant from pf_cells_kernel, "
                   "pf_ring_kernel and score_kernel<SumProd> at both lengths.  The context's scale, calibrated on the "
                   "sequence's own free ensemble, is -9.4 (100 nt) / -14.5 (150 nt) kcal/mol, so Z * sigma^N = "
                   "exp(-128) / exp(-136) is below FP32, and the step kernels have no second scale, fallback or error "
                   "(DESIGN.md, parity)")
@pytest.mark.parametrize("kernel", REACH_KERNELS)
def test_pf_step_kernels_beyond_the_reach_of_their_scale(native, oracle, monkeypatch, kernel):
    """The smallest pinned case out of a PF context's window: a feasible constrained
    fold more than 54 kcal/mol above the scale.  Kept failing until the step
    kernels refold such a variant on another scale or refuse it."""
    fold, L, env, inside = KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = 12
    seq, st = "UUUUG" * n + "A" * (L - 5 * n), "(...)" * n + "." * (L - 5 * n)
    ref = oracle.pf_energy(seq, Z.pinned(st))
    assert math.isfinite(ref) and ref - min(-0.05 * L, oracle.pf_energy(seq)) > 53.9
    eng = _engine(native, seq, st, fold)
    _, _, dg = eng.score_batch([seq])
    got = {v: float(dg[0, v]) for v in range(eng.info.n_variants) if eng.variant(v)[2] >= 0}
    assert all(abs(g - np.float32(ref)) <= DG_TOL for g in got.values()), (kernel, got, ref)


# ------------------------------------------------------------------ d. incremental refolds
REFOLD_CASES = {
    "mfe-100": ("mfe", 100, {}, MFE_PAIR),
    "mfe-100-cells": ("mfe", 100, {"ADX_MFE_PAIR": "0"}, MFE_CELLS),
    "mfe-150": ("mfe", 150, {}, MFE_CELLS),
    "pf-100": ("pf", 100, {}, CELLS),
    "pf-150": ("pf", 150, {}, RING),
}
REFOLD_SEEDS = [71, 72, 73, 74, 75, 76, 77, 78]
REFOLD_STEPS = 30


def _close(a, b):
    if math.isinf(b) or math.isnan(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


@pytest.mark.parametrize("case", list(REFOLD_CASES))
def test_refolds_across_large_loops(native, oracle, monkeypatch, case):
    """8 walkers, 30 hot steps under the pinned macrostate ('x' bases mutate freely,
    '(' bases drag their partner): positions, bases, outcomes and counters as the
    oracle's replay, proposed scores within the replay bounds of test_gpu_ring.py
    (pf) and test_gpu_mfe.py (mfe), the stored scores equal to rescore()."""
    fold, L, env, inside = REFOLD_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tmpl, st = Z.refold_structure(L)
    macro, terms, steps, W = [Z.pinned(st)], workloads.default_objective(), REFOLD_STEPS, len(REFOLD_SEEDS)
    eng = _engine(native, tmpl, st, fold, t=T_HOT)
    # mfe: randomised starts; pf: every walker starts at the template the context's scale was calibrated
    # on, and 30 moves keep its folds within the FP32 tables' reach of that scale (_pf_groups)
    seqs = Z.variants(tmpl, st, W, 4242 + L) if fold == "mfe" else [tmpl] * W
    eng.walkers_init(REFOLD_SEEDS, seqs)
    tr = eng.run_steps(steps, trace=True)
    assert tuple(eng.last_kernel_names()) == (inside, "")
    final, scores, counters = eng.download()
    sf = oracle.ScoreFunction(terms, aptamer=_motif(oracle), mode=fold)
    therm_o = oracle.thermostat("fixed", t=T_HOT)
    moved = 0
    for w, seed in enumerate(REFOLD_SEEDS):
        forced = [int(x) for x in tr["outcome"][:, w]]
        ref = oracle.mc_run(sf, seqs[w], macro, therm_o, seed, steps, forced=forced,
                            tie_eps=1e-12 if fold == "mfe" else 1e-6)
        assert ref["rc"] == 0
        assert list(tr["position"][:, w]) == ref["pos"], w
        assert tr["base"][w::W] == ref["base"], w
        assert list(tr["outcome"][:, w]) == ref["outcome"], w
        for s in range(steps):
            if ref["outcome"][s] != oracle.ACCEPT_UNCHANGED:
                a, b = tr["proposed_score"][s, w], ref["proposed_score"][s]
                assert math.isfinite(b), (case, w, s)
                ok = _close(a, b) if fold == "mfe" else close_score(a, b, tr["term_values"][s, w], terms)
                assert ok, (case, w, s, a, b)
                assert ref["outcome"][s] != oracle.REJECT, (case, w, s)   # hot: every finite proposal is accepted
                moved += 1
        assert final[w].upper() == ref["seq"].upper(), w
        assert list(counters[w]) == ref["counters"], w
    assert moved >= W * steps // 2
    fresh, _ = eng.rescore()
    assert (fresh == scores).all(), [(w, scores[w], fresh[w]) for w in range(W) if fresh[w] != scores[w]]
