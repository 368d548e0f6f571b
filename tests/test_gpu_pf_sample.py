"""Structures drawn from the Boltzmann ensemble on the GPU (pf_sample.hip)
through the per-fold call, the batched context call and the current walkers.

Frequencies are held to sample_check.py's bound, |f - p| <= 6 sqrt(p(1-p)/S) +
6/S, against references the engine has no part in: the enumerated distribution
exp(-E(s)/kT)/Z for short sequences and the oracle's McCaskill pair
probabilities at working lengths.  The returned energies come from an FP64 fill
of their own and must agree with the oracle and with adx_score_batch's dG to
1e-4 kcal/mol (the project's PF bound).  With fixed seeds the sampler is
deterministic, so none of this flakes.
"""
import math
import random

import numpy as np
import pytest

from addapt_amd import workloads
from sample_check import bound, distribution, frequency_violations, pair_frequencies, pair_violations, within
from structure_check import cons, pin, rand_seq, satisfies
from test_oracle_enum import SEQS

pytestmark = pytest.mark.gpu

PF_TOL = 1e-4   # kcal/mol
APT = workloads.THEO_SEQ
INNER = (9, 14)   # the motif's innermost pair (offsets into THEO_FOLD)


def _motif(oracle):
    return oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())


def _fold(native, seq, cst=None, motif=False):
    f = native.Fold(seq)
    if motif:
        f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    if cst:
        f.add_constraint(cst)
    return f


# ------------------------------------------------------------------ 1. exact distribution
ENUM_CASES = [(s, None) for s in SEQS] + [
    ("ACGUGAAAACGU", "xxxx........"), ("GCGCUUCGGCGC", "..|........."), ("GGACUUCGGUCC", "(..........)"),
    ("GCGCUUCGGCGC", "....xxxx...."),
    # multiloops carry real weight in these three
    ("GGGUGAAAGCUAGCGAAAGUCC", "(....................)"), ("GGGUGAAAACUAGUGAAAGCCC", "(...|...........|....)"),
    ("GGUGAAAACUGUGAAAGCC", "(..|...........|..)")]


@pytest.mark.parametrize("seq,cst", ENUM_CASES)
def test_fold_samples_follow_the_enumerated_distribution(native, oracle, seq, cst):
    S = 100_000
    e, samples = _fold(native, seq, cst).sample_structures(S, seed=20161015)
    assert len(samples) == S
    dist, Z = distribution(oracle, seq, cst)
    assert abs(-oracle.KT_KCAL * math.log(Z) - oracle.pf_energy(seq, cst)) < 1e-6   # enumeration = McCaskill
    foreign, off = frequency_violations(samples, dist)
    assert foreign == [], (seq, cst, foreign[:3])   # valid, and within the constraint
    assert off == [], (seq, cst, off[:3])
    assert abs(e - oracle.pf_energy(seq, cst)) <= PF_TOL, (seq, cst, e)


# ------------------------------------------------------------------ 2. pair frequencies
S_PAIR = 4096


def _check_pairs(oracle, seq, samples, cst=None, motif=None):
    """Validity, the constraint, and every pair frequency against oracle.bppm; returns bppm."""
    f, bad = pair_frequencies(samples, seq)
    assert bad == [], (seq, bad[:3])
    assert all(satisfies(s, cst) for s in set(samples)), (seq, cst)
    _, P = oracle.bppm(seq, cst, motif)
    v = pair_violations(f, P, len(samples))
    assert v == [], (seq, cst, v[:3])
    return P


def _check_motif_site(oracle, seq, samples, P, o, cst, m):
    """Where the motif's closing pair matters (P > 0.05), the fraction of samples
    holding the motif's own fold at offset o is held to two references:

    * exactly that event's probability, Z(site pinned to the fold) / Z from two
      oracle partition functions (the macrostate probability of the pinned site);
    * the oracle's probability of the motif's innermost pair, for the templates
      in which that pair forms only through the motif.  Whether it does is read
      off the oracle alone: the two references then agree to a tenth of the
      bound.  In the synthetic(N) and rhf(6) templates they do not (holo
      variants: P(inner pair) = 0.99997 against P(fold) = 0.998 at N = 60; the
      GCC-GAAA-GGC stem also closes without the ligand), so those templates
      drop out of this second assertion.

    Returns how many of the two assertions applied."""
    if P[o, o + len(APT) - 1] <= 0.05:
        return 0
    S = len(samples)
    f = sum(s[o:o + len(APT)] == workloads.THEO_FOLD for s in samples) / S
    base = cst or "." * len(seq)
    pinned = base[:o] + pin(workloads.THEO_FOLD) + base[o + len(APT):]
    p_fold = math.exp(-(oracle.pf_energy(seq, pinned, m) - oracle.pf_energy(seq, cst, m)) / oracle.KT_KCAL)
    assert within(f, p_fold, S), (seq, o, f, p_fold)
    p_inner = P[o + INNER[0], o + INNER[1]]
    if abs(p_inner - p_fold) > 0.1 * bound(p_fold, S):
        return 1
    assert within(f, p_inner, S), (seq, o, f, p_inner)
    return 2


def _fold_cases():
    rng = random.Random(31)
    out = []
    for n in (20, 37, 64, 65):
        seq = rand_seq(rng, n)
        out.append((seq, None, False))
        out.append((seq, cons(rng, seq), False))
    out.append((rand_seq(rng, 12) + APT + rand_seq(rng, 17), None, True))
    return out


@pytest.mark.parametrize("seq,cst,motif", _fold_cases())
def test_fold_pair_frequencies(native, oracle, seq, cst, motif):
    m = _motif(oracle) if motif else None
    e, samples = _fold(native, seq, cst, motif).sample_structures(S_PAIR, seed=7)
    P = _check_pairs(oracle, seq, samples, cst, m)
    assert abs(e - oracle.pf_energy(seq, cst, m)) <= PF_TOL, (seq, cst, e)
    if motif:
        assert _check_motif_site(oracle, seq, samples, P, seq.index(APT), cst, m) >= 1


def _engine(native, tmpl, macro, terms, thermostat=None, contexts=None, fold_mode="pf"):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    return native.Engine(tmpl, macro, terms, aptamer=apt, contexts=contexts, fold_mode=fold_mode,
                         thermostat=thermostat or native.make_thermostat("fixed", t=1.0))


def _check_batch(native, oracle, N, W, contexts=None):
    """Every variant of a synthetic(N) PF engine: pair frequencies, constraints,
    the motif site of holo variants, and the energies against dG and the oracle."""
    tmpl, active = workloads.synthetic(N)
    eng = _engine(native, tmpl, [active], workloads.default_objective(), contexts=contexts)
    seqs = workloads.walker_sequences(tmpl, [active], W)
    _, _, dg = eng.score_batch(seqs)
    m = _motif(oracle)
    kinds, sites = set(), 0
    for v in range(eng.info.n_variants):
        c, cond, mac = eng.variant(v)
        b, a = contexts[c] if contexts else ("", "")
        cst = "." * len(b) + active + "." * len(a) if mac >= 0 else None
        st, e = eng.sample_structures(seqs, v, S_PAIR, seed=1000 + v)
        assert e.dtype == np.float32 and len(st) == W and all(len(r) == S_PAIR for r in st)
        kinds.add((cond, mac >= 0))
        for w in range(W):
            full = (b + seqs[w] + a).upper()
            assert len(st[w][0]) == len(full)
            P = _check_pairs(oracle, full, st[w], cst, m if cond == 1 else None)
            ref = oracle.pf_energy(full, cst, m if cond == 1 else None)
            assert abs(e[w] - ref) <= PF_TOL, (N, v, w, e[w], ref)
            if math.isfinite(dg[w, v]):
                assert abs(e[w] - dg[w, v]) <= PF_TOL, (N, v, w, e[w], dg[w, v])
            if cond == 1:
                sites += _check_motif_site(oracle, full, st[w], P, full.index(APT), cst, m)
    assert kinds == {(0, False), (0, True), (1, False), (1, True)}   # apo / holo x free / constrained
    return sites


@pytest.mark.parametrize("N,W", [(60, 6), (100, 4), (150, 2)])
def test_batch_pair_frequencies_and_energies(native, oracle, N, W):
    assert _check_batch(native, oracle, N, W) > 0   # the ligand binds somewhere: the motif assertion ran


def test_batch_contexts(native, oracle):
    """Context-padded variants: L > N, the samples cover the padded sequence."""
    _check_batch(native, oracle, 60, 3, contexts=[("GGAC", "UUA"), ("", "CCCA")])


# ------------------------------------------------------------------ 3. energies
def test_extreme_energies_stay_finite(native, oracle):
    """-100 kcal/mol and lower in an engine whose pf scale was calibrated on an
    ordinary template: the FP64 fill has no range to leave."""
    seqs = ["G" * 70 + "AAAA" + "C" * 70, "GC" * 40 + "UUUU" + "GC" * 30, "GGGGCCCC" * 18]
    tmpl, active = workloads.synthetic(144)
    eng = _engine(native, tmpl, [active], workloads.default_objective())
    free = [v for v in range(eng.info.n_variants) if eng.variant(v)[1:] == (0, -1)]
    assert len(free) == 1
    st, e = eng.sample_structures(seqs, free[0], 4, seed=3)
    for w, seq in enumerate(seqs):
        ref = oracle.pf_energy(seq)
        assert ref < -100.0 and math.isfinite(e[w])
        assert abs(e[w] - ref) <= PF_TOL, (seq, e[w], ref)
        assert pair_frequencies(st[w], seq)[1] == [] and all("(" in s for s in st[w])


# ------------------------------------------------------------------ 4. deterministic facts
def test_pinned_infeasible_and_tiny(native, oracle):
    rng = random.Random(2)
    for n in (20, 64):
        seq = rand_seq(rng, n)
        _, s = oracle.mfe(seq)
        assert "(" in s
        e, samples = _fold(native, seq, pin(s)).sample_structures(64, seed=n)
        assert set(samples) == {s}
        assert abs(e - oracle.pf_energy(seq, pin(s))) <= PF_TOL
    e, samples = _fold(native, "AAAAAAAAAA", "(........)").sample_structures(8, seed=1)
    assert math.isinf(e) and e > 0 and set(samples) == {"." * 10}
    for seq in ("ACG", "ACGU"):
        e, samples = _fold(native, seq).sample_structures(8, seed=1)
        assert e == 0.0 and set(samples) == {"." * len(seq)}


# ------------------------------------------------------------------ 5. reproducibility
def test_reproducible(native):
    tmpl, active = workloads.synthetic(100)
    eng = _engine(native, tmpl, [active], workloads.default_objective())
    seqs = workloads.walker_sequences(tmpl, [active], 5)
    a, ea = eng.sample_structures(seqs, 1, 64, seed=11)
    b, eb = eng.sample_structures(seqs, 1, 64, seed=11)
    assert a == b and ea.tobytes() == eb.tobytes()
    c, _ = eng.sample_structures(seqs, 1, 16, seed=11)
    assert [r[:16] for r in a] == c   # sample k does not depend on n_samples
    d, ed = eng.sample_structures(seqs, 1, 64, seed=12)
    assert all(x != y for x, y in zip(a, d)) and ea.tobytes() == ed.tobytes()
    f = _fold(native, seqs[0].upper())
    assert f.sample_structures(32, seed=5) == f.sample_structures(32, seed=5)
    assert f.sample_structures(32, seed=5)[1] != f.sample_structures(32, seed=2 ** 40 + 5)[1]


def test_launch_chunks_do_not_show(native):
    """1100 sequences of 150 nt: their FP64 tables alone (0.26 MB each) pass the
    256 MiB bound of one launch, so the call is split; its first 70 rows equal a
    70-sequence call, which is one launch."""
    tmpl, active = workloads.synthetic(150)
    eng = _engine(native, tmpl, [active], workloads.default_objective())
    seqs = workloads.walker_sequences(tmpl, [active], 1100)
    tables = (3 * (146 * 147 // 2) + 152) * 8
    assert 1100 * tables > 256 << 20 > 70 * (tables + 4 * 150)
    big, eb = eng.sample_structures(seqs, 0, 4, seed=99)
    small, es = eng.sample_structures(seqs[:70], 0, 4, seed=99)
    assert big[:70] == small and eb[:70].tobytes() == es.tobytes()
    last, el = eng.sample_structures(seqs[1099:], 0, 4, seed=99)   # batch member 0 of its own call: other draws
    assert "(" in "".join(big[1099]) and np.float32(el[0]) == eb[1099]   # the second launch's rows are filled too


# ------------------------------------------------------------------ 6. current walkers
def test_walker_samples_and_untouched_state(native):
    tmpl, active = workloads.synthetic(60)
    terms = workloads.default_objective()
    W = 70
    seqs = workloads.walker_sequences(tmpl, [active], W)

    def engine():
        th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30)
        eng = _engine(native, tmpl, [active], terms, thermostat=th)
        eng.walkers_init(list(range(W)), seqs)
        eng.run_steps(5)
        return eng

    eng, plain = engine(), engine()
    cur = eng.download()[0]
    assert cur != seqs   # the walkers moved
    for v in range(eng.info.n_variants):
        st, e = eng.walker_samples(v, 8, seed=21)
        st2, e2 = eng.sample_structures(cur, v, 8, seed=21)
        assert st == st2 and e.tobytes() == e2.tobytes(), v
    a, b = eng.run_steps(5, trace=True), plain.run_steps(5, trace=True)
    assert a["base"] == b["base"]
    for k in ("position", "outcome", "temperature", "proposed_score", "current_score", "random_threshold",
              "term_values"):
        assert a[k].tobytes() == b[k].tobytes(), k
    fa, fb = eng.download(), plain.download()
    assert fa[0] == fb[0] and fa[1].tobytes() == fb[1].tobytes() and (fa[2] == fb[2]).all()


# ------------------------------------------------------------------ 7. errors
def test_errors(native):
    tmpl, active = workloads.synthetic(60)
    terms = workloads.default_objective()
    seqs = workloads.walker_sequences(tmpl, [active], 2)
    mfe = _engine(native, tmpl, [active], terms, fold_mode="mfe")
    with pytest.raises(native.AdxError) as ei:
        mfe.sample_structures(seqs, 0, 4)
    assert ei.value.status == native.EUNSUPPORTED
    mfe.walkers_init([0, 1], seqs)
    with pytest.raises(native.AdxError) as ei:
        mfe.walker_samples(0, 4)
    assert ei.value.status == native.EUNSUPPORTED
    eng = _engine(native, tmpl, [active], terms)
    for v in (-1, eng.info.n_variants):
        with pytest.raises(native.AdxError) as ei:
            eng.sample_structures(seqs, v, 4)
        assert ei.value.status == native.EINVAL
    for n in (0, -3):
        with pytest.raises(native.AdxError) as ei:
            eng.sample_structures(seqs, 0, n)
        assert ei.value.status == native.EINVAL
        with pytest.raises(native.AdxError) as ei:
            _fold(native, "GGGAAACCC").sample_structures(n)
        assert ei.value.status == native.EINVAL
    with pytest.raises(native.AdxError) as ei:
        eng.walker_samples(0, 4)
    assert ei.value.status == native.ESTATE
    eng.walkers_init([0, 1], seqs)
    for v in (-1, eng.info.n_variants):
        with pytest.raises(native.AdxError) as ei:
            eng.walker_samples(v, 4)
        assert ei.value.status == native.EINVAL
    with pytest.raises(native.AdxError) as ei:
        eng.walker_samples(0, 0)
    assert ei.value.status == native.EINVAL
    L = native.lib()
    buf = b"".join(s.encode() for s in seqs)
    assert L.adx_fold_sample_structures(None, 1, 0, None, None) == native.EINVAL
    assert L.adx_sample_structures_batch(eng.ptr, 2, buf, 0, 4, 0, None, None) == native.EINVAL
    assert L.adx_sample_structures_batch(eng.ptr, 2, None, 0, 4, 0, None, None) == native.EINVAL
    assert L.adx_sample_structures_batch(None, 2, buf, 0, 4, 0, None, None) == native.EINVAL
    assert L.adx_walkers_sample_structures(eng.ptr, 0, 4, 0, None, None) == native.EINVAL
    assert L.adx_walkers_sample_structures(None, 0, 4, 0, None, None) == native.EINVAL
