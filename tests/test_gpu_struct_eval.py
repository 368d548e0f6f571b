"""Energies, ensemble probabilities and status bytes of given structures on the
GPU (struct_eval.hip) through the per-fold call, the batched context call and
the current walkers, held to struct_eval_check.py: the oracle's pinned folds
(PF convention within 1e-9 kcal/mol, MFE convention exactly), the membership
rules as plain Python, and exp(-(E - G) / kT) against the oracle's G.

Probabilities: the engine's G comes from an FP64 fill of FP32 factors and is
held to the project's PF bound, 1e-4 kcal/mol, so p may be off by
exp(1e-4 / kT) - 1 = 1.6e-4 relative; the bound here is 2e-4.
"""
import math
import random

import numpy as np
import pytest

import struct_eval_check as sec
from addapt_amd import workloads
from structure_check import cons, rand_seq
from test_oracle_enum import structures
from test_struct_eval_check import CONSTRAINED

pytestmark = pytest.mark.gpu

TOL_PF = 1e-9      # kcal/mol, against the pinned fold
REL_P = 2e-4
MERS14 = sec.MERS14


def _motif(oracle):
    return oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())


def _fold(native, seq, cst=None, motif=False):
    f = native.Fold(seq)
    if motif:
        f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    if cst:
        f.add_constraint(cst)
    return f


def _mutants(n):
    """Strings of n chars that are no members (n >= 6)."""
    return ["(" + "." * (n - 1), "." * (n - 1) + ")", "." * (n - 3) + "(.)", "[" + "." * (n - 1), "()" + "." * (n - 2),
            "((...)" + "." * (n - 6)]


def _check_items(oracle, seq, sts, e, p, status, cst=None, motif=None, mfe=False):
    """Every item of one sequence against the yardstick; p None: no probabilities."""
    g = None
    for k, st in enumerate(sts):
        want = sec.status(seq, st, cst)
        assert status[k] == want, (seq, cst, st, status[k], want)
        if want == sec.BIGLOOP and motif is not None:
            continue
        ref = sec.expected_energy(oracle, seq, st, cst, motif, mfe)
        assert sec.same(e[k], ref, 0.0 if mfe else TOL_PF), (seq, cst, st, e[k], ref)
        if p is None:
            continue
        if want != 0:
            assert p[k] == 0.0, (seq, st, p[k])
        else:
            g = oracle.pf_energy(seq, cst, motif) if g is None else g
            pref = math.exp(-(ref - g) / sec.KT)
            assert abs(p[k] - pref) <= REL_P * pref, (seq, cst, st, p[k], pref)


# ------------------------------------------------------------------ fold layer
def test_fold_five_bases(native, oracle):
    for seq in ("AAAAA", "GAAAC"):
        sts = structures(seq) + ["(...)", "(..).", "((.))", "(....", "..x.."]
        e, p, st = _fold(native, seq).eval_structures(sts, with_probs=True)
        _check_items(oracle, seq, sts, e, p, st)
        e, p, st = _fold(native, seq).eval_structures(sts, convention="mfe")
        assert p is None
        _check_items(oracle, seq, sts, e, None, st, mfe=True)
    assert len(structures("AAAAA")) == 1 and len(structures("GAAAC")) == 2


@pytest.mark.parametrize("seq", MERS14)
def test_fold_enumerated_14mers(native, oracle, seq):
    sts = structures(seq)
    e, p, st = _fold(native, seq).eval_structures(sts, with_probs=True)
    _check_items(oracle, seq, sts, e, p, st)
    assert abs(p.sum() - 1.0) <= REL_P
    for k, s in enumerate(sts):   # apo, no loop above 30: the host's bits
        assert e[k] == oracle.eval_structure(seq, s), (seq, s)
    e, _, st = _fold(native, seq).eval_structures(sts, convention="mfe")
    _check_items(oracle, seq, sts, e, None, st, mfe=True)


@pytest.mark.parametrize("seq,cst", CONSTRAINED)
def test_fold_membership_under_constraints(native, oracle, seq, cst):
    sts = structures(seq) + _mutants(len(seq))
    admitted = set(structures(seq, cst))
    e, p, st = _fold(native, seq, cst).eval_structures(sts, with_probs=True)
    _check_items(oracle, seq, sts, e, p, st, cst)
    for k, s in enumerate(sts):
        assert (st[k] == 0) == (s in admitted), (seq, cst, s)
    if admitted:
        assert abs(p.sum() - 1.0) <= REL_P
    else:
        assert p.sum() == 0.0


def _length_cases():
    rng = random.Random(41)
    out = []
    for n in (63, 64, 65, 100):
        seq = rand_seq(rng, n)
        out.append((seq, None))
        out.append((seq, cons(rng, seq)))
    return out


@pytest.mark.parametrize("seq,cst", _length_cases())
def test_fold_lengths(native, oracle, seq, cst):
    """One, exactly one and two lane passes, and 100: the MFE structure, samples of the
    ensemble and non-members between them."""
    n = len(seq)
    f = _fold(native, seq, cst)
    _, samples = f.sample_structures(6, seed=3)
    _, best = f.mfe_structure()
    mut = _mutants(n)
    sts = [best, mut[0], samples[0], mut[2], samples[1], samples[2], mut[4], samples[3], samples[4], mut[5], samples[5]]
    e, p, st = f.eval_structures(sts, with_probs=True)
    _check_items(oracle, seq, sts, e, p, st, cst)
    assert st[0] == 0 and all(st[k] == 0 for k in (2, 4, 5, 7, 8, 10))
    e, _, st = f.eval_structures(sts, convention="mfe")
    _check_items(oracle, seq, sts, e, None, st, cst, mfe=True)
    assert np.float32(e[0]) == np.float32(oracle.mfe_energy(seq, cst))   # the optimum costs the optimum


def test_fold_motif_and_long_loops(native, oracle):
    apt = workloads.THEO_SEQ
    seq = workloads.synthetic(100)[0].upper()
    o = seq.index(apt)
    m = _motif(oracle)
    f = _fold(native, seq, motif=True)
    _, samples = f.sample_structures(16, seed=11)
    _, best = f.mfe_structure()
    assert best[o:o + 27] == workloads.THEO_FOLD   # the ligand pays
    opened = best[:o] + "." + best[o + 1:o + 26] + "." + best[o + 27:]   # the site unformed: the apo loops
    sts = [best] + samples + [opened]
    e, p, st = f.eval_structures(sts, with_probs=True)
    _check_items(oracle, seq, sts, e, p, st, None, m)
    e, _, st = f.eval_structures(sts, convention="mfe")
    _check_items(oracle, seq, sts, e, None, st, None, m, mfe=True)
    # hairpins of 31 and 57 and a 35-base interior loop (status 8: priced, no member)
    for st_ in ("((" + "." * 31 + "))", "((" + "." * 57 + "))", "((" + "." * 20 + "((.....))" + "." * 15 + "))"):
        s = "".join("G" if c == "(" else "C" if c == ")" else "A" for c in st_)
        e, p, st = _fold(native, s).eval_structures([st_, "." * len(s)], with_probs=True)
        _check_items(oracle, s, [st_, "." * len(s)], e, p, st)
        assert abs(e[0] - oracle.eval_structure(s, st_)) <= TOL_PF


# ------------------------------------------------------------------ contexts
def _engine(native, tmpl, macro, fold_mode, contexts=None):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    return native.Engine(tmpl, macro, workloads.default_objective(), aptamer=apt, contexts=contexts,
                         fold_mode=fold_mode, thermostat=native.make_thermostat("fixed", t=1.0))


def _variant_args(eng, v, active, ctx, oracle):
    c, cond, mac = eng.variant(v)
    b, a = ctx[c] if ctx else ("", "")
    cst = "." * len(b) + active + "." * len(a) if mac >= 0 else None
    return b, a, cst, (_motif(oracle) if cond == 1 else None)


@pytest.mark.parametrize("N,ctx", [(60, None), (143, [("GGAC", "UUA")])])
def test_mfe_walkers_structures_evaluate_to_their_energies(native, oracle, N, ctx):
    """MFE context, W = 8: what adx_walkers_mfe_structures returns prices to that call's
    energies bit for bit as float32; with the context, folds of 150."""
    tmpl, active = workloads.synthetic(N)
    W = 8
    eng = _engine(native, tmpl, [active], "mfe", ctx)
    seqs = workloads.walker_sequences(tmpl, [active], W)
    eng.walkers_init(list(range(W)), seqs)
    formed = 0
    for v in range(eng.info.n_variants):
        b, a, cst, m = _variant_args(eng, v, active, ctx, oracle)
        st, e32 = eng.walker_structures(v)
        assert len(st[0]) == N + len(b) + len(a)
        e, p, status = eng.eval_structures(seqs, v, [[s] for s in st])
        assert p is None and (status == 0).all(), (v, status)
        assert e[:, 0].astype(np.float32).tobytes() == e32.tobytes(), (v, e[:, 0], e32)
        o = len(b) + (N - 27) // 2
        formed += sum(m is not None and s[o:o + 27] == workloads.THEO_FOLD for s in st)
        w = v % W   # one pinned oracle fold per variant
        assert e[w, 0] == sec.mfe_energy(oracle, b + seqs[w] + a, st[w], m), (v, w)
    assert formed >= 1
    with pytest.raises(native.AdxError) as ei:
        eng.eval_structures(seqs, 0, [[s] for s in st], with_probs=True)
    assert ei.value.status == native.EUNSUPPORTED


def test_pf_samples_evaluate_to_the_pinned_folds(native, oracle):
    """PF context, W = 4, 64 samples: adx_sample_structures_batch's output passes straight in."""
    tmpl, active = workloads.synthetic(60)
    ctx = [("GGAC", "UUA")]
    W, S = 4, 64
    eng = _engine(native, tmpl, [active], "pf", ctx)
    seqs = workloads.walker_sequences(tmpl, [active], W)
    for v in range(eng.info.n_variants):
        b, a, cst, m = _variant_args(eng, v, active, ctx, oracle)
        samples, g32 = eng.sample_structures(seqs, v, S, seed=5)
        e, p, status = eng.eval_structures(seqs, v, samples, with_probs=True)
        assert e.shape == p.shape == status.shape == (W, S)
        assert (status == 0).all(), (v, status)
        for w in range(W):
            full = b + seqs[w] + a
            g = oracle.pf_energy(full, cst, m)
            memo = {}
            for k, s in enumerate(samples[w]):
                if s not in memo:
                    memo[s] = sec.pf_energy(oracle, full, s, m)
                assert abs(e[w, k] - memo[s]) <= TOL_PF, (v, w, s, e[w, k], memo[s])
                pref = math.exp(-(memo[s] - g) / sec.KT)
                assert abs(p[w, k] - pref) <= REL_P * pref, (v, w, s, p[w, k], pref)
        e2, p2, s2 = eng.eval_structures(seqs, v, samples)
        assert p2 is None and e2.tobytes() == e.tobytes() and s2.tobytes() == status.tobytes()
    fill, ev = eng.last_eval_ms()
    assert fill == 0.0 and ev > 0.0


def test_pf_items_at_a_padded_150(native, oracle):
    """PF context at N = 143 in a context: folds of 150, three lane passes, with probabilities."""
    tmpl, active = workloads.synthetic(143)
    ctx = [("GGAC", "UUA")]
    W, S = 2, 4
    eng = _engine(native, tmpl, [active], "pf", ctx)
    seqs = workloads.walker_sequences(tmpl, [active], W)
    for v in range(eng.info.n_variants):
        b, a, cst, m = _variant_args(eng, v, active, ctx, oracle)
        samples, _ = eng.sample_structures(seqs, v, S, seed=9)
        sts = [row + ["(" + "." * 149] for row in samples]
        e, p, status = eng.eval_structures(seqs, v, sts, with_probs=True)
        for w in range(W):
            assert len(sts[w][0]) == 150
            _check_items(oracle, b + seqs[w] + a, sts[w], e[w], p[w], status[w], cst, m)
            assert (status[w][:S] == 0).all() and status[w][S] == sec.MALFORMED


def test_results_do_not_depend_on_the_launch_chunks(native, monkeypatch):
    """ADX_EVAL_CHUNK cuts the sequences into launches of 3, 3 and 2: the same bytes."""
    tmpl, active = workloads.synthetic(60)
    W, S = 8, 5
    eng = _engine(native, tmpl, [active], "pf")
    seqs = workloads.walker_sequences(tmpl, [active], W)
    eng.walkers_init(list(range(W)), seqs)
    for v in (0, eng.info.n_variants - 1):
        samples, _ = eng.sample_structures(seqs, v, S, seed=2)
        whole = eng.eval_structures(seqs, v, samples, with_probs=True)
        shared = eng.walker_eval_structures(v, samples[0], with_probs=True)
        monkeypatch.setenv("ADX_EVAL_CHUNK", "3")
        cut = eng.eval_structures(seqs, v, samples, with_probs=True)
        cut_shared = eng.walker_eval_structures(v, samples[0], with_probs=True)
        monkeypatch.delenv("ADX_EVAL_CHUNK")
        for x, y in zip(whole + shared, cut + cut_shared):
            assert x.tobytes() == y.tobytes(), v
        assert (whole[2] == 0).all() and len(set(whole[0].ravel())) > W


@pytest.mark.parametrize("fold_mode", ["pf", "mfe"])
def test_walker_targets_equal_the_batch_call_and_leave_the_state(native, fold_mode):
    tmpl, active = workloads.synthetic(60)
    W = 8
    seqs = workloads.walker_sequences(tmpl, [active], W)
    probs = fold_mode == "pf"

    def engine():
        eng = _engine(native, tmpl, [active], fold_mode)
        eng.walkers_init(list(range(W)), seqs)
        eng.run_steps(4)
        return eng

    eng, plain = engine(), engine()
    with pytest.raises(native.AdxError) as ei:
        _engine(native, tmpl, [active], fold_mode).walker_eval_structures(0, [active.replace("x", ".")])
    assert ei.value.status == native.ESTATE
    cur = eng.download()[0]
    assert cur != seqs
    o = (60 - 27) // 2
    targets = [active.replace("x", "."), "." * 60, "." * o + workloads.THEO_FOLD + "." * (60 - 27 - o),
               "((((((" + "." * 47 + ")))))))", "." * 30 + "(.)" + "." * 27]
    for v in range(eng.info.n_variants):
        e, p, st = eng.walker_eval_structures(v, targets, with_probs=probs)
        e2, p2, st2 = eng.eval_structures(cur, v, [targets] * W, with_probs=probs)
        assert e.shape == (W, len(targets))
        assert e.tobytes() == e2.tobytes() and st.tobytes() == st2.tobytes(), v
        if probs:
            assert p.tobytes() == p2.tobytes(), v
        assert (st[:, 3] == sec.MALFORMED).all() and np.isnan(e[:, 3]).all()
        assert ((st[:, 4] & sec.HAIRPIN) != 0).all()
        assert (st[:, 1] == 0).all() or eng.variant(v)[2] >= 0   # the open chain: out under the macrostate only
    a, b = eng.run_steps(4, trace=True), plain.run_steps(4, trace=True)
    for k in ("position", "outcome", "proposed_score", "current_score"):
        assert a[k].tobytes() == b[k].tobytes(), k
    fa, fb = eng.download(), plain.download()
    assert fa[0] == fb[0] and fa[1].tobytes() == fb[1].tobytes()


# ------------------------------------------------------------------ malformed and excluded items
def test_bad_items_do_not_disturb_their_neighbours(native, oracle):
    seq, cst = "GCGCUUCGGCGC", "....xxxx...."
    good = structures(seq)
    f = _fold(native, seq, cst)
    e0, p0, s0 = f.eval_structures(good, with_probs=True)
    bad = _mutants(len(seq))
    mixed = []
    for k, s in enumerate(good):
        mixed += [s, bad[k % len(bad)]]
    e, p, st = f.eval_structures(mixed, with_probs=True)
    assert e[0::2].tobytes() == e0.tobytes() and p[0::2].tobytes() == p0.tobytes() and st[0::2].tobytes() == s0.tobytes()
    _check_items(oracle, seq, mixed, e, p, st, cst)
    seen = 0
    for k, s in enumerate(mixed):
        seen |= int(st[k])
        if st[k] & sec.MALFORMED:
            assert math.isnan(e[k]) and p[k] == 0.0
        elif st[k] & (sec.HAIRPIN | sec.EXCLUDED):
            assert e[k] == math.inf and p[k] == 0.0
    assert seen & 7 == 7


def test_errors(native):
    L = native.lib()
    f = _fold(native, "GGGAAACCC")
    buf = b"(((...)))"
    e = (native.C.c_double * 1)()
    assert L.adx_fold_eval_structures(None, 0, 1, buf, e, None, None) == native.EINVAL
    assert L.adx_fold_eval_structures(f.ptr, 0, 1, None, e, None, None) == native.EINVAL
    assert L.adx_fold_eval_structures(f.ptr, 0, 1, buf, None, None, None) == native.EINVAL
    assert L.adx_fold_eval_structures(f.ptr, 2, 1, buf, e, None, None) == native.EINVAL
    assert L.adx_fold_eval_structures(f.ptr, 0, 0, buf, e, None, None) == native.EINVAL
    assert L.adx_fold_eval_structures(f.ptr, 1, 1, buf, e, e, None) == native.EINVAL   # no probabilities in the MFE convention
    assert b"probabilities" in L.adx_last_error()
    assert L.adx_fold_eval_structures(f.ptr, 0, 1, buf, e, None, None) == native.OK   # probs and status optional
    tmpl, active = workloads.synthetic(60)
    eng = _engine(native, tmpl, [active], "pf")
    seqs = workloads.walker_sequences(tmpl, [active], 2)
    for v in (-1, eng.info.n_variants):
        with pytest.raises(native.AdxError) as ei:
            eng.eval_structures(seqs, v, [["." * 60]] * 2)
        assert ei.value.status == native.EINVAL
    sb = b"".join(s.encode() for s in seqs)
    e2 = (native.C.c_double * 2)()
    assert L.adx_eval_structures_batch(eng.ptr, 2, sb, 0, 0, b"." * 120, e2, None, None) == native.EINVAL
    assert L.adx_eval_structures_batch(eng.ptr, 2, sb, 0, 1, b"." * 120, None, None, None) == native.EINVAL
    assert L.adx_eval_structures_batch(eng.ptr, 0, sb, 0, 1, b"." * 120, e2, None, None) == native.EINVAL
    assert L.adx_last_eval_ms(eng.ptr, None, None) == native.EINVAL
