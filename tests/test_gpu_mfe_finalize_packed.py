"""The pair kernel's packed finalize (mfe_pair.hip, finalize_packed).

A step whose row window fits a half-wave finalizes both cells of a row side by
side on the finalize wave, lanes 0..31 the span-e0 cell and lanes 32..63 the
span-e1 cell (tests/test_finalize_packed_model.py has the model).  Every
result must stay what the two-cells-per-lane mode gives, bit for bit:

* short traced MC runs at N = 60 (the NM = 64 instantiation), 70 and 100
  reproduce the oracle's trajectory and the one-diagonal kernel's
  (ADX_MFE_PAIR=0), and the tables left in the walkers' slots score the final
  sequences as folds from scratch do.  The seeds were chosen with the oracle
  alone, on the CPU, so that the scored proposals reach every kind of sweep the
  model finds among the template's moves (_kinds below); the tests assert it.
  The N = 70 run has one workgroup (ADX_PAIR_GRID=1), which then meets items of
  every mode in turn;
* folds from scratch (native.Fold) at the lengths around the boundary: at
  N <= 36 every step is packed, at 37 the first is not, 64 and 65 switch the
  instantiation.
"""
import math
import random

import numpy as np
import pytest

from addapt_amd import workloads
from test_finalize_anchor_model import steps, window
from test_finalize_packed_model import _moves, choose
from test_gpu_mfe import _same, rand_constraint, rand_seq

pytestmark = pytest.mark.gpu

W, STEPS = 6, 50
SEEDS = list(range(W))
GRID1 = 70   # the length whose pair-kernel run has a single workgroup


def _modes(N, lo, hi):
    """The model's mode of every step of a refold with hull [lo, hi] (True: packed)."""
    ab, pk, out = np.int64(0), np.bool_(False), []
    for d in steps(N):
        if d - 2 <= N - 1:
            fr, lr, _ = window(d, N, lo, hi)
            _, ab, pk = choose(ab, pk, fr, lr)
            out.append(bool(pk))
    return out


def _kinds(N, p, lo, hi):
    """The kinds of sweep a move at 0-based position p (hull [lo, hi], 1-based) belongs to."""
    m = _modes(N, lo, hi)
    o = (N - 27) // 2                     # the frozen aptamer's offset (workloads.synthetic)
    changes = sum(a != b for a, b in zip(m, m[1:]))
    return {"every step packed (5' end)": all(m) and p <= 12,
            "packed -> two cells per lane -> packed": m[0] and m[-1] and changes == 2,
            "helix partners: two cells per lane early, packed late": lo != hi and not m[0] and m[-1],
            "3' end outside the helix (no ghost row on the long spans)": lo == hi and N - 12 <= p <= N - 7,
            "beside an x flank": p in (o - 7, o + 33)}


def _covers(N, positions, outcomes):
    """Which kinds the scored proposals reach, and which the template's moves can reach at all."""
    hull = {p: (lo, hi) for p, lo, hi in _moves(N)}
    can = {k: False for k in _kinds(N, 0, 1, N)}
    got = dict(can)
    for p, (lo, hi) in hull.items():
        for k, v in _kinds(N, p, lo, hi).items():
            can[k] = can[k] or v
    for p in set(int(p) for p, o in zip(positions, outcomes) if int(o) != 2):
        for k, v in _kinds(N, p, *hull[p]).items():
            got[k] = got[k] or v
    return got, can


def _close(a, b):
    if math.isinf(b) or math.isnan(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


_runs = {}


def _gpu_run(native, monkeypatch, N, pair="1"):
    """One traced MC run per (N, kernel), shared by the tests."""
    key = (N, pair)
    if key not in _runs:
        monkeypatch.setenv("ADX_MFE_PAIR", pair)
        if pair == "1" and N == GRID1:
            monkeypatch.setenv("ADX_PAIR_GRID", "1")
        else:
            monkeypatch.delenv("ADX_PAIR_GRID", raising=False)
        tmpl, active = workloads.synthetic(N)
        apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
        eng = native.Engine(tmpl, [active], workloads.default_objective(), aptamer=apt, fold_mode="mfe",
                            thermostat=native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=STEPS))
        seqs = workloads.walker_sequences(tmpl, [active], W)
        eng.walkers_init(SEEDS, seqs)
        tr = eng.run_steps(STEPS, trace=True)
        names = eng.last_kernel_names()[0]
        final, scores, counters = eng.download()
        rescored, _, _ = eng.score_batch(final)   # folds from scratch
        _runs[key] = dict(active=active, seqs=seqs, tr=tr, final=final, scores=scores, counters=counters,
                          rescored=rescored, kernel=names)
    return _runs[key]


def test_every_kind_of_sweep_exists_at_100():
    """The coverage asked of the N = 100 run is all five kinds; N = 60 has no
    one-position window of more than 32 rows (the model says which kinds exist)."""
    _, can = _covers(100, [], [])
    assert all(can.values()), can
    _, can = _covers(60, [], [])
    assert not can["packed -> two cells per lane -> packed"]


@pytest.mark.parametrize("N", [60, 70, 100])
def test_finalize_packed_trajectory(native, oracle, monkeypatch, N):
    r = _gpu_run(native, monkeypatch, N)
    assert "mfe_pair_kernel" in r["kernel"]
    tr = r["tr"]
    got, can = _covers(N, tr["position"].ravel(), tr["outcome"].ravel())
    assert got == can, (N, got, can)
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    sf = oracle.ScoreFunction(workloads.default_objective(), aptamer=m, mode="mfe")
    therm_o = oracle.thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=STEPS)
    for w, seed in enumerate(SEEDS):
        # exact energies; only a last-ulp exp() difference at |crit - u| < 1e-12 may be forced
        forced = [int(x) for x in tr["outcome"][:, w]]
        ref = oracle.mc_run(sf, r["seqs"][w], [r["active"]], therm_o, seed, STEPS, forced=forced, tie_eps=1e-12)
        assert ref["rc"] == 0
        assert list(tr["position"][:, w]) == ref["pos"], (N, w)
        assert list(tr["outcome"][:, w]) == ref["outcome"], (N, w)
        for s in range(STEPS):
            if ref["outcome"][s] != 2:
                assert _close(tr["proposed_score"][s, w], ref["proposed_score"][s]), (N, w, s)
        assert r["final"][w].upper() == ref["seq"].upper(), (N, w)
        assert _close(r["scores"][w], ref["score"]), (N, w)
        assert list(r["counters"][w]) == ref["counters"], (N, w)
        # a wrong table left in the walker's slot would show in the stored score
        assert _close(r["scores"][w], r["rescored"][w]), (N, w, r["scores"][w], r["rescored"][w])


@pytest.mark.parametrize("N", [60, 70, 100])
def test_finalize_packed_pair_equals_single(native, monkeypatch, N):
    """The same walkers with the one-diagonal kernel (ADX_MFE_PAIR=0, mfe_cells.hip)."""
    a = _gpu_run(native, monkeypatch, N, pair="1")
    b = _gpu_run(native, monkeypatch, N, pair="0")
    assert "mfe_pair_kernel" in a["kernel"] and "mfe_pair_kernel" not in b["kernel"]
    assert (a["tr"]["position"] == b["tr"]["position"]).all()
    assert (a["tr"]["outcome"] == b["tr"]["outcome"]).all()
    assert a["tr"]["base"] == b["tr"]["base"]
    ok = a["tr"]["outcome"] != 2   # a proposal that was not scored has no score
    assert (a["tr"]["proposed_score"][ok] == b["tr"]["proposed_score"][ok]).all()
    assert a["final"] == b["final"]
    assert (a["scores"] == b["scores"]).all()
    assert (a["counters"] == b["counters"]).all()


@pytest.mark.parametrize("N", [33, 36, 37, 38, 40, 64, 65])
def test_fold_from_scratch_around_the_boundary(native, oracle, N):
    """A fold from scratch has R = N - e0 rows: packed from the step with R <= 32 on, so
    from the first step at N <= 36.  Plain, under a random constraint, with the motif."""
    modes = _modes(N, -4096, 4096)
    assert all(modes) == (N <= 36) and modes[-1]
    rng = random.Random(3100 + N)
    apt, fold, bonus = workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus()
    motif = oracle.make_motif(apt, fold, bonus)
    for k in range(4):
        seq = rand_seq(rng, N) if k else "".join(rng.choice("GC") for _ in range(N))   # one with every cell pairable
        cst = rand_constraint(rng, N)
        tail = rand_seq(rng, N - len(apt) - 2) if N > len(apt) + 2 else ""
        with_apt = ("GG" + apt + tail)[:N] if N >= len(apt) + 2 else seq
        for s, c, mo in ((seq, None, None), (seq, cst, None), (with_apt, None, motif)):
            f = native.Fold(s)
            if mo is not None:
                f.add_motif(apt, fold, bonus)
            if c:
                f.add_constraint(c)
            g = f.mfe()
            ref = oracle.mfe_energy(s, c, mo)
            assert _same(g, ref), (N, s, c, mo is not None, g, ref)
