"""mfe_pair_kernel's persistent workgroups: what one fold leaves in a
workgroup's LDS and registers must not reach the next.

A workgroup takes (walker, fold group) items from a queue until it is empty
(mfe_pair.hip), so the energy tables it loaded once, the block_or words, the
16-bit range flag and every table of the fold before are still in LDS when the
next fold starts.  ADX_PAIR_GRID sets the number of workgroups: at 1 a single
workgroup runs every item of a launch back to back -- alternating fold groups
(free / constrained), refolds after folds from scratch, shorter folds after
longer ones -- and the results must not differ by a bit from any other grid,
from the one-diagonal kernel (ADX_MFE_PAIR=0) and from the oracle.
"""
import random

import numpy as np
import pytest

from addapt_amd import workloads
from test_gpu_mfe import _close, _engine, _oracle_sf, _same, rand_constraint

pytestmark = pytest.mark.gpu

TERMS2 = [("apo", 0, False, 1.0), ("holo", 0, True, 1.0), ("apo", 1, True, 0.5), ("holo", 1, False, 2.0)]


def _env(monkeypatch, grid=None, pair="1", no_order=False):
    for name, value in (("ADX_PAIR_GRID", grid), ("ADX_MFE_PAIR", pair), ("ADX_NO_ORDER", "1" if no_order else None)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


@pytest.mark.parametrize("N", [60, 100])
def test_trajectories_do_not_depend_on_the_grid(native, monkeypatch, N):
    """48 walkers, 25 annealing steps: at grid 1 one workgroup runs up to 96 items
    per step in sequence (both fold groups of every scored walker; step 0 folds
    from scratch, later steps refold, with unscored walkers behind the scored
    ones).  Grids 1, 3, the default, the one-diagonal kernel, and grid 3 without
    the order list: identical traces, final sequences, scores and counters."""
    tmpl, active = workloads.synthetic(N)
    terms = workloads.default_objective()
    W, steps = 48, 25
    seqs = workloads.walker_sequences(tmpl, [active], W)
    runs = {}
    for name, kw in (("grid1", dict(grid=1)), ("grid3", dict(grid=3)), ("default", dict()),
                     ("single", dict(pair="0")), ("grid3-no-order", dict(grid=3, no_order=True))):
        _env(monkeypatch, **kw)
        eng = _engine(native, tmpl, [active], terms,
                      thermostat=native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30))
        eng.walkers_init(list(range(W)), seqs)
        tr = eng.run_steps(steps, trace=True)
        assert ("mfe_pair_kernel" in eng.last_kernel_names()[0]) == (name != "single")
        runs[name] = (tr, eng.download())
    tr0, (s0, sc0, c0) = runs["single"]
    assert (tr0["outcome"] != 2).sum() < W * steps   # some proposals go unscored
    for name, (tr, (s, sc, c)) in runs.items():
        for key in ("position", "outcome"):
            assert (tr[key] == tr0[key]).all(), (N, name, key)
        assert tr["base"] == tr0["base"], (N, name)
        scored = tr0["outcome"] != 2
        assert (tr["proposed_score"][scored] == tr0["proposed_score"][scored]).all(), (N, name)
        assert s == s0, (N, name)
        assert (sc == sc0).all(), (N, name)
        assert (c == c0).all(), (N, name)


def _batch(N, seed):
    """12 sequences (every fourth GC-only: every cell pairable) and two random
    constraints; the engine folds every sequence free and under each constraint,
    so a workgroup's items alternate between unconstrained and constrained folds."""
    rng = random.Random(seed)
    seqs = ["".join(rng.choice("GC" if k % 4 == 3 else "ACGU") for _ in range(N)) for k in range(12)]
    return seqs, [rand_constraint(rng, N), rand_constraint(rng, N)]


@pytest.mark.parametrize("N", [20, 33, 64, 65, 100])
def test_score_batch_back_to_back(native, oracle, monkeypatch, N):
    """Folds without stored tables or an order list (score_batch), 36 items in one
    workgroup (grid 1) or two: bit-equal to the oracle and the one-diagonal kernel."""
    seqs, csts = _batch(N, 2000 + N)
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    motif = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    got = {}
    for name, kw in (("grid1", dict(grid=1)), ("grid2", dict(grid=2)), ("single", dict(pair="0"))):
        _env(monkeypatch, **kw)
        eng = native.Engine(seqs[0], csts, TERMS2, aptamer=apt, fold_mode="mfe",
                            thermostat=native.make_thermostat("fixed", t=1.0))
        _, _, dg = eng.score_batch(seqs)
        got[name] = dg.copy()
        names = [eng.variant(v) for v in range(eng.info.n_variants)]
    assert len({mac for _, _, mac in names}) == 3   # free and both constraints: three fold groups
    ref = np.array([[oracle.mfe_energy(s, csts[mac] if mac >= 0 else None, motif if cond == 1 else None)
                     for _, cond, mac in names] for s in seqs], np.float32)
    for name, dg in got.items():
        for w in range(len(seqs)):
            for v in range(len(names)):
                assert _same(dg[w, v], ref[w, v]), (N, name, w, v, dg[w, v], ref[w, v])
        assert dg.tobytes() == got["single"].tobytes(), (N, name)


def test_score_batch_back_to_back_lengths_change(native, oracle, monkeypatch):
    """Contexts of different lengths: the variants of one engine fold at 67, 64 and
    66 nt, so in a single workgroup a shorter fold follows a longer one in the
    tables the longer one filled."""
    N = 60
    seqs, csts = _batch(N, 2999)
    ctx = [("GGAC", "UUA"), ("", "CCCA"), ("AUAUAU", "")]
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    got = {}
    for name, kw in (("grid1", dict(grid=1)), ("grid2", dict(grid=2)), ("single", dict(pair="0"))):
        _env(monkeypatch, **kw)
        eng = native.Engine(seqs[0], csts, TERMS2, aptamer=apt, contexts=ctx, fold_mode="mfe",
                            thermostat=native.make_thermostat("fixed", t=1.0))
        sc, _, dg = eng.score_batch(seqs)
        got[name] = (sc.copy(), dg.copy())
    sf = _oracle_sf(oracle, TERMS2, contexts=ctx)
    for name, (sc, dg) in got.items():
        assert dg.tobytes() == got["single"][1].tobytes(), name
        for w, s in enumerate(seqs):
            ref, _ = sf.score(s, csts)
            assert _close(sc[w], ref), (name, w, sc[w], ref)


def test_range_flag_does_not_leak(native, oracle, monkeypatch):
    """A fold below the 16-bit floor (-120 kcal/mol) between ordinary ones in the
    same workgroup: it alone takes the FP32 fallback, and the folds after it are
    what they are when scored alone."""
    tmpl, active = workloads.synthetic(100)
    terms = workloads.default_objective()
    low = "G" * 48 + "AAAA" + "C" * 48
    assert oracle.mfe_energy(low) < -120.0
    ordinary = workloads.walker_sequences(tmpl, [active], 3)
    seqs = [ordinary[0], low, ordinary[1], ordinary[2]]
    _env(monkeypatch, grid=1)
    eng = _engine(native, tmpl, [active], terms)
    _, _, dg = eng.score_batch(seqs)
    motif = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    for v in range(eng.info.n_variants):
        _, cond, mac = eng.variant(v)
        for w, s in enumerate(seqs):
            ref = oracle.mfe_energy(s, active if mac >= 0 else None, motif if cond == 1 else None)
            assert _same(dg[w, v], ref), (v, w, dg[w, v], ref)
    for w in (0, 2, 3):
        _, _, alone = eng.score_batch([seqs[w]])
        assert alone[0].tobytes() == dg[w].tobytes(), w


def test_grid_larger_than_the_queue(native, monkeypatch):
    """4096 workgroups for 16 items: most find the queue empty at once."""
    tmpl, active = workloads.synthetic(100)
    terms = workloads.default_objective()
    seqs = workloads.walker_sequences(tmpl, [active], 8)
    got = {}
    for name, kw in (("default", dict()), ("grid4096", dict(grid=4096))):
        _env(monkeypatch, **kw)
        eng = _engine(native, tmpl, [active], terms,
                      thermostat=native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=30))
        _, _, dg = eng.score_batch(seqs)
        eng.walkers_init(list(range(8)), seqs)
        eng.run_steps(5)
        got[name] = (dg.copy(), eng.download())
    assert got["default"][0].tobytes() == got["grid4096"][0].tobytes()
    s0, sc0, c0 = got["default"][1]
    s1, sc1, c1 = got["grid4096"][1]
    assert s0 == s1 and (sc0 == sc1).all() and (c0 == c1).all()
