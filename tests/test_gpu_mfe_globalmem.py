"""The pair kernel's accesses to device memory (mfe_pair.hip: global loads and
stores through fold_common.hpp gld / gst) and its 1x1 .. 2x2 energies by code
pair (loop_codetab_core.hpp).  Every result must stay what it was, bit for bit:

* short traced MC runs with the synthetic template at N = 59, 60, 61, 62 (the
  NM = 64 instantiation; 1540, 1596, 1653 and 1711 cells per table: even and odd
  counts, a multiple of four and not, so the restore and the write-back go
  through their 16-byte, 8-byte and single-word paths and the odd last cell) and
  at N = 100 (the other instantiation), each with one workgroup
  (ADX_PAIR_GRID=1), which takes every item in turn.  The thermostat is hot
  (T = 1e9): nearly every proposal is accepted, so the walkers' slots alternate.
  Each run reproduces the oracle's trajectory and the one-diagonal kernel's
  (ADX_MFE_PAIR=0), and the tables left in the slots score the final sequences
  as folds from scratch do;
* folds (native.Fold) at the shortest lengths at which each of the four tables is
  read, the structure pinned by a constraint, for every pair of pair types.
"""
import itertools
import math
import random

import numpy as np
import pytest

from addapt_amd import workloads
from test_gpu_mfe import _same

pytestmark = pytest.mark.gpu

W, STEPS, T_HOT = 4, 30, 1e9
SEEDS = list(range(W))
LENGTHS = [59, 60, 61, 62, 100]
CELLS = {59: 1540, 60: 1596, 61: 1653, 62: 1711, 100: 4656}
PAIRS = ("AU", "CG", "GC", "GU", "UA", "UG")   # the six pair types


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
        if pair == "1":
            monkeypatch.setenv("ADX_PAIR_GRID", "1")
        else:
            monkeypatch.delenv("ADX_PAIR_GRID", raising=False)
        tmpl, active = workloads.synthetic(N)
        apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
        eng = native.Engine(tmpl, [active], workloads.default_objective(), aptamer=apt, fold_mode="mfe",
                            thermostat=native.make_thermostat("fixed", t=T_HOT))
        seqs = workloads.walker_sequences(tmpl, [active], W)
        eng.walkers_init(SEEDS, seqs)
        tr = eng.run_steps(STEPS, trace=True)
        names = eng.last_kernel_names()[0]
        final, scores, counters = eng.download()
        rescored, _, _ = eng.score_batch(final)   # folds from scratch
        _runs[key] = dict(active=active, seqs=seqs, tr=tr, final=final, scores=scores, counters=counters,
                          rescored=rescored, kernel=names)
    return _runs[key]


def test_the_lengths_walk_every_alignment():
    """Cells per table: 16-byte vectors need a multiple of four, 8-byte ones an even count."""
    for N, c in CELLS.items():
        assert (N - 4) * (N - 3) // 2 == c
    assert [CELLS[N] % 4 for N in (59, 60, 61, 62)] == [0, 0, 1, 3]
    assert CELLS[59] % 16 != 0 and CELLS[60] % 16 != 0   # the codes' last 16-byte vector is partly past the cells
    assert all(N <= 64 for N in LENGTHS[:4]) and LENGTHS[4] > 64


@pytest.mark.parametrize("N", LENGTHS)
def test_globalmem_trajectory(native, oracle, monkeypatch, N):
    r = _gpu_run(native, monkeypatch, N)
    assert "mfe_pair_kernel" in r["kernel"]
    tr = r["tr"]
    # hot: the slots alternate (an accepted proposal makes the written slot the current one)
    # (outcomes 1 and 3: accepted; 2: the proposal was the base already there, about one in four)
    assert np.isin(tr["outcome"], (1, 3)).sum() >= W * STEPS // 2
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    sf = oracle.ScoreFunction(workloads.default_objective(), aptamer=m, mode="mfe")
    therm_o = oracle.thermostat("fixed", t=T_HOT)
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


@pytest.mark.parametrize("N", LENGTHS)
def test_globalmem_pair_equals_single(native, monkeypatch, N):
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


# (name, unpaired bases 5' of the inner pair, 3' of it): the closing pair (0, n - 1),
# the inner pair around a hairpin of three, every other base barred from pairing
TABLES = [("1x1", 1, 1), ("1x2", 1, 2), ("2x1", 2, 1), ("2x2", 2, 2)]
STRUCTURE = {"1x1": "(.(...).)", "1x2": "(.(...)..)", "2x1": "(..(...).)", "2x2": "(..(...)..)"}


@pytest.mark.parametrize("outer", PAIRS)
@pytest.mark.parametrize("name,n1,n2", TABLES, ids=[t[0] for t in TABLES])
def test_fold_reads_each_table(native, oracle, name, n1, n2, outer):
    """The shortest fold that reads the table, for every pair of pair types (a case per
    closing pair, every inner pair in it); the loop's unpaired bases in every combination
    (1x1) or 64 seeded samples of them (the others), the hairpin's bases drawn with them."""
    db = STRUCTURE[name]
    assert db == "(" + "." * n1 + "(...)" + "." * n2 + ")" and len(db) == 7 + n1 + n2
    cst = db.replace(".", "x")
    rng = random.Random(4100 + 100 * PAIRS.index(outer) + 10 * n1 + n2)
    every = ["".join(t) for t in itertools.product("ACGU", repeat=n1 + n2)]
    for inner in PAIRS:
        loops = every if name == "1x1" else [rng.choice(every) for _ in range(64)]
        assert len(loops) == (16 if name == "1x1" else 64)
        for lp in loops:
            hp = "".join(rng.choice("ACGU") for _ in range(3))
            s = outer[0] + lp[:n1] + inner[0] + hp + inner[1] + lp[n1:] + outer[1]
            f = native.Fold(s)
            f.add_constraint(cst)
            g = f.mfe()
            ref = oracle.mfe_energy(s, cst)
            assert not math.isinf(ref), (s, cst)
            assert _same(g, ref), (name, s, g, ref)
