"""The pair kernel's finalize with anchored lanes (mfe_pair.hip, role F).

The finalize lanes keep their rows while an anchor holds and advance last
step's addresses by deltas; the closed forms run only when the anchor is
chosen (tests/test_finalize_anchor_model.py has the model).  Short traced MC
runs must reproduce the oracle's trajectory bit for bit, and the tables left
in the walkers' slots must score the final sequences as a fold from scratch
does, at

* N = 59: the shortest template workloads.synthetic accepts (NM = 64); no
  one-position refold re-anchors;
* N = 64: NM = 64 at its limit;
* N = 70: a short length at which one-position refolds re-anchor (changed
  1-based rows 62 to 64, the last mutable positions before the enforced
  helix; the predicate asks for row 63 or beyond);
* N = 100, also with MLbase = 30 (the ghost row's hand-down is non-trivial)
  and against the one-diagonal kernel (ADX_MFE_PAIR=0).

The seeds were chosen with the oracle alone, on the CPU, so that the scored
proposals of each run satisfy _covers below; the tests assert it.
"""
import math
import os

import pytest

from addapt_amd import workloads

pytestmark = pytest.mark.gpu

W, STEPS = 6, 50
SEEDS = list(range(W))
# a one-position refold re-anchors from this changed 1-based row on (the model's policy:
# anchor max(1, lr - 63), chosen again when the window's first row falls below it)
REANCHOR_ROW = {70: 63, 100: 62}


def _model_reanchors(N, row):
    """Whether the sweep of a one-position refold at `row` re-anchors (the model, restated)."""
    ab, n = 0, 0
    for d in range(6, N + 4, 2):
        e0, e1 = d - 2, d - 1
        if e0 > N - 1:
            break
        fr, lr = max(1, row - 2 - e1), min(N - e0, row + 3)
        if ab == 0 or fr < ab:
            n += ab != 0
            ab = max(1, lr - (63 if lr - fr < 64 else 126))
    return n > 0


def _covers(N, positions, outcomes):
    """The scored proposals (0-based device positions) reach every path of the anchored finalize."""
    s = set(int(p) for p, o in zip(positions, outcomes) if int(o) != 2)
    helix = lambda p: p <= 5 or p >= N - 6          # both partners of an enforced pair change
    cov = {"changed row <= 5 (the window clamps at row 1 from the first steps)": any(p + 1 <= 5 for p in s),
           "both partners of an enforced pair (two lane-sets)": any(helix(p) for p in s)}
    if N in REANCHOR_ROW:
        cov["one position at or beyond the re-anchor row"] = any(
            p + 1 >= REANCHOR_ROW[N] and not helix(p) for p in s)
    return cov


def _close(a, b):
    if math.isinf(b) or math.isnan(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


def _par_with_mlbase(tmp_path, mlbase):
    """The default parameter file with the multiloop unpaired-base energy set."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "addapt_amd", "data", "rna_turner2004_addapt.par")
    lines = open(src).read().split("\n")
    k = lines.index("# ML_params")
    while not lines[k].strip() or not lines[k].strip()[0].isdigit() and not lines[k].strip().startswith("-"):
        k += 1
    vals = lines[k].split()
    vals[0] = str(mlbase)
    lines[k] = "   " + "   ".join(vals)
    out = tmp_path / "mlbase.par"
    out.write_text("\n".join(lines))
    return str(out)


_runs = {}


def _gpu_run(native, monkeypatch, N, pair="1", par=None):
    """One traced MC run per (N, kernel, parameters), shared by the tests."""
    key = (N, pair, par)
    if key not in _runs:
        monkeypatch.setenv("ADX_MFE_PAIR", pair)
        tmpl, active = workloads.synthetic(N)
        apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
        eng = native.Engine(tmpl, [active], workloads.default_objective(), aptamer=apt, fold_mode="mfe",
                            params=native.Params(par) if par else None,
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


def _check_against_oracle(oracle, N, r, par=None):
    cov = _covers(N, r["tr"]["position"].ravel(), r["tr"]["outcome"].ravel())
    assert all(cov.values()), cov
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    sf = oracle.ScoreFunction(workloads.default_objective(), aptamer=m, mode="mfe",
                              params=oracle.Params(par) if par else None)
    therm_o = oracle.thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=STEPS)
    tr = r["tr"]
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


def test_reanchor_rows_are_the_models():
    """The coverage predicate's rows: the model re-anchors there, and nowhere at N <= 64."""
    for N, row in REANCHOR_ROW.items():
        assert _model_reanchors(N, row) and _model_reanchors(N, row + 1)
        assert not _model_reanchors(N, 61)
    for N in (59, 64):
        assert not any(_model_reanchors(N, row) for row in range(1, N + 1))


@pytest.mark.parametrize("N", [59, 64, 70, 100])
def test_finalize_anchor_trajectory(native, oracle, monkeypatch, N):
    r = _gpu_run(native, monkeypatch, N)
    assert "mfe_pair_kernel" in r["kernel"]
    _check_against_oracle(oracle, N, r)


def test_finalize_anchor_nonzero_mlbase(native, oracle, monkeypatch, tmp_path):
    """MLbase = 30: the ghost row's qm carries MLbase per unpaired row down the
    band.  ADX_MFE_PAIR=1 keeps the pair kernel for MLbase >= 0 (asserted)."""
    par = _par_with_mlbase(tmp_path, 30)
    r = _gpu_run(native, monkeypatch, 100, par=par)
    assert "mfe_pair_kernel" in r["kernel"]
    _check_against_oracle(oracle, 100, r, par=par)


def test_finalize_anchor_pair_equals_single(native, monkeypatch):
    """The same walkers with the one-diagonal kernel (ADX_MFE_PAIR=0, mfe_cells.hip)."""
    a = _gpu_run(native, monkeypatch, 100, pair="1")
    b = _gpu_run(native, monkeypatch, 100, pair="0")
    assert "mfe_pair_kernel" in a["kernel"] and "mfe_pair_kernel" not in b["kernel"]
    assert (a["tr"]["position"] == b["tr"]["position"]).all()
    assert (a["tr"]["outcome"] == b["tr"]["outcome"]).all()
    assert a["tr"]["base"] == b["tr"]["base"]
    ok = a["tr"]["outcome"] != 2   # a proposal that was not scored has no score
    assert (a["tr"]["proposed_score"][ok] == b["tr"]["proposed_score"][ok]).all()
    assert a["final"] == b["final"]
    assert (a["scores"] == b["scores"]).all()
    assert (a["counters"] == b["counters"]).all()
