"""The pair kernel's finalize over a refold's row window (mfe_pair.hip, role F).

An incremental refold finalizes only the rows whose qm it rewrites plus one
ghost row above them (tests/test_qm_boundary.py has the identity); a fold from
scratch still runs every row.  Short MC runs whose proposals reach every shape
of that window -- both partners of an enforced pair (the full band: two
lane-sets on the early spans at N = 100, and at spans 4 and 5 alone at N = 70;
N = 60 runs the NM = 64 instantiation with one lane-set always), a position
near the 5' end (the window clamps at row 1), one near the 3' end (the ghost
row is missing on the long spans) and one beside the 'x' flanks -- must
reproduce the oracle's trajectory bit for bit, and the tables left in the
walkers' slots must score the final sequences as a fold from scratch does."""
import math
import os

import pytest

from addapt_amd import workloads

pytestmark = pytest.mark.gpu

W, STEPS = 6, 50
SEEDS = list(range(W))   # chosen with the oracle alone: its proposals satisfy _covers (below)


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


def _covers(N, positions):
    """The proposals (0-based device positions) reach every window shape."""
    o = (N - 27) // 2                     # the frozen aptamer's offset (workloads.synthetic)
    s = set(int(p) for p in positions)
    return {"helix partner (full band)": any(p <= 5 for p in s),
            "5' end": any(6 <= p <= 8 for p in s),
            "3' end outside the helix": any(N - 12 <= p <= N - 7 for p in s),
            "beside an x flank": any(p in (o - 7, o + 33) for p in s)}


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
    cov = _covers(N, r["tr"]["position"].ravel())
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


@pytest.mark.parametrize("N", [60, 70, 100])
def test_finalize_rows_trajectory(native, oracle, monkeypatch, N):
    r = _gpu_run(native, monkeypatch, N)
    assert "mfe_pair_kernel" in r["kernel"]
    _check_against_oracle(oracle, N, r)


def test_finalize_rows_nonzero_mlbase(native, oracle, monkeypatch, tmp_path):
    """MLbase = 30: the ghost row's qm carries MLbase per unpaired row down the
    band.  ADX_MFE_PAIR=1 keeps the pair kernel for MLbase >= 0 (asserted)."""
    par = _par_with_mlbase(tmp_path, 30)
    r = _gpu_run(native, monkeypatch, 100, par=par)
    assert "mfe_pair_kernel" in r["kernel"]
    _check_against_oracle(oracle, 100, r, par=par)


def test_finalize_rows_pair_equals_single(native, monkeypatch):
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
