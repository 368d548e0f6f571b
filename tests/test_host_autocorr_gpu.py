"""The sequence autocorrelation through the addapt command line on the GPU
(--autocorr, --pick-window auto), on the reference's rhf(6) device and default
objective: the file's curves, correlation time and outcome shares against
Engine.autocorr and the host trace of the same run through the Python binding,
and the picks made with the correlation time as window against those made with
that number given."""
import os
import subprocess

import numpy as np
import pytest

from addapt_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "addapt_amd", "_lib", "addapt")
W, STEPS, SEED0, LAG, DISCARD = 8, 120, 40, 60, 20

CONFIG = """\
sequence: {seq}
macrostates:
  active: '{act}'
objective:
  apo: not active
  holo: active
aptamer:
  sequence: GAUACCAGCCGAAAGGCCCUUGGCAGC
  fold: (...((.(((....)))....))...)
  affinity: 0.32
thermostat: 5 to 0 in 40 steps
"""

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def config(tmp_path_factory):
    p = tmp_path_factory.mktemp("autocorr") / "rhf6.yml"
    p.write_text(CONFIG.format(seq=workloads.RHF6_SEQ, act=workloads.RHF6_ACTIVE))
    return str(p)


def _cli(config, tmp_path, *args, steps=STEPS):
    out = str(tmp_path / "walkers.tsv")
    r = subprocess.run([EXE, config, "-n", str(steps), "-r", str(SEED0), "--walkers", str(W), "-o", out, *args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def _read(path):
    lines = open(path).read().splitlines()
    head = dict(l[2:].split(": ", 1) for l in lines if l.startswith("# "))
    rows = [l.split("\t") for l in lines if not l.startswith("#")]
    return head, rows[0], np.array(rows[1:], np.float64)


@pytest.fixture(scope="module")
def expected(native):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=40)
    eng = native.Engine(workloads.RHF6_SEQ, [workloads.RHF6_ACTIVE], workloads.default_objective(), aptamer=apt,
                        thermostat=th)
    eng.walkers_init(list(range(SEED0, SEED0 + W)))
    eng.record(STEPS)
    outcome = eng.run_steps(STEPS, trace=True)["outcome"]
    return eng.autocorr(LAG, DISCARD), outcome


def test_cli_autocorr_file(config, expected, tmp_path):
    ac, outcome = expected
    path = str(tmp_path / "autocorr.tsv")
    _cli(config, tmp_path, "--autocorr", path, "--autocorr-lag", str(LAG), "--autocorr-discard", str(DISCARD))
    head, names, rows = _read(path)
    kept = STEPS - DISCARD
    chg = np.flatnonzero(ac["changeable"])
    assert names == ["lag", "pooled"] + [str(p) for p in chg] and len(chg) > 0
    assert rows.shape == (LAG + 1, 2 + len(chg)) and np.array_equal(rows[:, 0], np.arange(LAG + 1))
    # six decimals are printed
    assert np.abs(rows[:, 1] - ac["pooled"]).max() <= 0.5e-6 + 1e-12
    curves = ac["pos_matches"][chg].T / (float(W) * (kept - np.arange(LAG + 1)))[:, None]
    assert np.abs(rows[:, 2:] - curves).max() <= 0.5e-6 + 1e-12
    assert rows[:, 2:].min() < 1.0   # something moved
    assert int(head["tau"]) == ac["tau"]
    assert abs(float(head["baseline"]) - ac["baseline"]) <= 0.5e-6 + 1e-12
    for c, name in enumerate(("reject", "accept_worsened", "accept_unchanged", "accept_improved")):
        share = 100.0 * (outcome[DISCARD:] == c).sum() / float(W * kept)
        assert head[name].endswith("%") and abs(float(head[name][:-1]) - share) <= 0.005 + 1e-9, name


def _picks(path):
    return [l for l in open(path, encoding="utf-8").read().splitlines() if not l.startswith("#")]


def test_cli_auto_window_is_the_correlation_time(config, expected, tmp_path):
    tau = expected[0]["tau"]
    assert tau >= 1   # the curve of this run decays within LAG lags
    a, b = str(tmp_path / "auto.tsv"), str(tmp_path / "given.tsv")
    r = _cli(config, tmp_path, "--picks", a, "--pick-window", "auto", "--autocorr-lag", str(LAG),
             "--autocorr-discard", str(DISCARD))
    assert "Warning" not in r.stderr
    _cli(config, tmp_path, "--picks", b, "--pick-window", str(tau))
    assert _picks(a) == _picks(b) and len(_picks(a)) > 1
    other = str(tmp_path / "other.tsv")
    _cli(config, tmp_path, "--picks", other, "--pick-window", str(4 * tau + 7))
    assert _picks(other) != _picks(a)   # the window matters here


def test_cli_auto_window_falls_back_to_500(config, tmp_path):
    """A 3-step run, every (max_lag, discard) it allows.  Where the correlation
    time is below 1 the picks are those of --pick-window 500 and the warning is
    printed; that is the case at lag 1 and wherever a single step is kept.  At
    max_lag 2 without discard the rule itself gives 2, not -1: lag 2 has one
    comparison a series and the eight walkers start from one sequence, so a_2
    and the baseline are both about 0.98 and a_2 - baseline is below
    (1 - baseline) / e; there the picks must be those of --pick-window 2."""
    a, b, ac = str(tmp_path / "auto.tsv"), str(tmp_path / "given.tsv"), str(tmp_path / "autocorr.tsv")
    taus = {}
    for lag, discard in ((1, 0), (2, 0), (1, 1), (1, 2)):
        r = _cli(config, tmp_path, "--picks", a, "--pick-window", "auto", "--autocorr", ac, "--autocorr-lag", str(lag),
                 "--autocorr-discard", str(discard), steps=3)
        head, _, rows = _read(ac)
        tau = taus[lag, discard] = int(head["tau"])
        assert rows.shape[0] == min(lag, 3 - discard - 1) + 1
        assert tau == -1 or 1 <= tau <= lag
        if tau < 1:
            assert "Warning" in r.stderr and "500" in r.stderr
        else:
            assert "Warning" not in r.stderr
        _cli(config, tmp_path, "--picks", b, "--pick-window", str(500 if tau < 1 else tau), steps=3)
        assert _picks(a) == _picks(b) and len(_picks(a)) > 1
    assert taus[1, 0] == -1 and taus[1, 2] == -1
