"""Picks through the C++ host mirror on the GPU: MonteCarlo::apply_batch with a
pick window, and the addapt command line's --picks file, on the reference's
rhf(6) device and default objective.  The expected picks come from the numpy
restatement of the rule (traj_pick_check.py) on the host trace of the same run
through the Python binding, the expected sequences from a twin context advanced
one step at a time."""
import math
import os
import subprocess

import numpy as np
import pytest

from addapt_amd import workloads
from traj_pick_check import pick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "addapt_amd", "_lib")
EXE = os.path.join(LIB, "addapt")
W, STEPS, SEED0, WINDOW = 8, 120, 40, 25

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
    p = tmp_path_factory.mktemp("picks") / "rhf6.yml"
    p.write_text(CONFIG.format(seq=workloads.RHF6_SEQ, act=workloads.RHF6_ACTIVE))
    return str(p)


def _engine(native):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=40)
    eng = native.Engine(workloads.RHF6_SEQ, [workloads.RHF6_ACTIVE], workloads.default_objective(), aptamer=apt,
                        thermostat=th)
    eng.walkers_init(list(range(SEED0, SEED0 + W)))
    return eng


@pytest.fixture(scope="module")
def expected(native):
    """Per walker [(step, score, sequence)] by the restatement, and the final state."""
    cur = _engine(native).run_steps(STEPS, trace=True)["current_score"]
    twin, seqs = _engine(native), []
    for _ in range(STEPS):
        twin.run_steps(1)
        seqs.append(twin.download()[0])
    picks = [[(s, cur[s, w], seqs[s][w]) for s in pick(cur[:, w], WINDOW)] for w in range(W)]
    assert sum(map(len, picks)) > W   # more than one a walker somewhere
    return picks, twin.download()


def _counts(picks):
    n = len(workloads.RHF6_SEQ)
    hist = np.zeros((n, 4), np.int64)
    for per in picks:
        for _, _, seq in per:
            for k, ch in enumerate(seq.upper()):
                hist[k, "ACGU".index(ch)] += 1
    return hist


def test_apply_batch_with_a_window(config, expected, tmp_path):
    exe = str(tmp_path / "picks_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "picks_probe.cc"), "-L", LIB, "-laddapt_host",
                    "-laddapt_gpu", "-Wl,-rpath," + LIB], check=True)
    r = subprocess.run([exe, config, str(STEPS), str(SEED0), str(W), str(WINDOW)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    picks, (fseqs, fscores, _) = expected
    got = [[] for _ in range(W)]
    final = {}
    counts = np.zeros((len(workloads.RHF6_SEQ), 4), np.int64)
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "P":
            got[int(f[1])].append((int(f[2]), float(f[3]), f[4]))
        elif f[0] == "F":
            final[int(f[1])] = (float(f[2]), f[3])
        elif f[0] == "C":
            counts[int(f[1])] = [int(x) for x in f[2:6]]
    assert got == picks
    assert [final[w] for w in range(W)] == [(fscores[w], fseqs[w]) for w in range(W)]
    assert np.array_equal(counts, _counts(picks))


def test_cli_picks_file(config, expected, tmp_path):
    out, pk = str(tmp_path / "walkers.tsv"), str(tmp_path / "picks.tsv")
    r = subprocess.run([EXE, config, "-n", str(STEPS), "-r", str(SEED0), "--walkers", str(W), "-o", out,
                        "--picks", pk, "--pick-window", str(WINDOW)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    picks, (fseqs, _, _) = expected
    lines = open(pk, encoding="utf-8").read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    rows = [l.split("\t") for l in lines if not l.startswith("#")]
    assert rows[0] == ["walker", "seed", "step", "score", "seq"]
    got = [[] for _ in range(W)]
    for w, seed, step, score, seq in rows[1:]:
        assert int(seed) == SEED0 + int(w)
        got[int(w)].append((int(step), float(score), seq))
    assert got == picks
    scores = np.array([p[1] for per in picks for p in per])
    assert head == ["# Num Picks: %d" % len(scores), "# Best Score: %.4f" % scores.max(),
                    "# Worst Score: %.4f" % scores.min(),
                    "# Average Score: %.4f ± %.4f" % (scores.mean(), scores.std(ddof=1))]
    assert all(math.isfinite(s) for s in scores)
    # the walkers' file is what it is without --picks
    final = [l.split("\t") for l in open(out).read().splitlines()[1:]]
    assert [f[7] for f in final] == list(fseqs)


def test_cli_picks_needs_walkers(config, tmp_path):
    r = subprocess.run([EXE, config, "-n", "5", "--picks", str(tmp_path / "p.tsv")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 1 and "--walkers" in r.stderr
