"""Distinct designs through the C++ host mirror on the GPU: MonteCarlo::apply_batch
with a design radius, and the addapt command line's --designs file, on the
reference's rhf(6) device and default objective.  The expected designs come from
the numpy restatement of the rule (design_select_check.py) applied to the picks
the Python binding returns for the same run and window."""
import os
import subprocess

import numpy as np
import pytest

from addapt_amd import workloads
from design_select_check import codes_of, distances, pair_hist, select, walkers_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "addapt_amd", "_lib")
EXE = os.path.join(LIB, "addapt")
# Seeds 744..751: of the first seeds 0, 8, .., 3992 only 744 and 2656 make two of the eight walkers pick one
# sequence (the picks of seeds 40..47, test_host_picks_gpu.py's, are all distinct), so walkers > 1 is tested.
W, STEPS, SEED0, WINDOW = 8, 120, 744, 25

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
    p = tmp_path_factory.mktemp("designs") / "rhf6.yml"
    p.write_text(CONFIG.format(seq=workloads.RHF6_SEQ, act=workloads.RHF6_ACTIVE))
    return str(p)


@pytest.fixture(scope="module")
def run(native):
    """The picks of the run as entries (walker, step, score, sequence), walker-major,
    with their distances, and the walkers' final sequences."""
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=40)
    eng = native.Engine(workloads.RHF6_SEQ, [workloads.RHF6_ACTIVE], workloads.default_objective(), aptamer=apt,
                        thermostat=th)
    eng.walkers_init(list(range(SEED0, SEED0 + W)))
    eng.record(STEPS)
    eng.run_steps(STEPS)
    picks, _ = eng.picks(WINDOW)
    ent = [(w, step, score, seq) for w, per in enumerate(picks) if per is not None for step, score, seq in per]
    assert len(ent) > W
    codes = codes_of([e[3] for e in ent])
    return dict(ent=ent, codes=codes, scores=np.array([e[2] for e in ent]), walker=np.array([e[0] for e in ent]),
                dist=distances(codes), final=eng.download()[0])


def _expected(run, radius, K):
    """[(walker, step, score, picks, walkers, sequence)] per design, and the pair histogram."""
    ref = select(run["codes"], run["scores"], radius, K, run["dist"])
    nw = walkers_of(ref["member_of"], run["walker"], len(ref["leaders"]))
    rows = [run["ent"][lead][:3] + (int(size), int(n), run["ent"][lead][3])
            for lead, size, n in zip(ref["leaders"], ref["sizes"], nw)]
    return rows, pair_hist(run["codes"], run["scores"], run["dist"])


def test_the_run_rediscovers_a_design(run):
    """Some sequence is picked by more than one walker, so walkers > 1 is tested below."""
    rows, _ = _expected(run, 0, 1000)
    assert max(r[4] for r in rows) > 1
    assert len(rows) < len(run["ent"])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("designs_probe") / "designs_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "designs_probe.cc"), "-L", LIB, "-laddapt_host",
                    "-laddapt_gpu", "-Wl,-rpath," + LIB], check=True)
    return exe


@pytest.mark.parametrize("radius,K", [(0, 100), (3, 100), (2, 2)])
def test_apply_batch_with_a_design_radius(config, run, probe, radius, K):
    r = subprocess.run([probe, config, str(STEPS), str(SEED0), str(W), str(WINDOW), str(radius), str(K)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    designs, hist, picks, final, n = [], {}, [], {}, None
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "D":
            assert int(f[1]) == len(designs)
            designs.append((int(f[2]), int(f[3]), float(f[4]), int(f[5]), int(f[6]), f[7]))
        elif f[0] == "H":
            hist[int(f[1])] = int(f[2])
        elif f[0] == "P":
            picks.append((int(f[1]), int(f[2]), float(f[3]), f[4]))
        elif f[0] == "F":
            final[int(f[1])] = f[3]
        elif f[0] == "N":
            n = int(f[1])
    rows, ref_hist = _expected(run, radius, K)
    assert designs == rows and len(designs) <= K
    assert [hist[d] for d in range(len(ref_hist))] == ref_hist.tolist()
    assert n == len(run["ent"]) and picks == run["ent"]
    assert [final[w] for w in range(W)] == list(run["final"])


def test_apply_batch_designs_need_a_window(config, probe):
    r = subprocess.run([probe, config, "5", str(SEED0), str(W), "0", "-2", "10"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 1 and "pick window" in r.stderr


def _cli(config, tmp, name, extra):
    out, pk = str(tmp / (name + "_walkers.tsv")), str(tmp / (name + "_picks.tsv"))
    r = subprocess.run([EXE, config, "-n", str(STEPS), "-r", str(SEED0), "--walkers", str(W), "-o", out, "--picks", pk,
                        "--pick-window", str(WINDOW)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return open(out, "rb").read(), open(pk, "rb").read()


def test_cli_designs_file(config, run, tmp_path):
    plain = _cli(config, tmp_path, "plain", [])
    for name, extra, radius, K in (("default", [], 3, 100), ("exact", ["--design-radius", "0", "--max-designs", "4"], 0, 4)):
        ds = str(tmp_path / (name + "_designs.tsv"))
        assert _cli(config, tmp_path, name, ["--designs", ds] + extra) == plain   # walkers' and picks' files as without
        lines = open(ds).read().splitlines()
        head = [l for l in lines if l.startswith("#")]
        table = [l.split("\t") for l in lines if not l.startswith("#")]
        rows, hist = _expected(run, radius, K)
        assert head == ["# Num Picks: %d" % len(run["ent"]), "# Num Designs: %d" % len(rows), "# Radius: %d" % radius,
                        "# Pair Distances:" + "".join(" %d:%d" % (d, c) for d, c in enumerate(hist) if c)]
        assert table[0] == ["design", "walker", "seed", "step", "score", "picks", "walkers", "seq"]
        got = []
        for k, (d, w, seed, step, score, picks, walkers, seq) in enumerate(table[1:]):
            assert int(d) == k and int(seed) == SEED0 + int(w)
            got.append((int(w), int(step), float(score), int(picks), int(walkers), seq))
        assert got == rows and len(rows) <= K


def test_cli_designs_needs_walkers(config, tmp_path):
    r = subprocess.run([EXE, config, "-n", "5", "--designs", str(tmp_path / "d.tsv")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 1 and "--walkers" in r.stderr


def test_cli_designs_alone(config, run, tmp_path):
    """--designs without --picks picks all the same."""
    out, ds = str(tmp_path / "w.tsv"), str(tmp_path / "d.tsv")
    r = subprocess.run([EXE, config, "-n", str(STEPS), "-r", str(SEED0), "--walkers", str(W), "-o", out, "--designs", ds,
                        "--pick-window", str(WINDOW), "--design-radius", "1"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows, _ = _expected(run, 1, 100)
    table = [l.split("\t") for l in open(ds).read().splitlines() if not l.startswith("#")][1:]
    assert [(int(t[1]), int(t[3]), t[7]) for t in table] == [(r_[0], r_[1], r_[5]) for r_ in rows]
