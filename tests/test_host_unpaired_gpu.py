"""Unpaired-region probabilities through the C++ host mirror on the GPU:
GpuRnaFold::unpaired_probs against Fold.unpaired_probs, and the addapt command
line's --access file against Engine.walker_unpaired_probs on the same run.  Both
sides make the same library calls, so every number is compared exactly."""
import math
import os
import subprocess

import numpy as np
import pytest

from addapt_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "addapt_amd", "_lib")
EXE = os.path.join(LIB, "addapt")
W, STEPS, SEED0, N = 8, 30, 11, 60
TMPL, ACTIVE = workloads.synthetic(N)
CONTEXTS = [("GGAC", "UUA"), ("", "CCCA")]
REGIONS = [(0, 6), (20, 31), (56, 8)]   # (first 0-based, length): inside both contexts' folded lengths
ACCESS_LEN = 3

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
contexts:
  a: [GGAC, UUA]
  b: ['', CCCA]
"""

pytestmark = pytest.mark.gpu


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.fixture(scope="module")
def config(tmp_path_factory):
    p = tmp_path_factory.mktemp("unpaired") / "ctx.yml"
    p.write_text(CONFIG.format(seq=TMPL, act=ACTIVE))
    return str(p)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unpaired_probe") / "unpaired_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "unpaired_probe.cc"), "-L", LIB, "-laddapt_host",
                    "-laddapt_gpu", "-Wl,-rpath," + LIB], check=True)
    return exe


def test_fold_method(native, probe):
    seq = TMPL.upper()
    for cond, cst in (("apo", None), ("holo", None), ("holo", ACTIVE)):
        f = native.Fold(seq)
        if cond == "holo":
            f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
        if cst:
            f.add_constraint(cst)
        p, _, e = f.unpaired_probs(7)
        r = subprocess.run([probe, seq, cond, "7"] + ([cst] if cst else []), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [l.split() for l in r.stdout.splitlines()]
        assert lines[0][0] == "E" and np.float32(float(lines[0][1])) == np.float32(e)   # a float, printed with 9 digits
        got = np.array([[float(x) for x in l[2:]] for l in lines[1:]])
        assert got.shape == (7, N) and got.tobytes() == p.tobytes(), (cond, cst)
        assert 0.0 < p[0].min() or cst
    r = subprocess.run([probe, seq, "apo", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 1 and "max_len" in r.stderr


def test_cli_access_file(native, config, tmp_path):
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=40)
    eng = native.Engine(TMPL, [ACTIVE], workloads.default_objective(), aptamer=apt, thermostat=th, contexts=CONTEXTS)
    eng.walkers_init(list(range(SEED0, SEED0 + W)))
    eng.run_steps(STEPS)
    rows, folds = {}, 0
    for v in range(eng.info.n_variants):
        c, cond, mac = eng.variant(v)
        if mac >= 0:
            continue
        folds += 1
        L = N + sum(len(x) for x in CONTEXTS[c])
        prof, rp, _ = eng.walker_unpaired_probs(v, max_len=ACCESS_LEN, regions=REGIONS)
        for w in range(W):
            for k, (s, ln) in enumerate(REGIONS):
                rows[(w, c, cond, s + 1, s + ln)] = float(rp[w, k])
            for u in range(1, ACCESS_LEN + 1):
                for i in range(L - u + 1):
                    rows[(w, c, cond, i + 1, i + u)] = float(prof[w, u - 1, i])
    assert folds == 4

    out, plain, acc = str(tmp_path / "w.tsv"), str(tmp_path / "p.tsv"), str(tmp_path / "a.tsv")
    spec = ",".join("%d-%d" % (s + 1, s + ln) for s, ln in REGIONS)
    base = [EXE, config, "-n", str(STEPS), "-r", str(SEED0), "--walkers", str(W)]
    for cmd in (base + ["-o", plain],
                base + ["-o", out, "--access", acc, "--access-region", spec, "--access-len", str(ACCESS_LEN)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(plain, "rb").read()   # the walkers' file as without
    lines = open(acc).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert head[0] == "# Num Regions: %d" % len(REGIONS) and head[1] == "# Profile Length: %d" % ACCESS_LEN
    assert head[2].startswith("# Last Access ms: fill ")
    table = [l.split("\t") for l in lines if not l.startswith("#")]
    assert table[0] == ["walker", "seed", "context", "condition", "first", "last", "unpaired_probability"]
    per_fold = [len(REGIONS) + sum(N + sum(len(x) for x in ctx) - u + 1 for u in range(1, ACCESS_LEN + 1)) for ctx in CONTEXTS]
    assert len(table) - 1 == W * 2 * sum(per_fold)   # per walker: apo and holo of each context
    got, order = {}, []
    for w, seed, c, cond, first, last, p in table[1:]:
        assert int(seed) == SEED0 + int(w)
        order.append(int(w))
        got[(int(w), int(c), {"apo": 0, "holo": 1}[cond], int(first), int(last))] = float(p)
    assert order == sorted(order)   # walker-major
    assert sorted(got) == sorted(rows)
    for key, p in rows.items():
        assert _same(got[key], p), key
    assert any(0.0 < p < 1.0 for p in got.values())

    # regions alone: one row per walker, fold and region
    r = subprocess.run(base + ["-o", out, "--access", acc, "--access-region", spec], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    table = [l.split("\t") for l in open(acc).read().splitlines() if not l.startswith("#")]
    assert len(table) - 1 == W * 4 * len(REGIONS)
    for w, seed, c, cond, first, last, p in table[1:]:
        assert _same(float(p), rows[(int(w), int(c), {"apo": 0, "holo": 1}[cond], int(first), int(last))])


def test_cli_access_arguments(config, tmp_path):
    acc = str(tmp_path / "a.tsv")
    for extra, word in ((["--access", acc, "--access-region", "1-4"], "--walkers"),
                        (["--walkers", "2", "--access", acc], "--access-region"),
                        (["--walkers", "2", "--access-len", "3"], "--access"),
                        (["--walkers", "2", "--access", acc, "--access-region", "4-1"], "first"),
                        (["--walkers", "2", "--access", acc, "--access-region", "60-70"], "region")):
        r = subprocess.run([EXE, config, "-n", "2"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
