"""Given structures priced through the C++ host mirror on the GPU:
GpuRnaFold::eval_structures, MonteCarlo::apply_batch with target structures, and
the addapt command line's --eval file, each against the ctypes calls
(Fold.eval_structures, Engine.walker_eval_structures) on the same run.  Both
sides make the same library calls, so every number is compared exactly."""
import math
import os
import subprocess

import pytest

from addapt_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "addapt_amd", "_lib")
EXE = os.path.join(LIB, "addapt")
W, STEPS, SEED0, N = 8, 30, 11, 60
TMPL, ACTIVE = workloads.synthetic(N)
CONTEXTS = [("GGAC", "UUA"), ("", "CCCA")]   # "a", "b": the score function keeps them by name
O = (N - 27) // 2


def _target(before, after):
    return "." * (len(before) + O) + workloads.THEO_FOLD + "." * (N - 27 - O + len(after))


# one target per context's folded length, the enforced helix at the first length, and two non-members
TARGETS = [_target(*CONTEXTS[0]), _target(*CONTEXTS[1]), "." * 4 + ACTIVE.replace("x", ".") + "." * 3,
           "(" + "." * 66, "." * 30 + "(.)" + "." * 31]

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
{contexts}"""

pytestmark = pytest.mark.gpu


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.fixture(scope="module")
def configs(tmp_path_factory):
    d = tmp_path_factory.mktemp("struct_eval")
    out = {}
    for name, ctx in (("plain", ""), ("ctx", "contexts:\n  a: [GGAC, UUA]\n  b: ['', CCCA]\n")):
        p = d / (name + ".yml")
        p.write_text(CONFIG.format(seq=TMPL, act=ACTIVE, contexts=ctx))
        out[name] = str(p)
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("struct_eval_probe") / "struct_eval_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "struct_eval_probe.cc"), "-L", LIB, "-laddapt_host",
                    "-laddapt_gpu", "-Wl,-rpath," + LIB], check=True)
    return exe


@pytest.fixture(scope="module")
def run(native):
    """The rows the ctypes calls give for the run with contexts: {(walker, target, context, condition):
    (energy, prob, status)}, and the walkers' final sequences."""
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=40)
    eng = native.Engine(TMPL, [ACTIVE], workloads.default_objective(), aptamer=apt, thermostat=th, contexts=CONTEXTS)
    eng.walkers_init(list(range(SEED0, SEED0 + W)))
    eng.run_steps(STEPS)
    rows = {}
    for v in range(eng.info.n_variants):
        c, cond, mac = eng.variant(v)
        if mac >= 0:
            continue
        L = N + sum(len(x) for x in CONTEXTS[c])
        idx = [t for t, s in enumerate(TARGETS) if len(s) == L]
        e, p, st = eng.walker_eval_structures(v, [TARGETS[t] for t in idx], with_probs=True)
        for w in range(W):
            for k, t in enumerate(idx):
                rows[(w, t, c, cond)] = (float(e[w, k]), float(p[w, k]), int(st[w, k]))
    assert len(rows) == W * len(TARGETS) * 2
    assert {r[2] for r in rows.values()} >= {0, 1}
    assert any(r[2] == 0 and 0.0 < r[1] < 1.0 for r in rows.values())
    return rows, eng.download()[0]


def test_fold_method(native, configs, probe):
    seq = TMPL.upper()
    sts = [TARGETS[0][4:-3], ACTIVE.replace("x", "."), "." * N, "(" + "." * (N - 1), "." * 30 + "(.)" + "." * 27]
    for cst, conv in ((None, "pf"), (ACTIVE, "pf"), (None, "mfe")):
        f = native.Fold(seq)
        f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
        if cst:
            f.add_constraint(cst)
        e, p, st = f.eval_structures(sts, convention=conv, with_probs=conv == "pf")
        r = subprocess.run([probe, "fold", configs["plain"], cst or "-", conv, ",".join(sts)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = [l.split() for l in r.stdout.splitlines()]
        assert len(got) == len(sts)
        for k, (tag, ge, gp, gs) in enumerate(got):
            assert tag == "S" and _same(float(ge), float(e[k])) and int(gs) == st[k], (cst, conv, k)
            assert math.isnan(float(gp)) if conv == "mfe" else float(gp) == p[k]
        assert st[0] == (4 if cst else 0) and st[1] == 0 and (st[3:] != 0).all()   # the macrostate excludes the bare motif fold
    r = subprocess.run([probe, "fold", configs["plain"], "-", "pf", "..."], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 1 and "length" in r.stderr


def test_apply_batch_with_targets(configs, probe, run):
    rows, final = run
    r = subprocess.run([probe, "batch", configs["ctx"], str(STEPS), str(SEED0), str(W), ",".join(TARGETS)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got, order, seqs = {}, [], {}
    for f in (l.split() for l in r.stdout.splitlines()):
        if f[0] == "F":
            seqs[int(f[1])] = f[2]
        else:
            key = (int(f[1]), int(f[2]), int(f[3]), int(f[4]))
            order.append(key)
            got[key] = (float(f[5]), float(f[6]), int(f[7]))
    assert [seqs[w] for w in range(W)] == list(final)
    assert sorted(got) == sorted(rows) and order == sorted(order, key=lambda k: (k[0], k[1]))   # walker-major, then target
    for key, (e, p, st) in rows.items():
        assert _same(got[key][0], e) and got[key][1] == p and got[key][2] == st, key


def test_apply_batch_refuses_a_target_of_no_length(configs, probe):
    r = subprocess.run([probe, "batch", configs["ctx"], "2", "1", "2", "....."], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 1 and "folded length" in r.stderr


def test_cli_eval_file(configs, run, tmp_path):
    rows, final = run
    out, plain, ev = str(tmp_path / "w.tsv"), str(tmp_path / "p.tsv"), str(tmp_path / "e.tsv")
    base = [EXE, configs["ctx"], "-n", str(STEPS), "-r", str(SEED0), "--walkers", str(W)]
    for cmd in (base + ["-o", plain], base + ["-o", out, "--eval", ev, "--eval-structure", ",".join(TARGETS)]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(plain, "rb").read()   # the walkers' file as without
    lines = open(ev).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert head[0] == "# Num Targets: %d" % len(TARGETS) and head[1].startswith("# Last Eval ms: fill ")
    table = [l.split("\t") for l in lines if not l.startswith("#")]
    assert table[0] == ["walker", "seed", "target", "context", "condition", "energy", "probability", "status", "structure"]
    got = {}
    for w, seed, t, c, cond, e, p, st, db in table[1:]:
        assert int(seed) == SEED0 + int(w) and db == TARGETS[int(t)]
        got[(int(w), int(t), int(c), {"apo": 0, "holo": 1}[cond])] = (float(e), float(p), int(st))
    assert sorted(got) == sorted(rows)
    for key, (e, p, st) in rows.items():
        assert _same(got[key][0], e) and got[key][1] == p and got[key][2] == st, key


def test_cli_eval_needs_walkers_and_targets(configs, tmp_path):
    for extra, word in ((["--eval", str(tmp_path / "e.tsv"), "--eval-structure", "." * N], "--walkers"),
                        (["--walkers", "2", "--eval", str(tmp_path / "e.tsv")], "--eval-structure")):
        r = subprocess.run([EXE, configs["plain"], "-n", "2"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert r.returncode == 1 and word in r.stderr
