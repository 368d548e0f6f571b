"""pf_access_kernel's per-lane code (addapt_amd/csrc/pf_access_core.hpp) without a GPU:
a stand-alone program built against the header and the host setup code stages a
sequence as the kernels' setup does and runs the inside fill, the adjoints and the
window sums lane by lane in the kernels' order.  It is held to unpaired_check.py
(the CPU oracle's constrained partition functions), to the identity
sum_j P(i,j) + P_u(i,i) = 1 and to pinned structures.  The program is built once more
with the address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded).

The per-lane code is a template over the type of the factor tables.  The kernels
read FP32 factors, and so does the program by default ("f32"): those runs carry the
identity, the pinned structures and the comparison with the program's own two fills.
The oracle multiplies FP64 factors, so against it the FP32 tables' rounding alone
moves a probability by up to 1.4e-8 on these cases; the comparison with the oracle
at 1e-9 therefore runs the same code on the same setup code's tables in FP64 ("f64"),
where the two agree to 7e-15, and the FP32 run is held to the oracle at 1e-6."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

import loop_zoo as Z
import unpaired_check as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "pf_access_core_probe.cc")
BOUND = 1e-9
THEO_HOLO = "GCCACUGGGAA" + Z.THEO_SEQ + "GUAGCGUCACUG"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    out = str(tmp_path_factory.mktemp("pf_access_core") / "probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", *flags, "-I", CSRC, "-o", out,
                    SRC, os.path.join(CSRC, "energy.cpp")], check=True)
    return out


def run(exe, cases, lanes=64, sigma=1.0, prec="f32"):
    """cases: (seq, cst or None, motif (seq, fold, energy) or None, max_len).  Per case a dict of
    energy, identity (the largest |sum_j P(i,j) + P_u(i,i) - 1|), table (max_len, N), pairs {(i, j): p}."""
    lines = [str(len(cases))]
    for seq, cst, motif, max_len in cases:
        m = motif or ("-", "-", 0.0)
        lines.append("%s %s %s %s %r 0 %d" % (seq, cst or "-", m[0], m[1], m[2], max_len))
    r = subprocess.run([exe, Z.PAR, str(lanes), repr(sigma), prec], input="\n".join(lines) + "\n", stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out, cur, k = [], None, 0
    for f in (l.split() for l in r.stdout.split("\n") if l):
        if f[0] == "Z":
            n, ml = len(cases[k][0]), cases[k][3]
            cur = dict(energy=float(f[1]), identity=float(f[2]), table=np.zeros((min(ml, n), n)), pairs={})
        elif f[0] == "U":
            row = [float(x) for x in f[2:]]
            cur["table"][int(f[1]) - 1, :len(row)] = row
        elif f[0] == "P":
            cur["pairs"][(int(f[1]), int(f[2]))] = float(f[3])
        else:
            out.append(cur)
            k += 1
    assert len(out) == len(cases)
    return out


def _theo(oracle):
    return (Z.THEO_SEQ, Z.THEO_FOLD, oracle.theo_bonus())


def _cases(oracle):
    """(seq, cst, motif, max_len): every window of the enumeration cases, windows up to 6 of longer folds"""
    rng = random.Random(11)
    out = [(seq, cst, None, len(seq)) for seq, cst in uc.ENUM_CASES]
    for n in (40, 60):
        out.append(("".join(rng.choice("ACGU") for _ in range(n)), None, None, 6))
    out.append((THEO_HOLO, None, _theo(oracle), 6))
    return out


@pytest.fixture(scope="module")
def results(exe, oracle):
    cases = _cases(oracle)
    return cases, run(exe, cases)


@pytest.fixture(scope="module")
def brutes(oracle):
    return [uc.brute(oracle, seq, cst, max_len, oracle.make_motif(*motif) if motif else None)
            for seq, cst, motif, max_len in _cases(oracle)]


def test_every_window_is_the_oracles_ratio(exe, results, brutes, oracle):
    """FP64 tables: what is left is the arithmetic, and the identity holds there too."""
    cases, _ = results
    for (seq, cst, _, _), res, ref in zip(cases, run(exe, cases, prec="f64"), brutes):
        dev = np.abs(res["table"] - ref).max()
        print("probe (f64 factors) vs brute, %d nt, %s: %.3g" % (len(seq), cst, dev))
        assert dev <= BOUND, (seq, cst)
        assert res["identity"] <= 1e-12, (seq, cst)


def test_fp32_factors_stay_near_the_oracle(results, brutes):
    """The kernels' tables: each factor is rounded to a relative 6e-8, and a probability's
    logarithm moves by that times the change in how often the window's constraint makes
    the ensemble use the factor, a few uses at these lengths: 1e-6 leaves room."""
    cases, out = results
    for (seq, cst, _, _), res, ref in zip(cases, out, brutes):
        dev = np.abs(res["table"] - ref).max()
        print("probe (f32 factors) vs brute, %d nt, %s: %.3g" % (len(seq), cst, dev))
        assert dev <= 1e-6, (seq, cst)


def test_every_window_is_the_ratio_of_its_own_folds(exe, results, oracle):
    """brute's definition on the probe's own FP32-factor fill: G and G_x from the same
    tables.  What is left is FP64 rounding (about 1e-13 here), far inside the bound."""
    cases, out = results
    kT = oracle.KT_KCAL
    for (seq, cst, motif, max_len), res in zip(cases, out):
        n = len(seq)
        wins = [(u, i) for u in range(1, max_len + 1) for i in range(1, n - u + 2)]
        merged = [uc.merge(cst, i, i + u - 1, n) for u, i in wins]
        folds = run(exe, [(seq, m, motif, 1) for m in merged if m is not None])
        gx = iter(f["energy"] for f in folds)
        for (u, i), m in zip(wins, merged):
            ref = 0.0 if m is None else math.exp(-(next(gx) - res["energy"]) / kT)
            assert abs(res["table"][u - 1, i - 1] - ref) <= BOUND, (seq, cst, u, i)


def test_each_base_is_paired_or_not(results):
    for (seq, cst, _, _), res in zip(*results):
        assert res["identity"] <= 1e-12, (seq, cst)


def test_pair_probabilities_and_energy(results, oracle):
    """Within the rounding of the FP32 factors (a relative 6e-8 each): 1e-6 leaves room."""
    for (seq, cst, motif, _), res in zip(*results):
        g, P = oracle.bppm(seq, cst, oracle.make_motif(*motif) if motif else None)
        got = np.zeros_like(P)
        for (i, j), p in res["pairs"].items():
            got[i - 1, j - 1] = got[j - 1, i - 1] = p
        assert np.abs(got - P).max() <= 1e-6 and abs(res["energy"] - g) <= 1e-6, (seq, cst)


@pytest.mark.parametrize("sigma", [1.0, 0.62])
def test_pinned_structures(exe, sigma):
    """A constraint that admits one structure: 1 exactly on the windows that are all dots in it."""
    zoo = uc.zoo(wide=True)
    out = run(exe, [(seq, uc.pin(st), None, len(seq)) for _, seq, st in zoo], sigma=sigma)
    for (name, seq, st), res in zip(zoo, out):
        dots = uc.dots_table(st, len(seq))
        assert math.isfinite(res["energy"]), name
        assert res["table"][dots == 1].min() >= 1 - 1e-9, name
        assert res["table"][dots == 0].max() <= 1e-12, name


def test_lane_count_does_not_matter(exe, results):
    cases, out = results
    for lanes in (1, 7):
        for a, b in zip(out, run(exe, cases, lanes=lanes)):
            assert np.abs(a["table"] - b["table"]).max() <= 1e-13


def test_edges(exe):
    out = run(exe, [("ACG", None, None, 3), ("ACGU", None, None, 4), ("A" * 10, "(........)", None, 10),
                    ("GGGUGAAAACUAGUGAAAGCCC", "(...|...........|....)", None, 22)])
    for res, n in zip(out[:2], (3, 4)):
        for u in range(1, n + 1):
            assert (res["table"][u - 1, :n - u + 1] == 1.0).all() and (res["table"][u - 1, n - u + 1:] == 0.0).all()
    assert np.isnan(out[2]["table"][0]).all() and out[2]["energy"] == math.inf
    t = out[3]["table"]
    for k in (0, 4, 16, 21):   # every window over a forced base is exactly 0
        for u in range(1, 23):
            for i in range(max(0, k - u + 1), min(k, 22 - u) + 1):
                assert t[u - 1, i] == 0.0
    assert t[0, 1] > 0.0 and t[21, 0] == 0.0
