"""struct_eval_kernel's per-lane code (addapt_amd/csrc/struct_eval_core.hpp) without a
GPU: a stand-alone program built against the header and the host setup code
stages a sequence as the kernel's setup does and runs partners, loops,
admission, exterior loop, motif sites and totals lane by lane in the kernel's
order.  It is held to struct_eval_check.py.  The program is built once more with
the address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded).

Integer dcal sums are exact in double, so every energy without a loop above 30
is compared bit for bit; a loop above 30 adds at most L / 30 non-integer FP64
terms below 1e4 dcal each, summed in another order than the host's: 1e-9
kcal/mol is orders above that error."""
import math
import os
import subprocess

import pytest

import loop_zoo as Z
import struct_eval_check as sec
from test_oracle_enum import structures
from test_struct_eval_check import CONSTRAINED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "struct_eval_core_probe.cc")
MERS14 = sec.MERS14
MODES = (0, 1, 2)   # ADX_MOTIF_AUTO, ADD, REPLACE
TOL_LONG = 1e-9


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    out = str(tmp_path_factory.mktemp("struct_eval_core") / "probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", *flags, "-I", CSRC, "-o", out,
                    SRC, os.path.join(CSRC, "energy.cpp")], check=True)
    return out


def run(exe, cases):
    """cases: (convention, seq, cst or None, motif (seq, fold, energy, mode) or None, [structures]).
    Per case [(energy, status)]."""
    lines = [str(len(cases))]
    for conv, seq, cst, motif, sts in cases:
        m = motif or ("-", "-", 0.0, 0)
        lines.append("%s %s %s %s %s %r %d %d" % (conv, seq, cst or "-", m[0], m[1], m[2], m[3], len(sts)))
        lines += sts
    r = subprocess.run([exe, Z.PAR], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = [(float(a), int(b)) for a, b in (l.split() for l in r.stdout.split("\n") if l)]
    out, at = [], 0
    for case in cases:
        out.append(rows[at:at + len(case[4])])
        at += len(case[4])
    assert at == len(rows)
    return out


def has_long_loop(st):
    return any((lp["kind"] == "hairpin" and lp["size"] > 30) or (lp["kind"] == "interior" and lp["n1"] + lp["n2"] > 30)
               for lp in Z.loops(st))


# ------------------------------------------------------------------ apo energies
def test_apo_energies_are_the_hosts(exe, oracle, native):
    """Every zoo structure, every table entry and every structure of the 14-mers:
    oracle.eval_structure and adx_eval_structure, bit for bit without a loop above 30."""
    P = native.Params()
    cases = [("pf", seq, None, None, [st]) for seq, st in Z.shape_zoo(100)]
    for _, st, seqs in Z.table_batches():
        cases += [("pf", s, None, None, [st]) for s in seqs]
    cases += [("pf", seq, None, None, structures(seq)) for seq in MERS14]
    n_long = 0
    for (_, seq, _, _, sts), got in zip(cases, run(exe, cases)):
        for st, (e, status) in zip(sts, got):
            ref = oracle.eval_structure(seq, st)
            assert status == 0, (seq, st, status)
            if has_long_loop(st):
                n_long += 1
                assert abs(e - ref) <= TOL_LONG and abs(e - P.eval_structure(seq, st)) <= TOL_LONG, (seq, st, e, ref)
            else:
                assert e == ref == P.eval_structure(seq, st), (seq, st, e, ref)
    assert n_long >= 3   # the zoo's hairpins of 31, 40 and 96


def _long_cases():
    out = []
    for h in (31, 40, 57):
        st = Z.pad(Z.hairpin(h), h + 8, 2)
        out.append((Z.default_seq(st), st))
    st = "((" + "." * 20 + Z.hairpin(5) + "." * 15 + "))"   # a 35-base interior loop
    out.append((Z.default_seq(st), st))
    return out


def test_long_loops(exe, oracle):
    cases = [("pf", seq, None, None, [st]) for seq, st in _long_cases()]
    cases += [("mfe", seq, None, None, [st]) for seq, st in _long_cases()[:3]]
    got = run(exe, cases)
    for (conv, seq, _, _, (st,)), ((e, status),) in zip(cases, got):
        big = sec.status(seq, st)
        assert status == big and big in (0, sec.BIGLOOP)
        if conv == "mfe":
            assert e == sec.mfe_energy(oracle, seq, st), (seq, st)
            assert e != oracle.eval_structure(seq, st)   # the truncated ln term
        else:
            assert abs(e - oracle.eval_structure(seq, st)) <= TOL_LONG, (seq, st, e)
            if not big:
                assert abs(e - sec.pf_energy(oracle, seq, st)) <= TOL_LONG
    assert sum(1 for c in cases if sec.status(c[1], c[4][0]) == sec.BIGLOOP) == 1


def test_mfe_convention_is_the_oracles_fold(exe, oracle):
    cases = [("mfe", seq, None, None, [st]) for seq, st in Z.shape_zoo(100)]
    cases += [("mfe", seq, None, None, structures(seq)) for seq in MERS14[:2]]
    for (_, seq, _, _, sts), got in zip(cases, run(exe, cases)):
        for st, (e, status) in zip(sts, got):
            assert status == 0 and e == sec.mfe_energy(oracle, seq, st), (seq, st, e)


# ------------------------------------------------------------------ membership
def _mutants(seq):
    """Strings that are no members, with the enumerated ones around them."""
    n = len(seq)
    return ["(" + "." * (n - 1), "." * (n - 1) + ")", ")" + "." * (n - 2) + "(", "." * (n - 3) + "(.)", "[" + "." * (n - 1),
            "(" * 2 + "." * (n - 4) + ")" * 2, ".(..)" + "." * (n - 5), "()" + "." * (n - 2), "((...)" + "." * (n - 6)]


def test_status_and_documented_energies(exe, oracle):
    cases = [("pf", seq, cst, None, structures(seq) + _mutants(seq)) for seq, cst in CONSTRAINED]
    cases += [("pf", seq, None, None, structures(seq)[:40] + _mutants(seq)) for seq in MERS14[:2]]
    cases.append(("pf", "GGGAAACCC", "..>...<..", None, ["(((...)))", "((.....))", "........."]))
    cases.append(("pf", "GGGAAACCC", "..<......", None, ["(((...)))", "........."]))
    seen = 0
    for (_, seq, cst, _, sts), got in zip(cases, run(exe, cases)):
        for st, (e, status) in zip(sts, got):
            assert status == sec.status(seq, st, cst), (seq, cst, st, status)
            assert sec.same(e, sec.expected_energy(oracle, seq, st, cst), 1e-9), (seq, cst, st, e)
            seen |= status
    assert seen & 7 == 7


# ------------------------------------------------------------------ the motif
def _theo_cases(oracle):
    """THEO in the zoo's two flanks, formed and with its outer pair opened."""
    out = []
    for seq, st in Z.shape_zoo(100):
        o = Z.theo_offset(seq, st)
        if o < 0:
            continue
        e = o + len(Z.THEO_FOLD) - 1
        out.append((seq, [st, st[:o] + "." + st[o + 1:e] + "." + st[e + 1:]]))
    assert len(out) == 2
    return out


@pytest.mark.parametrize("mode", MODES)
def test_theo_in_both_conventions(exe, oracle, mode):
    bonus = oracle.theo_bonus()
    motif = (Z.THEO_SEQ, Z.THEO_FOLD, bonus, mode)
    om = oracle.make_motif(Z.THEO_SEQ, Z.THEO_FOLD, bonus, mode)
    cases = [(conv, seq, None, motif, sts) for seq, sts in _theo_cases(oracle) for conv in ("pf", "mfe")]
    for (conv, seq, _, _, sts), got in zip(cases, run(exe, cases)):
        for k, (st, (e, status)) in enumerate(zip(sts, got)):
            assert status == 0
            apo = oracle.eval_structure(seq, st)
            if conv == "mfe":
                assert e == sec.mfe_energy(oracle, seq, st, om), (mode, seq, st, e)
            else:
                assert abs(e - sec.pf_energy(oracle, seq, st, om)) <= 1e-9, (mode, seq, st, e)
            if k == 1:   # unformed: the apo loops
                assert e == apo
            elif conv == "pf":
                assert e != apo


HP_SEQ = "GCAGAAAUGCAAGC"        # holds the motif below at 2: an A-U closing pair, so enc != eint
HP_MOTIF = ("AGAAAU", "(....)", -4.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cst", [None, "x............."])
def test_holo_ensemble_of_a_14mer(exe, oracle, mode, cst):
    """Every structure's weight: their sum is the oracle's holo partition function."""
    assert HP_SEQ[2:8] == HP_MOTIF[0]
    om = oracle.make_motif(*HP_MOTIF, mode)
    sts = structures(HP_SEQ)
    (got,) = run(exe, [("pf", HP_SEQ, cst, HP_MOTIF + (mode,), sts)])
    formed = 0
    z = 0.0
    for st, (e, status) in zip(sts, got):
        assert status == sec.status(HP_SEQ, st, cst)
        if status:
            assert e == math.inf
            continue
        assert abs(e - sec.pf_energy(oracle, HP_SEQ, st, om)) <= 1e-9, (st, e)
        formed += e != oracle.eval_structure(HP_SEQ, st)
        z += math.exp(-e / sec.KT)
    assert formed >= 1
    assert abs(-sec.KT * math.log(z) - oracle.pf_energy(HP_SEQ, cst, om)) <= 1e-6
    (mfe,) = run(exe, [("mfe", HP_SEQ, cst, HP_MOTIF + (mode,), sts)])
    best = min(e for e, status in mfe if status == 0)
    assert best == oracle.mfe_energy(HP_SEQ, cst, om)
    for st, (e, status) in zip(sts, mfe):
        if status == 0:
            assert e == sec.mfe_energy(oracle, HP_SEQ, st, om), (st, e)
