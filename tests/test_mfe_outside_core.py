"""mfe_subopt_kernel's per-lane code (addapt_amd/csrc/mfe_outside_core.hpp) without a GPU:
a stand-alone program built against the header and the host setup code stages a
sequence as the kernel's setup does and runs the inside fill, f5, f3, the outside
fill, the through energies, the selection and the tracebacks lane by lane in the
kernel's order.  It is held to subopt_check.py: every pair's energy is the CPU
oracle's fold under that forced pair, in exact dcal.  The program is built once more
with the address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded)."""
import os
import subprocess

import pytest

import loop_zoo as Z
import struct_eval_check as sec
import subopt_check as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "mfe_outside_core_probe.cc")
DELTA_DCAL = int(round(100 * sc.DELTA))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    out = str(tmp_path_factory.mktemp("mfe_outside_core") / "probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", *flags, "-I", CSRC, "-o", out,
                    SRC, os.path.join(CSRC, "energy.cpp")], check=True)
    return out


def run(exe, cases, lanes=64, delta=DELTA_DCAL, max_structs=sc.MAX_STRUCTS):
    """cases: (name, seq, cst or None, motif (seq, fold, energy) or None).  (per case a dict
    of mfe (dcal or None), within, th {(i, j): dcal}, found [(i, j, dcal, structure)]; the raw output)."""
    lines = [str(len(cases))]
    for _, seq, cst, motif in cases:
        m = motif or ("-", "-", 0.0)
        lines.append("%s %s %s %s %r 0 %d %d" % (seq, cst or "-", m[0], m[1], m[2], delta, max_structs))
    r = subprocess.run([exe, Z.PAR, str(lanes)], input="\n".join(lines) + "\n", stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out, cur = [], None
    for f in (l.split() for l in r.stdout.split("\n") if l):
        if f[0] == "M":
            cur = dict(mfe=None if f[1] == "inf" else int(f[1]), within=int(f[2]), th={}, found=[])
        elif f[0] == "T":
            cur["th"][(int(f[1]), int(f[2]))] = int(f[3])
        elif f[0] == "S":
            cur["found"].append((int(f[1]), int(f[2]), int(f[3]), f[4]))
        else:
            out.append(cur)
    assert len(out) == len(cases)
    return out, r.stdout


@pytest.fixture(scope="module")
def results(exe, oracle):
    cases = sc.cases(oracle)
    out, raw = run(exe, cases)
    return cases, out, raw


def _motif(oracle, motif):
    return oracle.make_motif(*motif) if motif else None


def test_through_is_the_fold_under_the_forced_pair(results, oracle):
    cases, out, _ = results
    for (name, seq, cst, motif), res in zip(cases, out):
        om = _motif(oracle, motif)
        assert res["mfe"] == sc.dcal(oracle.mfe_energy(seq, cst, om)), name
        assert res["th"] == sc.through(oracle, seq, cst, om), name
        if res["th"]:
            assert min(res["th"].values()) == res["mfe"] or res["mfe"] == 0, name


def test_lane_count_does_not_matter(exe, results):
    cases, _, raw = results
    assert run(exe, cases, lanes=1)[1] == raw
    assert run(exe, cases, lanes=7)[1] == raw


def test_the_list_obeys_zukers_rule(results, oracle):
    cases, out, _ = results
    for (name, seq, cst, motif), res in zip(cases, out):
        within = sc.check_list(res["th"], res["mfe"], res["found"])
        assert len(within) == res["within"], name
        om = _motif(oracle, motif)
        for i, j, e, st in res["found"]:   # each prices to its reported energy, under the constraint
            assert sec.status(seq, st, cst) == 0, (name, st)
            assert sc.dcal(sec.mfe_energy(oracle, seq, st, om)) == e, (name, st)


def test_nothing_pairs_nothing_found(results):
    cases, out, _ = results
    res = out[[c[0] for c in cases].index("allA")]
    assert res == dict(mfe=0, within=0, th={}, found=[])


def test_infeasible_constraint(exe):
    (res,), _ = run(exe, [("none", "A" * 20, "....|...............", None)])
    assert res == dict(mfe=None, within=0, th={}, found=[])


def test_max_structs_truncates_the_same_list(exe, results):
    cases, out, _ = results
    short, _ = run(exe, cases, max_structs=3)
    for res, cut in zip(out, short):
        assert cut["found"] == res["found"][:3] and cut["th"] == res["th"]


def test_every_traceback_branch_is_met(results):
    """A multiloop and an interior loop with both sides >= 2 beyond the first
    structure, and a structure seeded through the motif."""
    cases, out, _ = results
    by = {c[0]: r for c, r in zip(cases, out)}
    later = [f[3] for r in out for f in r["found"][1:]]
    assert any(sc.has_multiloop(st) for st in later)
    assert any(sc.has_wide_interior(st) for st in later)
    assert sc.seeded_through_motif(by["alt"]["found"], sc.ALT_SITE, sc.ALT_MOTIF)
    theo = by["theo"]["found"]
    assert theo and theo[0][3][sc.THEO_SITE:sc.THEO_SITE + len(Z.THEO_FOLD)] == Z.THEO_FOLD   # the site forms
