"""GpuRnaFold::sample_structures of the C++ host mirror on the GPU: validity,
the constraint, and pair frequencies against the oracle under the bound of
sample_check.py."""
import math
import os
import subprocess

import pytest

from addapt_amd import workloads
from sample_check import bound, pair_frequencies, pair_violations, within
from structure_check import pin, satisfies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 4096

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    lib = os.path.join(ROOT, "addapt_amd", "_lib")
    exe = str(tmp_path_factory.mktemp("probe") / "pf_sample_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "pf_sample_probe.cc"), "-L", lib, "-laddapt_host",
                    "-laddapt_gpu", "-Wl,-rpath," + lib], check=True)
    return exe


@pytest.mark.parametrize("case", ["rhf6-apo", "rhf6-holo", "rhf6-holo-active"])
def test_cpp_samples_follow_the_oracle(oracle, probe, case):
    seq = workloads.RHF6_SEQ.upper()
    cond, cst = {"rhf6-apo": ("apo", None), "rhf6-holo": ("holo", None),
                 "rhf6-holo-active": ("holo", workloads.RHF6_ACTIVE)}[case]
    r = subprocess.run([probe, seq, cond, str(S), "2016"] + ([cst] if cst else []), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split()
    e, samples = float(lines[0]), lines[1:]
    assert len(samples) == S
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus()) if cond == "holo" else None
    ref, P = oracle.bppm(seq, cst, m)
    assert abs(e - ref) <= 1e-4, (e, ref)
    f, bad = pair_frequencies(samples, seq)
    assert bad == [] and all(satisfies(s, cst) for s in set(samples))
    v = pair_violations(f, P, S)
    assert v == [], v[:3]
    if m is not None:
        # the ligand pays on rhf(6): the motif's own fold at its site, against that event's
        # probability Z(site pinned) / Z from two oracle partition functions, and against the
        # motif's innermost pair where the oracle says the pair forms only through the motif
        # (the two references agree to a tenth of the bound; see test_gpu_pf_sample.py)
        o = seq.index(workloads.THEO_SEQ)
        assert P[o, o + 26] > 0.05
        fm = sum(s[o:o + 27] == workloads.THEO_FOLD for s in samples) / S
        base = cst or "." * len(seq)
        pinned = base[:o] + pin(workloads.THEO_FOLD) + base[o + 27:]
        p_fold = math.exp(-(oracle.pf_energy(seq, pinned, m) - ref) / oracle.KT_KCAL)
        assert within(fm, p_fold, S), (fm, p_fold)
        if abs(P[o + 9, o + 14] - p_fold) <= 0.1 * bound(p_fold, S):
            assert within(fm, P[o + 9, o + 14], S), (fm, P[o + 9, o + 14])
