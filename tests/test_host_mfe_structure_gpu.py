"""GpuRnaFold::mfe_structure of the C++ host mirror on the GPU, against the
oracle (the yardstick of structure_check.py; apo folds also string for string)."""
import os
import subprocess

import pytest

from addapt_amd import workloads
from structure_check import check, same_energy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    lib = os.path.join(ROOT, "addapt_amd", "_lib")
    exe = str(tmp_path_factory.mktemp("probe") / "mfe_structure_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "mfe_structure_probe.cc"), "-L", lib, "-laddapt_host",
                    "-laddapt_gpu", "-Wl,-rpath," + lib], check=True)
    return exe


@pytest.mark.parametrize("case", ["theo-apo", "theo-holo", "rhf6-active"])
def test_cpp_mfe_structure_matches_oracle(oracle, probe, case):
    seq, cond, cst = {"theo-apo": (workloads.THEO_SEQ, "apo", None),
                      "theo-holo": (workloads.THEO_SEQ, "holo", None),
                      "rhf6-active": (workloads.RHF6_SEQ.upper(), "apo", workloads.RHF6_ACTIVE)}[case]
    r = subprocess.run([probe, seq, cond] + ([cst] if cst else []), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    s, e = r.stdout.split()
    e = float(e)
    m = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus()) if cond == "holo" else None
    check(oracle, seq, s, e, cst, m)
    if m is None:
        oe, os_ = oracle.mfe(seq, cst)
        assert s == os_ and same_energy(e, oe)
    else:   # the ligand pays on its own aptamer: the motif's fold, at the bonus
        assert s == workloads.THEO_FOLD
