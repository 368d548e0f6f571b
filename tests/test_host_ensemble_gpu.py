"""GpuRnaFold::ensemble_structures of the C++ host mirror on the GPU: the same
fold compound as the Python face builds (motif bonus kT ln(Kd / 1 M) on both
sides), so the strings and the three statistics are the Python face's bit for
bit; the Python face itself is held to the definitions in
test_gpu_ensemble_struct.py."""
import os
import subprocess

import pytest

from addapt_amd import workloads
from ensemble_check import pairs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    lib = os.path.join(ROOT, "addapt_amd", "_lib")
    exe = str(tmp_path_factory.mktemp("probe") / "ensemble_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "ensemble_probe.cc"), "-L", lib, "-laddapt_host",
                    "-laddapt_gpu", "-Wl,-rpath," + lib], check=True)
    return exe


@pytest.mark.parametrize("case", ["rhf6-apo", "rhf6-holo", "rhf6-holo-active", "rhf6-apo-gamma4"])
def test_cpp_ensemble_structures_equal_the_python_face(native, probe, case):
    seq = workloads.RHF6_SEQ.upper()
    cond, cst, gamma = {"rhf6-apo": ("apo", None, 1.0), "rhf6-holo": ("holo", None, 1.0),
                        "rhf6-holo-active": ("holo", workloads.RHF6_ACTIVE, 1.0),
                        "rhf6-apo-gamma4": ("apo", None, 4.0)}[case]
    r = subprocess.run([probe, seq, cond, repr(gamma)] + ([cst] if cst else []), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cen, mea, nums = r.stdout.split("\n")[:3]
    f = native.Fold(seq)
    if cond == "holo":
        f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    if cst:
        f.add_constraint(cst)
    pc, pm, st = f.ensemble_structures(gamma)
    assert (cen, mea) == (pc, pm)
    assert [float(x) for x in nums.split()] == [st.mea, st.centroid_dist, st.diversity]
    assert pairs_of(cen) and pairs_of(mea) and len(cen) == len(seq)


def test_cpp_empty_ensemble(probe):
    r = subprocess.run([probe, "AAAAAAAAAA", "apo", "1", "(........)"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cen, mea, nums = r.stdout.split("\n")[:3]
    assert cen == mea == "." * 10 and [x.lstrip("-") for x in nums.split()] == ["nan"] * 3
