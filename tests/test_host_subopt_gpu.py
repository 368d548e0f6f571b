"""GpuRnaFold::subopt_structures of the C++ host mirror on the GPU: the Python fold
layer's list (test_gpu_subopt.py holds that one to the oracle), value for value."""
import os
import subprocess

import numpy as np
import pytest

import subopt_check as sc
from addapt_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    lib = os.path.join(ROOT, "addapt_amd", "_lib")
    exe = str(tmp_path_factory.mktemp("probe") / "subopt_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "subopt_probe.cc"), "-L", lib, "-laddapt_host",
                    "-laddapt_gpu", "-Wl,-rpath," + lib], check=True)
    return exe


@pytest.mark.parametrize("case", ["r40-apo", "theo-holo-constrained"])
def test_cpp_subopt_equals_the_python_fold_layer(native, probe, case):
    seq, cond, cst = {"r40-apo": (sc.S40, "apo", None),
                      "theo-holo-constrained": (sc.THEO_HOLO, "holo", "x" + "." * (len(sc.THEO_HOLO) - 1))}[case]
    r = subprocess.run([probe, seq, cond, repr(sc.DELTA), str(sc.MAX_STRUCTS)] + ([cst] if cst else []),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    f = native.Fold(seq)
    if cond == "holo":
        f.add_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    if cst:
        f.add_constraint(cst)
    sub = f.subopt_structures(sc.DELTA, sc.MAX_STRUCTS)
    rows = [l.split() for l in r.stdout.split("\n") if l]
    assert rows[0][0] == "M" and np.float32(float(rows[0][1])) == np.float32(sub.mfe) and int(rows[0][2]) == sub.n_pairs_within
    got = [((int(a), int(b)), np.float32(float(e)), st) for _, a, b, e, st in rows[1:]]
    assert got == list(zip(sub.seeds, sub.energies, sub.structures)) and len(got) >= 2
