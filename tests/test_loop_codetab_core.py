"""The 1x1 .. 2x2 interior-loop energies by code pair (addapt_amd/csrc/loop_codetab_core.hpp)
without a GPU: a stand-alone program built against the header alone fills the three
source tables with values that differ in every entry and builds E[k][oc][c]; every
entry is compared with the 4-, 5- and 6-dimensional index formulas the pair kernel
used before, restated here on numpy arrays, for every code pair -- the codes of
non-pairable inner cells (type 0) included.  The program is built once more with
the address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "loop_codetab_core_probe.cc")
CODES = 175          # type * 25 + x * 5 + y, type 0 .. 6
ALLOC = 4 * CODES * CODES + 256
N11, N21, N22 = 8 * 8 * 25, 8 * 8 * 125, 8 * 8 * 625


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    out = str(tmp_path_factory.mktemp("loop_codetab_core") / ("probe" + "_san" * bool(flags)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", out, SRC], check=True)
    return out


def _sources():
    """The probe's source tables: entry n of int11 | int21 | int22 laid end to end holds n."""
    v = np.arange(N11 + N21 + N22, dtype=np.int64)
    return (v[:N11].reshape(8, 8, 5, 5), v[N11:N11 + N21].reshape(8, 8, 5, 5, 5),
            v[N11 + N21:].reshape(8, 8, 5, 5, 5, 5))


def _expected():
    """E[k][oc][c] by the kernel's former formulas: the closing pair's code gives its type and
    the unpaired bases S[i+1], S[j-1]; the inner pair's code its reversed type t2 and the bases
    beside it, S[q+1] (second digit) and S[p-1] (last digit)."""
    int11, int21, int22 = _sources()
    oc, c = np.meshgrid(np.arange(CODES), np.arange(CODES), indexing="ij")
    ty, si1, sj1 = oc // 25, (oc // 5) % 5, oc % 5
    t2, cq, cp = c // 25, (c // 5) % 5, c % 5
    return np.stack([int11[ty, t2, si1, sj1],             # 1x1: int11[type][t2][si1][sj1]
                     int21[ty, t2, si1, cq, sj1],         # 1x2: int21[type][t2][si1][sq1][sj1]
                     int21[t2, ty, cq, si1, cp],          # 2x1: int21[t2][type][sq1][si1][sp1]
                     int22[ty, t2, si1, cp, cq, sj1]])    # 2x2: int22[type][t2][si1][sp1][sq1][sj1]


def test_the_sources_differ_in_every_entry():
    a, b, c = _sources()
    assert len(set(a.ravel()) | set(b.ravel()) | set(c.ravel())) == N11 + N21 + N22 < 65536


def test_type_by_multiply_shift():
    """The kernel takes a code's type as (code * 41) >> 10: code // 25 for every code."""
    k = np.arange(CODES)
    assert np.array_equal((k * 41) >> 10, k // 25)


def test_every_code_pair(exe):
    r = subprocess.run([exe, "build"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    E = np.frombuffer(r.stdout, dtype=np.uint16)
    assert E.size == ALLOC
    got = E[:4 * CODES * CODES].reshape(4, CODES, CODES).astype(np.int64)
    ref = _expected()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    # each table reads more than one entry per (type, type) block: the bases matter
    for k in range(4):
        assert len(np.unique(got[k])) > 49 * 24
    # the entries past the table are impossible, not left as they were
    assert (E[4 * CODES * CODES:] == 0x7FFF).all()


@pytest.mark.parametrize("table,entry", [(0, 0), (1, N21 // 2 + 3), (2, 6 * 5000 + 6 * 625 + 624)])
def test_unequal_halves_are_refused(exe, table, entry):
    """entry: one that some code pair reads (types <= 6 on both sides)."""
    r = subprocess.run([exe, "uneven", str(table), str(entry)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.strip() == "0"
