"""The sequence autocorrelation's per-lane pieces (addapt_amd/csrc/traj_autocorr_core.hpp)
without a GPU: a stand-alone program built against the header alone packs series
given on stdin into bit planes and counts the matches at every lag with the word-
pair shift, the tail mask and the popcount, as the lag kernel does; its counts and
its correlation times are compared with the numpy restatement in
traj_autocorr_check.py.  The program is built once more with the address and
undefined-behaviour sanitizers (stand-alone: nothing is preloaded)."""
import os
import subprocess

import numpy as np
import pytest

from traj_autocorr_check import families, matches, tau, tau_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "traj_autocorr_core_probe.cc")
SIZES = (1, 2, 63, 64, 65, 128, 129, 600)


def _program(tmp, flags=()):
    exe = str(tmp / ("probe" + "_san" * bool(flags)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    return _program(tmp_path_factory.mktemp("traj_autocorr_core"), flags)


def _run(exe, series=(), taus=()):
    lines = ["%d %d" % (len(series), len(taus))]
    for x in series:
        lines.append(" ".join([str(len(x))] + [str(int(c)) for c in x]))
    for m, n_series, kept, baseline in taus:
        lines.append(" ".join(["%d %d %d %r" % (len(m) - 1, n_series, kept, float(baseline))] + [str(int(v)) for v in m]))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)   # 3, 4: the shift or the mask differs from its bit-by-bit form
    out = r.stdout.split("\n")
    return ([np.array(l.split(), np.int64) for l in out[:len(series)]],
            [int(l) for l in out[len(series):len(series) + len(taus)]])


@pytest.fixture(scope="module")
def series():
    out = []
    for S in SIZES:
        for name, x in sorted(families(3, S, 2000 + S).items()):
            for p in range(x.shape[1]):
                out.append((name, x[:, p]))
    return out


def test_every_lag_matches_the_restatement(exe, series):
    got, _ = _run(exe, [x for _, x in series])
    for (name, x), m in zip(series, got):
        S = len(x)
        assert np.array_equal(m, matches(x, S - 1)), (name, S)
        assert m[0] == S
        if name == "constant":
            assert np.array_equal(m, S - np.arange(S))
        if name == "alternating":
            assert np.array_equal(m, np.where(np.arange(S) % 2 == 0, S - np.arange(S), 0))
    # the cycle needs both planes: its low plane alone repeats with period 2
    cyc = [m for (name, x), m in zip(series, got) if name == "cycle" and len(x) == 600][0]
    assert cyc[2] == 0 and cyc[4] == 596


def test_correlation_time(exe):
    cases = []
    for S in SIZES:
        for name, x in sorted(families(5, S, 3000 + S).items()):
            for K in sorted({min(1, S - 1), min(64, S - 1), S - 1}):
                m = matches(x, K).sum(axis=1)
                counts = np.stack([(x == c).sum(axis=0) for c in (1, 2, 3, 4)], axis=1)
                f = counts / float(S)
                for base in (0.25, float((f * f).sum(axis=1).mean()), 0.0):
                    if base < 1.0 and tau_margin(m, 5, S, base) < 1e-9:
                        continue   # a tie with the level: rounding may decide
                    cases.append((m, 5, S, base))
    # by hand: a_k = 1, 0.9, 0.6, 0.3 against (1 - 0.25) / e = 0.2759 above 0.25
    cases.append((np.array([100, 81, 48, 21]), 10, 10, 0.25))
    cases.append((np.array([100, 81, 48, 21]), 10, 10, 1.0))     # nothing ever changed
    cases.append((np.array([100, 90, 80, 70]), 10, 10, 0.25))    # not decayed
    cases.append((np.array([100]), 10, 10, 0.25))                # no lag to look at
    _, got = _run(exe, taus=cases)
    want = [tau(*c) for c in cases]
    assert got == want
    assert got[-4:] == [3, 0, -1, -1]
    assert len(cases) > 100 and len({t for t in got}) > 4
