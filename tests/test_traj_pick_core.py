"""The trajectory picking rule's per-lane pieces (addapt_amd/csrc/traj_pick_core.hpp)
without a GPU: a stand-alone program built against the header picks from
trajectories given on stdin; its thresholds are compared with np.percentile
and its peaks with the numpy restatement in traj_pick_check.py.  The program is
built once more with the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded)."""
import os
import subprocess

import numpy as np
import pytest

from traj_pick_check import families, pick, pick_overwrite, threshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "traj_pick_core_probe.cc")
SIZES = (1, 2, 3, 5, 63, 64, 65, 257, 600)
WINDOWS = (1, 2, 7, 64, 1000)


def _program(tmp, flags=()):
    exe = str(tmp / ("probe" + "_san" * bool(flags)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    return _program(tmp_path_factory.mktemp("traj_pick_core"), flags)


def _run(exe, cases, replays=()):
    lines = ["%d %d" % (len(cases), len(replays))]
    for c, window in cases:
        lines.append(" ".join(["%d %d" % (len(c), window)] + [repr(float(x)) for x in c]))
    lines += ["%d %d %d %d" % r for r in replays]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.split("\n")
    picked = []
    for l in out[:len(cases)]:
        f = l.split()
        picked.append((float(f[0]), int(f[1]), [int(x) for x in f[2:]]))
    return picked, [int(l) for l in out[len(cases):len(cases) + len(replays)]]


@pytest.fixture(scope="module")
def cases():
    out = []
    for S in SIZES:
        for name, c in sorted(families(S, 1000 + S).items()):
            for window in WINDOWS:
                out.append((name, c, window))
    return out


def test_threshold_and_peaks_match_the_restatement(exe, cases):
    got, _ = _run(exe, [(c, w) for _, c, w in cases])
    ended = 0
    for (name, c, window), (T, n, steps) in zip(cases, got):
        ref = pick(c, window)
        assert T == threshold(c), (name, len(c), window)   # value equality: exact but for the sign of a zero
        assert n == len(steps) and steps == ref, (name, len(c), window, steps, ref)
        assert n <= -(-len(c) // window)
        assert all(b - a >= window for a, b in zip(steps, steps[1:]))
        # the overwrite-with-minimum form agrees wherever it terminates (min < T)
        other = pick_overwrite(c, window)
        if other is not None:
            ended += 1
            assert steps == other, (name, len(c), window)
        else:
            assert not c.min() < threshold(c)
    assert ended >= len(cases) // 3
    assert any(n == len(c) for (_, c, w), (_, n, _) in zip(cases, got) if w == 1 and len(c) > 1)   # all ties: every step


def test_edges(exe):
    c = np.array([1.0, 5.0, 5.0, 2.0, 5.0, 0.0, 7.0])
    cases = [(c, 1), (c, 2), (c, 100), (c[::-1], 2),
             (np.array([3.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0]), 3),   # peaks at step 0 and at step S - 1
             (np.array([0.0, -0.0, 0.0, -0.0]), 1), (np.array([-0.0, 0.0, -1.0, 0.0]), 2),
             (np.array([1.0, float("nan"), 2.0]), 1), (np.array([1.0, float("-inf"), 2.0]), 1),
             (np.array([1.0, float("inf")]), 1),
             (np.array([-1e308, 1e308, 1e308, 0.0, 5e-324, -5e-324]), 2147483647)]
    got, _ = _run(exe, cases)
    for (c, window), (T, n, steps) in zip(cases, got):
        ref = pick(c, window)
        if ref is None:
            assert n == -1 and steps == []
        else:
            assert T == threshold(c) and steps == ref, (c, window, steps, ref)
    assert got[4][2] == [0, 7]
    assert got[5][2] == [0, 1, 2, 3]   # signed zeros are equal: the lowest step first, all of them peaks


def test_replay_step(exe):
    replays = [(cur, outcome, base, parity) for cur in (1, 2, 3, 4) for outcome in (0, 1, 2, 3) for base in (1, 2, 3, 4)
               for parity in (0, 1)]
    _, got = _run(exe, [], replays)
    for (cur, outcome, base, parity), b in zip(replays, got):
        want = cur if outcome in (0, 2) else (5 - base if parity else base)
        assert b == want, (cur, outcome, base, parity, b)
