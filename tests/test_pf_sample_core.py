"""The sampler's random numbers and selection rule (addapt_amd/csrc/pf_sample_core.hpp)
without a GPU: a stand-alone program built against the header prints its
generator's words and pick()'s choices; the words are compared with a
Python-integer restatement of Philox4x32-10 written here, the choices with the
inverse CDF.  The program is built once more with the address and
undefined-behaviour sanitizers (stand-alone: nothing is preloaded)."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "pf_sample_core_probe.cc")
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Salmon et al. (SC'11): ten rounds, multipliers D2511F53 / CD9E8D57, Weyl key bumps."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, w, k, t):
    return philox4x32_10((t, k, w, 0), (seed & M32, seed >> 32))[0]


def _tuples():
    rng = random.Random(77)
    out = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (2 ** 64 - 1, M32, M32, 8 * 255),
           (2 ** 32, 0, 0, 0), (2 ** 32 + 1, 4095, 99999, 2040), (0xDEADBEEFCAFEF00D, 0, M32, 0)]
    for t in range(0, 8 * 255 + 1, 60):
        out.append((12345678901234567, 7, 3, t))
    while len(out) < 1200:
        out.append((rng.getrandbits(64) if rng.random() < 0.7 else rng.getrandbits(31),
                    rng.choice((0, 1, 69, 4095, 2 ** 31 - 1, rng.getrandbits(32))),
                    rng.choice((0, 1, 15, 99999, 2 ** 31 - 1, rng.getrandbits(32))), rng.randrange(0, 8 * 255 + 1)))
    return out


def _inverse_cdf(w, u):
    """pick()'s rule in exact order: the first positive weight whose running sum exceeds u * total."""
    total = 0.0
    for x in w:
        if x > 0.0:
            total += x
    thr, cum, last = u * total, 0.0, -1
    for c, x in enumerate(w):
        if x > 0.0:
            cum += x
            last = c
            if cum > thr:
                return c
    return last


WEIGHTS = [
    [1.0],
    [0.0, 0.0, 2.0, 0.0, 1.0, 0.0],
    [0.25, 0.25, 0.25, 0.25],
    [1e-300, 1.0, 1e-300],
    [3.0, 0.0, 0.0, 5.0, 0.0, 1e-9, 2.0, 0.0],
    [0.0, 0.0, 0.0],
    [],
    [0.1] * 10,
    [0.0, -1.0, 2.0, 0.0],   # a negative weight is as good as none
    [float(k % 7) for k in range(200)],
]


def _program(tmp, flags=()):
    exe = str(tmp / ("probe" + "_san" * bool(flags)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


def _run(exe, tuples, picks):
    lines = ["%d %d" % (len(tuples), len(picks))]
    lines += ["%d %d %d %d" % t for t in tuples]
    for w, u in picks:
        lines.append(" ".join([repr(u), str(len(w))] + [repr(x) for x in w]))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    words = [l.split() for l in out[:len(tuples)]]
    chosen = [int(l) for l in out[len(tuples):len(tuples) + len(picks)]]
    return words, chosen


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    return _program(tmp_path_factory.mktemp("pf_sample_core"), flags)


def _picks():
    grid = [k / 64.0 for k in range(64)] + [0.999999940395355224609375, 1e-30, 0.5 + 2 ** -24]
    return [(w, u) for w in WEIGHTS for u in grid]


def test_known_answer():
    """Random123's kat_vectors: philox4x32 10 rounds."""
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32, M32, M32, M32), (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)


def test_generator_matches_restatement(exe):
    tuples = _tuples()
    assert len(tuples) >= 1000 and any(s > 2 ** 32 for s, _, _, _ in tuples)
    words, _ = _run(exe, tuples, [])
    for (seed, w, k, t), (x, u) in zip(tuples, words):
        ref = draw(seed, w, k, t)
        assert int(x) == ref, (seed, w, k, t)
        assert float(u) == (ref >> 8) / 16777216.0 and 0.0 <= float(u) < 1.0


def test_pick_is_the_inverse_cdf(exe):
    picks = _picks()
    _, chosen = _run(exe, [], picks)
    for (w, u), c in zip(picks, chosen):
        assert c == _inverse_cdf(w, u), (w, u, c)
        assert c == -1 or w[c] > 0.0, (w, u, c)   # a zero weight is never returned


def test_pick_edges(exe):
    cases = [([0.0, 0.0, 2.0, 0.0, 1.0, 0.0], 0.0, 2),       # u = 0: the first nonzero candidate
             ([0.0, 3.0], 0.0, 1),
             ([1.0, 0.0, 1.0, 0.0], 0.999999940395355224609375, 2),
             ([0.0, 0.0, 0.0], 0.5, -1),
             ([], 0.5, -1),
             # u * total rounds up to the last partial sum: no sum exceeds it, the last nonzero candidate wins
             ([1e16, 1.0, 0.0], 1.0, 1),
             ([0.1] * 10 + [0.0], 1.0, 9)]
    _, chosen = _run(exe, [], [(w, u) for w, u, _ in cases])
    assert chosen == [c for _, _, c in cases]
