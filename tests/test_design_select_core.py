"""The design selection rule's per-lane pieces (addapt_amd/csrc/design_select_core.hpp)
without a GPU: a stand-alone program built against the header alone packs
sequences given on stdin into bit planes, orders them by the sort key and
selects in rank order; its designs and pair histogram are compared with the
numpy restatement in design_select_check.py, and it checks for itself that
packing, unpacking and the packed distance agree with the characters.  The
program is built once more with the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded)."""
import os
import subprocess

import numpy as np
import pytest

from design_select_check import chars, cloud, codes_of, distances, multiply_covered, pair_hist, select, walkers_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "design_select_core_probe.cc")
LENGTHS = (1, 5, 63, 64, 65, 128, 129, 255)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    out = str(tmp_path_factory.mktemp("design_select_core") / ("probe" + "_san" * bool(flags)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", out, SRC], check=True)
    return out


def _run(exe, cases=(), orders=(), firsts=()):
    lines = ["%d %d %d" % (len(cases), len(orders), len(firsts))]
    for ch, scores, radius, K in cases:
        lines.append("%d %d %d %d" % (ch.shape[0], ch.shape[1], radius, K))
        lines += ["%s %r" % (row.tobytes().decode(), float(s)) for row, s in zip(ch, scores)]
    lines += ["%r %d %r %d" % (float(a), ia, float(b), ib) for a, ia, b, ib in orders]
    lines += [" ".join(map(str, [len(d) - 1] + list(d))) for d in firsts]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.split("\n")
    ints = lambda l: np.array(l.split(), np.int64)
    got = [dict(n=int(out[5 * c]), leaders=ints(out[5 * c + 1]), sizes=ints(out[5 * c + 2]),
                member_of=ints(out[5 * c + 3]), pair_hist=ints(out[5 * c + 4])) for c in range(len(cases))]
    rest = [int(l) for l in out[5 * len(cases):] if l.strip()]
    return got, rest[:len(orders)], rest[len(orders):]


def _same(got, codes, scores, radius, K, what):
    dist = distances(codes)
    ref = select(codes, scores, radius, K, dist)
    assert got["n"] == len(ref["leaders"]), what
    for k in ("leaders", "sizes", "member_of"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    assert np.array_equal(got["pair_hist"], pair_hist(codes, scores, dist)), what
    return ref, dist


def test_distances_of_the_restatement():
    codes, _ = cloud(40, 65, 3)
    plain = (codes[:, None, :] != codes[None, :, :]).sum(axis=2)
    assert np.array_equal(distances(codes), plain)


def test_pack_distance_and_selection(exe):
    cases = []
    for N in LENGTHS:
        codes, scores = cloud(64, N, 100 + N)
        ch = chars(codes)
        ch[::3] |= 0x20   # lower against upper case: the same bases
        for radius in (0, 1, 3, N):
            cases.append((ch, scores, radius, 64, codes))
    for M, N, seed in ((600, 65, 1), (257, 129, 2), (600, 5, 3)):
        codes, scores = cloud(M, N, seed)
        for radius, K in ((0, M), (3, M), (6, 7)):
            cases.append((chars(codes), scores, radius, K, codes))
    got, _, _ = _run(exe, [c[:4] for c in cases])
    several = leftover = 0
    for g, (ch, scores, radius, K, codes) in zip(got, cases):
        ref, dist = _same(g, codes, scores, radius, K, (ch.shape, radius, K))
        several += multiply_covered(dist, ref, radius) > 0
        leftover += bool((ref["member_of"] < 0).any())
    assert several > 0 and leftover > 0   # the lowest-numbered-leader clause and the cap were exercised


def test_order_ties_zeros_and_non_finite(exe):
    orders = [(2.0, 5, 1.0, 0), (1.0, 0, 2.0, 5), (1.5, 3, 1.5, 4), (1.5, 4, 1.5, 3), (0.0, 1, -0.0, 2),
              (-0.0, 1, 0.0, 2), (-0.0, 2, 0.0, 1), (-1e308, 0, -5e-324, 1), (5e-324, 1, 0.0, 0), (0.0, 0, 5e-324, 1)]
    _, got, _ = _run(exe, orders=orders)
    assert got == [int(a > b or (a == b and ia < ib)) for a, ia, b, ib in orders]
    # signed zeros tie (index order); NaN and the infinities take no part
    codes = codes_of(["ACGUA", "ACGUC", "ACGUA", "GGGGG", "ACGUA", "ACGUC"])
    scores = np.array([-0.0, 0.0, 0.0, np.nan, np.inf, -np.inf])
    got, _, _ = _run(exe, [(chars(codes), scores, 0, 6)])
    assert got[0]["leaders"].tolist() == [0, 1] and got[0]["member_of"].tolist() == [0, 1, 0, -1, -1, -1]
    assert got[0]["pair_hist"].sum() == 3
    _same(got[0], codes, scores, 0, 6, "zeros")


def test_first_of_walker(exe):
    firsts = [[0], [-1], [0, 0], [0, 1], [1, 0, 1], [1, 0, 2], [-1, -1], [3, -1, 3], [0, 1, 2, 3, 0], [0, 1, 2, 3, 4]]
    _, _, got = _run(exe, firsts=firsts)
    assert got == [int(d[-1] >= 0 and d[-1] not in d[:-1]) for d in firsts]
    # over a walker's picks these flags count its distinct designs, as walkers_of does over all walkers
    member = np.array([0, 1, 0, -1, 2, 2, 0])
    walker = np.array([0, 0, 0, 1, 1, 1, 2])
    firsts = [member[walker == w][:k + 1].tolist() for w in range(3) for k in range((walker == w).sum())]
    _, _, got = _run(exe, firsts=firsts)
    counts = np.zeros(3, np.int64)
    for flag, d in zip(got, [f[-1] for f in firsts]):
        counts[d] += flag if d >= 0 else 0
    assert np.array_equal(counts, walkers_of(member, walker, 3))
