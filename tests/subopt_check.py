"""What the Zuker suboptimal-structure calls must return, from the CPU oracle alone;
test_mfe_outside_core.py (the per-lane code on the host) and test_gpu_subopt.py
(the kernel) apply it.

The best structure through a pair (i, j) is the fold under the constraint merged
with that forced pair: oracle.mfe_energy(seq, merge(constraint, i, j), motif).
Energies are integer dcal/mol on both sides, so the comparison is exact.

Directions follow the oracle's (and the engine's) reading of the constraint
characters: '<' pairs upstream, so it may stand at the 3' end j of a pair, '>'
pairs downstream and may stand at the 5' end i."""
import math
import random

import loop_zoo as Z

DELTA = 3.0          # kcal/mol
MAX_STRUCTS = 32


def rand_seq(n, seed, alphabet="GCGCAU"):
    r = random.Random(seed)
    return "".join(r.choice(alphabet) for _ in range(n))


S12, S24, S40 = rand_seq(12, 1), rand_seq(24, 2), rand_seq(40, 3)
# THEO between 11 and 12 bases, chosen so that the site forms in the holo MFE and
# structures beyond the first hold a multiloop
THEO_HOLO = "GCCACUGGGAA" + Z.THEO_SEQ + "GUAGCGUCACUG"
THEO_SITE = 11   # 0-based start
# A motif whose fold competes with the natural fold of its site, 0.5 kcal/mol above
# it: the site's outer pair is listed with the natural fold first, so a pair of the
# motif's own fold is still unmarked and seeds a structure THROUGH the motif
ALT_SEQ = "CGGGAGCAU" "GCACUGCCGACCGGGUUUGC" "CCAGAUGCUGA"
ALT_MOTIF = ("GCACUGCCGACCGGGUUUGC", "(((...((....))...)))", -3.8)
ALT_SITE = 9   # 0-based start


def cases(oracle):
    """(name, seq, constraint or None, motif (seq, fold, energy kcal/mol) or None)"""
    theo = (Z.THEO_SEQ, Z.THEO_FOLD, oracle.theo_bonus())
    return [
        ("r12", S12, None, None), ("r24", S24, None, None), ("r40", S40, None, None),
        ("allA", "A" * 20, None, None),
        ("x", S24, "....x...................", None),
        ("bar", S24, ".......|................", None),
        ("gt", S24, "....>...................", None),
        ("lt", S24, "................<.......", None),
        ("lt5", S24, "......<.................", None),
        ("helix", S24, ".(((.............)))....", None),
        ("mixed", S24, "xxxx..(........)...xx...", None),
        ("theo", THEO_HOLO, None, theo),
        ("alt", ALT_SEQ, None, ALT_MOTIF),
    ]


def seeded_through_motif(found, site, motif):
    """The listed structures whose seed lies strictly inside the motif site and which hold the motif's fold there."""
    n = len(motif[0])
    return [f for f in found if site + 1 < f[0] and f[1] < site + n and f[3][site:site + n] == motif[1]]


def _tables(cst, n):
    """1-based partner and innermost enclosing forced pair of every position."""
    pt, enc, stk = [0] * (n + 2), [0] * (n + 2), []
    for k in range(1, n + 1):
        c = cst[k - 1]
        enc[k] = stk[-1] if stk else 0
        if c == "(":
            stk.append(k)
        elif c == ")":
            a = stk.pop()
            pt[a], pt[k] = k, a
            enc[k] = stk[-1] if stk else 0
    assert not stk
    return pt, enc


def merge(cst, i, j, n):
    """The constraint with '(' at i and ')' at j (1-based), or None where it excludes the pair."""
    cst = cst or "." * n
    pt, enc = _tables(cst, n)
    a, b = cst[i - 1], cst[j - 1]
    if a == "x" or b == "x" or a == "<" or b == ">":
        return None
    if pt[i] or pt[j]:
        return cst if pt[i] == j else None
    if enc[i] != enc[j]:
        return None   # crosses a forced pair
    return cst[:i - 1] + "(" + cst[i:j - 1] + ")" + cst[j:]


def dcal(e):
    return None if math.isinf(e) else int(round(100.0 * e))


def through(oracle, seq, cst=None, motif=None, pairs=None):
    """{(i, j): dcal} of every pair (or of `pairs`) that some structure holds."""
    n = len(seq)
    out = {}
    for i, j in pairs if pairs is not None else [(i, j) for i in range(1, n + 1) for j in range(i + 4, n + 1)]:
        m = merge(cst, i, j, n)
        if m is None:
            continue
        e = dcal(oracle.mfe_energy(seq, m, motif))
        if e is not None:
            out[(i, j)] = e
    return out


def pairs_of(st):
    pt = Z.pair_table(st)
    return {(k + 1, p + 1) for k, p in enumerate(pt) if p > k}


def has_multiloop(st):
    return any(lp["kind"] == "multi" for lp in Z.loops(st))


def has_wide_interior(st):
    return any(lp["kind"] == "interior" and lp["n1"] >= 2 and lp["n2"] >= 2 for lp in Z.loops(st))


def check_list(th, mfe, found, delta_dcal=int(round(100 * DELTA)), max_structs=MAX_STRUCTS):
    """th: {(i, j): dcal}; mfe: dcal or None; found: [(i, j, dcal, structure)].
    Every property of the list that needs no pricing; returns the pairs within delta."""
    if mfe is None:
        assert not found
        return set()
    limit = mfe + delta_dcal
    within = {p for p, e in th.items() if e <= limit}
    es = [f[2] for f in found]
    assert es == sorted(es)
    assert len({f[3] for f in found}) == len(found)
    if found and min(th.values(), default=None) == mfe:
        assert found[0][2] == mfe
    marked = set()
    for i, j, e, st in found:   # Zuker's rule, replayed
        left = sorted((th[p], p) for p in within - marked)
        assert left and left[0] == (e, (i, j)), (left[:3], (i, j, e))
        ps = pairs_of(st)
        assert (i, j) in ps and th[(i, j)] == e
        marked |= ps
    assert len(found) <= max_structs
    if len(found) < max_structs:
        assert within <= marked
    return within
