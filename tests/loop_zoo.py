"""Pinned structures: the fixtures of test_loop_zoo.py and test_gpu_loop_zoo.py.

A hard constraint in which every position is an enforced pair or 'x' admits
exactly one structure S, so the constrained MFE, the constrained ensemble energy,
every sample, the traceback, the centroid and the MEA structure are S and its
loop-energy sum: one mishandled loop of S is a wrong answer, with no minimum or
average to hide it.

shape_zoo(L)     structures of exactly L nt that hold every interior-loop and
                 bulge shape (n1, n2), 0 < n1 + n2 <= 30, every hairpin size
                 3..30 and 31, 40, L - 4, multiloops, exterior loops and the THEO
                 aptamer under chains of large loops
table_batches()  a few structures of <= 100 nt, each with an enumerated batch of
                 sequences that together reach every energy-table entry canonical
                 pairs can reach
loops(st)        a plain loop decomposition; loop_keys() names the table entries a
                 loop of a sequence reads, all_keys() the entries there are

Deterministic: fixed seeds, nothing written."""
import itertools
import os
import random

from addapt_amd import workloads

PAR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "addapt_amd", "data",
                   "rna_turner2004_addapt.par")
BASES = "ACGU"
PAIRS = ("CG", "GC", "GU", "UG", "AU", "UA")
MAXLOOP = 30
STEM = 2          # pairs of the G.C stems between the loops
THEO_SEQ, THEO_FOLD = workloads.THEO_SEQ, workloads.THEO_FOLD


def pair_table(st):
    pt, stk = [-1] * len(st), []
    for k, c in enumerate(st):
        if c == "(":
            stk.append(k)
        elif c == ")":
            a = stk.pop()
            pt[a], pt[k] = k, a
    assert not stk, st
    return pt


def pinned(st):
    """The constraint that admits st alone: '.' -> 'x', brackets kept."""
    return st.replace(".", "x")


def loops(st):
    """Every loop of st: dicts of kind ('exterior', 'hairpin', 'interior', 'multi'),
    closing pair (i, j) (None for the exterior loop), the inner pairs `branches` in
    5' to 3' order and `gaps`, the unpaired runs before, between and after them.
    A hairpin also has `size`; an interior loop (stacks and bulges included)
    `n1`, `n2`, the 5' and the 3' run."""
    pt, n = pair_table(st), len(st)

    def inside(i, j):
        br, gaps, g, k = [], [], 0, i + 1
        while k < j:
            if pt[k] > k:
                br.append((k, pt[k]))
                gaps.append(g)
                g, k = 0, pt[k] + 1
            else:
                g, k = g + 1, k + 1
        return br, gaps + [g]

    br, gaps = inside(-1, n)
    out = [dict(kind="exterior", closing=None, branches=br, gaps=gaps)]
    for i in range(n):
        j = pt[i]
        if j < i:
            continue
        br, gaps = inside(i, j)
        lp = dict(closing=(i, j), branches=br, gaps=gaps)
        if not br:
            lp.update(kind="hairpin", size=gaps[0])
        elif len(br) == 1:
            lp.update(kind="interior", n1=gaps[0], n2=gaps[1])
        else:
            lp.update(kind="multi")
        out.append(lp)
    return out


# ------------------------------------------------------------ table entries
def special_hairpins(path=PAR):
    """{'Triloops': [...], 'Tetraloops': [...], 'Hexaloops': [...]}: the listed
    loops with their closing bases, read from the parameter file."""
    out, sec = {"Triloops": [], "Tetraloops": [], "Hexaloops": []}, None
    for line in open(path):
        w = line.split()
        if line.startswith("#"):
            sec = w[1] if len(w) > 1 and w[1] in out else None
        elif sec and w:
            out[sec].append(w[0])
    return out


_SPECIAL = None


def _special():
    global _SPECIAL
    if _SPECIAL is None:
        _SPECIAL = special_hairpins()
    return _SPECIAL


def loop_keys(seq, lp):
    """The energy-table entries the loop lp of seq reads, as tuples headed by the
    table's name.  Pair types are the two bases 5' to 3' as the table sees them
    (the inner pair of an interior loop reversed, a multiloop's closing pair
    reversed), mismatch bases in the table's own index order."""
    kind = lp["kind"]
    if kind == "exterior":
        keys = []
        for p, q in lp["branches"]:
            t = seq[p] + seq[q]
            if p > 0 and q + 1 < len(seq):
                keys.append(("mm_ext", t, seq[p - 1], seq[q + 1]))
            elif p > 0:
                keys.append(("dangle5", t, seq[p - 1]))
            elif q + 1 < len(seq):
                keys.append(("dangle3", t, seq[q + 1]))
        return keys
    i, j = lp["closing"]
    t = seq[i] + seq[j]
    if kind == "hairpin":
        u, s = lp["size"], seq[i:j + 1]
        for size, name in ((3, "Triloops"), (4, "Tetraloops"), (6, "Hexaloops")):
            if u == size and s in _special()[name]:
                return [(name, s)]
        if u == 3:
            return [("hairpin3", t)]
        return [("mm_hairpin", t, seq[i + 1], seq[j - 1])]
    if kind == "multi":
        return [("mm_multi", t[::-1], seq[j - 1], seq[i + 1])] + \
               [("mm_multi", seq[p] + seq[q], seq[p - 1], seq[q + 1]) for p, q in lp["branches"]]
    (p, q), n1, n2 = lp["branches"][0], lp["n1"], lp["n2"]
    t2 = seq[q] + seq[p]
    si1, sj1, sp1, sq1 = seq[i + 1], seq[j - 1], seq[p - 1], seq[q + 1]
    nl, ns = max(n1, n2), min(n1, n2)
    if nl == 0:
        return [("stack", t, t2)]
    if ns == 0:
        return [("bulge1" if nl == 1 else "bulge_au", t, t2)]
    if ns == 1 and nl == 1:
        return [("int11", t, t2, si1, sj1)]
    if ns == 1 and nl == 2:
        return [("int21_1x2", t, t2, si1, sq1, sj1) if n1 == 1 else ("int21_2x1", t2, t, sq1, si1, sp1)]
    if ns == 2 and nl == 2:
        return [("int22", t, t2, si1, sp1, sq1, sj1)]
    name = "mm_1n" if ns == 1 else "mm_23" if (ns, nl) == (2, 3) else "mm_interior"
    return [(name + "_outer", t, si1, sj1), (name + "_inner", t2, sq1, sp1)]


def table_keys(seq, st):
    """loop_keys of every loop of (seq, st)."""
    return {k for lp in loops(st) for k in loop_keys(seq, lp)}


def all_keys():
    """Every entry canonical pairs and the four bases reach, in loop_keys' names."""
    def prod(name, n_pairs, n_bases):
        return {(name,) + c for c in itertools.product(*([PAIRS] * n_pairs + [BASES] * n_bases))}

    keys = prod("stack", 2, 0) | prod("bulge1", 2, 0) | prod("bulge_au", 2, 0)
    keys |= prod("int11", 2, 2) | prod("int21_1x2", 2, 3) | prod("int21_2x1", 2, 3) | prod("int22", 2, 4)
    for name in ("mm_interior", "mm_1n", "mm_23"):
        keys |= prod(name + "_outer", 1, 2) | prod(name + "_inner", 1, 2)
    keys |= prod("mm_hairpin", 1, 2) | prod("mm_multi", 1, 2) | prod("mm_ext", 1, 2)
    keys |= prod("dangle5", 1, 1) | prod("dangle3", 1, 1)
    for name, loops_ in _special().items():
        keys |= {(name, s) for s in loops_}
    return keys


# ------------------------------------------------------------ structures
def hairpin(h):
    return "(" * STEM + "." * h + ")" * STEM


def chain(shapes, core):
    """core under interior loops of the given (n1, n2), the first outermost, each
    closed by a stem of STEM pairs."""
    s = core
    for n1, n2 in reversed(shapes):
        s = "(" * STEM + "." * n1 + s + "." * n2 + ")" * STEM
    return s


def multiloop(n_branches, gap, branch=None):
    """A multiloop of hairpin branches with `gap` unpaired bases before, between
    and after them."""
    b = branch or hairpin(4)
    return "(" * STEM + "." * gap + ("." * gap).join([b] * n_branches) + "." * gap + ")" * STEM


def pad(st, L, where):
    """st with unpaired exterior bases up to L nt: where 0: 5' of it (the last stem
    ends at L - 1), 1: 3' of it (the first stem starts at 0), 2: both."""
    r = L - len(st)
    assert r >= 0, (len(st), L)
    a = (r, 0, r // 2)[where]
    return "." * a + st + "." * (r - a)


def default_seq(st):
    """G.C and C.G pairs in turn, A unpaired, the THEO aptamer's own bases under
    its fold."""
    pt, s, k = pair_table(st), [], 0
    for i, c in enumerate(st):
        if c == "(":
            s.append("GC"[k % 2])
            k += 1
        elif c == ")":
            s.append({"G": "C", "C": "G"}[s[pt[i]]])
        else:
            s.append("A")
    o = st.find(THEO_FOLD)
    if o >= 0:
        s[o:o + len(THEO_SEQ)] = THEO_SEQ
    return "".join(s)


def theo_offset(seq, st):
    """Where (seq, st) holds the THEO aptamer with its fold, or -1."""
    o = st.find(THEO_FOLD)
    return o if o >= 0 and seq[o:o + len(THEO_SEQ)].upper() == THEO_SEQ else -1


SHAPES = [(n1, n2) for n1 in range(MAXLOOP + 1) for n2 in range(MAXLOOP + 1 - n1) if n1 + n2 > 0]
HAIRPINS = list(range(3, 31))
THEO_CHAINS = {100: [[(17, 1), (9, 12), (0, 12)], [(1, 17), (12, 9), (10, 0)]],
               150: [[(17, 1), (9, 12), (0, 23), (15, 15)], [(1, 17), (12, 9), (23, 0), (2, 20)]]}
REFOLD_CHAINS = {100: [(22, 3), (0, 12)], 150: [(22, 3), (0, 12), (1, 17), (12, 9)]}


def refold_structure(L):
    """The zoo structure of the incremental-refold cases: a loop with 22 nt on one
    side, a 12-nt bulge and a 3-branch multiloop under them."""
    ml = "((" + "." + hairpin(4) + hairpin(5) + ".." + hairpin(3) + "." + "))"
    st = pad(chain(REFOLD_CHAINS[L], ml), L, 2)
    return default_seq(st), st


def _special_structures(L):
    out = [hairpin(L - 2 * STEM),
           pad(chain([(2, 2), (0, 3)], hairpin(31)), L, 0),
           pad(chain([(3, 1), (4, 0), (1, 1)], hairpin(40)), L, 1)]
    # multiloops of 2, 3, 4 branches with 0, 1, 3 unpaired between them, side by side in
    # the exterior loop with 0, 1, 2 unpaired between the stems
    out.append(pad(multiloop(2, 0) + multiloop(3, 0) + multiloop(4, 0), L, 1))
    out.append(pad(multiloop(2, 1) + "." + multiloop(3, 1) + "." + multiloop(4, 1), L, 0))
    out.append(pad(multiloop(2, 3) + ".." + multiloop(3, 3), L, 2))
    out.append(pad(multiloop(4, 3) + "." + chain([(5, 5)], multiloop(2, 2, hairpin(7))), L, 2))
    out.extend(pad(chain(shapes, THEO_FOLD), L, k) for k, shapes in enumerate(THEO_CHAINS[L]))
    out.append(refold_structure(L)[1])
    return out


_zoo = {}


def shape_zoo(L):
    """[(sequence, dot-bracket)], each of exactly L nt (see the module docstring)."""
    if L in _zoo:
        return list(_zoo[L])
    sts = _special_structures(L)
    pending = sorted(SHAPES, key=lambda s: (-(s[0] + s[1]), s))
    hps = list(HAIRPINS)
    rng = random.Random(20161015 + L)
    while pending:
        h = hps.pop() if hps else 4
        room, picked = L - (h + 2 * STEM), []
        for s in list(pending):             # first fit, largest first
            if s[0] + s[1] + 2 * STEM <= room:
                picked.append(s)
                pending.remove(s)
                room -= s[0] + s[1] + 2 * STEM
        rng.shuffle(picked)
        sts.append(pad(chain(picked, hairpin(h)), L, len(sts) % 3))
    while hps:                              # (never at 100 or 150: fewer sizes than chains)
        sts.append(pad(hairpin(hps.pop()), L, 2))
    _zoo[L] = [(default_seq(st), st) for st in sts]
    assert all(len(s) == L == len(t) for s, t in _zoo[L])
    return list(_zoo[L])


def variants(seq, st, n, seed):
    """n sequences that realise st: every pair one of the six canonical ones, every
    unpaired base one of the four, drawn from Random(seed); the THEO aptamer's
    bases stay.  test_loop_zoo.py holds their energies inside the packed range."""
    rng, pt, o = random.Random(seed), pair_table(st), theo_offset(seq, st)
    out = []
    for _ in range(n):
        s = list(seq)
        for i in range(len(s)):
            if o <= i < o + len(THEO_SEQ) and o >= 0:
                continue
            if pt[i] > i:       # C.G and G.C three times as often: the sum of many weak loops stays in MFE16's range
                s[i], s[pt[i]] = rng.choice(PAIRS + PAIRS[:2] * 2)
            elif pt[i] < 0:     # A half of the time before the draw: the free ensemble stays within reach of the
                s[i] = rng.choice("A" * 4 + BASES)      # pinned structure (test_gpu_loop_zoo.py _pf_groups)
        out.append("".join(s))
    return out


def zoo_variants(L, n=8):
    """variants() of every shape_zoo(L) structure, in its order, under fixed seeds."""
    return [variants(seq, st, n, 1000 * L + k) for k, (seq, st) in enumerate(shape_zoo(L))]


def enclosed(seq, st):
    """(seq, st) and the part under each of its pairs, as (sequence, dot-bracket)."""
    return [(seq, st)] + [(seq[i:j + 1], st[i:j + 1]) for i, j in enumerate(pair_table(st)) if j > i]


# ------------------------------------------------------------ table batches
def _decode(c, radices):
    out = []
    for r in reversed(radices):
        out.append(c % r)
        c //= r
    return out[::-1]


def _fill_interior(s, lp, c):
    """Combination c of an interior loop's slot: both pair types and the bases next
    to the pairs in full for int11 / int21 / int22, the two pair types for stacks
    and bulges, else (pair, 5' base, 3' base) written at both ends of the loop."""
    (i, j), (p, q), shape = lp["closing"], lp["branches"][0], (lp["n1"], lp["n2"])
    if min(shape) == 0:
        a, b = _decode(c % 36, [6, 6])
        (s[i], s[j]), (s[p], s[q]) = PAIRS[a], PAIRS[b]
    elif shape in ((1, 1), (1, 2), (2, 1), (2, 2)):
        free = sorted({i + 1, p - 1, q + 1, j - 1})
        d = _decode(c % (36 * 4 ** len(free)), [6, 6] + [4] * len(free))
        (s[i], s[j]), (s[p], s[q]) = PAIRS[d[0]], PAIRS[d[1]]
        for pos, b in zip(free, d[2:]):
            s[pos] = BASES[b]
    else:
        t, a, b = _decode(c % 96, [6, 4, 4])
        (s[i], s[j]), (s[p], s[q]) = PAIRS[t], PAIRS[t]
        s[i + 1] = s[p - 1] = BASES[a]
        s[j - 1] = s[q + 1] = BASES[b]


def _n_combos(shape):
    if min(shape) == 0:
        return 36
    if shape in ((1, 1), (1, 2), (2, 1), (2, 2)):
        return 36 * 4 ** len({0, shape[0] - 1}) * 4 ** len({0, shape[1] - 1})
    return 96


def _chain_batch(shapes, h):
    """The chain of `shapes` over a hairpin of h nt, and the sequences in which the
    slots of one shape walk through its combinations in turn; the hairpin walks
    through (pair, first base, last base)."""
    st = chain(shapes, hairpin(h))
    # the stems' own stacks are no slots; a (0, 0) shape is the middle stack of a 4-pair helix
    by_close = {lp["closing"]: lp for lp in loops(st) if lp["kind"] == "interior"}
    pt, slots, pos = pair_table(st), [], 0
    for shape in shapes:                    # the loop closed by the stem's inner pair
        i = pos + STEM - 1
        lp = by_close[(i, pt[i])]
        assert (lp["n1"], lp["n2"]) == shape, (shape, lp)
        slots.append(lp)
        pos = lp["branches"][0][0]
    hp = [lp for lp in loops(st) if lp["kind"] == "hairpin"][0]
    count = {s: shapes.count(s) for s in set(shapes)}
    # each shape starts its walk at another pair type, so that one sequence mixes strong and weak pairs
    start = {s: g * (_n_combos(s) // 6) for g, s in enumerate(sorted(count, key=shapes.index))}
    n_seq = max(96, max(-(-_n_combos(s) // m) for s, m in count.items()))
    base = default_seq(st)
    seqs = []
    for n in range(n_seq):
        s, rank = list(base), {}
        for lp, shape in zip(slots, shapes):
            r = rank.get(shape, 0)
            rank[shape] = r + 1
            _fill_interior(s, lp, start[shape] + n * count[shape] + r)
        t, a, b = _decode(n % 96, [6, 4, 4])
        i, j = hp["closing"]
        (s[i], s[j]), s[i + 1], s[j - 1] = PAIRS[t], BASES[a], BASES[b]
        seqs.append("".join(s))
    return st, seqs


def _stem_end_batch():
    """Exterior and multiloop stem ends: a stem at position 0, a multiloop of two
    branches and a stem that ends the sequence, two unpaired bases between any two
    stems so that every stem end has its own neighbours.  Each stem end walks
    through (pair, 5' neighbour, 3' neighbour)."""
    st = hairpin(4) + ".." + "((" + ".." + hairpin(4) + ".." + hairpin(4) + ".." + "))" + ".." + hairpin(4)
    base, n = default_seq(st), len(st)
    ends = []                               # (i, j, position of the 5' neighbour, of the 3' neighbour)
    for lp in loops(st):
        if lp["kind"] == "exterior":
            ends += [(p, q, p - 1 if p > 0 else None, q + 1 if q + 1 < n else None) for p, q in lp["branches"]]
        elif lp["kind"] == "multi":
            i, j = lp["closing"]
            ends += [(i, j, i + 1, j - 1)] + [(p, q, p - 1, q + 1) for p, q in lp["branches"]]
    seqs = []
    for c in range(96):
        s = list(base)
        t, a, b = _decode(c, [6, 4, 4])
        for i, j, n5, n3 in ends:
            s[i], s[j] = PAIRS[t]
            if n5 is not None:
                s[n5] = BASES[a]
            if n3 is not None:
                s[n3] = BASES[b]
        seqs.append("".join(s))
    return st, seqs


def _special_batch():
    """The listed triloops, tetraloops and hexaloops with their closing bases, side
    by side, each under one more G.C pair."""
    sp = _special()
    st = "..".join("(" * STEM + "." * h + ")" * STEM for h in (3, 4, 6))
    base = default_seq(st)
    hps = sorted((lp for lp in loops(st) if lp["kind"] == "hairpin"), key=lambda lp: lp["size"])
    seqs = []
    for n in range(max(len(v) for v in sp.values())):
        s = list(base)
        for lp, name in zip(hps, ("Triloops", "Tetraloops", "Hexaloops")):
            i, j = lp["closing"]
            s[i:j + 1] = sp[name][n % len(sp[name])]
        seqs.append("".join(s))
    return st, seqs


def _fit(st, seqs, L):
    """(st, seqs) with unpaired A up to L nt: in the middle of a run of two or more
    between two exterior stems where there is one (every stem keeps its neighbours,
    the first and the last stay at the ends), else on both sides."""
    r, ext = L - len(st), loops(st)[0]
    assert r >= 0
    at = [ext["branches"][m - 1][1] + 2 for m in range(1, len(ext["branches"])) if ext["gaps"][m] >= 2]
    if at:
        return st[:at[0]] + "." * r + st[at[0]:], [s[:at[0]] + "A" * r + s[at[0]:] for s in seqs]
    a = r // 2
    return "." * a + st + "." * (r - a), ["A" * a + s + "A" * (r - a) for s in seqs]


def fitted_batches(L):
    """table_batches() at exactly L nt."""
    return [(name,) + _fit(st, seqs, L) for name, st, seqs in table_batches()]


_batches = None


def table_batches():
    """[(name, dot-bracket, [sequences])]: see the module docstring.  Over a batch
    every sequence realises the structure; over all batches table_keys reaches
    all_keys()."""
    global _batches
    if _batches is None:
        _batches = [
            ("int22",) + _chain_batch([(2, 2)] * 9, 4),   # 1024 sequences; 11 loops take the weak ones to 46 kcal/mol
            ("int21-int11",) + _chain_batch([(1, 2), (2, 1)] * 4 + [(1, 1)] * 2, 4),
            ("mismatches",) + _chain_batch([(1, 4), (4, 1), (2, 3), (3, 2), (3, 3), (2, 5), (0, 1), (1, 0), (0, 3),
                                            (3, 0), (0, 0)], 5),
            ("stem-ends",) + _stem_end_batch(),
            ("special-hairpins",) + _special_batch(),
        ]
        assert all(len(st) <= 100 and all(len(s) == len(st) for s in seqs) for _, st, seqs in _batches)
    return list(_batches)
