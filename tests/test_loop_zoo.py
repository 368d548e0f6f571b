"""The pinned-structure fixtures of loop_zoo.py, on the CPU: that a pinned
constraint really admits one structure (oracle MFE == loop-energy sum == ensemble
energy), that the zoo and the table batches hold every shape and reach every
table entry they are meant to (counted from loops(), not from the generator),
that the energies stay inside the packed 16-bit kernels' exact range, and the
host evaluator (energy.cpp) on every entry."""
import math

import pytest

import loop_zoo as Z

LENGTHS = (100, 150)
PF_TOL = 1e-9
# fold_common.hpp: MFE16_FLOOR = -120, MFE16_CEIL = 61.44 kcal/mol; outside them the FP32
# fallback would answer in place of the packed kernels the GPU module is about
RANGE = (-100.0, 40.0)
# the randomised and enumerated sequences (weaker pairs than the zoo's G.C), the ones the GPU cases
# fold: 10 kcal/mol under MFE16_CEIL.  The kernels range-check what they store: c(i, j), which is the
# enclosed energy asserted here, and fm / fm1 / f5.  Under a pinned constraint fm and fm1 of a cell
# are the branches' energies plus MLintern and MLbase terms, without the closing pair's MLclosing,
# so they lie about 1 kcal/mol off the enclosed multiloop's energy, and f5 is at most the whole
# structure's; 10 kcal/mol covers them
RANGE_VARIANTS = (-100.0, 51.0)


def _batch_sample(seqs):
    """Every fifth sequence and the last."""
    return seqs[::5] + seqs[-1:]


def _has_long_hairpin(st):
    return any(lp["kind"] == "hairpin" and lp["size"] > 30 for lp in Z.loops(st))


def _check_singleton(oracle, seq, st):
    e = oracle.eval_structure(seq, st)
    cst = Z.pinned(st)
    g = oracle.pf_energy(seq, cst)
    assert math.isfinite(e) and math.isfinite(g), (seq, st, e, g)
    if _has_long_hairpin(st):
        # the MFE truncates lxc * ln(u / 30) to whole dcal and the ensemble does not: the two
        # flavours differ by < 0.01 kcal/mol here, and each is the GPU's reference for its own mode;
        # eval_structure is the untruncated one
        assert abs(oracle.mfe_energy(seq, cst) - e) < 0.01, (seq, st)
        assert abs(g - e) <= PF_TOL, (seq, st, g, e)
        return
    assert oracle.mfe_energy(seq, cst) == e, (seq, st, oracle.mfe_energy(seq, cst), e)
    assert abs(g - e) <= PF_TOL, (seq, st, g, e)


@pytest.mark.parametrize("L", LENGTHS)
def test_zoo_ensembles_are_singletons(oracle, L):
    zoo = Z.shape_zoo(L)
    assert all(len(seq) == L and len(st) == L and seq == seq.upper() for seq, st in zoo)
    for (seq, st), var in zip(zoo, Z.zoo_variants(L)):
        _check_singleton(oracle, seq, st)
        for s in var:
            _check_singleton(oracle, s, st)


def test_batch_ensembles_are_singletons(oracle):
    for name, st, seqs in Z.table_batches():
        for s in _batch_sample(seqs):
            _check_singleton(oracle, s, st)


def test_oversize_interior_loop_has_no_structure(oracle):
    """16 + 15 > MAXLOOP: the pinned fold is infeasible, not an extrapolated energy."""
    st = Z.chain([(16, 15)], Z.hairpin(4))
    seq = Z.default_seq(st)
    assert oracle.mfe_energy(seq, Z.pinned(st)) == math.inf
    assert oracle.pf_energy(seq, Z.pinned(st)) == math.inf
    st = Z.chain([(15, 15)], Z.hairpin(4))
    assert math.isfinite(oracle.mfe_energy(Z.default_seq(st), Z.pinned(st)))


@pytest.mark.parametrize("L", LENGTHS)
def test_zoo_coverage(L):
    zoo = Z.shape_zoo(L)
    all_loops = [lp for _, st in zoo for lp in Z.loops(st)]
    shapes = {(lp["n1"], lp["n2"]) for lp in all_loops if lp["kind"] == "interior"}
    want = {(a, b) for a in range(31) for b in range(31) if 0 < a + b <= 30}
    assert len(want) == 495 and want <= shapes, sorted(want - shapes)
    assert max(a + b for a, b in shapes) == 30
    hairpins = {lp["size"] for lp in all_loops if lp["kind"] == "hairpin"}
    assert set(range(3, 31)) | {31, 40, L - 2 * Z.STEM} <= hairpins, sorted(hairpins)
    assert max(hairpins) == L - 2 * Z.STEM       # the largest that fits under a stem of two pairs
    multi = {(len(lp["branches"]), min(g, 2)) for lp in all_loops if lp["kind"] == "multi" for g in lp["gaps"][1:-1]}
    assert {(nb, g) for nb in (2, 3, 4) for g in (0, 1, 2)} <= multi, sorted(multi)
    ext = [lp for lp in all_loops if lp["kind"] == "exterior"]
    assert any(lp["gaps"][0] == 0 for lp in ext) and any(lp["gaps"][-1] == 0 for lp in ext)
    between = {g for lp in ext for g in lp["gaps"][1:-1]}
    assert {0, 1} <= between, between
    # the THEO aptamer innermost, under interior loops of 18 nt and more
    theo = [(seq, st) for seq, st in zoo if Z.theo_offset(seq, st) >= 0]
    assert len(theo) >= 2
    for seq, st in theo:
        o = Z.theo_offset(seq, st)
        over = [lp for lp in Z.loops(st) if lp["kind"] == "interior" and lp["closing"][0] < o]
        assert sum(lp["n1"] + lp["n2"] >= 18 for lp in over) >= 2, st
    # the refold cases' structure is one of the zoo
    seq, st = Z.refold_structure(L)
    assert (seq, st) in zoo
    lps = Z.loops(st)
    assert any(lp["kind"] == "interior" and max(lp["n1"], lp["n2"]) >= 20 and min(lp["n1"], lp["n2"]) > 0 for lp in lps)
    assert any(lp["kind"] == "interior" and min(lp["n1"], lp["n2"]) == 0 and lp["n1"] + lp["n2"] >= 10 for lp in lps)
    assert any(lp["kind"] == "multi" and len(lp["branches"]) == 3 for lp in lps)


def test_table_coverage():
    """Every entry canonical pairs reach, in every table: nothing left out."""
    want = Z.all_keys()
    n = {}
    for k in want:
        n[k[0]] = n.get(k[0], 0) + 1
    sp = Z.special_hairpins()
    assert n == dict(stack=36, bulge1=36, bulge_au=36, int11=576, int21_1x2=2304, int21_2x1=2304, int22=9216,
                     mm_interior_outer=96, mm_interior_inner=96, mm_1n_outer=96, mm_1n_inner=96, mm_23_outer=96,
                     mm_23_inner=96, mm_hairpin=96, mm_multi=96, mm_ext=96, dangle5=24, dangle3=24,
                     Triloops=len(sp["Triloops"]), Tetraloops=len(sp["Tetraloops"]), Hexaloops=len(sp["Hexaloops"]))
    assert (len(sp["Triloops"]), len(sp["Tetraloops"]), len(sp["Hexaloops"])) == (2, 16, 4)
    got = set()
    for name, st, seqs in Z.table_batches():
        assert len(st) <= 100
        for s in seqs:
            got |= Z.table_keys(s, st)
    assert want <= got, sorted(want - got)[:20]


@pytest.mark.parametrize("L", LENGTHS)
def test_fitted_batches_keep_their_coverage(oracle, L):
    """The batches as the GPU module folds them, padded to a kernel's length."""
    got = set()
    for (name, st, seqs), (_, st0, seqs0) in zip(Z.fitted_batches(L), Z.table_batches()):
        assert len(st) == L and len(seqs) == len(seqs0) and all(len(s) == L for s in seqs)
        for s in _batch_sample(seqs):
            _check_singleton(oracle, s, st)
            assert RANGE_VARIANTS[0] < oracle.eval_structure(s, st) < RANGE_VARIANTS[1], (name, s)
        for s in seqs:
            got |= Z.table_keys(s, st)
    assert Z.all_keys() <= got, sorted(Z.all_keys() - got)[:20]


@pytest.mark.parametrize("L", LENGTHS)
def test_zoo_stays_in_the_packed_range(oracle, L):
    for (seq, st), var in zip(Z.shape_zoo(L), Z.zoo_variants(L)):
        for s, t in Z.enclosed(seq, st):
            assert RANGE[0] < oracle.eval_structure(s, t) < RANGE[1], (s, t)
        for v in var:
            for s, t in Z.enclosed(v, st):
                assert RANGE_VARIANTS[0] < oracle.eval_structure(s, t) < RANGE_VARIANTS[1], (s, t)


def test_batches_stay_in_the_packed_range(oracle):
    for name, st, seqs in Z.table_batches():
        for v in seqs:
            for s, t in Z.enclosed(v, st):
                assert RANGE_VARIANTS[0] < oracle.eval_structure(s, t) < RANGE_VARIANTS[1], (name, s, t)


def test_host_evaluator(native, oracle):
    """energy.cpp's loop energies (adx_eval_structure, no device needed) under every
    shape and every table entry."""
    P = native.Params()
    for L in LENGTHS:
        for (seq, st), var in zip(Z.shape_zoo(L), Z.zoo_variants(L)):
            for s in [seq] + var:
                assert P.eval_structure(s, st) == oracle.eval_structure(s, st), (s, st)
    for name, st, seqs in Z.table_batches():
        for s in seqs:
            assert P.eval_structure(s, st) == oracle.eval_structure(s, st), (name, s, st)
