"""struct_eval_check.py, the yardstick of the structure-evaluation tests, pinned on
the CPU oracle alone (no GPU, no engine code)."""
import math

import pytest

import struct_eval_check as sec
from test_oracle_enum import SEQS, structures

# the constrained cases of test_oracle_enum.py
CONSTRAINED = [
    ("ACGUGAAAACGU", "xxxx........"),
    ("ACGUGAAAACGU", "((........))"),
    ("GCGCUUCGGCGC", "..|........."),
    ("GCGCUUCGGCGC", "....xxxx...."),
    ("GGACUUCGGUCC", "(..........)"),
]
MERS = [s for s in SEQS if len(s) == 12] + sec.MERS14


@pytest.mark.parametrize("seq,cst", CONSTRAINED)
def test_membership_is_the_enumerators(seq, cst):
    admitted = set(structures(seq, cst))
    free = structures(seq)
    assert admitted <= set(free)
    for s in free:
        assert sec.member(seq, s, cst) == (s in admitted), (seq, cst, s)
        assert sec.status(seq, s, cst) in (0, sec.EXCLUDED)


@pytest.mark.parametrize("seq", MERS)
def test_every_enumerated_structure_is_a_member(oracle, seq):
    for s in structures(seq):
        assert sec.status(seq, s) == 0
        # the pinned fold prices exactly s: eval_structure's loops
        assert abs(sec.pf_energy(oracle, seq, s) - oracle.eval_structure(seq, s)) <= 1e-9


def test_upstream_and_downstream_marks():
    seq = "GGGAAACCC"
    assert sec.status(seq, "(((...)))", "..>...<..") == 0
    assert sec.status(seq, "(((...)))", "..<......") == sec.EXCLUDED
    assert sec.status(seq, "(((...)))", "......>..") == sec.EXCLUDED
    assert sec.status(seq, "((.....))", "..>......") == sec.EXCLUDED   # a marked base must pair


def test_status_bits():
    seq = "GGGAAAACCC"
    assert sec.status(seq, "(((....)))") == 0
    assert sec.status(seq, "(((....)).") == sec.MALFORMED
    assert sec.status(seq, "(((..[.)))") == sec.MALFORMED
    assert sec.status(seq, ".((....)))") == sec.MALFORMED
    assert sec.status(seq, "((((..))))") == sec.MALFORMED | sec.HAIRPIN      # G-A, A-C and a hairpin of 2
    assert sec.status("GGGGAACCCC", "((((..))))") == sec.HAIRPIN
    assert sec.status(seq, "(((....)))", "x.........") == sec.EXCLUDED
    long = "G" + "A" * 31 + "GGAAAACC" + "C"
    assert sec.status(long, "(" + "." * 31 + "((....))" + ")") == sec.BIGLOOP
    assert sec.status(long[1:], "." * 31 + "((....))" + ".") == 0


@pytest.mark.parametrize("seq,cst", [(s, None) for s in sec.MERS14[:3]] + CONSTRAINED)
def test_probabilities_of_an_enumeration_sum_to_one(oracle, seq, cst):
    free = structures(seq)
    total = sum(sec.prob(oracle, seq, s, cst) for s in free)
    if not structures(seq, cst):
        assert total == 0.0
    else:
        # the bar of test_oracle_enum.py: 1e-6 kcal/mol on the ensemble energy
        assert abs(sec.KT * math.log(total)) <= 1e-6, (seq, cst, total)


def test_expected_energy_of_non_members(oracle):
    seq = "GGGGAACCCC"
    assert math.isnan(sec.expected_energy(oracle, seq, "((((..)).)"))
    assert sec.expected_energy(oracle, seq, "((((..))))") == math.inf
    assert sec.expected_energy(oracle, "GGGAAAACCC", "(((....)))", "x.........") == math.inf
    long = "G" + "A" * 31 + "GGAAAACC" + "C"
    s = "(" + "." * 31 + "((....))" + ")"
    assert sec.expected_energy(oracle, long, s) == oracle.eval_structure(long, s)
    assert sec.pf_energy(oracle, long, s) > 1e5   # no fold holds it
