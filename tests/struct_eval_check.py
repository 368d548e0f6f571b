"""Yardstick of the structure-evaluation tests (test_struct_eval_check.py pins it on
the CPU oracle; test_struct_eval_core.py and test_gpu_struct_eval.py apply it to
the engine's per-lane code and to the kernel).

For a folded sequence, a condition (motif m or None) and a dot-bracket s:

    pf_energy(seq, s, m)   E(s) = -kT ln w(s): the oracle's partition function
                           with s pinned as an all-'x' / '()' constraint, which
                           leaves exactly s admissible (motif included)
    mfe_energy(seq, s, m)  the same through the oracle's integer MFE fold
    status(seq, s, cst)    the membership rules as plain Python, as a status byte
    prob(seq, s, cst, m)   exp(-(E(s) - G) / kT), G the oracle's ensemble energy
                           under cst; 0 for a non-member

A pinned fold of a non-member is +inf (nothing is admissible), so the two
energies agree with the documented +inf of status bits 2, 4; bit 8 (an interior
loop above MAXLOOP) is priced by eval_structure but folds to +inf, and a
malformed s has no pinned fold at all (NaN by definition).
"""
import math

from structure_check import pair_table, pin

KT = (37.0 + 273.15) * 1.98717 / 1000.0
PAIRS = {"AU", "UA", "GC", "CG", "GU", "UG"}
MAXLOOP = 30
MALFORMED, HAIRPIN, EXCLUDED, BIGLOOP = 1, 2, 4, 8
# six 14-mers whose 777 structures the tests enumerate in full
MERS14 = ["ACGGGAUGUUUAGC", "GCUUUAAGCAUCGU", "CUGGAAAGGAACUA", "AUUCUUGUUUUAGU", "UCUUACUGUAUUAG", "GUGGGCAUGAUAAC"]


def pf_energy(oracle, seq, s, motif=None):
    return oracle.pf_energy(seq, pin(s), motif)


def mfe_energy(oracle, seq, s, motif=None):
    return oracle.mfe_energy(seq, pin(s), motif)


def _admitted(s, pt, cst):
    """DB_DEFAULT | ENFORCE_BP: '.' free, 'x' unpaired, '|' paired, '<' paired with a
    base upstream, '>' downstream, '()' that pair; no pair crosses an enforced pair."""
    want = pair_table(cst)
    for k, c in enumerate(cst):
        j = pt.get(k)
        if j is None:
            if c in "|<>()":
                return False
            continue
        if c == "x" or (c == "<" and j > k) or (c == ">" and j < k):
            return False
        if c in "()" and want[k] != j:
            return False
        if j > k and any(a < b and (k < a < j < b or a < k < b < j) for a, b in want.items()):
            return False
    return True


def status(seq, s, cst=None):
    """The status byte of (seq, s) under the constraint cst (None: unconstrained)."""
    pt = pair_table(s)
    if pt is None or len(s) != len(seq) or any(c not in ".()" for c in s):
        return MALFORMED
    bits = 0
    for i, j in pt.items():
        if j < i:
            continue
        if seq[i].upper().replace("T", "U") + seq[j].upper().replace("T", "U") not in PAIRS:
            bits |= MALFORMED
        inner, k = [], i + 1
        while k < j:
            if pt.get(k, -1) > k:
                inner.append((k, pt[k]))
                k = pt[k]
            k += 1
        if not inner and j - i - 1 < 3:
            bits |= HAIRPIN
        if len(inner) == 1 and (inner[0][0] - i - 1) + (j - inner[0][1] - 1) > MAXLOOP:
            bits |= BIGLOOP
    if cst is not None and not _admitted(s, pt, cst):
        bits |= EXCLUDED
    return bits


def member(seq, s, cst=None):
    return status(seq, s, cst) == 0


def expected_energy(oracle, seq, s, cst=None, motif=None, mfe=False):
    """What the engine reports for (seq, s) under cst: NaN when malformed, +inf for
    status bits 2 and 4, else the pinned fold's energy (bit 8 apart, which no
    pinned fold prices: eval_structure, apo only)."""
    st = status(seq, s, cst)
    if st & MALFORMED:
        return math.nan
    if st & (HAIRPIN | EXCLUDED):
        return math.inf
    if st & BIGLOOP:
        assert motif is None
        return oracle.eval_structure(seq, s)
    return (mfe_energy if mfe else pf_energy)(oracle, seq, s, motif)


def prob(oracle, seq, s, cst=None, motif=None):
    if not member(seq, s, cst):
        return 0.0
    g = oracle.pf_energy(seq, cst, motif)
    return math.exp(-(pf_energy(oracle, seq, s, motif) - g) / KT)


def same(a, b, tol=0.0):
    """a == b within tol, NaN and the infinities as themselves."""
    if math.isnan(b):
        return math.isnan(a)
    if math.isinf(b):
        return a == b
    return math.isfinite(a) and abs(a - b) <= tol
