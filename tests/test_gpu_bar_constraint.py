"""A macrostate whose only constraint characters are '|' ("this base is paired").

The fold kernels apply the unpaired-run limits of interior loops only when
their setup found the fold constrained, and that test reads the positions'
flags and enforced partners.  A '|' once set neither, only up[i] = 0 (the base
may not stay unpaired), so a '|'-only constraint folded with interior loops
closed over the marked base; it has a flag bit of its own now (setup_core.hpp
build_constraint).  Each fold kernel's energies are compared with the oracle's here
(pf_cells / pf_ring / mfe_pair / mfe_cells through score_batch; the rows kernel
and bppm_kernel through test_gpu_bppm.py's constrained matrices).
"""
import pytest

from addapt_amd import workloads
from parity_bounds import DG_TOL
from structure_check import same_energy

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fold,N", [("pf", 60), ("pf", 101), ("pf", 150), ("mfe", 60), ("mfe", 101), ("mfe", 150)])
def test_bar_only_macrostate(native, oracle, fold, N):
    tmpl, _ = workloads.synthetic(N)
    bars = (N // 5, N // 2 + 17, N - 9)              # a free base, one after the aptamer, one near the end
    macro = "".join("|" if k in bars else "." for k in range(N))
    terms = workloads.default_objective()
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    eng = native.Engine(tmpl, [macro], terms, aptamer=apt, fold_mode=fold,
                        thermostat=native.make_thermostat("fixed", t=1.0))
    seqs = workloads.walker_sequences(tmpl, [macro], 6)
    _, _, dg = eng.score_batch(seqs)
    motif = oracle.make_motif(workloads.THEO_SEQ, workloads.THEO_FOLD, oracle.theo_bonus())
    energy = oracle.pf_energy if fold == "pf" else oracle.mfe_energy
    differs = 0
    for v in range(eng.info.n_variants):
        _, cond, mac = eng.variant(v)
        for w, seq in enumerate(seqs):
            m = motif if cond == 1 else None
            ref = energy(seq, macro if mac >= 0 else None, m)
            if fold == "pf":
                assert abs(dg[w, v] - ref) <= DG_TOL, (fold, N, v, w, dg[w, v], ref)
            else:
                assert same_energy(dg[w, v], ref), (fold, N, v, w, dg[w, v], ref)
            if mac >= 0:
                differs += abs(ref - energy(seq, None, m)) > 0.05
    assert differs >= 6, differs                     # the constraint binds: most folds move by > 0.05 kcal/mol
