"""Which kernels the dispatcher (addapt_amd/csrc/dispatch.hip) chooses, by name.

One context, two walkers and one MC step per case; `last_kernel_names()` must
equal the table entry exactly.  The cases are fold mode {pf, mfe} x {no pair
term, one pair term} x the lengths on both sides of every coverage boundary
the code names, the four kernel-choice environment overrides, ADX_NO_MFE16,
and the lengths that are refused:

  100 / 101   PX_NMAX (pf_cells) and mfe_pair_covers; OR_NMIN / RG_NMIN = 101
  112 / 113   OX_NMAX (outside_cells): the ring kernels take every PF length
              from 101, so both sides dispatch to them.  outside_cells beyond
              100 needs ADX_PF_KERNEL=rows, and there its LDS check binds
              before OX_NMAX: it covers 105, bppm_kernel takes over from 108.
              The library this table was recorded from fails score_kernel's
              or bppm_kernel's launch at 106, 107, 112 and 113 with "invalid
              argument", so the override's cases are the nearest lengths that
              run: 105 / 108, and 111 / 114 (the last lockstep length)
  150 / 151   the largest mfe_cells layout (CLay<150>)
  152 / 153   the largest length whose outside pass fits one CU's LDS
  154 / 155   the largest length the rows kernel (lds_bytes) accepts; it bounds
              every context, so RG_NMAX = 190 / 191 is refused, not dispatched

The expected strings were recorded by running this table against the library
built from the commit before dispatch.hip existed (one file then held the rows
fold, the MC step and the dispatcher), not against the code under test.
"""
import pytest

from addapt_amd import workloads

pytestmark = pytest.mark.gpu

CELLS = "pf_cells_kernel (scores combined in step_tail_kernel)"
RING = "pf_ring_kernel (scores combined in step_tail_kernel)"
MFE_PAIR = "mfe_pair_kernel + score_kernel<MinPlus> (FP32 fallback launch); scores combined in step_tail_kernel"
MFE_CELLS = "mfe_cells_kernel + score_kernel<MinPlus> (FP32 fallback launch); scores combined in step_tail_kernel"
ROWS16 = "score_kernel<512, 1, MinPlus16> + score_kernel<MinPlus> (FP32 fallback launch)"
REFOLD = " (inside refold + outside)"

# (fold mode, pair terms, length, environment) -> (inside, outside)
CASES = [
    ("pf", 0, 100, {}, CELLS, ""),
    ("pf", 0, 101, {}, RING, ""),
    ("pf", 0, 150, {}, RING, ""),
    ("pf", 0, 151, {}, RING, ""),
    ("pf", 0, 153, {}, RING, ""),
    ("pf", 0, 154, {}, "score_kernel<768, 1, SumProd>", ""),
    ("pf", 1, 100, {}, CELLS, "outside_cells_kernel"),
    ("pf", 1, 101, {}, RING, "outside_ring_kernel"),
    ("pf", 1, 112, {}, RING, "outside_ring_kernel"),
    ("pf", 1, 113, {}, RING, "outside_ring_kernel"),
    ("pf", 1, 150, {}, RING, "outside_ring_kernel"),
    ("pf", 1, 151, {}, RING, "outside_ring_kernel"),
    ("pf", 1, 152, {}, RING, "outside_ring_kernel"),
    ("mfe", 0, 100, {}, MFE_PAIR, ""),
    ("mfe", 0, 101, {}, MFE_CELLS, ""),
    ("mfe", 0, 150, {}, MFE_CELLS, ""),
    ("mfe", 0, 151, {}, ROWS16, ""),
    ("mfe", 0, 154, {}, ROWS16, ""),
    ("mfe", 1, 100, {}, ROWS16, "bppm_kernel<512>" + REFOLD),
    ("mfe", 1, 101, {}, ROWS16, "bppm_kernel<512>" + REFOLD),
    ("mfe", 1, 150, {}, ROWS16, "bppm_kernel<1024, GOUT>" + REFOLD),
    ("mfe", 1, 151, {}, ROWS16, "bppm_kernel<1024, GOUT>" + REFOLD),
    ("mfe", 0, 100, {"ADX_MFE_KERNEL": "rows"}, ROWS16, ""),
    ("mfe", 0, 100, {"ADX_MFE_PAIR": "0"}, MFE_CELLS, ""),
    ("pf", 0, 100, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 2, SumProd>", ""),
    ("pf", 0, 150, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 1, SumProd>", ""),
    ("pf", 1, 100, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 2, SumProd>", "outside_cells_kernel"),
    ("pf", 1, 105, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 2, SumProd>", "outside_cells_kernel"),
    ("pf", 1, 108, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 2, SumProd>", "bppm_kernel<512>"),
    ("pf", 1, 111, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 2, SumProd>", "bppm_kernel<512>"),
    ("pf", 1, 114, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 1, SumProd>", "bppm_kernel<1024, GOUT>"),
    ("pf", 1, 150, {"ADX_PF_KERNEL": "rows"}, "score_kernel<768, 1, SumProd>", "bppm_kernel<1024, GOUT>"),
    ("pf", 1, 100, {"ADX_OUTSIDE_KERNEL": "bppm"}, CELLS, "bppm_kernel<512>"),
    ("pf", 1, 101, {"ADX_OUTSIDE_KERNEL": "bppm"}, RING, "outside_ring_kernel"),
    ("mfe", 0, 100, {"ADX_NO_MFE16": "1"}, "score_kernel<768, 2, MinPlus>", ""),
    ("mfe", 0, 150, {"ADX_NO_MFE16": "1"}, "score_kernel<512, 1, MinPlus>", ""),
    ("mfe", 1, 100, {"ADX_NO_MFE16": "1"}, "score_kernel<768, 2, MinPlus>", "bppm_kernel<512>" + REFOLD),
]

# lengths no kernel covers: ADX_EUNSUPPORTED with this text
REFUSED = [
    ("pf", 0, 155, "sequence length 155 needs 165504 B of LDS (> 163840)"),
    ("mfe", 0, 155, "sequence length 155 needs 165504 B of LDS (> 163840)"),
    ("pf", 0, 190, "sequence length 190 needs 243376 B of LDS (> 163840)"),
    ("pf", 0, 191, "sequence length 191 needs 246000 B of LDS (> 163840)"),
    ("pf", 1, 153, "base-pair probabilities of length 153 do not fit one CU's LDS yet"),
    ("mfe", 1, 153, "base-pair probabilities of length 153 do not fit one CU's LDS yet"),
]

ENV_VARS = ("ADX_MFE_KERNEL", "ADX_MFE_PAIR", "ADX_PF_KERNEL", "ADX_OUTSIDE_KERNEL", "ADX_NO_MFE16")


def _engine(native, fold, pair, N):
    tmpl, active = workloads.synthetic(N)
    terms = workloads.default_objective()
    if pair:
        terms = terms + [("holo", ("pair", 0, N - 1), True, 1.0)]
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    eng = native.Engine(tmpl, [active], terms, aptamer=apt, fold_mode=fold,
                        thermostat=native.make_thermostat("fixed", t=1.0))
    return eng, workloads.walker_sequences(tmpl, [active], 2)


def _case_id(c):
    return "%s-%s-%d%s" % (c[0], "pair" if c[1] else "nopair", c[2],
                           "".join("-%s=%s" % kv for kv in sorted(c[3].items())) if isinstance(c[3], dict) else "")


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_dispatch_names(native, monkeypatch, case):
    fold, pair, N, env, inside, outside = case
    for k in ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng, seqs = _engine(native, fold, pair, N)
    eng.walkers_init([1, 2], seqs)
    eng.run_steps(1)
    got = eng.last_kernel_names()
    print(case[:4], got)
    assert tuple(got) == (inside, outside)


@pytest.mark.parametrize("case", REFUSED, ids=_case_id)
def test_dispatch_refuses(native, monkeypatch, case):
    fold, pair, N, text = case
    for k in ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(native.AdxError) as ei:
        _engine(native, fold, pair, N)
    print(case[:3], str(ei.value))
    assert ei.value.status == native.EUNSUPPORTED
    assert text in str(ei.value)
