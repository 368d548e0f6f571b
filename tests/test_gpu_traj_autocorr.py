"""The per-position sequence autocorrelation on the GPU (addapt_amd/csrc/traj_autocorr.hip)
against the numpy restatement in traj_autocorr_check.py: the stateless
adx_autocorr_codes on synthetic code trajectories, and adx_record_autocorr on the
pick record of real runs in both fold modes, where the expected sequences come
from a twin context advanced one step at a time and the expected outcomes from
the host trace of the same run.  Every count is compared for equality."""
import numpy as np
import pytest
import torch

from addapt_amd import workloads
from traj_autocorr_check import baseline, families, matches, tau

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 129, 1000)
LAGS = (0, 1, 63, 64, 65)   # and S - 1
N_POS = (1, 3, 70)
N_TRAJ = (1, 37)


def _codes(S):
    """(S, 37, 70): the families over and over with fresh seeds, one per trajectory."""
    cols, k = [], 0
    while len(cols) < max(N_TRAJ):
        cols += [x for _, x in sorted(families(max(N_POS), S, 9000 + 17 * S + k).items())]
        k += 1
    return np.ascontiguousarray(np.stack(cols[:max(N_TRAJ)], axis=1))


@pytest.mark.parametrize("S", SIZES)
def test_autocorr_codes(native, S):
    codes = _codes(S)
    full = matches(codes, S - 1)   # (S, 37, 70), once for every sub-shape and lag below
    for nt in N_TRAJ:
        for npos in N_POS:
            sub, ref = codes[:, :nt, :npos], full[:, :nt, :npos]
            for K in sorted({min(k, S - 1) for k in LAGS + (S - 1,)}):
                pm, tm = native.autocorr_codes(sub, K)
                assert pm.shape == (npos, K + 1) and tm.shape == (nt, K + 1)
                assert np.array_equal(pm, ref[:K + 1].sum(axis=1).T), (S, nt, npos, K)
                assert np.array_equal(tm, ref[:K + 1].sum(axis=2).T), (S, nt, npos, K)
    if S > 2:   # the families differ: the test is not one of constants
        assert full[1].min() == 0 and full[1].max() == S - 1


def test_autocorr_codes_more_than_one_tile_of_steps(native):
    """The lag kernel stages 256 words (16 384 steps) of a plane at a time: two
    tiles and a last word of one bit, with lags in three tiles and up to S - 1."""
    S = 16384 + 65
    fam = families(3, S, 4242)
    codes = np.ascontiguousarray(np.stack([fam[k] for k in ("cycle", "iid", "last_step", "rare")], axis=1))
    assert codes.shape == (S, 4, 3)
    m = matches(codes, 700)
    pm, tm = native.autocorr_codes(codes, 700)
    assert np.array_equal(pm, m.sum(axis=1).T) and np.array_equal(tm, m.sum(axis=2).T)
    one = codes[:, 1:2, :1]   # iid
    full = matches(one, S - 1)
    pm, tm = native.autocorr_codes(one, S - 1)
    assert np.array_equal(pm, full.sum(axis=1).T) and np.array_equal(tm, full.sum(axis=2).T)
    assert 0 < pm[0, 1] < S - 1


def test_autocorr_codes_errors(native):
    codes = _codes(65)[:, :3, :3]
    for wrong in (0, 5):
        c = codes.copy()
        c[64, 2, 1] = wrong
        with pytest.raises(native.AdxError) as e:
            native.autocorr_codes(c, 10)
        assert e.value.status == native.EINVAL
    with pytest.raises(native.AdxError) as e:
        native.autocorr_codes(codes, 65)       # max_lag = S
    assert e.value.status == native.EINVAL and "64" in str(e.value)
    with pytest.raises(native.AdxError) as e:
        native.autocorr_codes(codes, -1)
    assert e.value.status == native.EINVAL
    pm, _ = native.autocorr_codes(codes, 64)   # the largest lag allowed: one comparison a series
    assert np.array_equal(pm[:, 64], (codes[64] == codes[0]).sum(axis=0))


W = 37
SEEDS = list(range(500, 500 + W))
CHUNKS = (150, 250)
PICK_WINDOW = 40


def _engine(native, fold):
    tmpl, active = workloads.synthetic(64)
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=50)
    eng = native.Engine(tmpl, [active], workloads.default_objective(), aptamer=apt, thermostat=th, fold_mode=fold)
    eng.walkers_init(SEEDS, workloads.walker_sequences(tmpl, [active], W))
    return eng, tmpl, active


def _closure_positions(tmpl, active):
    """(changeable flags, partner positions): a freely mutable position (upper case,
    not a ')') and the partner its '(' pairs with."""
    stack, partner = [], {}
    for i, ch in enumerate(active):
        if ch == "(":
            stack.append(i)
        elif ch == ")":
            partner[stack.pop()] = i
    free = [i for i, ch in enumerate(tmpl) if ch.isupper() and active[i] != ")"]
    flags = np.zeros(len(tmpl), bool)
    flags[free] = True
    partners = [partner[i] for i in free if i in partner]
    flags[partners] = True
    return flags, partners


@pytest.fixture(scope="module", params=["mfe", "pf"])
def recorded(request, native):
    """A recorded run with its host trace, the autocorrelation taken before and
    after picks(), the same run without a record or any call, and the codes after
    every step from a twin advanced one step at a time."""
    fold = request.param
    eng, tmpl, active = _engine(native, fold)
    eng.record(sum(CHUNKS))
    traces = [eng.run_steps(n, trace=True) for n in CHUNKS]
    before = eng.autocorr(120, 0)
    picks = eng.picks(PICK_WINDOW)
    plain, _, _ = _engine(native, fold)
    for n in CHUNKS:
        plain.run_steps(n)
    twin, _, _ = _engine(native, fold)
    x = np.zeros((sum(CHUNKS), W, len(tmpl)), np.uint8)
    for s in range(sum(CHUNKS)):
        twin.run_steps(1)
        for w, seq in enumerate(twin.download()[0]):
            x[s, w] = ["ACGU".index(ch) + 1 for ch in seq.upper()]
    return dict(eng=eng, plain=plain, tmpl=tmpl, active=active, x=x, before=before, picks=picks,
                outcome=np.concatenate([t["outcome"] for t in traces]))


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("discard", (0, 1, 150, 399))
def test_record_autocorr(recorded, discard):
    r = recorded
    eng, x, outcome = r["eng"], r["x"], r["outcome"]
    S, N = x.shape[0], x.shape[2]
    kept = S - discard
    K = min(120, kept - 1)
    got = eng.autocorr(K, discard)
    chg, partners = _closure_positions(r["tmpl"], r["active"])
    assert np.array_equal(got["changeable"], chg) and 0 < chg.sum() < N and partners
    m = matches(x[discard:], K)                                        # (K + 1, W, N)
    assert np.array_equal(got["pos_matches"], m.sum(axis=1).T)
    assert np.array_equal(got["walker_matches"], m[:, :, chg].sum(axis=2).T)
    counts = np.stack([(x[discard:] == c).sum(axis=(0, 1)) for c in (1, 2, 3, 4)], axis=1)
    assert np.array_equal(got["base_counts"], counts)
    assert np.array_equal(got["outcome_counts"],
                          np.stack([(outcome[discard:] == c).sum(axis=0) for c in range(4)], axis=1))
    assert got["outcome_counts"].sum() == W * kept and got["kept_steps"] == kept
    # every other position matches at every step by definition
    assert np.array_equal(got["pos_matches"][~chg], np.repeat(W * (kept - np.arange(K + 1))[None], (~chg).sum(), axis=0))
    b = baseline(counts, chg, W * kept)
    assert got["baseline"] == b
    assert got["tau"] == tau(m[:, :, chg].sum(axis=(1, 2)), W * int(chg.sum()), kept, b)
    if K >= 1:
        # not vacuous: positions did change from one step to the next, among them a
        # partner, which is never chosen itself and only ever written as a complement
        moved = [p for p in np.flatnonzero(chg) if got["pos_matches"][p][1] < W * (kept - 1)]
        assert moved and set(moved) & set(partners)
    pm, lm = eng.last_autocorr_ms()
    assert pm > 0.0 and lm > 0.0


def test_record_autocorr_has_no_side_effects(recorded):
    r = recorded
    eng = r["eng"]
    first = eng.autocorr(120, 0)
    _same(first, r["before"])            # before and after picks(), and twice
    _same(eng.autocorr(120, 0), first)
    picks, counts = eng.picks(PICK_WINDOW)
    assert picks == r["picks"][0] and np.array_equal(counts, r["picks"][1])
    assert first["tau"] >= 1 or first["tau"] == -1
    # the final walker state equals that of a run without a record or the call
    a, b = eng.download(), r["plain"].download()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_record_autocorr_errors(native):
    eng, _, _ = _engine(native, "mfe")
    with pytest.raises(native.AdxError) as e:
        eng.autocorr(10)                       # before record()
    assert e.value.status == native.ESTATE
    eng.record(30)
    with pytest.raises(native.AdxError) as e:
        eng.autocorr(10)                       # nothing recorded yet
    assert e.value.status == native.ESTATE
    eng.run_steps(20)
    for lag, discard in ((-1, 0), (5, -1), (5, 20), (0, 25)):
        with pytest.raises(native.AdxError) as e:
            eng.autocorr(lag, discard)
        assert e.value.status == native.EINVAL, (lag, discard)
    with pytest.raises(native.AdxError) as e:
        eng.autocorr(20)                       # 20 kept steps: lags up to 19
    assert e.value.status == native.EINVAL and "19" in str(e.value)
    with pytest.raises(native.AdxError) as e:
        eng.autocorr(15, 5)                    # 15 kept steps: lags up to 14
    assert e.value.status == native.EINVAL and "14" in str(e.value)
    assert eng.autocorr(19)["pos_matches"].shape == (eng.N, 20)
    assert eng.autocorr(0, 19)["kept_steps"] == 1
    # an import changes sequences outside the log: the record is broken
    seqs = torch.empty(W * eng.N, dtype=torch.uint8, device="cuda")
    scores = torch.empty(W, dtype=torch.float64, device="cuda")
    eng.export_walkers(seqs.data_ptr(), scores.data_ptr())
    eng.import_walkers(seqs.data_ptr(), scores.data_ptr())
    with pytest.raises(native.AdxError) as e:
        eng.autocorr(10)
    assert e.value.status == native.ESTATE
    eng.record_end()
    with pytest.raises(native.AdxError) as e:
        eng.autocorr(10)
    assert e.value.status == native.ESTATE
