"""Picking each trajectory's best steps on the GPU (addapt_amd/csrc/traj_pick.hip)
against the numpy restatement of the rule in traj_pick_check.py: the stateless
adx_pick_scores on synthetic trajectories, and the pick record of a context
(adx_record_*) on real runs in both fold modes, where the expected steps and
scores come from the host trace of the same run and the expected sequences from
a twin context advanced one step at a time."""
import numpy as np
import pytest
import torch

from addapt_amd import workloads
from traj_pick_check import families, pick, threshold

pytestmark = pytest.mark.gpu

N_TRAJ = 70
SIZES = (1, 64, 65, 1000, 4099)
WINDOWS = (1, 7, 500, 5000)


def _trajectories(S):
    """(S, N_TRAJ): the score families over and over with fresh seeds, then the edge columns."""
    cols, k = [], 0
    while len(cols) < N_TRAJ - 5:
        for name, c in sorted(families(S, 7000 + 13 * S + k).items()):
            cols.append(c)
        k += 1
    cols = cols[:N_TRAJ - 5]
    ends = np.full(S, -1.0)          # peaks at step 0 and at step S - 1
    ends[0] = ends[-1] = 2.0
    first = np.arange(S, 0, -1.0)    # a peak at step 0 alone (strictly falling)
    last = np.arange(S) * 1.0        # and at step S - 1 alone
    nan = cols[0].copy()
    nan[S // 2] = np.nan
    ninf = cols[1].copy()
    ninf[S - 1] = -np.inf
    cols += [ends, first, last, nan, ninf]
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("S", SIZES)
def test_pick_scores(native, S):
    sc = _trajectories(S)
    assert sc.shape == (S, N_TRAJ)
    for window in WINDOWS:
        got = native.pick_scores(sc, window)
        assert len(got) == N_TRAJ
        for w in range(N_TRAJ):
            assert got[w] == pick(sc[:, w], window), (S, window, w)
        assert got[N_TRAJ - 2] is None and got[N_TRAJ - 1] is None   # NaN, -inf
        assert got[N_TRAJ - 4][0] == 0 and got[N_TRAJ - 3][-1] == S - 1
        assert got[N_TRAJ - 5][0] == 0
        if window <= S - 1:   # else step 0, taken first among equals, blocks step S - 1
            assert got[N_TRAJ - 5][-1] == S - 1
        if window > S:
            assert all(g is None or len(g) == 1 for g in got)
    # a larger cap than needed changes nothing
    assert native.pick_scores(sc, 7, cap=-(-S // 7) + 3) == native.pick_scores(sc, 7)


def test_pick_scores_errors(native):
    sc = _trajectories(65)
    with pytest.raises(native.AdxError) as e:
        native.pick_scores(sc, 7, cap=9)   # ceil(65 / 7) = 10
    assert e.value.status == native.EINVAL and "10" in str(e.value)
    with pytest.raises(native.AdxError) as e:
        native.pick_scores(sc, 0, cap=100)
    assert e.value.status == native.EINVAL


W = 37
SEEDS = list(range(500, 500 + W))
CHUNKS = (150, 250)


def _engine(native, fold):
    tmpl, active = workloads.synthetic(64)
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=50)
    eng = native.Engine(tmpl, [active], workloads.default_objective(), aptamer=apt, thermostat=th, fold_mode=fold)
    eng.walkers_init(SEEDS, workloads.walker_sequences(tmpl, [active], W))
    return eng, tmpl, active


@pytest.fixture(scope="module", params=["mfe", "pf"])
def recorded(request, native):
    """A recorded run with its host trace, the same run without a record, and the
    sequences after every step from a twin advanced one step at a time."""
    fold = request.param
    eng, tmpl, active = _engine(native, fold)
    start = eng.download()[0]
    eng.record(sum(CHUNKS))
    traces = [eng.run_steps(n, trace=True) for n in CHUNKS]
    plain, _, _ = _engine(native, fold)
    for n in CHUNKS:
        plain.run_steps(n)
    twin, _, _ = _engine(native, fold)
    seqs = []
    for _ in range(sum(CHUNKS)):
        twin.run_steps(1)
        seqs.append(twin.download()[0])
    return dict(eng=eng, plain=plain, tmpl=tmpl, active=active, start=start, seqs=seqs,
                cur=np.concatenate([t["current_score"] for t in traces]),
                pos=np.concatenate([t["position"] for t in traces]),
                outcome=np.concatenate([t["outcome"] for t in traces]))


def _check_picks(r, window):
    eng, cur, seqs = r["eng"], r["cur"], r["seqs"]
    S, N = cur.shape[0], len(r["tmpl"])
    got, counts = eng.picks(window)
    assert len(got) == W
    hist = np.zeros((N, 4), np.int64)
    total = 0
    for w in range(W):
        ref = pick(cur[:, w], window)
        if ref is None:   # a score of -inf (ln of a zero probability): not picked
            assert got[w] is None, w
            continue
        assert got[w] is not None and [p[0] for p in got[w]] == ref, (w, window)
        for step, score, seq in got[w]:
            assert score == cur[step, w]          # both read the same doubles
            assert seq == seqs[step][w], (w, step)
            for k, ch in enumerate(seq.upper()):
                hist[k, "ACGU".index(ch)] += 1
        total += len(ref)
    assert total > 0 and np.array_equal(counts, hist)
    assert all(g is None or len(g) <= -(-S // window) for g in got)
    return got


def test_record_picks(recorded):
    r = recorded
    cur, pos, outcome, active = r["cur"], r["pos"], r["outcome"], r["active"]
    assert cur.shape == (sum(CHUNKS), W)
    # the test is worth something: an accepted move on a position with a partner
    # (its closure list writes the complement too), sequences that moved, and no
    # trajectory the reference's form would not end on
    paired = [k for k, ch in enumerate(active) if ch in "()"]
    accepted = (outcome == 1) | (outcome == 3)
    assert np.any(accepted & np.isin(pos, paired))
    assert any(r["seqs"][-1][w] != r["start"][w] for w in range(W))
    used = [w for w in range(W) if np.all(np.isfinite(cur[:, w]))]
    print("%d of %d trajectories finite" % (len(used), W))
    assert 2 * len(used) > W   # (an MFE score is -inf where a constrained fold is the free one)
    assert all(cur[:, w].min() < threshold(cur[:, w]) for w in used)
    got = _check_picks(r, 40)
    assert any(len(got[w]) > 1 for w in used)
    again = _check_picks(r, 7)   # picking again, another window
    assert sum(len(again[w]) for w in used) > sum(len(got[w]) for w in used)
    assert _check_picks(r, 40) == got
    # recording changes nothing: the same final state as the run without a record
    a, b = r["eng"].download(), r["plain"].download()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    pm, rm = r["eng"].last_pick_ms()
    assert pm > 0.0 and rm > 0.0


def test_record_steps_are_global(native):
    """Steps count from the context's first step, not from the record's."""
    eng, _, _ = _engine(native, "mfe")
    eng.run_steps(20)
    eng.record(60)
    tr = eng.run_steps(60, trace=True)
    got, _ = eng.picks(10)
    for w in range(W):
        ref = pick(tr["current_score"][:, w], 10)
        assert (got[w] is None) if ref is None else ([p[0] - 20 for p in got[w]] == ref)
    assert any(g for g in got)
    eng.record_end()


def test_record_errors(native):
    eng, _, _ = _engine(native, "mfe")
    with pytest.raises(native.AdxError) as e:
        eng.picks(10)                      # before record()
    assert e.value.status == native.ESTATE
    eng.record(30)
    with pytest.raises(native.AdxError) as e:
        eng.picks(10)                      # nothing recorded yet
    assert e.value.status == native.ESTATE
    eng.run_steps(20)
    before = eng.download()
    with pytest.raises(native.AdxError) as e:
        eng.run_steps(11)                  # 31 > 30: refused before anything is launched
    assert e.value.status == native.ESTATE
    after = eng.download()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    with pytest.raises(native.AdxError) as e:
        eng.picks(10, cap=1)               # ceil(20 / 10) = 2
    assert e.value.status == native.EINVAL and "2" in str(e.value)
    eng.run_steps(10)
    got, _ = eng.picks(10)
    assert len(got) == W and all(g is None or len(g) >= 1 for g in got) and any(g for g in got)
    sc, _ = eng.rescore()                  # rescoring does not disturb the record
    assert eng.picks(10)[0] == got
    # an import changes sequences outside the log: the record is broken
    seqs = torch.empty(W * eng.N, dtype=torch.uint8, device="cuda")
    scores = torch.empty(W, dtype=torch.float64, device="cuda")
    eng.export_walkers(seqs.data_ptr(), scores.data_ptr())
    eng.import_walkers(seqs.data_ptr(), scores.data_ptr())
    with pytest.raises(native.AdxError) as e:
        eng.picks(10)
    assert e.value.status == native.ESTATE
    eng.run_steps(5)                       # runs on, unrecorded
    eng.record(10)                         # a new record starts clean
    eng.run_steps(10)
    assert len(eng.picks(5)[0]) == W
    eng.record_end()
    with pytest.raises(native.AdxError) as e:
        eng.picks(5)
    assert e.value.status == native.ESTATE
    # so does initialising the walkers anew
    eng.record(10)
    eng.run_steps(3)
    eng.walkers_init(SEEDS)
    with pytest.raises(native.AdxError) as e:
        eng.picks(5)
    assert e.value.status == native.ESTATE
    # a record the device cannot hold (2^30 steps x 37 walkers x 17 B = 675 GB): refused clean
    with pytest.raises(native.AdxError) as e:
        eng.record(1 << 30)
    assert e.value.status == native.ENOMEM
    with pytest.raises(native.AdxError) as e:
        eng.picks(5)
    assert e.value.status == native.ESTATE
    eng.record(10)
    eng.run_steps(10)
    assert len(eng.picks(5)[0]) == W
