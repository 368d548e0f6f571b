"""Distinct designs by greedy Hamming selection on the GPU
(addapt_amd/csrc/design_select.hip) against the numpy restatement of the rule in
design_select_check.py, bit for bit: the stateless adx_select_designs on clouds
of sequences around a few centres, and adx_record_designs on the picks of
recorded runs in both fold modes, where the entries are what Engine.picks
returns for the same window."""
import numpy as np
import pytest

from addapt_amd import workloads
from design_select_check import chars, cloud, codes_of, distances, multiply_covered, pair_hist, select, walkers_of

pytestmark = pytest.mark.gpu

LENGTHS = (5, 64, 65, 129, 255)


def _invariants(got, dist, scores, radius, what):
    M = len(scores)
    F = int(np.isfinite(scores).sum())
    lead, member = got["leaders"], got["member_of"]
    assert got["sizes"].sum() + (member == -1).sum() == M, what
    if got["pair_hist"] is not None:
        assert got["pair_hist"].sum() == F * (F - 1) // 2, what
    apart = dist[np.ix_(lead, lead)] + (radius + 1) * np.eye(len(lead), dtype=np.int64)
    assert (apart > radius).all(), what                      # leaders pairwise more than r apart
    inside = member >= 0
    assert (dist[np.flatnonzero(inside), lead[member[inside]]] <= radius).all(), what   # members within r of theirs


def _compare(native, ch, codes, scores, radius, K, dist, what, **kw):
    got = native.select_designs(ch, scores, radius, K, **kw)
    ref = select(codes, scores, radius, K, dist)
    assert len(got["leaders"]) == len(ref["leaders"]), what
    for k in ("leaders", "sizes", "member_of"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k)
    if got["pair_hist"] is not None:
        assert got["pair_hist"].dtype == np.int64
        assert np.array_equal(got["pair_hist"], pair_hist(codes, scores, dist)), what
    _invariants(got, dist, scores, radius, what)
    return got, ref


@pytest.mark.parametrize("M", (1, 2, 64, 65, 1000))
def test_select_designs(native, M):
    several = leftover = 0
    for N in LENGTHS:
        codes, scores = cloud(M, N, 31 * M + N)
        ch, dist = chars(codes), distances(codes)
        dups = int(pair_hist(codes, scores, dist)[0])
        if M >= 64:
            assert dups >= 4, (M, N)   # exact duplicates: r = 0 has something to remove
        for radius in (0, 1, 3, 6, N):
            for K in (1, 7, M):
                _, ref = _compare(native, ch, codes, scores, radius, K, dist, (M, N, radius, K))
                n = len(ref["leaders"])
                assert 1 <= n <= min(K, M)
                assert radius < N or n == 1
                if K == M and radius == 0 and M >= 64:
                    assert 1 < n < M
                several += radius >= 3 and multiply_covered(dist, ref, radius) > 0
                leftover += K == 7 and bool((ref["member_of"] < 0).any())
    if M >= 64:   # the lowest-numbered-leader clause and the cap were exercised
        assert several > 0 and leftover > 0


@pytest.mark.parametrize("N", (65, 255))
def test_select_designs_4099(native, N):
    M = 4099   # five tiles of ranked entries, seventeen of the pair histogram
    codes, scores = cloud(M, N, 77 + N)
    ch, dist = chars(codes), distances(codes)
    assert pair_hist(codes, scores, dist)[0] > 100
    for radius in (0, 6):
        for K in (7, M):
            _, ref = _compare(native, ch, codes, scores, radius, K, dist, (M, N, radius, K))
            assert 1 <= len(ref["leaders"]) <= K
            if K == 7:
                assert (ref["member_of"] < 0).any()
            elif radius == 0:
                assert len(ref["leaders"]) > 1024   # leaders made in more than one tile
            else:
                assert multiply_covered(dist, ref, radius) > 0


def test_edge_inputs(native):
    rng = np.random.default_rng(5)
    N = 65
    one = rng.integers(0, 4, N)
    # all entries identical
    codes = np.tile(one, (70, 1))
    scores = rng.normal(size=70)
    got, _ = _compare(native, chars(codes), codes, scores, 0, 70, distances(codes), "identical")
    assert got["leaders"].tolist() == [int(np.argmax(scores))] and got["sizes"].tolist() == [70]
    assert got["pair_hist"][0] == 70 * 69 // 2
    # all scores equal: the order is the index order
    codes, _ = cloud(300, N, 9)
    dist = distances(codes)
    got, _ = _compare(native, chars(codes), codes, np.full(300, -3.25), 2, 300, dist, "equal scores")
    assert got["leaders"][0] == 0 and np.all(np.diff(got["leaders"]) > 0)
    # a NaN, a -inf and a +inf score: -1, left out of the histogram, never a leader
    codes, scores = cloud(200, N, 10)
    scores[18] = scores.max() + 1.0
    scores[[0, 17, 199]] = [np.nan, -np.inf, np.inf]
    codes[17] = codes[18]
    for radius in (0, 3, N):
        got, _ = _compare(native, chars(codes), codes, scores, radius, 200, distances(codes), "non-finite")
        assert got["member_of"][[0, 17, 199]].tolist() == [-1, -1, -1] and got["leaders"][0] == 18
        assert not set(got["leaders"].tolist()) & {0, 17, 199}
    # 0.0 against -0.0: equal, so the lower index first
    codes = np.stack([one, (one + 1) % 4, (one + 2) % 4])
    for scores in ([-0.0, 0.0, -1.0], [0.0, -0.0, -1.0]):
        got, _ = _compare(native, chars(codes), codes, np.array(scores), 0, 3, distances(codes), "zeros")
        assert got["leaders"].tolist() == [0, 1, 2]
    # a chain: d(a, b) <= r, d(b, c) <= r, d(a, c) > r, in each score order
    a = one.copy()
    b, c = a.copy(), a.copy()
    b[:2] = (b[:2] + 1) % 4
    c[:4] = (c[:4] + 1) % 4
    codes = np.stack([a, b, c])
    dist = distances(codes)
    assert dist[0, 1] == 2 and dist[1, 2] == 2 and dist[0, 2] == 4
    for perm in ([3, 2, 1], [3, 1, 2], [2, 3, 1], [1, 3, 2], [2, 1, 3], [1, 2, 3]):
        got, _ = _compare(native, chars(codes), codes, np.array(perm, float), 2, 3, dist, ("chain", perm))
        if perm[1] == 3:   # b first: it covers both
            assert got["leaders"].tolist() == [1] and got["member_of"].tolist() == [0, 0, 0]
        else:              # a or c first takes b; the other end leads its own
            assert len(got["leaders"]) == 2 and got["member_of"][1] == 0
    # lower-case input and strings give what upper-case arrays give; no histogram on request
    codes, scores = cloud(130, 129, 11)
    dist = distances(codes)
    up, _ = _compare(native, chars(codes), codes, scores, 3, 130, dist, "upper")
    low, _ = _compare(native, chars(codes, lower=True), codes, scores, 3, 130, dist, "lower")
    mixed = [row.tobytes().decode() for row in chars(codes)]
    mixed[::2] = [s.lower() for s in mixed[::2]]
    assert np.array_equal(codes_of(mixed), codes)
    mix, _ = _compare(native, mixed, codes, scores, 3, 130, dist, "strings")
    bare, _ = _compare(native, chars(codes), codes, scores, 3, 130, dist, "no histogram", with_hist=False)
    assert bare["pair_hist"] is None
    for other in (low, mix, bare):
        assert all(np.array_equal(up[k], other[k]) for k in ("leaders", "sizes", "member_of"))


def test_select_designs_errors(native):
    ok = ["ACGUA", "acgua"]
    assert len(native.select_designs(ok, [1.0, 2.0], 0, 1)["leaders"]) == 1
    bad = [([], [], 0, 1),                      # n_seqs < 1
           ([""], [1.0], 0, 1),                 # length 0
           (["A" * 256], [1.0], 0, 1),          # length 256
           (ok, [1.0, 2.0], -1, 1),             # radius < 0
           (ok, [1.0, 2.0], 0, 0),              # max_designs < 1
           (["ACGUA", "ACGNA"], [1.0, 2.0], 0, 2),
           (["ACGUA", "ACGTA"], [1.0, 2.0], 0, 2),
           (["A" * 200 + "x"], [1.0], 0, 1)]    # a bad character in the last word
    for seqs, scores, radius, K in bad:
        with pytest.raises(native.AdxError) as e:
            native.select_designs(seqs, scores, radius, K)
        assert e.value.status == native.EINVAL, (seqs, radius, K)


W = 37
SEEDS = list(range(500, 500 + W))
CHUNKS = (150, 250)


def _engine(native, fold):
    tmpl, active = workloads.synthetic(64)
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=50)
    eng = native.Engine(tmpl, [active], workloads.default_objective(), aptamer=apt, thermostat=th, fold_mode=fold)
    eng.walkers_init(SEEDS, workloads.walker_sequences(tmpl, [active], W))
    return eng


@pytest.fixture(scope="module", params=["mfe", "pf"])
def recorded(request, native):
    eng = _engine(native, request.param)
    eng.record(sum(CHUNKS))
    for n in CHUNKS:
        eng.run_steps(n)
    return eng


def _entries(eng, window):
    """The picks as entries, walker-major and then by step: (walker, step, score, sequence)."""
    picks, _ = eng.picks(window)
    return [(w, step, score, seq) for w, per in enumerate(picks) if per is not None for step, score, seq in per]


def test_record_designs(native, recorded):
    eng = recorded
    for window in (7, 25):
        ent = _entries(eng, window)
        assert len(ent) > W   # more than one pick a walker somewhere
        codes = codes_of([e[3] for e in ent])
        scores = np.array([e[2] for e in ent])
        walker = np.array([e[0] for e in ent])
        dist = distances(codes)
        hist = pair_hist(codes, scores, dist)
        shared = 0
        for radius in (0, 2, 64):
            for K in (3, 1000):
                ref = select(codes, scores, radius, K, dist)
                got, ghist, n_picks = eng.designs(window, radius, K)
                what = (window, radius, K)
                assert n_picks == len(ent) and np.array_equal(ghist, hist), what
                assert len(got) == len(ref["leaders"]) <= K, what
                nw = walkers_of(ref["member_of"], walker, len(got))
                for d, (lead, size) in enumerate(zip(ref["leaders"], ref["sizes"])):
                    assert got[d] == ent[lead] + (int(size), int(nw[d])), (what, d)
                shared += int((nw > 1).sum())
                flat = native.select_designs([e[3] for e in ent], scores, radius, K)
                assert np.array_equal(flat["leaders"], ref["leaders"]) and np.array_equal(flat["sizes"], ref["sizes"])
                assert np.array_equal(flat["pair_hist"], ghist)
                if radius == 64:
                    assert len(got) == 1 and got[0][4] == len(ent)
        assert shared > 0   # a design found by more than one walker
    sel, hst = eng.last_design_ms()
    assert sel > 0.0 and hst > 0.0


def test_record_designs_leave_the_record_alone(native, recorded):
    eng = recorded
    first = eng.designs(25, 2, 50)
    picks = eng.picks(25)
    ac = eng.autocorr(40, 10)
    again = eng.designs(25, 2, 50)
    assert again[0] == first[0] and np.array_equal(again[1], first[1]) and again[2] == first[2]
    other = eng.designs(7, 0, 5)
    assert other[2] > first[2] and len(other[0]) == 5
    after = eng.picks(25)
    assert after[0] == picks[0] and np.array_equal(after[1], picks[1])
    assert np.array_equal(eng.autocorr(40, 10)["pos_matches"], ac["pos_matches"])
    third = eng.designs(25, 2, 50)
    assert third[0] == first[0] and np.array_equal(third[1], first[1])


def test_record_designs_leave_the_walkers_alone(native):
    a, b = _engine(native, "mfe"), _engine(native, "mfe")
    a.record(60)
    a.run_steps(50)
    b.run_steps(50)
    designs, _, n = a.designs(10, 1, 20)
    assert n > 0 and designs
    a.run_steps(10)
    b.run_steps(10)
    x, y = a.download(), b.download()
    assert x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
    assert a.designs(10, 1, 20)[2] >= n   # the record went on


def test_record_designs_errors(native):
    eng = _engine(native, "mfe")
    with pytest.raises(native.AdxError) as e:
        eng.designs(10, 1)                  # before record()
    assert e.value.status == native.ESTATE
    eng.record(30)
    with pytest.raises(native.AdxError) as e:
        eng.designs(10, 1)                  # nothing recorded yet
    assert e.value.status == native.ESTATE
    eng.run_steps(20)
    for window, radius, K in ((0, 1, 10), (10, -1, 10), (10, 1, 0)):
        with pytest.raises(native.AdxError) as e:
            eng.designs(window, radius, K)
        assert e.value.status == native.EINVAL, (window, radius, K)
    assert eng.designs(10, 1)[2] > 0
    eng.walkers_init(SEEDS)                 # sequences change outside the log: the record is broken
    with pytest.raises(native.AdxError) as e:
        eng.designs(10, 1)
    assert e.value.status == native.ESTATE
    eng.record_end()
    with pytest.raises(native.AdxError) as e:
        eng.designs(10, 1)
    assert e.value.status == native.ESTATE
