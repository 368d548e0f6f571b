"""The sequence autocorrelation restated with numpy, for the tests of
addapt_amd/csrc/traj_autocorr_core.hpp and traj_autocorr.hip: the match counts
m(p, k) by direct comparison of shifted arrays, the correlation-time rule, and
seeded families of base-code trajectories."""
import numpy as np


def matches(x, max_lag):
    """x: (S, ...) codes.  (max_lag + 1, ...) int64: m[k] = #{i < S - k: x[i + k] == x[i]}."""
    x = np.asarray(x)
    S = x.shape[0]
    assert 0 <= max_lag <= S - 1
    return np.stack([(x[k:] == x[:S - k]).sum(axis=0, dtype=np.int64) for k in range(max_lag + 1)])


def tau(m, n_series, kept, baseline):
    """The least k >= 1 with m[k] / (n_series (kept - k)) - baseline <= (1 - baseline) / e;
    -1 if there is none among the lags given, 0 if baseline >= 1."""
    if baseline >= 1.0:
        return 0
    level = (1.0 - baseline) / np.e
    for k in range(1, len(m)):
        if int(m[k]) / (float(n_series) * float(kept - k)) - baseline <= level:
            return k
    return -1


def tau_margin(m, n_series, kept, baseline):
    """The least |a_k - baseline - level| over the lags: how far the rule is from a tie."""
    level = (1.0 - baseline) / np.e
    return min([abs(int(m[k]) / (float(n_series) * float(kept - k)) - baseline - level) for k in range(1, len(m))],
               default=1.0)


def baseline(base_counts, changeable, n_series_steps):
    """The mean over the changeable positions of sum_c f_pc^2, f = counts / (W S')."""
    f = np.asarray(base_counts)[np.asarray(changeable, bool)] / float(n_series_steps)
    return float((f * f).sum(axis=1).mean())


def families(P, S, seed):
    """name -> (S, P) uint8 codes 1..4."""
    rng = np.random.default_rng(seed)
    step = np.arange(S)[:, None]
    start = rng.integers(0, 4, size=(1, P))
    other = (start + rng.integers(1, 4, size=(1, P))) % 4

    def runs(n):   # a new random base every n steps
        draws = rng.integers(0, 4, size=(S // n + 1, P))
        return draws[np.arange(S) // n]

    rare = np.cumsum(np.concatenate([start, (rng.random((S - 1, P)) < 0.02) * rng.integers(1, 4, size=(S - 1, P))]),
                     axis=0) % 4
    last = np.repeat(start, S, axis=0)
    last[S - 1] = other[0]
    out = {
        "constant": np.repeat(start, S, axis=0),
        "alternating": np.where(step % 2 == 0, start, other),
        "runs64": runs(64),
        "runs65": runs(65),
        "iid": rng.integers(0, 4, size=(S, P)),
        "rare": rare,
        "last_step": last,
        "cycle": (start + step) % 4,   # A -> C -> G -> U: neighbours differ in one plane or in both
    }
    return {k: (v + 1).astype(np.uint8) for k, v in out.items()}
