"""The trajectory picking rule restated with numpy, for the tests of
addapt_amd/csrc/traj_pick_core.hpp and traj_pick.hip: the 75th percentile as
the threshold, then the largest unblocked score (lowest step among equals) while
it is >= the threshold, each peak blocking `window` steps on either side."""
import numpy as np


def threshold(c):
    return np.percentile(np.asarray(c, np.float64), 75)


def pick(c, window):
    """Ascending steps of the peaks of one trajectory; None for a non-finite score."""
    c = np.asarray(c, np.float64)
    if not np.all(np.isfinite(c)):
        return None
    S, T = len(c), threshold(c)
    free = np.ones(S, bool)
    out = []
    while free.any():
        idx = np.flatnonzero(free)
        i = int(idx[np.argmax(c[idx])])   # argmax: the first of equal maxima
        if not c[i] >= T:
            break
        out.append(i)
        free[max(i - window, 0):min(i + window, S)] = False
    return sorted(out)


def pick_overwrite(c, window):
    """The form that overwrites blocked steps with the minimum and tests max >= T;
    it ends only when min < T (None otherwise)."""
    c = np.array(c, np.float64)
    S, T, lowest = len(c), threshold(c), c.min()
    if not lowest < T:
        return None
    out = []
    while c.max() >= T:
        i = int(np.argmax(c))
        out.append(i)
        c[max(i - window, 0):min(i + window, S)] = lowest
    return sorted(out)


def families(S, seed):
    """name -> trajectory of S scores: a random walk, the same rounded (ties), a
    running-maximum staircase, a constant, and signed zeros mixed."""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.normal(size=S))
    zeros = np.where(rng.random(S) < 0.5, 0.0, -0.0)
    zeros[rng.random(S) < 0.2] = -1.5
    return {"walk": walk, "rounded": np.round(walk), "staircase": np.maximum.accumulate(np.round(walk * 2) / 2),
            "constant": np.full(S, -3.25), "zeros": zeros}
