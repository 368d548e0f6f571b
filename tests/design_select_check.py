"""The design selection rule restated with numpy, for the tests of
addapt_amd/csrc/design_select_core.hpp and design_select.hip.  Entries are rows
of base codes 0..3 (A, C, G, U) with a score each; the distance is the Hamming
distance; the order is score descending, ties by the lower index, entries with
a non-finite score taking no part.  While fewer than max_designs designs exist
and an uncovered entry is left, the first uncovered entry in order leads the
next design, which covers every uncovered entry within the radius of it."""
import numpy as np

BASES = np.frombuffer(b"ACGU", np.uint8)


def chars(codes, lower=False):
    """(M, N) uint8 characters of (M, N) codes."""
    ch = BASES[np.asarray(codes)]
    return ch | 0x20 if lower else ch


def codes_of(seqs):
    """(M, N) codes of equally long strings over ACGU / acgu."""
    return np.array([["ACGU".index(c) for c in s.upper()] for s in seqs], np.int64).reshape(len(seqs), -1)


def distances(codes):
    """(M, M) Hamming distances: N minus the matches, the matches as a product of
    one-hot rows (exact: counts of at most N <= 255 in float32)."""
    codes = np.asarray(codes)
    M, N = codes.shape
    hot = (codes[:, :, None] == np.arange(4)).reshape(M, 4 * N).astype(np.float32)
    return N - np.rint(hot @ hot.T).astype(np.int64)


def order(scores):
    """The finite entries, best score first, the lower index among equals."""
    s = np.asarray(scores, np.float64)
    fin = np.flatnonzero(np.isfinite(s))
    return fin[np.argsort(-s[fin], kind="stable")]   # -(-0.0) == -(+0.0): ties stay in index order


def select(codes, scores, radius, max_designs, dist=None):
    """dict(leaders, sizes, member_of) of the greedy selection."""
    M = len(scores)
    dist = distances(codes) if dist is None else dist
    member = np.full(M, -1, np.int64)
    leaders, sizes = [], []
    for e in order(scores):
        if len(leaders) >= max_designs:
            break
        if member[e] >= 0:
            continue
        cover = (dist[e] <= radius) & (member < 0) & np.isfinite(scores)
        member[cover] = len(leaders)
        leaders.append(int(e))
        sizes.append(int(cover.sum()))
    return dict(leaders=np.array(leaders, np.int64), sizes=np.array(sizes, np.int64), member_of=member)


def pair_hist(codes, scores, dist=None):
    """[d] = the unordered pairs of finite-score entries at distance d, d = 0..N."""
    N = np.asarray(codes).shape[1]
    dist = distances(codes) if dist is None else dist
    fin = np.flatnonzero(np.isfinite(np.asarray(scores, np.float64)))
    sub = dist[np.ix_(fin, fin)]
    return np.bincount(sub[np.triu_indices(len(fin), 1)], minlength=N + 1).astype(np.int64)


def walkers_of(member_of, walker, n_designs):
    """Per design the number of distinct walkers among its members (walker[e]: entry e's)."""
    member_of, walker = np.asarray(member_of), np.asarray(walker)
    return np.array([len(set(walker[member_of == d].tolist())) for d in range(n_designs)], np.int64)


def cloud(M, N, seed, centres=5, kmax=6):
    """(codes, scores): each entry is one of `centres` random sequences with k in
    0..min(kmax, N) random positions redrawn; scores in quarters, so ties are frequent."""
    rng = np.random.default_rng(seed)
    cen = rng.integers(0, 4, (centres, N))
    codes = cen[rng.integers(0, centres, M)].copy()
    for e in range(M):
        k = int(rng.integers(0, min(kmax, N) + 1))
        pos = rng.choice(N, k, replace=False)
        codes[e, pos] = rng.integers(0, 4, k)
    scores = np.round(rng.normal(size=M) * 4) / 4
    return codes, scores


def multiply_covered(dist, sel, radius):
    """Entries within the radius of more than one leader."""
    near = dist[:, sel["leaders"]] <= radius
    return int(((near.sum(axis=1) > 1) & (sel["member_of"] >= 0)).sum())
