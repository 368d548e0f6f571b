"""The centroid / MEA definitions (addapt_amd/csrc/ensemble_struct_core.hpp)
restated in plain Python floats, for the tests of the kernel and of its host
probe.  P is a list of L lists of L floats (0-based, symmetric, zero diagonal)."""
import math


def tol(L, gamma):
    """Each value is a sum of at most L terms of size at most max(1, 2 gamma), the
    terms' own error is at most L ulps, and only the summation order differs."""
    return 8 * L * L * max(1.0, 2.0 * gamma) * 2.0 ** -53


def pairs_of(db):
    """The pairs (i, j), i < j, of a dot-bracket string; None if it is not well-formed."""
    st, out = [], []
    for k, c in enumerate(db):
        if c == "(":
            st.append(k)
        elif c == ")":
            if not st:
                return None
            out.append((st.pop(), k))
        elif c != ".":
            return None
    return None if st else sorted(out)


def unpaired_probabilities(P):
    out = []
    for row in P:
        s = 0.0
        for x in row:   # ascending j
            s += x
        out.append(1.0 - s)
    return out


def centroid(P):
    """(pairs, dot-bracket): P > 1/2 in ascending (i, j) through the conflict filter."""
    L = len(P)
    taken = []
    for i in range(L):
        for j in range(i + 1, L):
            if P[i][j] > 0.5 and not any(i in (a, b) or j in (a, b) or (a < i < b < j) or (i < a < j < b)
                                         for a, b in taken):
                taken.append((i, j))
    db = ["."] * L
    for i, j in taken:
        db[i], db[j] = "(", ")"
    return taken, "".join(db)


def centroid_dist(P, pairs):
    L, inc = len(P), set(pairs)
    return math.fsum((1.0 - P[i][j]) if (i, j) in inc else P[i][j] for i in range(L) for j in range(i + 1, L))


def diversity(P):
    L = len(P)
    return 2.0 * math.fsum(P[i][j] * (1.0 - P[i][j]) for i in range(L) for j in range(i + 1, L))


def expected_accuracy(pairs, P, gamma):
    L = len(P)
    pu = unpaired_probabilities(P)
    free = set(range(L))
    for i, j in pairs:
        free -= {i, j}
    return math.fsum([pu[i] for i in sorted(free)] + [2.0 * gamma * P[i][j] for i, j in pairs])


class Mea:
    """The recursion's table: M(i, j) = self.at(i, j), an empty span is 0.  The
    candidates are added in the header's order ((left + w) + inner), so on the
    same doubles the table equals a host build's bit for bit."""

    def __init__(self, P, gamma):
        self.P, self.L, self.g2 = P, len(P), 2.0 * gamma
        self.pu = unpaired_probabilities(P)
        self.ks = [[k for k in range(j) if P[k][j] > 0.0] for j in range(self.L)]
        self.M = [[0.0] * (self.L + 1) for _ in range(self.L + 1)]   # M[i][j + 1] = M(i, j)
        for d in range(self.L):
            for i in range(self.L - d):
                best = None
                for _, v in self.candidates(i, i + d):
                    if best is None or v > best:
                        best = v
                self.M[i][i + d + 1] = best

    def at(self, i, j):
        return self.M[i][j + 1] if j >= i else 0.0

    def candidates(self, i, j):
        """(index, value) in ascending index: 0 is "j unpaired", 1 + (k - i) is pair (k, j)."""
        M = self.M
        yield 0, M[i][j] + self.pu[j] + 0.0
        for k in self.ks[j]:
            if k >= i:
                yield 1 + k - i, M[i][k] + self.g2 * self.P[k][j] + M[k + 1][j]

    @property
    def mea(self):
        return self.at(0, self.L - 1)
