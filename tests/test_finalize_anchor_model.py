"""A CPU model of the pair kernel's finalize role with anchored lanes
(addapt_amd/csrc/mfe_pair.hip, role F): the step's row window, the anchor
policy and every running value, restated in Python and held against the closed
forms (fold_common.hpp off / rowb / colb and the slot expressions of F).

Lane l of lane-set fls finalizes row ab + 63 fls + l while the anchor ab
holds; a step's window is [fr, lr] and lanes outside it are masked.  Between
re-anchors the kernel advances last step's addresses by deltas instead of
recomputing them.  Three parts, for every N from 5 to 100:

* the sweep of every hull 1 <= m_lo <= m_hi <= N and of the fold from scratch,
  all hulls of one N at once (numpy): the window, the anchor, the lane-sets
  that run, the uniform running values (the spans' cell offsets, the ring
  slots) at every step against their closed forms, the re-anchor counts;
* the per-lane running values by induction: for every anchor ab, every lane of
  both lane-sets and every step d, advancing the closed forms at (ab, d) gives
  the closed forms at (ab, d + 2) -- a superset of the (anchor, step, lane)
  triples the sweeps reach, whose slow path starts from the closed forms;
* the rows that are written, enumerated lane by lane for a sample of N, against
  the parent's mapping (lane = fr + 63 fls + l): each window row exactly once,
  the overlap lane on and silent, every written row's upper neighbour on.
"""
import numpy as np
import pytest

SCRATCH = (-4096, 4096)   # the fold from scratch: a hull that clamps nowhere (mloF, mhiF)


# ---------------------------------------------------------------- closed forms
def off(dd, N):
    return ((dd - 4) * (2 * N - 3 - dd)) >> 1


def rowb(i, N):
    return (i - 1) * (N - 3) - (((i - 1) * i) >> 1)


def colb(j):
    return ((j - 5) * (j - 4)) >> 1


def np4_of(N):
    return ((64 if N <= 64 else 100) + 2) * 4   # NP words of a ring slot, in bytes (NM = 64 | 100)


def steps(N):
    return range(6, N + 4, 2)   # for (d = 6; d - 3 <= N; d += 2)


def uniform_closed(d, N):
    """The uniform values of step d: off() of spans e0, e1, e0-1, e0-2, e0-3 (span 3
    stands in below span 4), split slots e0 % 6 and (e0 + 4) % 6, U slot e0 & 3 (bytes)."""
    e0, e1, P = d - 2, d - 1, np4_of(N)
    return dict(oE0=off(e0, N), oE1=off(e1, N), oS1=off(max(e0 - 1, 3), N), oS2=off(max(e0 - 2, 3), N),
                oS3=off(max(e0 - 3, 3), N), mS=(e0 % 6) * P, mM=((e0 + 4) % 6) * P, cW=(e0 & 3) * P)


def uniform_advance(u, d, N):
    e1, P = d - 1, np4_of(N)
    oE0 = u["oE1"] + (N - e1)
    mS = np.where(u["mS"] == 4 * P, 0, u["mS"] + 2 * P)
    return dict(oS3=u["oS1"], oS2=u["oE0"], oS1=u["oE1"], oE0=oE0, oE1=oE0 + (N - e1 - 1),
                mM=u["mS"], mS=mS, cW=u["cW"] ^ (2 * P))


def lane_closed(i, d, N):
    """Per-lane running values of row i at step d (byte offsets from their tables)."""
    jA = i + d - 2
    return dict(fJ4=4 * jA, fSj=jA - 1, fQ1=4 * (colb(jA - 1) + i - 1))


def lane_addresses(s, u, i, d, N):
    """Every address F forms from the running values (bytes from the table's base;
    S / up / dn in bytes of their own)."""
    e0, P = d - 2, np4_of(N)
    i4 = 4 * i
    q1A = s["fQ1"] + (s["fJ4"] - 20)
    q1B = q1A + (s["fJ4"] - 16)
    pA = 2 * u["cW"] + i4
    uW = u["cW"] + s["fJ4"]
    mA = u["mM"] + 4 + i4
    sA = u["mS"] + i4
    gq = 4 * (rowb(i, N) - 4) + 4 * e0
    return dict(qA=4 * (u["oE0"] - 1) + i4, qB=4 * (u["oE1"] - 1) + i4, kA=u["oE0"] - 1 + i, kB=u["oE1"] - 1 + i,
                q3=4 * u["oS3"] + i4, q2=4 * u["oS2"] + i4, q1=4 * u["oS1"] + i4,
                k3=u["oS3"] + i, k2=u["oS2"] + i, k1=u["oS1"] + i,
                q1P=s["fQ1"], q1A=q1A, q1B=q1B, mA=mA, mB=mA + P, sA=sA, sB=sA + P,
                pA0=pA, pA1=pA + P, pB0=pA + 2 * P, pB1=pA + 3 * P,
                uA=3 * P - u["cW"] + s["fJ4"], uWA=uW, uWB=uW + P + 4, gqA=gq, gqB=gq + 4,
                sjm=s["fSj"], sj=s["fSj"] + 1, sjp=s["fSj"] + 2, ujA=s["fSj"] + 1, ujB=s["fSj"] + 2,
                djm=s["fSj"], dj=s["fSj"] + 1)


def lane_addresses_closed(i, d, N):
    """The same addresses as the parent forms them, from scratch."""
    e0, e1, NP = d - 2, d - 1, np4_of(N) // 4
    jA = i + e0
    s3, s2, s1 = max(e0 - 3, 3), max(e0 - 2, 3), max(e0 - 1, 3)
    ceA, ceB = off(e0, N) + i - 1, off(e1, N) + i - 1
    return dict(qA=4 * ceA, qB=4 * ceB, kA=ceA, kB=ceB,
                q3=4 * (off(s3, N) + i), q2=4 * (off(s2, N) + i), q1=4 * (off(s1, N) + i),
                k3=off(s3, N) + i, k2=off(s2, N) + i, k1=off(s1, N) + i,
                q1P=4 * (colb(jA - 1) + i - 1), q1A=4 * (colb(jA) + i - 1), q1B=4 * (colb(jA + 1) + i - 1),
                mA=4 * (((e0 + 4) % 6) * NP + i + 1), mB=4 * (((e1 + 4) % 6) * NP + i + 1),
                sA=4 * ((e0 % 6) * NP + i), sB=4 * ((e1 % 6) * NP + i),
                pA0=4 * ((e0 & 3) * 2 * NP + i), pA1=4 * ((e0 & 3) * 2 * NP + NP + i),
                pB0=4 * ((e1 & 3) * 2 * NP + i), pB1=4 * ((e1 & 3) * 2 * NP + NP + i),
                uA=4 * (((e0 + 3) & 3) * NP + jA), uWA=4 * ((e0 & 3) * NP + jA), uWB=4 * ((e1 & 3) * NP + jA + 1),
                gqA=4 * (rowb(i, N) + e0 - 4), gqB=4 * (rowb(i, N) + e1 - 4),
                sjm=jA - 1, sj=jA, sjp=jA + 1, ujA=jA, ujB=jA + 1, djm=jA - 1, dj=jA)


# ---------------------------------------------------------------- window and anchor
def window(d, N, mlo, mhi):
    e0, e1 = d - 2, d - 1
    R = N - e0
    return np.maximum(1, mlo - 2 - e1), np.minimum(R, mhi + 3), R


def reanchor(ab, fr, lr):
    """The policy: the lowest anchor whose lane-sets still reach lr."""
    need = (ab == 0) | (fr < ab)
    return need, np.where(need, np.maximum(1, lr - np.where(lr - fr < 64, 63, 126)), ab)


def hulls(N):
    lo, hi = np.meshgrid(np.arange(1, N + 1), np.arange(1, N + 1), indexing="ij")
    k = lo <= hi
    return np.append(lo[k], SCRATCH[0]), np.append(hi[k], SCRATCH[1])


def sweep(N):
    """All hulls of N at once: yields per step (d, fr, lr, R, ab, anchored-this-step, valid)."""
    mlo, mhi = hulls(N)
    ab = np.zeros_like(mlo)
    for d in steps(N):
        fr, lr, R = window(d, N, mlo, mhi)
        if d - 2 <= N - 1:
            need, ab = reanchor(ab, fr, lr)
        else:
            need = np.zeros(mlo.shape, bool)
        yield d, fr, lr, R, ab.copy(), need, d - 2 <= N - 1


@pytest.mark.parametrize("N0", [5, 29, 53, 77])
def test_window_anchor_and_uniform_values(N0):
    for N in range(N0, min(N0 + 24, 101)):
        mlo, mhi = hulls(N)
        one = mlo == mhi
        scratch = mlo == SCRATCH[0]
        fd = np.zeros_like(mlo)                 # wave 7: the step its running values stand for
        u = {k: np.zeros_like(mlo) for k in uniform_closed(6, N)}
        count = np.zeros_like(mlo)              # re-anchors after the first choice
        first = True
        for d, fr, lr, R, ab, need, valid in sweep(N):
            if not valid:
                continue
            assert (fr <= lr).all() and (fr >= 1).all() and (lr <= R).all()
            # every window row has a lane; two lane-sets (overlapping by a row) reach lr
            assert (ab >= 1).all() and (ab <= fr).all() and (lr - ab <= 126).all(), N
            count += need & (not first)
            first = False
            # lane-set 0 (wave 7) runs every step: slow path exactly when it was re-anchored
            fd = np.where(need, 0, fd)
            slow = fd != d
            assert (slow == need).all(), (N, d)
            c = uniform_closed(d, N)
            for k in u:
                u[k] = np.where(slow, c[k], u[k])
                assert (u[k] == c[k]).all(), (N, d, k)
            u = uniform_advance(u, d, N)
            fd = np.full_like(fd, d + 2)
            # the parent ran a second lane-set when the window had more than 64 rows; the
            # anchored one when lr lies past row ab + 63.  A one-lane-set window never needs two
            # under its own anchor, and two lane-sets only run under the wide anchor
            two = lr - ab > 63
            assert (~two | (ab == np.maximum(1, lr - 126)) | (ab == 1)).all()
            assert not two[one].any(), N
        # a fold from scratch never re-anchors; a one-position refold at most once, and
        # only with its changed row at 62 or beyond
        assert count[scratch].sum() == 0
        assert (count[one] <= 1).all(), N
        assert (count[one & (mlo <= 61)] == 0).all(), N


@pytest.mark.parametrize("N0", [5, 29, 53, 77])
def test_lane_running_values_by_induction(N0):
    for N in range(N0, min(N0 + 24, 101)):
        ab = np.arange(1, N + 1)[:, None]
        for fls in (0, 1):
            i = ab + 63 * fls + np.arange(64)[None, :]          # every lane of the lane-set
            for d in steps(N):
                if d - 2 > N - 1:
                    continue
                s = lane_closed(i, d, N)
                u = uniform_closed(d, N)
                got, want = lane_addresses(s, u, i, d, N), lane_addresses_closed(i, d, N)
                assert got.keys() == want.keys()
                for k in want:
                    assert (np.asarray(got[k]) == np.asarray(want[k])).all(), (N, fls, d, k)
                # the advance (lane-set 0 keeps state; lane-set 1 recomputes each step it runs)
                nxt = dict(fQ1=got["q1B"], fJ4=s["fJ4"] + 8, fSj=s["fSj"] + 2)
                c = lane_closed(i, d + 2, N)
                for k in c:
                    assert (nxt[k] == c[k]).all(), (N, fls, d, k)
                un, uc = uniform_advance(u, d, N), uniform_closed(d + 2, N)
                for k in uc:
                    assert int(un[k]) == uc[k], (N, d, k)


def _parent_rows(fr, lr):
    """(rows run, rows written) per lane-set as the parent maps them: lane = fr + 63 fls + l."""
    nr = lr - fr + 1
    Lf = 1 if nr <= 64 else (nr - 1 + 62) // 63
    run, wr = [], []
    for fls in range(Lf):
        rows = [fr + 63 * fls + l for l in range(64)]
        run.append([r for r in rows if r <= lr])
        wr.append([r for l, r in enumerate(rows) if r <= lr and (l < 63 or fls == Lf - 1)])
    return run, wr


@pytest.mark.parametrize("N", [5, 12, 59, 64, 70, 100])
def test_active_rows_equal_the_parents(N):
    mlo, mhi = hulls(N)
    for d, fr, lr, R, ab, need, valid in sweep(N):
        if not valid:
            continue
        # hulls with equal (fr, lr, ab) behave alike this step
        for f, l, a in set(zip(fr.tolist(), lr.tolist(), ab.tolist())):
            Lf = 2 if l - a > 63 else 1
            written, on = [], set()
            for fls in range(Lf):
                for lane in range(64):
                    i = a + 63 * fls + lane
                    if not (f <= i <= l):
                        continue                                   # masked
                    on.add((fls, lane))
                    if lane < 63 or fls == 1 or l - a <= 63:
                        written.append(i)
                        # U of row i + 1 comes from the next lane of the same lane-set
                        if i < l:
                            assert lane < 63 and f <= i + 1 <= l, (N, d, f, l, a, i)
            p_run, p_wr = _parent_rows(f, l)
            assert sorted(written) == list(range(f, l + 1)) == sorted(r for w in p_wr for r in w), (N, d, f, l, a)
            if Lf == 2:
                assert (0, 63) in on                               # the overlap lane is on, and silent
