"""A CPU model of the packed mode of the pair kernel's finalize role
(addapt_amd/csrc/mfe_pair.hip, finalize_packed on the finalize wave): the mode
rule, the anchor, the lane -> (row, cell) map and every running value, restated
in Python on top of tests/test_finalize_anchor_model.py (its closed forms and
its two-cells-per-lane mapping are imported, not repeated).

A step whose row window [fr, lr] fits a half-wave (lr - fr <= 31) runs packed:
lane l is row ab + (l & 31), lanes 0..31 finalize the row's span-e0 cell,
lanes 32..63 its span-e1 cell.  The mode is chosen with the anchor; a change of
mode is a re-anchor.  For every N from 5 to 100, every hull
1 <= m_lo <= m_hi <= N and the fold from scratch:

* each (row, span) cell of every step's window is finalized exactly once by a
  lane that is on, and the rows written are the parent mapping's;
* the addresses of the packed read batch equal their closed forms, by
  induction over the deltas (every anchor, lane and step: a superset of what
  the sweeps reach, whose slow path starts from the closed forms);
* the upper half's U source lane is on whenever its value is used;
* the mode changes per sweep stay within the model's own maximum (asserted).
"""
import numpy as np
import pytest

from addapt_amd import workloads
from test_finalize_anchor_model import (SCRATCH, _parent_rows, colb, hulls, lane_addresses_closed, np4_of, rowb,
                                        steps, uniform_advance, uniform_closed, window)

HALF = 32            # rows of a packed step: one half-wave
MODE_CHANGES = 2     # per sweep after the first choice: packed -> two cells per lane -> packed


# ---------------------------------------------------------------- the rule
def choose(ab, pk, fr, lr):
    """(re-anchored, anchor, mode) from the window and the previous anchor and mode: the
    mode follows the window's fit, the anchor is the lowest whose lanes still reach lr."""
    fit = lr - fr <= HALF - 1
    need = (ab == 0) | (fr < ab) | (fit != pk)
    reach = np.where(fit, HALF - 1, np.where(lr - fr < 64, 63, 126))
    return need, np.where(need, np.maximum(1, lr - reach), ab), np.where(need, fit, pk)


def sweep(N):
    """All hulls of N at once: per valid step (d, fr, lr, R, ab, pk, re-anchored)."""
    mlo, mhi = hulls(N)
    ab, pk = np.zeros_like(mlo), np.zeros(mlo.shape, bool)
    for d in steps(N):
        if d - 2 > N - 1:
            continue
        fr, lr, R = window(d, N, mlo, mhi)
        need, ab, pk = choose(ab, pk, fr, lr)
        yield d, fr, lr, np.full_like(mlo, R), ab.copy(), pk.copy(), need


# ---------------------------------------------------------------- per-lane values
def lane_row_half(ab, lane):
    return ab + (lane & (HALF - 1)), lane >> 5


def lane_closed(i, h, d, N):
    """The running values of a packed lane at step d: those of the two-cells-per-lane mode
    at the lane's own column j = i + e0 + h (bytes from their tables)."""
    j = i + d - 2 + h
    return dict(fJ4=4 * j, fSj=j - 1, fQ1=4 * (colb(j - 1) + i - 1), fH=h * np4_of(N))


def packed_addresses(s, u, i, h, d, N):
    """Every address finalize_packed forms from the running values."""
    P, i4 = np4_of(N), 4 * i
    iH = i4 + s["fH"]
    oE = np.where(h == 1, u["oE1"], u["oE0"])
    o2 = np.where(h == 1, u["oS1"], u["oS2"])
    o3 = np.where(h == 1, u["oS2"], u["oS3"])
    q1 = s["fQ1"] + (s["fJ4"] - 20)
    pA = 2 * u["cW"] + iH + s["fH"]
    return dict(qX=4 * (oE - 1) + i4, kX=oE - 1 + i, q1P=s["fQ1"], q1=q1, nextQ1=q1 + (s["fJ4"] - 16),
                mA=u["mM"] + 4 + iH, sA=u["mS"] + iH, uA=3 * P - u["cW"] + s["fJ4"], p0=pA, p1=pA + P,
                q2=4 * o2 + i4, q3=4 * o3 + i4, q3b=4 * o3 + i4 + 4, k2=o2 + i, k3=o3 + i, k3b=o3 + i + 1,
                sjm=s["fSj"], sj=s["fSj"] + 1, uj=s["fSj"] + 1, djm=s["fSj"],
                gq=4 * (rowb(i, N) - 4) + (s["fJ4"] - i4), uW=u["cW"] + s["fH"] + s["fJ4"])


# the parent's name of each packed address, by half (lane_addresses_closed of the anchor model)
PARENT_NAME = dict(qX=("qA", "qB"), kX=("kA", "kB"), q1P=("q1P", "q1A"), q1=("q1A", "q1B"), mA=("mA", "mB"),
                   sA=("sA", "sB"), p0=("pA0", "pB0"), p1=("pA1", "pB1"), q2=("q2", "q1"), q3=("q3", "q2"),
                   k2=("k2", "k1"), k3=("k3", "k2"), sjm=("sjm", "sj"), sj=("sj", "sjp"), uj=("ujA", "ujB"),
                   djm=("djm", "dj"), gq=("gqA", "gqB"), uW=("uWA", "uWB"))


def _unique(*cols):
    return np.unique(np.stack([np.asarray(c).astype(np.int64) for c in cols], 1), axis=0)


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("N0", [5, 29, 53, 77])
def test_each_cell_once(N0):
    lanes = np.arange(64)
    for N in range(N0, min(N0 + 24, 101)):
        mlo, mhi = hulls(N)
        u = {k: np.zeros_like(mlo) for k in uniform_closed(6, N)}
        fd = np.zeros_like(mlo)
        for d, fr, lr, R, ab, pk, need in sweep(N):
            e0, e1 = d - 2, d - 1
            assert (fr <= lr).all() and (ab >= 1).all() and (ab <= fr).all()
            assert (pk == (lr - fr <= HALF - 1)).all(), (N, d)              # the mode is the window's fit
            assert (lr - ab <= np.where(pk, HALF - 1, 126)).all(), (N, d)    # every window row has a lane
            # the uniform values are shared by both modes: slow path exactly at a re-anchor
            fd = np.where(need, 0, fd)
            c = uniform_closed(d, N)
            for k in u:
                u[k] = np.where(fd != d, c[k], u[k])
                assert (u[k] == c[k]).all(), (N, d, k)
            u, fd = uniform_advance(u, d, N), np.full_like(fd, d + 2)
            # the finalizations of every (row, half) cell, lane by lane, for the distinct
            # (fr, lr, ab, mode, R) of this step: one where the window has the cell, none elsewhere
            f, l, a, p, r = _unique(fr, lr, ab, pk, R).T[:, :, None]
            t = np.arange(f.shape[0])[:, None] + 0 * lanes
            cnt = np.zeros((f.shape[0], N + 2, 2), np.int64)
            rows = np.arange(N + 2)[None, :]
            want = np.stack([(rows >= f) & (rows <= l),
                             (rows >= f) & (rows <= np.minimum(l, r - 1)) & (e1 <= N - 1)], 2)
            i, h = lane_row_half(a, lanes)                                   # packed: one wave, a cell per lane
            cell = (p == 1) & (i >= f) & (i <= l) & (i + e0 + h <= N)        # row R has no span-e1 cell
            np.add.at(cnt, (t[cell], i[cell], (h + 0 * i)[cell]), 1)
            for fls in (0, 1):                                               # two cells per lane, two lane-sets
                i = a + 63 * fls + lanes
                own = (p == 0) & (i >= f) & (i <= l) & ((lanes < 63) | (fls == 1) | (l - a <= 63))
                own &= (fls == 0) | (l - a > 63)
                np.add.at(cnt, (t[own], i[own], 0), 1)
                own &= (i <= r - 1) & (e1 <= N - 1)
                np.add.at(cnt, (t[own], i[own], 1), 1)
            assert (cnt == want).all(), (N, d)


@pytest.mark.parametrize("N", [5, 12, 36, 37, 59, 64, 70, 100])
def test_written_rows_equal_the_parents(N):
    """Packed and two-cells-per-lane steps together write the rows of the parent's mapping
    (lane = fr + 63 fls + l; _parent_rows of the anchor model), each once."""
    lanes = np.arange(64)
    for d, fr, lr, R, ab, pk, need in sweep(N):
        for f, l, a, p in _unique(fr, lr, ab, pk).tolist():
            if p:
                i, h = lane_row_half(a, lanes)
                rows = i[(i >= f) & (i <= l) & (h == 0)].tolist()
            else:
                rows = [a + 63 * fls + lane for fls in range(2 if l - a > 63 else 1) for lane in range(64)
                        if f <= a + 63 * fls + lane <= l and (lane < 63 or fls == 1 or l - a <= 63)]
            assert sorted(rows) == sorted(x for w in _parent_rows(f, l)[1] for x in w), (N, d, f, l, a, p)


@pytest.mark.parametrize("N0", [5, 29, 53, 77])
def test_packed_addresses_by_induction(N0):
    lane = np.arange(64)[None, :]
    for N in range(N0, min(N0 + 24, 101)):
        i, h = lane_row_half(np.arange(1, N + 1)[:, None], lane)           # every anchor, every lane
        for d in steps(N):
            if d - 2 > N - 1:
                continue
            s, u = lane_closed(i, h, d, N), uniform_closed(d, N)
            got, want = packed_addresses(s, u, i, h, d, N), lane_addresses_closed(i, d, N)
            for k, (ka, kb) in PARENT_NAME.items():
                assert (got[k] == np.where(h == 1, want[kb], want[ka])).all(), (N, d, k)
            assert (got["q3b"] == np.where(h == 1, want["q2"], want["q3"]) + 4).all()
            assert (got["k3b"] == np.where(h == 1, want["k2"], want["k3"]) + 1).all()
            # U(i + 1, jA) of span e0-1: the lower half's; the upper half's read stays in the slot
            assert (got["uA"] == want["uA"] + 4 * h).all()
            # the advance
            nxt = dict(fQ1=got["nextQ1"], fJ4=s["fJ4"] + 8, fSj=s["fSj"] + 2, fH=s["fH"])
            c = lane_closed(i, h, d + 2, N)
            for k in c:
                assert (nxt[k] == c[k]).all(), (N, d, k)


@pytest.mark.parametrize("N0", [5, 29, 53, 77])
def test_upper_half_u_neighbour_is_on(N0):
    lanes = np.arange(64)
    for N in range(N0, min(N0 + 24, 101)):
        mlo, mhi = hulls(N)
        for d, fr, lr, R, ab, pk, need in sweep(N):
            ghost = np.minimum(mhi + 3, N + 1)                               # the ghost row, if the span has it
            f, l, a, r, g = _unique(fr[pk], lr[pk], ab[pk], R[pk], ghost[pk]).T[:, :, None]
            i, h = lane_row_half(a, lanes)
            on = (i >= f) & (i <= l)
            used = on & (h == 1) & (i <= r - 1) & (i != g)                   # its cell exists, U is not the restored qm
            src = (lanes & (HALF - 1)) + 1 + 0 * i
            assert (src[used] <= HALF - 1).all(), (N, d)                     # a lower-half lane,
            assert (np.take_along_axis(on, np.minimum(src, 63), 1)[used]).all(), (N, d)   # which is on,
            assert ((i + 1)[used] <= (l + 0 * i)[used]).all(), (N, d)        # as row i + 1 is in the window
            assert on[:, :HALF][on[:, HALF:]].all()                          # and so is the qm1 predecessor's lane
            assert ((l == r) | (l == g)).all(), (N, d)                       # the last row is row R or the ghost


def test_mode_changes_per_sweep():
    worst = 0
    for N in range(5, 101):
        mlo, _ = hulls(N)
        changes, last = np.zeros_like(mlo), None
        for d, fr, lr, R, ab, pk, need in sweep(N):
            if last is not None:
                changes += pk != last
                assert (need | (pk == last)).all()                           # a change of mode is a re-anchor
            last = pk
        assert (changes <= MODE_CHANGES).all(), N
        assert changes[mlo == SCRATCH[0]].sum() <= 1                         # from scratch: two cells per lane, then packed
        worst = max(worst, int(changes.max()))
    assert worst == MODE_CHANGES


def _moves(N):
    """The hulls (1-based) of the moves of workloads.synthetic(N): a mutable position, with its
    partner where the active macrostate enforces a pair."""
    tmpl, active = workloads.synthetic(N)
    out = []
    for p in range(N):
        if not tmpl[p].isupper():
            continue
        q = N - 1 - p if active[p] in "()" else p
        out.append((p, min(p, q) + 1, max(p, q) + 1))
    return out


def test_packed_share_of_the_benchmark(capsys):
    N = 100
    share = {}
    for p, lo, hi in _moves(N):
        ab, pk, n, k = np.int64(0), np.bool_(False), 0, 0
        for d in steps(N):
            if d - 2 > N - 1:
                continue
            fr, lr, _ = window(d, N, lo, hi)
            _, ab, pk = choose(ab, pk, fr, lr)
            n, k = n + 1, k + int(pk)
        share[p] = (k, n, lo != hi)
    tot = lambda sel: sum(share[p][0] for p in sel) / sum(share[p][1] for p in sel)
    single = [p for p in share if not share[p][2]]
    helix = [p for p in share if share[p][2]]
    with capsys.disabled():
        print("\npacked share of (move, step) pairs, synthetic(100): all %d moves %.3f, %d single %.3f, "
              "positions 30-44 %.3f, %d helix-partner %.3f"
              % (len(share), tot(share), len(single), tot(single), tot([p for p in single if 30 <= p <= 44]),
                 len(helix), tot(helix)))
    assert len(share) == 73 and len(helix) == 12
    assert abs(tot(share) - 0.80) < 0.01
