// The per-lane pieces of pf_access_kernel (pf_access.hip): the adjoints of
// pf_fill_kernel's inside fill and the sums over the loops that hold a window,
// which together give P_u(i,j), the probability that i..j is all unpaired.
// Free of HIP builtins, in mfe_outside_core.hpp's style: the includer provides
// special_hp() in namespace adx and defines TR_FN before this header.
//
// The adjoints are dZ/d(table entry), Z = q5(N): PfModel's fill_cell and w_q5
// differentiated term for term, each a gather over larger spans (so one barrier
// per descending diagonal, and within a cell am, then am1, then ab):
//   a5(m)    = a5(m+1) sigma [m+1 unpaired]  +  sum_j a5(j) qb(m+1,j) ext(m+1,j)
//   am(a,b)  = sum_j ab(a-1,j) mlc(a-1,j) qm1(b+1,j-1)  +  sum_j am(a,j) qm1(b+1,j)
//   am1(k,b) = sum_i ab(i,b+1) mlc(i,b+1) qm(i+1,k-1)
//              + sum_i am(i,b) ( pwml[k-i] [i..k-1 unpaired] + qm(i,k-1) )
//              + am1(k,b+1) mlbase sigma [b+1 unpaired]
//   ab(p,q)  = a5(q) q5(p-1) ext(p,q)  +  am1(p,q) mlstem(p,q)
//              + sum_(i,j) ab(i,j) int(p-i-1, j-q-1)          (0 where (p,q) cannot pair)
// Every factor is the fill's own, sigma included, so weight * adjoint / Z is
// free of the scale; qb ab / Z is the pair probability.
//
// A window that is all unpaired lies in exactly one loop:
//   exterior          q5(i-1) sigma^len a5(j)
//   multiloop, after  sum_s qm1(s,i-1) (mlbase sigma)^len am1(s,j)
//   a stem            (the unpaired tail of qm1: the runs between two stems and
//                     before the closing pair)
//   anything else     through R(a,b), the mass of the structures in which a..b
//                     is a MAXIMAL unpaired run of a hairpin, of either side of
//                     an interior loop, of a multiloop's leading run (the
//                     unpaired prefix of qm) or of a formed motif site's own
//                     fold: the window's share is the sum of R over a <= i,
//                     b >= j, which two prefix passes leave in R itself
// The powers sigma^k and (mlbase sigma)^k are products of the one factor the
// fill multiplies per base (pw5, pwm), not DevScaled::sig[k]: a structure's
// weight here is then the fill's to rounding, and a pinned structure gives 1.
#pragma once

#include <cmath>
#include <cstdint>

#include "pf_sample_cells.hpp"

namespace adx {
namespace {

template <class F>
struct AccessT {
    const PfModelT<F> &M;
    double *ab, *am, *am1;    // the adjoint triangles, laid out as M.qb
    double *a5;               // [0, N]
    double *R;                // [N][N] row a-1, column b-1 (a <= b)
    const double *pw5, *pwm;  // [0, N] sigma^k and (mlbase sigma)^k

    TR_FN int idx(int i, int j) const { return M.idx(i, j); }
    TR_FN double &run(int a, int b) const { return R[size_t(a - 1) * M.N + b - 1]; }

    // ---- a5(m), m = N-1 .. 0: lane `lane` of `lanes` takes its share of the stems (m+1, j)
    TR_FN double a5_unpaired(int m) const { return M.L.up[m + 1] >= 1 ? a5[m + 1] * double(M.X->sig[1]) : 0.0; }
    TR_FN double a5_pairs(int m, int lane, int lanes) const {
        double v = 0.0;
        for (int j = m + 5 + lane; j <= M.N; j += lanes) {
            const double b = M.qb[idx(m + 1, j)];
            if (b != 0.0) v += a5[j] * b * M.ext(M.type(m + 1, j), m + 1, j);
        }
        return v;
    }

    // ---- am, am1, ab of one cell (every larger span is finished)
    TR_FN void adjoint_cell(int p, int q) const {
        const int N = M.N, at = idx(p, q);
        double m = 0.0;
        if (p >= 2)
            for (int j = q + 6; j <= N; j++) {   // closings (p-1, j): the cell is their qm part
                const double x = ab[idx(p - 1, j)];
                if (x != 0.0) m += x * M.ml_closing(p - 1, j, M.type(p - 1, j)) * M.qm1[idx(q + 1, j - 1)];
            }
        for (int j = q + 5; j <= N; j++) m += am[idx(p, j)] * M.qm1[idx(q + 1, j)];   // qm(p,j)'s prefix
        am[at] = m;

        double m1 = 0.0;
        if (q + 1 <= N) {
            for (int i = 1; i <= p - 6; i++) {   // closings (i, q+1): the cell is their last stem
                const double x = ab[idx(i, q + 1)];
                if (x != 0.0) m1 += x * M.ml_closing(i, q + 1, M.type(i, q + 1)) * M.qm[idx(i + 1, p - 1)];
            }
            if (M.L.up[q + 1] >= 1) m1 += am1[idx(p, q + 1)] * double(M.X->mlbase_sig);
        }
        for (int i = 1; i <= p; i++) {   // qm(i,q)'s last stem
            const double x = am[idx(i, q)];   // i = p: this cell's, just stored
            if (x == 0.0) continue;
            double pre = (i == p || M.L.up[i] >= p - i) ? double(M.X->pwml[p - i]) : 0.0;
            if (p - 1 - i >= 4) pre += M.qm[idx(i, p - 1)];
            m1 += x * pre;
        }
        am1[at] = m1;

        double b = 0.0;
        if (M.can_pair(p, q)) {
            const int t = M.type(p, q), t2 = M.type(q, p);
            b = a5[q] * M.q5[p - 1] * M.ext(t, p, q) + m1 * M.mlstem(t, M.L.S[p - 1], M.L.S[q + 1]);
            for (int n1 = 0; n1 <= PS_MAXLOOP && p - 1 - n1 >= 1; n1++) {
                const int i = p - 1 - n1;
                if (n1 > 0 && M.L.up[i + 1] < n1) break;
                for (int n2 = 0; n1 + n2 <= PS_MAXLOOP && q + 1 + n2 <= N; n2++) {
                    const int j = q + 1 + n2;
                    if (n2 > 0 && M.L.up[q + 1] < n2) break;
                    const double x = ab[idx(i, j)];
                    if (x != 0.0)
                        b += x * M.f_int(n1, n2, M.type(i, j), t2, M.L.S[i + 1], M.L.S[j - 1], M.L.S[p - 1], M.L.S[q + 1]);
                }
            }
        }
        ab[at] = b;
    }

    // ---- R(a,b): the mass of the structures whose maximal unpaired run a..b lies in a
    // hairpin, an interior loop, a multiloop's leading run or a formed motif site
    TR_FN double run_mass(int a, int b) const {
        const int N = M.N, len = b - a + 1;
        if (M.L.up[a] < len) return 0.0;
        double s = 0.0;
        const int i = a - 1, j = b + 1;
        if (i >= 1 && j <= N && len >= 3) {   // the hairpin of (a-1, b+1)
            const double x = ab[idx(i, j)];
            if (x != 0.0) s += x * M.w_qb(i, j, M.type(i, j), PC_HAIRPIN);
        }
        if (len <= PS_MAXLOOP) {
            if (i >= 1)   // the 5' side of (a-1, jj) over (b+1, qq)
                for (int qq = j + 4; qq < N; qq++) {
                    if (M.qb[idx(j, qq)] == 0.0) continue;
                    for (int n2 = 0; len + n2 <= PS_MAXLOOP && qq + 1 + n2 <= N; n2++) {
                        if (n2 > 0 && M.L.up[qq + 1] < n2) break;
                        const int jj = qq + 1 + n2;
                        const double x = ab[idx(i, jj)];
                        if (x != 0.0) s += x * M.interior(i, jj, M.type(i, jj), len, n2);
                    }
                }
            if (j <= N)   // the 3' side of (ii, b+1) over (pp, a-1)
                for (int pp = i - 4; pp > 1; pp--) {
                    if (M.qb[idx(pp, i)] == 0.0) continue;
                    for (int n1 = 0; n1 + len <= PS_MAXLOOP && pp - 1 - n1 >= 1; n1++) {
                        if (n1 > 0 && M.L.up[pp - n1] < n1) break;
                        const int ii = pp - 1 - n1;
                        const double x = ab[idx(ii, j)];
                        if (x != 0.0) s += x * M.interior(ii, j, M.type(ii, j), n1, len);
                    }
                }
        }
        {   // qm(a, .)'s unpaired prefix a..b before the stem at b+1
            double m = 0.0;
            for (int e = j + 4; e <= N; e++) m += am[idx(a, e)] * M.qm1[idx(j, e)];
            s += m * double(M.X->pwml[len]);
        }
        if (M.holo && M.mL > 0) {   // a run of dots of the motif's own fold, the site formed
            int from = -1;
            for (int k = 0; k <= M.mL; k++) {
                const bool dot = k < M.mL && M.L.mpt[k] < 0;
                if (dot && from < 0) from = k;
                if (!dot && from >= 0) {
                    const int p = a - from, q = p + M.mL - 1;
                    if (k - from == len && p >= 1 && q <= N && M.motif_at(p, q) && M.can_pair(p, q))
                        s += ab[idx(p, q)] * double(M.X->motif_extra);
                    from = -1;
                }
            }
        }
        return s;
    }
    // the two prefix passes: lane r's row, then lane c's column (a barrier between)
    TR_FN void sum_row(int a) const {
        for (int b = M.N - 1; b >= a; b--) run(a, b) += run(a, b + 1);
    }
    TR_FN void sum_column(int b) const {
        for (int a = 2; a <= b; a++) run(a, b) += run(a - 1, b);
    }

    // ---- Z P_u(i,j) after the passes
    TR_FN double window_mass(int i, int j) const {
        const int len = j - i + 1;
        if (M.L.up[i] < len) return 0.0;
        double s = M.q5[i - 1] * pw5[len] * a5[j];
        double t = 0.0;
        for (int k = 1; k <= i - 5; k++) t += M.qm1[idx(k, i - 1)] * am1[idx(k, j)];
        s += t * pwm[len];
        return s + run(i, j);
    }
    // P_u(i,j); Z = q5(N).  NaN: the constraint admits nothing.  N < 5: nothing can pair
    TR_FN double unpaired_prob(int i, int j, double Z) const {
        if (!(Z > 0.0) || !(Z < double(INFINITY))) return double(NAN);
        if (M.N < 5) return 1.0;
        return window_mass(i, j) / Z;
    }
    // P(x,y), x < y: qb ab / Z, and on a formed motif site the site's inner pairs
    TR_FN double pair_prob(int x, int y, double Z) const {
        if (!(Z > 0.0) || !(Z < double(INFINITY))) return double(NAN);
        double s = y - x >= 4 ? M.qb[idx(x, y)] * ab[idx(x, y)] : 0.0;
        if (M.holo && M.mL > 0)
            for (int k = 1; k < M.mL - 1; k++) {
                const int pk = M.L.mpt[k], p = x - k, q = p + M.mL - 1;
                if (pk > k && pk - k == y - x && p >= 1 && q <= M.N && M.motif_at(p, q) && M.can_pair(p, q))
                    s += ab[idx(p, q)] * double(M.X->motif_extra);
            }
        return s / Z;
    }
};
using Access = AccessT<float>;

}  // namespace
}  // namespace adx
