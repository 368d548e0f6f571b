// The per-lane pieces of pf_fill_kernel and pf_sample_kernel (pf_sample.hip):
// the weight of every candidate of every item kind.  The fill sums an item's
// candidate weights into its table entry and the sampler draws among the same
// weights, so the two decompositions agree term for term by construction.
// Free of HIP builtins, in mfe_trace_core.hpp's style: off(), ptype(), rtype()
// and allowed() come from fold_setup_core.hpp; the includer provides
// special_hp() (fold_common.hpp) in namespace adx before this header and
// defines TR_FN (the kernels: __device__).
//
// The recursion is oracle/fold.c pf_inside with the context's FP32 factors
// (DevTables / DevScaled, every factor carrying sigma per covered nucleotide),
// multiplied and summed in FP64:
//   q5(j)    = q5(j-1) sigma [j unpaired]  +  sum_k q5(k-1) qb(k,j) ext(k,j)
//   qb(i,j)  = hairpin + motif_extra + sum_(n1,n2) qb(p,q) int(n1,n2)
//              + mlclosing mlstem(j,i) sum_k qm(i+1,k-1) qm1(k,j-1)
//   qm(i,j)  = sum_k ( (mlbase sigma)^(k-i) [i..k-1 unpaired] + qm(i,k-1) ) qm1(k,j)
//   qm1(i,j) = qb(i,j) mlstem(i,j)  +  qm1(i,j-1) mlbase sigma [j unpaired]
// Each structure is reached by exactly one sequence of choices.
#pragma once

#include <cstdint>

#include "dev_types.hpp"
#include "fold_setup_core.hpp"

namespace adx {
namespace {

constexpr int PS_NP = NMAX + 2;
constexpr int PS_MAXLOOP = 30;
// item kinds
constexpr int PI_Q5 = 0, PI_QB = 1, PI_QM = 2, PI_QM1 = 3;
// candidate indices of a qb(i,j) item: hairpin, motif, the interior shapes
// ordered by loop size u = n1 + n2 and then n1 (index u(u+1)/2 + n1, so the
// shapes a span allows, u <= min(30, j-i-6), are a prefix), the multiloop splits
constexpr int PC_HAIRPIN = 0, PC_MOTIF = 1, PC_INT = 2;
constexpr int PS_NSHAPES = (PS_MAXLOOP + 1) * (PS_MAXLOOP + 2) / 2;   // 496
constexpr int PS_MAXCAND = 1024;   // >= 2 + 496 + NMAX, 2 NMAX: bounds every candidate loop

// the sequence-side data of one (sequence, variant), in LDS; F: the factors' type
// (dev_types.hpp DevTablesT: float in the kernels)
template <class F>
struct PfSeqLdsT {
    alignas(16) uint32_t spk[MAX_SPECIAL_HP];   // special-hairpin keys (fold_common.hpp special_hp)
    F spv[MAX_SPECIAL_HP];
    uint8_t S[PS_NP], up[PS_NP], ptn[PS_NP], enc[PS_NP], flg[PS_NP], mat[PS_NP];
    uint8_t mcode[MAX_MOTIF];
    int8_t mpt[MAX_MOTIF];
};

using PfSeqLds = PfSeqLdsT<float>;

template <class F>
struct PfModelT {
    const DevTablesT<F> *T;
    const DevScaledT<F> *X;
    const PfSeqLdsT<F> &L;
    double *qb, *qm, *qm1;   // the sequence's scratch slice (diagonal-major cells)
    double *q5;              // [0, N]
    int N, mL;
    bool holo;

    TR_FN int idx(int i, int j) const { return off(j - i, N) + i - 1; }   // j - i >= 4
    TR_FN int type(int i, int j) const { return ptype(L.S[i], L.S[j]); }
    TR_FN bool can_pair(int i, int j) const { return j - i >= 4 && type(i, j) != 0 && allowed(L, i, j); }
    TR_FN double mlstem(int t, int n5, int n3) const { return T->mlstem[t][n5][n3]; }
    TR_FN double ext(int t, int k, int j) const { return T->ext[t][k > 1 ? L.S[k - 1] : 5][j < N ? L.S[j + 1] : 5]; }
    // L.mat[o]: fold_setup_core.hpp motif_site at start o (fold_common.hpp seq_setup)
    TR_FN bool motif_at(int i, int j) const { return holo && mL > 0 && j - i == mL - 1 && L.mat[i] != 0; }

    TR_FN double hairpin(int i, int j, int t) const {
        const int u = j - i - 1;
        if (u == 3 || u == 4 || u == 6) {
            const int hit = special_hp(L.spk, hp_key(L.S, i, u + 2));
            if (hit >= 0) return L.spv[hit];
        }
        const double e = X->hp[u];
        if (u == 3) return e * double(T->termAU[t]);
        return e * double(T->mmH[t][L.S[i + 1]][L.S[j - 1]]);
    }

    // exp(-E_IntLoop / kT) sigma^(n1 + n2 + 2) (oracle/fold.c E_int); t2 = type of the reversed inner pair (q,p)
    TR_FN double f_int(int n1, int n2, int t, int t2, int si1, int sj1, int sp1, int sq1) const {
        const F *ct = X->ctab;
        const int nl = n1 > n2 ? n1 : n2, ns = n1 > n2 ? n2 : n1;
        if (nl == 0) return double(ct[CT_FSM + 0]) * ct[CT_STK + t * 8 + t2];
        if (ns == 0) {
            if (nl == 1) return double(ct[CT_FSM + 1]) * ct[CT_STK + t * 8 + t2];
            return double(ct[CT_FB + nl]) * T->termAU[t] * T->termAU[t2];
        }
        if (ns == 1) {
            if (nl == 1) return double(ct[CT_FSM + 2]) * T->int11[t][t2][si1][sj1];
            if (nl == 2)
                return double(ct[CT_FSM + 3]) * (n1 == 1 ? T->int21[t][t2][si1][sq1][sj1] : T->int21[t2][t][sq1][si1][sp1]);
            return double(ct[CT_F1N + nl]) * T->mm1n[t][si1][sj1] * T->mm1n[t2][sq1][sp1];
        }
        if (ns == 2) {
            if (nl == 2) return double(ct[CT_FSM + 4]) * T->int22[t][t2][si1][sp1][sq1][sj1];
            if (nl == 3) return double(ct[CT_FSM + 5]) * T->mm23[t][si1][sj1] * T->mm23[t2][sq1][sp1];
        }
        return double(X->fgen[(nl + ns - 6) * FG_ROW + n1 - 2]) * T->mmI[t][si1][sj1] * T->mmI[t2][sq1][sp1];
    }

    // qb(p,q) times the interior loop of the closing pair (i,j), type t, with n1 / n2
    // unpaired bases on the 5' / 3' side; 0 when the shape is not available
    TR_FN double interior(int i, int j, int t, int n1, int n2) const {
        const int p = i + 1 + n1, q = j - 1 - n2;
        if (q - p < 4) return 0.0;
        if (n1 > 0 && L.up[i + 1] < n1) return 0.0;
        if (n2 > 0 && L.up[q + 1] < n2) return 0.0;
        if (!can_pair(p, q)) return 0.0;
        const double v = qb[idx(p, q)];
        if (v == 0.0) return 0.0;
        return v * f_int(n1, n2, t, type(q, p), L.S[i + 1], L.S[j - 1], L.S[p - 1], L.S[q + 1]);
    }
    TR_FN double ml_closing(int i, int j, int t) const {
        return double(X->mlclosing) * mlstem(rtype(t), L.S[j - 1], L.S[i + 1]);
    }

    // ---- candidates: how many an item has, and the weight of candidate c
    TR_FN int n_shapes(int i, int j) const {   // interior shapes the span allows
        int um = j - i - 6;
        if (um < 0) return 0;
        if (um > PS_MAXLOOP) um = PS_MAXLOOP;
        return (um + 1) * (um + 2) / 2;
    }
    TR_FN int n_splits(int i, int j) const { return j - i - 10 > 0 ? j - i - 10 : 0; }   // k = i+6 .. j-5
    TR_FN int n_cand(int kind, int i, int j) const {
        if (kind == PI_Q5) return j >= 5 ? j - 3 : 1;          // "j unpaired", then k = 1 .. j-4
        if (kind == PI_QB) return PC_INT + n_shapes(i, j) + n_splits(i, j);
        if (kind == PI_QM) return 2 * (j - i - 3);             // k = i .. j-4: unpaired prefix, qm prefix
        return 2;                                              // qm1: the pair (i,j), j unpaired
    }
    // shape index s -> (n1, n2)
    TR_FN void shape(int s, int &n1, int &n2) const {
        int u = 0;
        for (int t = 1; t <= PS_MAXLOOP; t++)
            if (t * (t + 1) / 2 <= s) u = t;
        n1 = s - u * (u + 1) / 2;
        n2 = u - n1;
    }

    TR_FN double w_q5(int j, int c) const {
        if (c == 0) return L.up[j] >= 1 ? q5[j - 1] * double(X->sig[1]) : 0.0;
        const int k = c;
        if (k + 4 > j) return 0.0;
        const double b = qb[idx(k, j)];
        if (b == 0.0) return 0.0;
        return q5[k - 1] * b * ext(type(k, j), k, j);
    }
    // (i,j) can pair, t = its type
    TR_FN double w_qb(int i, int j, int t, int c) const {
        if (c == PC_HAIRPIN) return L.up[i + 1] >= j - i - 1 ? hairpin(i, j, t) : 0.0;
        if (c == PC_MOTIF) return motif_at(i, j) ? double(X->motif_extra) : 0.0;
        const int ns = n_shapes(i, j);
        if (c < PC_INT + ns) {
            int n1, n2;
            shape(c - PC_INT, n1, n2);
            return interior(i, j, t, n1, n2);
        }
        const int k = i + 6 + (c - PC_INT - ns);
        if (k > j - 5) return 0.0;
        return qm[idx(i + 1, k - 1)] * qm1[idx(k, j - 1)] * ml_closing(i, j, t);
    }
    TR_FN double w_qm(int i, int j, int c) const {
        const int k = i + (c >> 1);
        if (k > j - 4) return 0.0;
        const double b = qm1[idx(k, j)];
        if (b == 0.0) return 0.0;
        if ((c & 1) == 0) return (k == i || L.up[i] >= k - i) ? double(X->pwml[k - i]) * b : 0.0;
        return k - 1 - i >= 4 ? qm[idx(i, k - 1)] * b : 0.0;
    }
    TR_FN double w_qm1(int i, int j, int c) const {
        if (c == 0) {
            const double b = qb[idx(i, j)];
            return b == 0.0 ? 0.0 : b * mlstem(type(i, j), L.S[i - 1], L.S[j + 1]);
        }
        return (L.up[j] >= 1 && j - 1 - i >= 4) ? qm1[idx(i, j - 1)] * double(X->mlbase_sig) : 0.0;
    }
    TR_FN double weight(int kind, int i, int j, int c) const {
        if (c < 0 || c >= n_cand(kind, i, j)) return 0.0;
        if (kind == PI_Q5) return w_q5(j, c);
        if (kind == PI_QB) return w_qb(i, j, type(i, j), c);
        if (kind == PI_QM) return w_qm(i, j, c);
        return w_qm1(i, j, c);
    }

    // ---- fill: qb, qm1, qm of one cell (every shorter span is finished): the
    // sums of the candidate weights above, the interior shapes walked as
    // oracle/fold.c walks them
    TR_FN void fill_cell(int i, int j) const {
        double b = 0.0;
        const int t = type(i, j);
        if (t != 0 && allowed(L, i, j)) {
            b = w_qb(i, j, t, PC_HAIRPIN) + w_qb(i, j, t, PC_MOTIF);
            for (int n1 = 0; n1 <= PS_MAXLOOP && i + 1 + n1 < j - 4; n1++) {
                if (n1 > 0 && L.up[i + 1] < n1) break;
                for (int n2 = 0; n1 + n2 <= PS_MAXLOOP; n2++) {
                    const int q = j - 1 - n2;
                    if (q - (i + 1 + n1) < 4 || (n2 > 0 && L.up[q + 1] < n2)) break;
                    b += interior(i, j, t, n1, n2);
                }
            }
            double s = 0.0;
            for (int k = i + 6; k <= j - 5; k++) s += qm[idx(i + 1, k - 1)] * qm1[idx(k, j - 1)];
            b += s * ml_closing(i, j, t);
        }
        const int at = idx(i, j);
        qb[at] = b;
        qm1[at] = w_qm1(i, j, 0) + w_qm1(i, j, 1);   // reads qb[at] back
        double w = 0.0;
        for (int c = 0; c < 2 * (j - i - 3); c++) w += w_qm(i, j, c);   // reads qm1[at] back
        qm[at] = w;
    }

    // lane `lane` of `lanes`: its share of q5(j)'s stems (k, j)
    TR_FN double q5_pairs(int j, int lane, int lanes) const {
        double v = 0.0;
        for (int k = 1 + lane; k + 4 <= j; k += lanes) v += w_q5(j, k);
        return v;
    }
};
using PfModel = PfModelT<float>;

}  // namespace
}  // namespace adx
