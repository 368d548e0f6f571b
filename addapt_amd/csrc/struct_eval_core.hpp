// The per-lane pieces of struct_eval_kernel (struct_eval.hip): the energy a
// sequence pays for a given dot-bracket, loop by loop.  A position's partner
// from the bracket string, the loop one closing pair owns (hairpin, stack /
// bulge / interior, multiloop), the exterior loop's stems, the admission of a
// position or pair by the constraint arrays, the motif-site test on a structure
// and the site's adjustment, in the two conventions of dev_types.hpp EvalTab:
//
//   PF   E(s) = -kT ln w(s), w the weight the partition-function kernels give s:
//        energy.cpp eval_structure's loops (lxc ln(u / 30) as computed), and per
//        formed motif site the factor exp(-enc / kT) of the substructure the site
//        encloses replaced by exp(-enc / kT) + exp(-eint / kT) (exp(-beff / kT) - 1)
//   MFE  the integer dcal arithmetic of the MFE kernels: the ln term truncated,
//        a formed site's enclosed energy min(enc, m_mfe_dcal)
//
// Free of HIP builtins: the kernel supplies the barriers and the wave sums, so
// a host program can run the same code lane by lane against the CPU oracle
// (tests/test_struct_eval_core.py).  ptype(), rtype(), allowed() come from
// fold_setup_core.hpp; the includer provides special_hp() (fold_common.hpp; on
// a host, any scan of the keys that returns the last match) in namespace adx
// before this header and defines SE_FN (the kernel: __device__).
#pragma once

#include <cmath>
#include <cstdint>

#include "dev_types.hpp"
#include "fold_setup_core.hpp"

namespace adx {
namespace {

constexpr int SE_NP = NMAX + 2;
constexpr int SE_MAXLOOP = 30;
constexpr int SE_TURN = 3;
// status bits of one item
constexpr int SE_MALFORMED = 1;   // unbalanced, a character outside ".()", a non-canonical pair
constexpr int SE_HAIRPIN = 2;     // a hairpin below 3
constexpr int SE_EXCLUDED = 4;    // the variant's constraint excludes it
constexpr int SE_BIGLOOP = 8;     // an interior loop above MAXLOOP (priced, but no fold produces it)
// bracket codes of the staged structure
constexpr uint8_t SB_DOT = 0, SB_OPEN = 1, SB_CLOSE = 2, SB_BAD = 3;

// what seq_setup (fold_common.hpp) stages for a workgroup's sequence
struct EvalSeqLds {
    alignas(16) uint32_t spk[MAX_SPECIAL_HP];   // special-hairpin keys (fold_common.hpp special_hp)
    int spv[MAX_SPECIAL_HP];                    // their energies (EvalTab::sp_e)
    uint8_t S[SE_NP], up[SE_NP], ptn[SE_NP], enc[SE_NP], flg[SE_NP], mat[SE_NP];
    uint8_t mcode[MAX_MOTIF];
    int8_t mpt[MAX_MOTIF];
};

SE_FN inline uint8_t bracket_code(char c) { return c == '.' ? SB_DOT : c == '(' ? SB_OPEN : c == ')' ? SB_CLOSE : SB_BAD; }

// The partner of 1-based position k in the bracket codes b[1..N]: 0 for an
// unpaired base (or a character outside ".()"), -1 for a bracket without a
// match.  A scan to the matching bracket: O(L) at worst.
SE_FN inline int partner_of(const uint8_t *b, int N, int k) {
    const int c = b[k];
    if (c != SB_OPEN && c != SB_CLOSE) return 0;
    const int step = c == SB_OPEN ? 1 : -1;
    int depth = 1;
    for (int p = k + step; p >= 1 && p <= N; p += step) {
        const int d = b[p];
        if (d == c) depth++;
        else if (d == (SB_OPEN + SB_CLOSE) - c && --depth == 0) return p;
    }
    return -1;
}

// one lane's running totals: integer dcal, the non-integer dcal terms, status bits
struct EvalAcc {
    int e = 0;
    double d = 0.0;
    int status = 0;
};

template <class LT>
struct StructEval {
    const DevTables *T;    // energy-valued (setup_core.hpp build_tables, mfe image)
    const EvalTab *E;
    const LT &L;           // the sequence's stage (EvalSeqLds)
    const uint8_t *pt;     // the item's partners, 1-based, 0 = unpaired
    int N;

    SE_FN int ti(float x) const { return static_cast<int>(x); }   // a table energy (integral)
    SE_FN int type(int i, int j) const { return ptype(L.S[i], L.S[j]); }
    SE_FN int mlstem(int t, int n5, int n3) const { return ti(T->mlstem[t][n5][n3]); }

    // the length energy of a loop of u unpaired bases: an integer, but for the
    // PF convention's loops above 30
    SE_FN void add_len(int kind, int u, EvalAcc &a) const {
        const double v = E->len[kind][u];
        if (u <= 30 || E->mfe) a.e += static_cast<int>(v);
        else a.d += v;
    }

    SE_FN void hairpin(int i, int j, int t, EvalAcc &a) const {
        const int u = j - i - 1;
        if (u < SE_TURN) {
            a.status |= SE_HAIRPIN;
            return;
        }
        if (u == 3 || u == 4 || u == 6) {
            const int hit = special_hp(L.spk, hp_key(L.S, i, u + 2));
            if (hit >= 0) {
                a.e += L.spv[hit];
                return;
            }
        }
        add_len(EV_HP, u, a);
        a.e += u == 3 ? ti(T->termAU[t]) : ti(T->mmH[t][L.S[i + 1]][L.S[j - 1]]);
    }

    // energy.cpp interior_energy; t2 = type of the reversed inner pair (q, p)
    SE_FN void interior(int n1, int n2, int t, int t2, int si1, int sj1, int sp1, int sq1, EvalAcc &a) const {
        const int nl = n1 > n2 ? n1 : n2, ns = n1 > n2 ? n2 : n1;
        if (nl + ns > SE_MAXLOOP) a.status |= SE_BIGLOOP;
        if (nl == 0) {
            a.e += ti(T->stack[t][t2]);
        } else if (ns == 0) {
            add_len(EV_BUL, nl, a);
            a.e += nl == 1 ? ti(T->stack[t][t2]) : ti(T->termAU[t]) + ti(T->termAU[t2]);
        } else if (ns == 1 && nl == 1) {
            a.e += ti(T->int11[t][t2][si1][sj1]);
        } else if (ns == 1 && nl == 2) {
            a.e += n1 == 1 ? ti(T->int21[t][t2][si1][sq1][sj1]) : ti(T->int21[t2][t][sq1][si1][sp1]);
        } else if (ns == 1) {
            add_len(EV_INT, nl + 1, a);
            a.e += E->nin[nl - ns] + ti(T->mm1n[t][si1][sj1]) + ti(T->mm1n[t2][sq1][sp1]);
        } else if (ns == 2 && nl == 2) {
            a.e += ti(T->int22[t][t2][si1][sp1][sq1][sj1]);
        } else if (ns == 2 && nl == 3) {
            add_len(EV_INT, 5, a);
            a.e += E->nin[1] + ti(T->mm23[t][si1][sj1]) + ti(T->mm23[t2][sq1][sp1]);
        } else {
            add_len(EV_INT, nl + ns, a);
            a.e += E->nin[nl - ns] + ti(T->mmI[t][si1][sj1]) + ti(T->mmI[t2][sq1][sp1]);
        }
    }

    // The loop the pair (i, j = pt[i] > i) closes, classified by a walk over its
    // branches, added to a; a non-canonical pair is malformed and prices nothing,
    // but its loop's shape is still reported.
    SE_FN void loop_of(int i, EvalAcc &a) const {
        const int j = pt[i];
        const int t = type(i, j);
        int nb = 0, p = 0, q = 0, unp = 0, ml = 0;
        bool ok = true;
        for (int k = i + 1; k < j; k++) {
            const int pk = pt[k];
            if (pk > k) {
                if (++nb == 1) {
                    p = k;
                    q = pk;
                }
                const int tk = type(k, pk);
                ok = ok && tk != 0;
                if (tk != 0) ml += mlstem(tk, L.S[k - 1], L.S[pk + 1]);
                k = pk;
            } else {
                unp++;
            }
        }
        if (t == 0) {
            a.status |= SE_MALFORMED;
            if (nb == 0 && j - i - 1 < SE_TURN) a.status |= SE_HAIRPIN;
            if (nb == 1 && (p - i - 1) + (j - q - 1) > SE_MAXLOOP) a.status |= SE_BIGLOOP;
        } else if (nb == 0) {
            hairpin(i, j, t, a);
        } else if (nb == 1) {
            const int t2 = type(q, p);
            if (t2 != 0) interior(p - i - 1, j - q - 1, t, t2, L.S[i + 1], L.S[j - 1], L.S[p - 1], L.S[q + 1], a);
            else if ((p - i - 1) + (j - q - 1) > SE_MAXLOOP) a.status |= SE_BIGLOOP;
        } else if (ok) {   // (a non-canonical branch reports itself)
            a.e += E->mlclosing + mlstem(rtype(t), L.S[j - 1], L.S[i + 1]) + ml + unp * E->mlbase;
        }
    }

    // the exterior loop's stems (one lane: a walk over the top-level pairs)
    SE_FN void exterior(EvalAcc &a) const {
        for (int i = 1; i <= N; i++) {
            const int j = pt[i];
            if (j <= i) continue;
            const int t = type(i, j);
            if (t != 0) a.e += ti(T->ext[t][i > 1 ? L.S[i - 1] : 5][j < N ? L.S[j + 1] : 5]);
            i = j;
        }
    }

    // does the variant's constraint admit position k as the structure has it
    // (build_constraint's arrays: unpaired where the run allows, paired as allowed())?
    SE_FN bool admits(int k) const {
        const int pk = pt[k];
        if (pk == 0) return L.up[k] >= 1;
        return pk < k || allowed(L, k, pk);
    }

    // motif position m of the site at start o (L.mat[o] != 0: seq_setup's
    // motif_site): does the structure have the motif's own fold there?
    SE_FN bool site_position(int o, int m) const {
        const int pm = L.mpt[m];
        return int(pt[o + m]) == (pm < 0 ? 0 : o + pm);
    }

    // A formed site whose enclosed substructure costs enc dcal: what the total changes by.
    // PF, kcal/mol (+inf for a weight that is not positive):
    SE_FN double site_adjust_pf(double enc_dcal) const {
        const double kT = E->kT;
        const double w = 1.0 + exp(-(E->m_eint - enc_dcal / 100.0) / kT) * (exp(-E->m_beff / kT) - 1.0);
        return w > 0.0 ? -kT * log(w) : INFINITY;
    }
    // MFE, dcal: min(enc, m_mfe_dcal) - enc
    SE_FN int site_adjust_mfe(int enc) const { return E->m_mfe_dcal < enc ? E->m_mfe_dcal - enc : 0; }
};

// The status an item reports: a string without a pair table (unbalanced, or a
// character outside ".()": `unparsed`) is malformed and nothing else, since the
// other bits are statements about its pairs
SE_FN inline int item_status(bool unparsed, int status) { return unparsed ? SE_MALFORMED : status; }

// The energy an item reports from its wave totals (kcal/mol): NaN for a
// malformed item, +inf for one a fold can never hold, else the sum
SE_FN inline double item_energy(int e, double d, double adj_kcal, int status) {
    if (status & SE_MALFORMED) return NAN;
    if (status & (SE_HAIRPIN | SE_EXCLUDED)) return INFINITY;
    return (double(e) + d) / 100.0 + adj_kcal;
}
// p(s) = exp(-(E - G) / kT) with G = -kT lnZ; 0 for a non-member or an empty ensemble
SE_FN inline double item_prob(double energy, int status, double lnZ, double kT) {
    if (status != 0 || !(lnZ == lnZ) || lnZ == -INFINITY || lnZ == INFINITY) return 0.0;
    return exp(-energy / kT - lnZ);
}

}  // namespace
}  // namespace adx
