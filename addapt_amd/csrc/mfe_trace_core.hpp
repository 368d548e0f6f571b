// The per-lane pieces of mfe_trace_kernel (mfe_trace.hip): one cell of the
// Zuker fill, one lane's share of a traceback item's candidates, and what the
// winning candidate pushes.  Free of HIP builtins: the kernel supplies the
// barriers and the LDS atomicMin between them, so a host program can run the
// same code lane by lane against the CPU oracle.  off(), ptype(), rtype() and
// allowed() come from fold_setup_core.hpp, which a host program can include
// too; the includer provides special_hp() (fold_common.hpp; on a host, any
// scan of the keys that returns the last match) in namespace adx before this
// header and defines TR_FN (the kernel: __device__).
#pragma once

#include <cstdint>

#include "dev_types.hpp"
#include "fold_setup_core.hpp"

namespace adx {
namespace {

constexpr int TR_INF = 100000000;        // "impossible" (oracle/fold.c MINF)
constexpr int TR_NP = NMAX + 2;
constexpr int TR_STACK = 4 * NMAX + 8;   // items (oracle/fold.c:697)
constexpr int TR_NONE = 0x7fffffff;      // no candidate matched
constexpr int TR_MAXLOOP = 30;
// item kinds of the traceback stack, as oracle/fold.c orc_mfe
constexpr int TI_F5 = 0, TI_C = 1, TI_FM = 2, TI_FM1 = 3;
// candidate indices of a c(i,j) item, growing in the oracle's search order:
// hairpin, motif, interior loops (p ascending, then q descending), multiloop (k ascending)
constexpr int TC_HAIRPIN = 0, TC_MOTIF = 1, TC_INT = 2, TC_ML = TC_INT + 32 * 32;

struct TraceLds {
    alignas(16) uint32_t spk[MAX_SPECIAL_HP];   // special-hairpin keys (fold_common.hpp special_hp)
    int spv[MAX_SPECIAL_HP];
    int f5[TR_NP];
    int stk[3 * TR_STACK];
    int cur[3];                                 // the popped item (kind < 0: stack empty)
    int top, win, red;
    uint8_t S[TR_NP], up[TR_NP], ptn[TR_NP], enc[TR_NP], flg[TR_NP], mat[TR_NP];
    uint8_t mcode[MAX_MOTIF];
    int8_t mpt[MAX_MOTIF];
    char out[TR_NP];
};

TR_FN inline int ei(float x) { return static_cast<int>(x); }   // a table energy (integral)
TR_FN inline int tmin(int a, int b) { return a < b ? a : b; }

struct Trace {
    const DevTables *T;
    const DevScaled *X;
    TraceLds &L;
    int *c, *fm, *fm1;   // the workgroup's scratch slice (diagonal-major cells)
    int N;
    int mlclosing, mlbase, mextra, mL;
    bool holo;

    TR_FN int idx(int i, int j) const { return off(j - i, N) + i - 1; }   // j - i >= 4
    TR_FN int type(int i, int j) const { return ptype(L.S[i], L.S[j]); }
    TR_FN bool can_pair(int i, int j) const { return j - i >= 4 && type(i, j) != 0 && allowed(L, i, j); }
    TR_FN int mlstem(int t, int n5, int n3) const { return ei(T->mlstem[t][n5][n3]); }
    TR_FN int ext(int t, int k, int j) const {
        return ei(T->ext[t][k > 1 ? L.S[k - 1] : 5][j < N ? L.S[j + 1] : 5]);
    }

    TR_FN int hairpin(int i, int j, int t) const {
        const int u = j - i - 1;
        const int e = ei(X->hp[u]);
        if (u == 3 || u == 4 || u == 6) {
            const int hit = special_hp(L.spk, hp_key(L.S, i, u + 2));
            if (hit >= 0) return L.spv[hit];
        }
        if (u == 3) return e + ei(T->termAU[t]);
        return e + ei(T->mmH[t][L.S[i + 1]][L.S[j - 1]]);
    }

    // E_IntLoop (oracle/fold.c E_int); t2 = type of the reversed inner pair (q,p)
    TR_FN int e_int(int n1, int n2, int t, int t2, int si1, int sj1, int sp1, int sq1) const {
        const int nl = n1 > n2 ? n1 : n2, ns = n1 > n2 ? n2 : n1;
        if (nl == 0) return ei(T->stack[t][t2]);
        if (ns == 0) {
            const int e = ei(X->ctab[CT_FB + nl]);
            if (nl == 1) return e + ei(T->stack[t][t2]);
            return e + ei(T->termAU[t]) + ei(T->termAU[t2]);
        }
        if (ns == 1) {
            if (nl == 1) return ei(T->int11[t][t2][si1][sj1]);
            if (nl == 2) return n1 == 1 ? ei(T->int21[t][t2][si1][sq1][sj1]) : ei(T->int21[t2][t][sq1][si1][sp1]);
            return ei(X->il[nl + 1]) + ei(X->nin[nl - 1]) + ei(T->mm1n[t][si1][sj1]) + ei(T->mm1n[t2][sq1][sp1]);
        }
        if (ns == 2) {
            if (nl == 2) return ei(T->int22[t][t2][si1][sp1][sq1][sj1]);
            if (nl == 3) return ei(X->ctab[CT_FSM + 5]) + ei(T->mm23[t][si1][sj1]) + ei(T->mm23[t2][sq1][sp1]);
        }
        return ei(X->il[nl + ns]) + ei(X->nin[nl - ns]) + ei(T->mmI[t][si1][sj1]) + ei(T->mmI[t2][sq1][sp1]);
    }

    // c(p,q) + interior loop of the closing pair (i,j), type t, with n1 / n2
    // unpaired bases on the 5' / 3' side; TR_INF when the shape is not available
    TR_FN int interior(int i, int j, int t, int n1, int n2) const {
        const int p = i + 1 + n1, q = j - 1 - n2;
        if (q - p < 4) return TR_INF;
        if (n1 > 0 && L.up[i + 1] < n1) return TR_INF;
        if (n2 > 0 && L.up[q + 1] < n2) return TR_INF;
        if (!can_pair(p, q)) return TR_INF;
        const int cpq = c[idx(p, q)];
        if (cpq >= TR_INF) return TR_INF;
        return cpq + e_int(n1, n2, t, type(q, p), L.S[i + 1], L.S[j - 1], L.S[p - 1], L.S[q + 1]);
    }
    TR_FN int ml_closing(int i, int j, int t) const { return mlclosing + mlstem(rtype(t), L.S[j - 1], L.S[i + 1]); }
    // L.mat[o]: fold_setup_core.hpp motif_site at start o (fold_common.hpp seq_setup)
    TR_FN bool motif_at(int i, int j) const { return holo && mL > 0 && j - i == mL - 1 && L.mat[i] != 0; }

    // ---- fill: c, fm1, fm of one cell (every shorter span is finished)
    TR_FN void fill_cell(int i, int j) const {
        int cij = TR_INF;
        const int t = type(i, j);
        if (t != 0 && allowed(L, i, j)) {
            int best = TR_INF;
            if (L.up[i + 1] >= j - i - 1) best = hairpin(i, j, t);
            for (int n1 = 0; n1 <= TR_MAXLOOP && i + 1 + n1 < j - 4; n1++) {
                if (n1 > 0 && L.up[i + 1] < n1) break;
                for (int n2 = 0; n1 + n2 <= TR_MAXLOOP; n2++) {
                    const int q = j - 1 - n2;
                    if (q - (i + 1 + n1) < 4 || (n2 > 0 && L.up[q + 1] < n2)) break;
                    best = tmin(best, interior(i, j, t, n1, n2));
                }
            }
            int s = TR_INF;
            for (int k = i + 6; k <= j - 5; k++) {   // fm(i+1, k-1) and fm1(k, j-1) span >= 4
                const int a = fm[idx(i + 1, k - 1)], b = fm1[idx(k, j - 1)];
                if (a < TR_INF && b < TR_INF) s = tmin(s, a + b);
            }
            if (s < TR_INF) best = tmin(best, s + ml_closing(i, j, t));
            if (motif_at(i, j)) best = tmin(best, mextra);
            cij = best;
        }
        c[idx(i, j)] = cij;
        int v = TR_INF;
        if (cij < TR_INF) v = cij + mlstem(t, L.S[i - 1], L.S[j + 1]);
        if (L.up[j] >= 1 && j - 1 - i >= 4) {
            const int b = fm1[idx(i, j - 1)];
            if (b < TR_INF) v = tmin(v, b + mlbase);
        }
        fm1[idx(i, j)] = v;
        int w = TR_INF;
        for (int k = i; k <= j - 4; k++) {
            const int b = k == i ? v : fm1[idx(k, j)];
            if (b >= TR_INF) continue;
            int pre = TR_INF;
            if (k == i || L.up[i] >= k - i) pre = (k - i) * mlbase;
            if (k - 1 - i >= 4) {
                const int a = fm[idx(i, k - 1)];
                if (a < TR_INF) pre = tmin(pre, a);
            }
            if (pre < TR_INF) w = tmin(w, pre + b);
        }
        fm[idx(i, j)] = w;
    }

    // lane `lane` of `lanes`: its share of f5(j)'s pairs (k, j); min with the
    // "j unpaired" form gives f5[j]
    TR_FN int f5_pairs(int j, int lane, int lanes) const {
        int v = TR_INF;
        for (int k = 1 + lane; k + 4 <= j; k += lanes) {
            const int ck = c[idx(k, j)], f = L.f5[k - 1];
            if (ck < TR_INF && f < TR_INF) v = tmin(v, f + ck + ext(type(k, j), k, j));
        }
        return v;
    }

    // ---- traceback: the smallest matching candidate index among this lane's
    // share of item (kind, i, j), or TR_NONE
    TR_FN int candidate(int kind, int i, int j, int lane, int lanes) const {
        if (kind == TI_F5) {   // the smallest k; resolve() tries "j unpaired" first
            if (j <= 0) return TR_NONE;
            const int target = L.f5[j];
            for (int k = 1 + lane; k + 4 <= j; k += lanes) {
                const int ck = c[idx(k, j)], f = L.f5[k - 1];
                if (ck < TR_INF && f < TR_INF && f + ck + ext(type(k, j), k, j) == target) return k;
            }
        } else if (kind == TI_C) {
            const int t = type(i, j);
            const int target = c[idx(i, j)];
            if (lane == 0) {
                if (L.up[i + 1] >= j - i - 1 && hairpin(i, j, t) == target) return TC_HAIRPIN;
                if (motif_at(i, j) && mextra == target) return TC_MOTIF;
            }
            for (int s = lane; s < 31 * 31; s += lanes) {   // n1 ascending, then n2 ascending
                const int n1 = s / 31, n2 = s - 31 * n1;
                if (n1 + n2 <= TR_MAXLOOP && interior(i, j, t, n1, n2) == target) return TC_INT + 32 * n1 + n2;
            }
            const int cl = ml_closing(i, j, t);
            for (int k = i + 6 + lane; k <= j - 5; k += lanes) {
                const int a = fm[idx(i + 1, k - 1)], b = fm1[idx(k, j - 1)];
                if (a < TR_INF && b < TR_INF && a + b + cl == target) return TC_ML + k;
            }
        } else if (kind == TI_FM) {   // k ascending; at each k the unpaired prefix before the fm + fm1 split
            const int target = fm[idx(i, j)];
            for (int k = i + lane; k <= j - 4; k += lanes) {
                const int b = fm1[idx(k, j)];
                if (b >= TR_INF) continue;
                if ((k == i || L.up[i] >= k - i) && (k - i) * mlbase + b == target) return 2 * (k - i);
                if (k - 1 - i >= 4) {
                    const int a = fm[idx(i, k - 1)];
                    if (a < TR_INF && a + b == target) return 2 * (k - i) + 1;
                }
            }
        }
        return TR_NONE;   // fm1 items have no search: resolve() decides them
    }

    TR_FN void push(int kind, int i, int j) const {
        if (L.top >= TR_STACK) return;   // never with consistent tables; keeps the stack in bounds
        int *s = L.stk + 3 * L.top++;
        s[0] = kind;
        s[1] = i;
        s[2] = j;
    }

    // one lane, after the item's candidates are reduced to `win`: mark the
    // structure and push what the winner decomposes into
    TR_FN void resolve(int kind, int i, int j, int win) const {
        if (kind == TI_F5) {
            if (j <= 0) return;
            if (L.up[j] >= 1 && L.f5[j - 1] == L.f5[j]) {
                push(TI_F5, 0, j - 1);
            } else if (win != TR_NONE) {
                push(TI_F5, 0, win - 1);
                push(TI_C, win, j);
            }
        } else if (kind == TI_C) {
            L.out[i - 1] = '(';
            L.out[j - 1] = ')';
            if (win == TR_NONE || win == TC_HAIRPIN) return;
            if (win == TC_MOTIF) {   // the motif's own fold over i..j
                for (int k = 0; k < mL; k++) L.out[i - 1 + k] = L.mpt[k] < 0 ? '.' : (L.mpt[k] > k ? '(' : ')');
            } else if (win >= TC_ML) {
                const int k = win - TC_ML;
                push(TI_FM, i + 1, k - 1);
                push(TI_FM1, k, j - 1);
            } else {
                const int n1 = (win - TC_INT) >> 5, n2 = (win - TC_INT) & 31;
                push(TI_C, i + 1 + n1, j - 1 - n2);
            }
        } else if (kind == TI_FM1) {   // the pair before shortening j
            const int cij = c[idx(i, j)];
            if (cij < TR_INF && cij + mlstem(type(i, j), L.S[i - 1], L.S[j + 1]) == fm1[idx(i, j)]) push(TI_C, i, j);
            else if (j - 1 - i >= 4) push(TI_FM1, i, j - 1);
        } else if (win != TR_NONE) {
            const int k = i + (win >> 1);
            if (win & 1) push(TI_FM, i, k - 1);
            push(TI_FM1, k, j);
        }
    }
};

}  // namespace
}  // namespace adx
