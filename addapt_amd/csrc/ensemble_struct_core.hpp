// The per-lane pieces of ensemble_struct_kernel (ensemble_struct.hip): the
// centroid and the maximum-expected-accuracy (MEA) structure of one sequence
// from its pair-probability matrix.  Free of HIP builtins: the kernel supplies
// the barriers and the LDS atomicMin between them, so a host program can run
// the same code lane by lane (tests/cpp/ensemble_struct_core_probe.cc).  The
// includer may define ES_FN (the kernel: __device__).
//
// Definitions.  P is the symmetric L x L matrix launch_bppm writes (doubles,
// zero diagonal), 0-based here; gamma > 0 is the caller's weight.
//   pu[i]          = 1 - sum_j P[i][j], summed in ascending j, not clamped.
//   centroid       pair (i, j), i < j, iff P[i][j] > 0.5; pairs are taken in
//                  ascending (i, j) and one that shares a base with, or crosses,
//                  a pair already taken is dropped (exact probabilities never
//                  conflict above 1/2, rounded ones might).
//   centroid_dist  = sum_{i<j} (pair in centroid ? 1 - P[i][j] : P[i][j])
//   diversity      = 2 sum_{i<j} P[i][j] (1 - P[i][j])    (vrna_mean_bp_distance)
//   MEA            the nested structure s over pairs with P > 0 that maximises
//                  EA(s) = sum_{i unpaired} pu[i] + sum_{(i,j) in s} w[i][j],  w = 2 gamma P:
//                  M(i,j) = max( M(i,j-1) + pu[j],
//                                max_{i <= k < j, P[k][j] > 0} M(i,k-1) + w[k][j] + M(k+1,j-1) ),
//                  an empty span is 0, mea = M(0, L-1).  Candidate 0 is "j
//                  unpaired", candidate 1 + (k - i) is pair (k, j); the traceback
//                  takes the smallest candidate that equals the cell.
// Everything is FP64.  w is computed in one place (es_weight()) and stored, and a
// candidate (es_value()) is two additions, so no multiply feeds an add: the
// device's FMA contraction has nothing to contract, the traceback reproduces
// the fill bit for bit and a host build reproduces the device.  The one
// product that is summed (diversity) is kept from contracting explicitly.
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef ES_FN
#define ES_FN
#endif

namespace adx {
namespace {

constexpr int ES_LMAX = 255;          // the longest sequence (the kernel holds it to dev_types.hpp NMAX)
constexpr int ES_NT = 256;            // threads per workgroup: one per cell of a diagonal, one per column
static_assert(ES_LMAX < ES_NT, "a diagonal of the MEA fill (<= NMAX cells) takes one pass of the workgroup");
constexpr int ES_NONE = 0x7fffffff;   // no candidate matched
constexpr int ES_STACK = ES_LMAX + 8;   // live intervals are disjoint and hold >= 1 base each
constexpr int ES_WORDS = (ES_LMAX + 31) / 32;

struct EnsLds {
    double pu[ES_LMAX + 1];
    double part[2][ES_NT];                // per-column shares of centroid_dist and diversity
    uint32_t hi[ES_LMAX + 1][ES_WORDS];   // row i: bit j set iff j > i and P[i][j] > 0.5
    int16_t pt[ES_LMAX + 1];              // the centroid's pair table (-1: unpaired)
    int16_t stk[2 * ES_STACK];            // traceback intervals (i, j)
    int cur[2];                           // the popped interval (i < 0: stack empty)
    int top, win, pops, bad;
    uint8_t any[ES_LMAX + 1];             // row i has a bit set
    char out[ES_LMAX + 1];                // the MEA structure
};

// cells of diagonals 0 .. d-1 of an L-base triangle: diagonal d (cells (i, i + d)) holds L - d
constexpr int es_off(int d, int L) { return d * L - d * (d - 1) / 2; }
constexpr size_t es_cells(int L) { return size_t(L) * size_t(L + 1) / 2; }

// w[k][j] as the fill reads it: 2 gamma P where a pair is admitted (P > 0), else negative
ES_FN inline double es_weight(double p, double g2) { return p > 0.0 ? g2 * p : -1.0; }
// one candidate: M(i, k-1) + w[k][j] + M(k+1, j-1), or M(i, j-1) + pu[j] + 0
ES_FN inline double es_value(double left, double w, double inner) { return left + w + inner; }
// the order every reduction's shares are summed in
ES_FN inline double es_sum(const double *v, int n) {
    double s = 0.0;
    for (int k = 0; k < n; k++) s += v[k];
    return s;
}

struct Ens {
    EnsLds &S;
    const double *P;   // L x L, row stride L
    double *M, *W;     // the workgroup's scratch slice: es_cells(L) each, diagonal-major
    int L;

    ES_FN int idx(int i, int j) const { return es_off(j - i, L) + i; }
    ES_FN double m(int i, int j) const { return j < i ? 0.0 : M[idx(i, j)]; }

    // ---- one thread per column c.  P is symmetric, so column c read top to bottom
    // is row c in ascending j, and neighbouring threads read neighbouring doubles.
    // pu[c], row c of the > 1/2 bitmap and of w; raises S.bad on a non-finite entry.
    ES_FN void column(int c, double g2) const {
        double s = 0.0;
        bool bad = false;
        uint32_t any = 0;
        for (int k = 0; k < ES_WORDS; k++) {   // one bitmap word per 32 rows, r ascending throughout
            uint32_t word = 0;
            for (int r = 32 * k; r < 32 * k + 32 && r < L; r++) {
                const double p = P[size_t(r) * L + c];
                s += p;
                if (!(p - p == 0.0)) bad = true;   // inf or NaN
                if (r > c) {
                    W[idx(c, r)] = es_weight(p, g2);
                    if (p > 0.5) word |= 1u << (r & 31);
                }
            }
            S.hi[c][k] = word;
            any |= word;
        }
        S.any[c] = any != 0;
        S.pu[c] = 1.0 - s;
        S.pt[c] = -1;
        S.out[c] = '.';
        if (bad) S.bad = 1;   // every writer writes 1
    }

    // ---- the centroid's conflict filter: may (i, j), i < j, join the pairs in S.pt?
    ES_FN bool compatible(int i, int j) const {
        if (S.pt[i] >= 0 || S.pt[j] >= 0) return false;   // shares a base
        for (int x = i + 1; x < j; x++) {
            const int y = S.pt[x];
            if (y >= 0 && (y < i || y > j)) return false;   // crosses (x, y)
        }
        return true;
    }
    // one lane: the pairs above 1/2 in ascending (i, j)
    ES_FN void centroid_scan() const {
        for (int i = 0; i < L; i++) {
            if (!S.any[i]) continue;
            for (int k = 0; k < ES_WORDS; k++) {
                uint32_t bits = S.hi[i][k];
                while (bits) {
                    const int j = 32 * k + __builtin_ctz(bits);
                    bits &= bits - 1;
                    if (compatible(i, j)) {
                        S.pt[i] = int16_t(j);
                        S.pt[j] = int16_t(i);
                    }
                }
            }
        }
    }

    // one thread per column c: its share (rows above the diagonal, ascending) of
    // centroid_dist and of sum P (1 - P)
    ES_FN void column_stats(int c) const {
#if defined(__clang__)
#pragma clang fp contract(off)   // p * q is rounded before it is added, as a host build does
#endif
        double dist = 0.0, div = 0.0;
        for (int r = 0; r < c; r++) {
            const double p = P[size_t(r) * L + c];
            const double q = 1.0 - p;
            dist += S.pt[r] == c ? q : p;
            const double t = p * q;
            div += t;
        }
        S.part[0][c] = dist;
        S.part[1][c] = div;
    }

    // the larger of `best` and pair candidate (left, w, inner), if w admits the pair
    ES_FN static double better(double best, double w, double left, double inner) {
        const double v = es_value(left, w, inner);
        return (w >= 0.0 && v > best) ? v : best;
    }

    // ---- fill: cell (i, j), i <= j; every cell of a shorter span is final
    ES_FN void fill_cell(int i, int j) const {
        double best = es_value(m(i, j - 1), S.pu[j], 0.0);
        if (i < j) best = better(best, W[idx(i, j)], 0.0, m(i + 1, j - 1));                // k = i: nothing to the left
        if (i < j - 1) best = better(best, W[idx(j - 1, j)], M[idx(i, j - 2)], 0.0);   // k = j - 1: nothing inside
        // in between both spans hold a base, and the three loads of a k wait for
        // nothing: no branch on w stands before M's, so several k are in flight
        for (int k = i + 1; k < j - 1; k++) best = better(best, W[idx(k, j)], M[idx(i, k - 1)], M[idx(k + 1, j - 1)]);
        M[idx(i, j)] = best;
    }

    // ---- traceback: the smallest candidate index among this lane's share of
    // interval (i, j) whose value equals the cell, or ES_NONE
    ES_FN int candidate(int i, int j, int lane, int lanes) const {
        const double target = M[idx(i, j)];
        for (int c = lane; c <= j - i; c += lanes) {
            if (c == 0) {
                if (es_value(m(i, j - 1), S.pu[j], 0.0) == target) return 0;
                continue;
            }
            const int k = i + c - 1;
            const double w = W[idx(k, j)];
            if (w >= 0.0 && es_value(m(i, k - 1), w, m(k + 1, j - 1)) == target) return c;
        }
        return ES_NONE;
    }

    ES_FN void push(int i, int j) const {
        if (j < i || S.top >= ES_STACK) return;   // an empty span; the bound keeps the stack in its array
        S.stk[2 * S.top] = int16_t(i);
        S.stk[2 * S.top + 1] = int16_t(j);
        S.top++;
    }
    // one lane: pop the next interval into S.cur (i = -1: done) and reset the
    // reduction.  Every pop shrinks its span, so a traceback pops at most L
    // intervals; the bound of 2 L ends one that non-finite values misled.
    ES_FN void next_item() const {
        if (S.top == 0 || S.pops >= 2 * L) {
            S.cur[0] = -1;
        } else {
            S.top--;
            S.pops++;
            S.cur[0] = S.stk[2 * S.top];
            S.cur[1] = S.stk[2 * S.top + 1];
        }
        S.win = ES_NONE;
    }
    // one lane, after the interval's candidates are reduced to `win`: mark the
    // pair and push what is left.  No candidate matched (only with non-finite
    // values): the interval stays unpaired.
    ES_FN void resolve(int i, int j, int win) const {
        if (win == ES_NONE) return;
        if (win == 0) {
            push(i, j - 1);
            return;
        }
        const int k = i + win - 1;
        S.out[k] = '(';
        S.out[j] = ')';
        push(i, k - 1);
        push(k + 1, j - 1);
    }
};

}  // namespace
}  // namespace adx
