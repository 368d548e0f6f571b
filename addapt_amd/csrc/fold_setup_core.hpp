// What every kernel that folds a sequence does before its first cell, stated
// once: the folded sequence inside its context (SeqSrc, seq_src), ViennaRNA's
// S1 wrap-around (wrap_pos, wrap_ends), the ligand motif's sites (motif_seq_match,
// motif_site), the constant factor of an interior-loop shape (shape_factor),
// the hairpin entry of the LDS table block (hairpin_dt_index), and the pure
// index helpers these need: cell indexing (off, rowb, colb), pair types (ptype,
// rtype), loop kinds (loop_kind) and the hard-constraint test (allowed).
//
// Free of HIP builtins: fold_common.hpp includes it for the kernels with FS_FN
// defined as __device__ __forceinline__; a host program includes it alone
// (tests/test_fold_setup_core.py does) and runs the same code.
#pragma once

#include <cstdint>

#ifndef __HIPCC__   // dev_types.hpp marks its inline helpers for both sides
#define __host__
#define __device__
#endif
#ifndef FS_FN
#define FS_FN inline
#endif

#include "dev_types.hpp"

namespace adx {
namespace {

// index of the first cell of diagonal dd (cells with j - i = dd >= 4)
FS_FN int off(int dd, int N) { return ((dd - 4) * (2 * N - 3 - dd)) >> 1; }

// Cell indexing (1-based i < j, span j - i >= 4):
//   qbm, cc  diagonal-major  off(j-i) + i - 1   (cells of one anti-diagonal contiguous)
//   qm       row-major       rowb(i) + j - i - 4 (qm[i][*] contiguous)
//   qm1      column-major    colb(j) + i - 1     (qm1[*][j] contiguous)
// so every inner loop of the recurrence walks contiguous LDS at a per-lane base.
FS_FN int rowb(int i, int N) { return (i - 1) * (N - 3) - (((i - 1) * i) >> 1); }
FS_FN int colb(int j) { return ((j - 5) * (j - 4)) >> 1; }

// LDS per-cell table block (L.dt), copied from DevTables / DevScaled
constexpr int DT_MMH = 0;      // [type][x][y] hairpin mismatch
constexpr int DT_MMI = 200;    // [type][x][y] interior mismatch
constexpr int DT_MLS = 400;    // [type][x][y] multiloop stem
constexpr int DT_EXT = 600;    // [type][6][6] exterior stem
constexpr int DT_TAU = 888;    // [type] terminal AU
constexpr int DT_HP = 896;     // [u] hairpin length factor

// Pair type / reversed type / terminal-AU flag without a memory lookup:
// PAIR[a][b] for codes a, b in 0..4 (ViennaRNA types 1..6) packed 3 bits per
// entry of index 5a+b-9 (the canonical pairs sit at 9..23).
constexpr unsigned long long pack_pairs() {
    unsigned long long k = 0;
    k |= 5ull << (3 * (9 - 9));    // A-U
    k |= 1ull << (3 * (13 - 9));   // C-G
    k |= 2ull << (3 * (17 - 9));   // G-C
    k |= 3ull << (3 * (19 - 9));   // G-U
    k |= 6ull << (3 * (21 - 9));   // U-A
    k |= 4ull << (3 * (23 - 9));   // U-G
    return k;
}
FS_FN int ptype(int a, int b) {
    const int idx = 5 * a + b - 9;
    return (idx >= 0 && idx <= 14) ? int((pack_pairs() >> (3 * idx)) & 7ull) : 0;
}
FS_FN int rtype(int t) { return t ? (((t - 1) ^ 1) + 1) : 0; }

// interior-loop shape kinds (dev_types.hpp TermKind; -1 = generic)
constexpr int loop_kind(int n1, int n2) {
    return (n1 == 0 && n2 == 0) ? TK_STK
         : (n1 + n2 == 1) ? TK_B1
         : (n1 == 0 || n2 == 0) ? TK_BUL
         : (n1 == 1 && n2 == 1) ? TK_I11
         : (n1 == 1 && n2 == 2) ? TK_I12
         : (n1 == 2 && n2 == 1) ? TK_I21
         : (n1 == 2 && n2 == 2) ? TK_I22
         : ((n1 == 2 && n2 == 3) || (n1 == 3 && n2 == 2)) ? TK_M23
         : (n1 == 1 || n2 == 1) ? TK_1N
         : -1;
}

// constant factor of shape (u, n1), 0 <= n1 <= u <= 30 (setup_core.hpp addS / fgen):
// generic fgen, bulge / 1xn length factors, the sigma powers of the tabulated loops
FS_FN float shape_factor(const DevScaled *XS, int u, int n1) {
    const int kd = loop_kind(n1, u - n1);
    const float *p = kd < 0 ? XS->fgen + (u - 6) * FG_ROW + n1 - 2
                   : kd == TK_STK ? XS->ctab + CT_FSM + 0
                   : kd == TK_B1 ? XS->ctab + CT_FSM + 1
                   : kd == TK_BUL ? XS->ctab + CT_FB + u
                   : kd == TK_1N ? XS->ctab + CT_F1N + u - 1
                   : kd == TK_I11 ? XS->ctab + CT_FSM + 2
                   : kd == TK_I22 ? XS->ctab + CT_FSM + 4
                   : kd == TK_M23 ? XS->ctab + CT_FSM + 5
                   : XS->ctab + CT_FSM + 3;   // 1x2 / 2x1
    return *p;
}

// L.dt index of the factor a hairpin of u unpaired bases multiplies its length
// factor by: the terminal-AU term (u = 3) or the mismatch of its closing pair
// of type `type` with the neighbours s5 = S[i+1], s3 = S[j-1]
FS_FN int hairpin_dt_index(int u, int type, int s5, int s3) {
    return u == 3 ? DT_TAU + type : DT_MMH + type * 25 + s5 * 5 + s3;
}

// ---------------------------------------------------------------- hard constraints
// flg bits: 1 = 'x' (no pair), 2 = '<' (pairs upstream), 4 = '>' (downstream),
// 8 = '|' (pairs; allowed() does not read it, but the kernels' setup takes any
// flag or partner as "this fold is constrained", and a '|' sets nothing else);
// ptn = enforced partner (0 none); enc = innermost enclosing enforced pair id.
// L: any LDS carve with the byte arrays flg, ptn, enc.
template <class LT>
FS_FN bool allowed(const LT &L, int i, int j) {
    const int fi = L.flg[i], fj = L.flg[j];
    if ((fi | fj) & 1) return false;
    if ((fi & 2) || (fj & 4)) return false;
    const int pi = L.ptn[i], pj = L.ptn[j];
    if (pi) return pi == j;
    if (pj) return pj == i;
    return L.enc[i] == L.enc[j];
}

// ---------------------------------------------------------------- the folded sequence
// The walker's nraw raw bases between its context's `before` (blen bases) and
// `after` strings; no context: blen = 0 and the raw bases alone
struct SeqSrc {
    const uint8_t *bef, *raw, *aft;
    int blen, nraw;
    // where folded 0-based position pp lies (no load: the caller chooses its kind)
    FS_FN const uint8_t *at(int pp) const {
        return pp < blen ? bef + pp : (pp < blen + nraw ? raw + (pp - blen) : aft + (pp - blen - nraw));
    }
    // the base at 1-based k of a fold of length N; 0 outside 1..N
    FS_FN uint8_t code(int k, int N) const { return (k >= 1 && k <= N) ? *at(k - 1) : uint8_t(0); }
};
// of variant V's context, read with plain loads
FS_FN SeqSrc seq_src(const KArgs &ka, const DevVariant &V, const uint8_t *raw) {
    SeqSrc s{nullptr, raw, nullptr, 0, ka.Nraw};
    if (V.ctx >= 0) {
        s.bef = ka.ctx_seq + ka.ctx_off[4 * V.ctx + 0];
        s.blen = ka.ctx_off[4 * V.ctx + 1];
        s.aft = ka.ctx_seq + ka.ctx_off[4 * V.ctx + 2];
    }
    return s;
}

// ViennaRNA's S1 wrap-around: position 0 reads base N, position N + 1 base 1
// (only cells (1, j) and (i, N) see them, as dangles no used value takes) ...
FS_FN int wrap_pos(int k, int N) { return k == 0 ? N : (k == N + 1 ? 1 : k); }
// ... and the same on a stored sequence L.S[1..N] (one thread, between barriers)
template <class LT>
FS_FN void wrap_ends(LT &L, int N) {
    L.S[0] = L.S[N];
    L.S[N + 1] = L.S[1];
}

// ---------------------------------------------------------------- motif sites
// does S[o .. o + mL) spell the motif's bases?
FS_FN bool motif_seq_match(const uint8_t *S, const uint8_t *mcode, int mL, int o) {
    bool ok = true;
    for (int k = 0; k < mL && ok; k++) ok = S[o + k] == mcode[k];
    return ok;
}
// Is the motif formable with its outer pair at (o, o + mL - 1)?  (oracle/fold.c
// motif_at: the sequence matches, the constraint admits every motif pair and
// every unpaired motif base.)  mpt: partner offset or -1; L: S, up and allowed()'s arrays
template <class LT>
FS_FN bool motif_site(const LT &L, const uint8_t *mcode, const int8_t *mpt, int mL, int o) {
    bool ok = motif_seq_match(L.S, mcode, mL, o);
    for (int k = 0; k < mL && ok; k++) {
        const int pk = mpt[k];
        if (pk < 0) ok = L.up[o + k] >= 1;
        else if (pk > k) ok = allowed(L, o + k, o + pk);
    }
    return ok;
}

}  // namespace
}  // namespace adx
