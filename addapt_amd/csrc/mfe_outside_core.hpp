// The per-lane pieces of mfe_subopt_kernel (mfe_subopt.hip): the MFE outside
// pass over mfe_trace_core.hpp's inside tables, the energy of the best structure
// through every pair, the outside traceback and Zuker's selection of suboptimal
// structures.  Free of HIP builtins, as mfe_trace_core.hpp: the kernel supplies
// the barriers and the LDS atomicMin between them, so a host program can run the
// same code lane by lane against the CPU oracle.  Trace's fill_cell, e_int,
// interior, ml_closing, can_pair and motif_at are used as they stand.
//
// Each outside table holds the minimum energy of everything OUTSIDE a cell, given
// that the cell is used in that role (TR_INF: no structure uses it so):
//   co(i,j)    the pair (i,j)           fm1o(i,j)  the cell as fm1(i,j)
//   fmo(i,j)   the cell as fm(i,j)      f3[i]      the exterior suffix i..N (f5's mirror)
// Descending diagonals, one barrier per diagonal; within a cell fmo, then fm1o,
// then co: everything else a cell reads lies on a longer span.
//   th(i,j) = c(i,j) + co(i,j), the best structure that holds the pair (i,j): the
// fold under that forced pair.  On a holo variant a pair of the motif's own fold
// strictly inside a formed site (o, o+mL-1) also takes co(site) + mextra (the
// closing pair carries the motif through c).
#pragma once

#include "mfe_trace_core.hpp"

namespace adx {
namespace {

// outside item kinds, next to mfe_trace_core.hpp's TI_F5 .. TI_FM1
constexpr int TI_CO = 4, TI_FM1O = 5, TI_FMO = 6, TI_F3 = 7;
// Candidate indices, growing in the search order:
//   TI_CO    exterior; interior loops closed by (p,q) (n1 = i-p-1 ascending, then
//            n2 = q-j-1 ascending); the multiloop stem
//   TI_FM1O  j+1 unpaired; the closing pairs (p, j+1), p ascending; the fm(i',j)
//            it ends, i' ascending, at each i' the unpaired prefix before the fm prefix
//   TI_FMO   the closing pairs (i-1, q), q ascending; the longer fm(i,j'), j' ascending
//   TI_F3    the pairs (i, l), l ascending (resolve() tries "i unpaired" first)
constexpr int OC_EXT = 0, OC_INT = 1, OC_ML = OC_INT + 32 * 32;
constexpr int O1_UNP = 0, O1_CLOSE = 1, O1_FM = O1_CLOSE + TR_NP;
constexpr int OM_CLOSE = 0, OM_FM = TR_NP;
constexpr unsigned long long SO_NOKEY = ~0ull;   // no pair left

struct Outside {
    const Trace &M;
    int *co, *fm1o, *fmo, *th;   // the workgroup's scratch slice, after M.c / M.fm / M.fm1
    int *f3;                     // [TR_NP], f3[N + 1] = 0

    // lane `lane` of `lanes`: its share of f3(i)'s pairs (i, l); min with the
    // "i unpaired" form gives f3[i]
    TR_FN int f3_pairs(int i, int lane, int lanes) const {
        int v = TR_INF;
        for (int l = i + 4 + lane; l <= M.N; l += lanes) {
            const int cl = M.c[M.idx(i, l)], f = f3[l + 1];
            if (cl < TR_INF && f < TR_INF) v = tmin(v, f + cl + M.ext(M.type(i, l), i, l));
        }
        return v;
    }

    // co(p,q) + the interior loop of the closing pair (p,q) around (i,j), with n1 / n2
    // unpaired bases on the 5' / 3' side (Trace::interior seen from the inner pair);
    // TR_INF when the shape is not available.  co is TR_INF where (p,q) cannot pair
    TR_FN int outer(int i, int j, int n1, int n2) const {
        const int p = i - 1 - n1, q = j + 1 + n2;
        if (p < 1 || q > M.N) return TR_INF;
        if (n1 > 0 && M.L.up[p + 1] < n1) return TR_INF;
        if (n2 > 0 && M.L.up[j + 1] < n2) return TR_INF;
        const int o = co[M.idx(p, q)];
        if (o >= TR_INF) return TR_INF;
        return o + M.e_int(n1, n2, M.type(p, q), M.type(j, i), M.L.S[p + 1], M.L.S[q - 1], M.L.S[i - 1], M.L.S[j + 1]);
    }
    // fm(i',j) = pre + fm1(i,j): fill_cell's prefix term
    TR_FN int pre_unp(int ip, int i) const { return (ip == i || M.L.up[ip] >= i - ip) ? (i - ip) * M.mlbase : TR_INF; }
    TR_FN int pre_fm(int ip, int i) const { return i - 1 - ip >= 4 ? M.fm[M.idx(ip, i - 1)] : TR_INF; }
    TR_FN int closed(int p, int q, int inside) const {   // co(p,q) + ml_closing + the rest of its multiloop
        const int o = co[M.idx(p, q)];
        return (o < TR_INF && inside < TR_INF) ? o + inside + M.ml_closing(p, q, M.type(p, q)) : TR_INF;
    }
    TR_FN int sum(int a, int b) const { return (a < TR_INF && b < TR_INF) ? a + b : TR_INF; }

    // ---- fill: fmo, fm1o, co of one cell (every longer span is finished)
    TR_FN void outside_cell(int i, int j) const {
        const int N = M.N, at = M.idx(i, j);
        int vm = TR_INF;
        if (i >= 2)
            for (int q = j + 6; q <= N; q++) vm = tmin(vm, closed(i - 1, q, M.fm1[M.idx(j + 1, q - 1)]));
        for (int jp = j + 5; jp <= N; jp++) vm = tmin(vm, sum(fmo[M.idx(i, jp)], M.fm1[M.idx(j + 1, jp)]));
        fmo[at] = vm;
        int v1 = TR_INF;
        if (j + 1 <= N) {
            if (M.L.up[j + 1] >= 1) v1 = sum(fm1o[M.idx(i, j + 1)], M.mlbase);
            for (int p = 1; p <= i - 6; p++) v1 = tmin(v1, closed(p, j + 1, M.fm[M.idx(p + 1, i - 1)]));
        }
        for (int ip = 1; ip <= i; ip++) {
            const int o = ip == i ? vm : fmo[M.idx(ip, j)];
            if (o < TR_INF) v1 = tmin(v1, sum(o, tmin(pre_unp(ip, i), pre_fm(ip, i))));
        }
        fm1o[at] = v1;
        int vc = TR_INF;
        const int t = M.type(i, j);
        if (t != 0 && allowed(M.L, i, j)) {
            vc = sum(sum(M.L.f5[i - 1], f3[j + 1]), M.ext(t, i, j));
            for (int n1 = 0; n1 <= TR_MAXLOOP && i - 1 - n1 >= 1; n1++) {
                if (n1 > 0 && M.L.up[i - n1] < n1) break;
                for (int n2 = 0; n1 + n2 <= TR_MAXLOOP && j + 1 + n2 <= N; n2++) {
                    if (n2 > 0 && M.L.up[j + 1] < n2) break;
                    vc = tmin(vc, outer(i, j, n1, n2));
                }
            }
            vc = tmin(vc, sum(v1, M.mlstem(t, M.L.S[i - 1], M.L.S[j + 1])));
        }
        co[at] = vc;
    }

    // the formed motif site o whose own fold holds (i,j) strictly inside, with the
    // smallest value co(site) + mextra below `below`; 0: none.  v: that value
    TR_FN int site_through(int i, int j, int below, int &v) const {
        int site = 0;
        v = below;
        if (!M.holo || M.mL <= 0) return 0;
        for (int o = j - M.mL + 2 > 1 ? j - M.mL + 2 : 1; o <= i - 1; o++) {
            if (!M.L.mat[o] || M.L.mpt[i - o] != j - o) continue;
            const int s = sum(co[M.idx(o, o + M.mL - 1)], M.mextra);
            if (s < v) {
                v = s;
                site = o;
            }
        }
        return site;
    }
    // ---- th of one cell (co is finished everywhere)
    TR_FN void through_cell(int i, int j) const {
        const int at = M.idx(i, j);
        int v;
        site_through(i, j, sum(M.c[at], co[at]), v);
        th[at] = v;
    }

    // ---- selection.  Lane `lane` of `lanes`: the number of its cells within `limit` ...
    TR_FN int count_within(int limit, int lane, int lanes) const {
        int n = 0;
        for (int d = 4; d <= M.N - 1; d++)
            for (int r = lane; r < M.N - d; r += lanes) n += th[off(d, M.N) + r] <= limit ? 1 : 0;
        return n;
    }
    // ... and the first of them by (th ascending, i ascending, j ascending) as a key
    // the kernel reduces by min; a marked pair holds TR_INF
    TR_FN unsigned long long lane_best(int limit, int lane, int lanes) const {
        unsigned long long best = SO_NOKEY;
        for (int d = 4; d <= M.N - 1; d++)
            for (int r = lane; r < M.N - d; r += lanes) {
                const int v = th[off(d, M.N) + r];
                if (v > limit || v >= TR_INF) continue;
                const unsigned long long key = (static_cast<unsigned long long>(static_cast<uint32_t>(v + 0x40000000)) << 32) |
                                               static_cast<uint32_t>(((r + 1) << 16) | (r + 1 + d));
                best = key < best ? key : best;
            }
        return best;
    }
    TR_FN static int key_i(unsigned long long key) { return int((key >> 16) & 0xffff); }
    TR_FN static int key_j(unsigned long long key) { return int(key & 0xffff); }

    // one lane, L.out all '.' and the stack empty: the first items of seed (i,j).
    // Through the pair itself: inside and outside of (i,j).  Through a motif site:
    // the motif's fold at the site and the outside of the site cell
    TR_FN void seed_begin(int i, int j) const {
        const int at = M.idx(i, j);
        int v;
        const int o = site_through(i, j, sum(M.c[at], co[at]), v);
        if (o == 0) {
            M.push(TI_CO, i, j);
            M.push(TI_C, i, j);
        } else {
            for (int k = 0; k < M.mL; k++) M.L.out[o - 1 + k] = M.L.mpt[k] < 0 ? '.' : (M.L.mpt[k] > k ? '(' : ')');
            M.push(TI_CO, o, o + M.mL - 1);
        }
    }
    // one lane, after the trace: every pair of L.out leaves the selection.
    // The (empty) item stack serves the bracket matching
    TR_FN void mark_structure() const {
        int sp = 0;
        for (int k = 1; k <= M.N; k++) {
            if (M.L.out[k - 1] == '(') M.L.stk[sp++] = k;
            else if (M.L.out[k - 1] == ')' && sp > 0) th[M.idx(M.L.stk[--sp], k)] = TR_INF;
        }
    }

    // ---- traceback: mfe_trace_core.hpp's for the inside kinds; the smallest matching
    // candidate index among this lane's share of an outside item, or TR_NONE
    TR_FN int candidate(int kind, int i, int j, int lane, int lanes) const {
        const int N = M.N;
        if (kind < TI_CO) return M.candidate(kind, i, j, lane, lanes);
        if (kind == TI_F3) {
            if (i > N) return TR_NONE;
            const int target = f3[i];
            for (int l = i + 4 + lane; l <= N; l += lanes)
                if (sum(sum(M.c[M.idx(i, l)], f3[l + 1]), M.ext(M.type(i, l), i, l)) == target) return l;
            return TR_NONE;
        }
        const int at = M.idx(i, j);
        if (kind == TI_CO) {
            const int target = co[at], t = M.type(i, j);
            if (lane == 0 && sum(sum(M.L.f5[i - 1], f3[j + 1]), M.ext(t, i, j)) == target) return OC_EXT;
            for (int s = lane; s < 31 * 31; s += lanes) {
                const int n1 = s / 31, n2 = s - 31 * n1;
                if (n1 + n2 <= TR_MAXLOOP && outer(i, j, n1, n2) == target) return OC_INT + 32 * n1 + n2;
            }
            if (lane == 0 && sum(fm1o[at], M.mlstem(t, M.L.S[i - 1], M.L.S[j + 1])) == target) return OC_ML;
        } else if (kind == TI_FM1O) {
            const int target = fm1o[at];
            if (j + 1 <= N) {
                if (lane == 0 && M.L.up[j + 1] >= 1 && sum(fm1o[M.idx(i, j + 1)], M.mlbase) == target) return O1_UNP;
                for (int p = 1 + lane; p <= i - 6; p += lanes)
                    if (closed(p, j + 1, M.fm[M.idx(p + 1, i - 1)]) == target) return O1_CLOSE + p;
            }
            for (int ip = 1 + lane; ip <= i; ip += lanes) {
                const int o = fmo[M.idx(ip, j)];
                if (o >= TR_INF) continue;
                if (sum(o, pre_unp(ip, i)) == target) return O1_FM + 2 * ip;
                if (sum(o, pre_fm(ip, i)) == target) return O1_FM + 2 * ip + 1;
            }
        } else {   // TI_FMO
            const int target = fmo[at];
            if (i >= 2)
                for (int q = j + 6 + lane; q <= N; q += lanes)
                    if (closed(i - 1, q, M.fm1[M.idx(j + 1, q - 1)]) == target) return OM_CLOSE + q;
            for (int jp = j + 5 + lane; jp <= N; jp += lanes)
                if (sum(fmo[M.idx(i, jp)], M.fm1[M.idx(j + 1, jp)]) == target) return OM_FM + jp;
        }
        return TR_NONE;
    }

    TR_FN void mark(int p, int q) const {
        M.L.out[p - 1] = '(';
        M.L.out[q - 1] = ')';
    }
    // one lane, after the item's candidates are reduced to `win`: mark the pairs it
    // passes and push the inside and outside items the winner decomposes into
    TR_FN void resolve(int kind, int i, int j, int win) const {
        if (kind < TI_CO) {
            M.resolve(kind, i, j, win);
        } else if (kind == TI_F3) {
            if (i > M.N) return;
            if (M.L.up[i] >= 1 && f3[i + 1] == f3[i]) {
                M.push(TI_F3, i + 1, 0);
            } else if (win != TR_NONE) {
                M.push(TI_F3, win + 1, 0);
                M.push(TI_C, i, win);
            }
        } else if (win == TR_NONE) {   // never with consistent tables
        } else if (kind == TI_CO) {
            if (win == OC_EXT) {
                M.push(TI_F5, 0, i - 1);
                M.push(TI_F3, j + 1, 0);
            } else if (win == OC_ML) {
                M.push(TI_FM1O, i, j);
            } else {
                const int p = i - 1 - ((win - OC_INT) >> 5), q = j + 1 + ((win - OC_INT) & 31);
                mark(p, q);
                M.push(TI_CO, p, q);
            }
        } else if (kind == TI_FM1O) {
            if (win == O1_UNP) {
                M.push(TI_FM1O, i, j + 1);
            } else if (win < O1_FM) {
                const int p = win - O1_CLOSE;
                mark(p, j + 1);
                M.push(TI_CO, p, j + 1);
                M.push(TI_FM, p + 1, i - 1);
            } else {
                const int ip = (win - O1_FM) >> 1;
                M.push(TI_FMO, ip, j);
                if ((win - O1_FM) & 1) M.push(TI_FM, ip, i - 1);
            }
        } else if (win < OM_FM) {
            const int q = win - OM_CLOSE;
            mark(i - 1, q);
            M.push(TI_CO, i - 1, q);
            M.push(TI_FM1, j + 1, q - 1);
        } else {
            const int jp = win - OM_FM;
            M.push(TI_FMO, i, jp);
            M.push(TI_FM1, j + 1, jp);
        }
    }
};

}  // namespace
}  // namespace adx
