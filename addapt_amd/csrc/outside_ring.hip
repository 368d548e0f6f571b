// gfx950 outside pass (base-pair probabilities, BASELINE config 4: N = 150)
// with lanes = cells, for the folds pf_ring_kernel (pf_ring.hip) leaves in the
// walker's table slot -- the equations of outside_cells.hip (the adjoint of the
// inside recursions in gather form, descending span order), with the LDS
// carved for lengths where outside_cells' four cell tables (4 x 43 KB at
// N = 150) do not fit:
//
//   * Y = qmb + X stays in LDS, ROW-major only (43 KB).  The r2 sum walks a
//     column of Y: lane (i, j) reads Y(i-u, j) at rowb(i-u) + d + u - 4, a
//     per-lane base that moves by an add per term (consecutive rows start in
//     distinct banks, so the reads stay conflict-free);
//   * the inside tables qm1 and qm are read from the slot, where pf_ring_kernel
//     keeps them DIAGONAL-major: with lanes = consecutive cells, the term
//     qm1(j+1, j+5+t) of every lane lies on diagonal t+4 and qm(i-u, i-1) on
//     diagonal u-1, so each term is one coalesced global load (L2-resident:
//     86 KB per fold);
//   * three lane-sets per diagonal (N - 4 <= 192): three finalize waves, three
//     record sets, the multiloop items one per M wave.
//
// Covered: pf_ring contexts (unconstrained folds with pair terms, N <= the
// LDS limit); dispatch.hip chooses it with the inside kernel.
//
// What it shares with outside_cells.hip is in outside_common.hpp; here: the
// multiloop items' assignment (massign), the traits (OrK), one part of an item
// (or_mpart) and the kernel (prologue, setup calls, the B switch, the M sweep,
// epilogue).
#include "outside_common.hpp"

OX_STAMP_TABLE(g_stamps_or, adx_debug_stamps_outside_ring)

namespace adx {
namespace {

constexpr int OR_SETS = 3;
constexpr int OR_NB = 8;              // interior-loop waves 0-7 (records on 7); multiloop sums on 8-15
constexpr int OR_NMIN = 101, OR_NMAX = 190;

// Multiloop-sum work of a diagonal with nls lane-sets: items qmb(ls) and
// r2(ls), each cut into np parts (split-point ranges), one or two parts per M wave
// (8-15; their global loads wait on L2, so the sums get as many waves as the
// interior loops).  Code: 0 = none, else 1 | isq << 1 | ls << 2 | pi << 4 | (np-1) << 6.
__host__ __device__ constexpr int mcode(bool isq, int ls, int pi, int np) {
    return 1 | (isq ? 2 : 0) | (ls << 2) | (pi << 4) | ((np - 1) << 6);
}
__device__ __forceinline__ int massign(int nls, int w) {
    constexpr int Q = 1, R = 0;
    if (nls >= 3) {
        // wave 11 takes two parts: qmb of lane-set 2 (the shortest) and r2 of
        // lane-set 0 (slot 3 = 11 - 8: the M loop runs massign(nls, w - 8) as a
        // wave's second part); r2 of lane-set 1 split over 12 and 13 (round 5:
        // one wave carried it whole, 123 terms where the others had <= 71)
        switch (w) {
            case 8: return mcode(Q, 0, 0, 2);
            case 9: return mcode(Q, 0, 1, 2);
            case 10: return mcode(Q, 1, 0, 1);
            case 11: return mcode(Q, 2, 0, 1);
            case 3: return mcode(R, 0, 0, 1);
            case 12: return mcode(R, 1, 0, 2);
            case 13: return mcode(R, 1, 1, 2);
            case 14: return mcode(R, 2, 0, 2);
            case 15: return mcode(R, 2, 1, 2);
            default: return 0;
        }
    }
    if (nls == 2) {
        switch (w) {
            case 8: return mcode(Q, 0, 0, 2);
            case 9: return mcode(Q, 0, 1, 2);
            case 10: return mcode(Q, 1, 0, 1);
            case 11: return mcode(R, 0, 0, 2);
            case 12: return mcode(R, 0, 1, 2);
            case 13: return mcode(R, 1, 0, 3);
            case 14: return mcode(R, 1, 1, 3);
            case 15: return mcode(R, 1, 2, 3);
            default: return 0;
        }
    }
    if (nls == 1) {
        if (w >= 8 && w < 12) return mcode(Q, 0, w - 8, 4);
        if (w >= 12 && w < 16) return mcode(R, 0, w - 12, 4);
    }
    return 0;
}

struct OrK {
    static constexpr int SETS = OR_SETS;    // lane-sets per diagonal (N - 4 <= 192 cells)
    static constexpr int FB = OR_NB;        // interior-loop block waves, summed in the finalize
    static constexpr int NMLP = OX_NW;      // mlp slots per parity: one per wave (massign's slots)
    static constexpr int SLACK = 64;        // zeroed floats after Y
    static constexpr bool COLS = false;     // Y row-major only; qm1 / qm stay in the slot
    // window row: outer a from i-31 (zero pad in front)
    __host__ __device__ static int row_len(int N) { return ((N + OX_PAD + 4) + 3) & ~3; }
    // the lane's qmb and r2 of lane-set fl: the parts of this lane-set's items (massign)
    __device__ __forceinline__ static void msums(const float *mp, int nle, int fl, float &qmbv, float &r2) {
        qmbv = 0.f;
        r2 = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < OX_NW; w2++) {
            const int c = massign(nle, w2);
            if (c && ((c >> 2) & 3) == fl) {
                if (c & 2) qmbv += mp[w2 * WAVE];
                else r2 += mp[w2 * WAVE];
            }
        }
    }
};

// One part of a multiloop-sum item of diagonal d (massign): qmb or r2 of
// lane-set ls, split points pi / np of the lane-set's longest range; q1g / qmg:
// the slot's qm1 / qm (diagonal-major).  Not force-inlined: left to the inliner
// (which inlines both calls) the M loops come out as they always were, forced
// early they cost config 4 0.4 % (profiles/outside_common_ab.txt)
__device__ inline float or_mpart(const OxL &L, const float *q1g, const float *qmg, int N, int lane, int d,
                                          bool isq, int ls, int pi, int np) {
    int i = 1 + ls * WAVE + lane;
    const int ilast = min(N - d, (ls + 1) * WAVE);
    if (i > N - d) i = N - d;
    const int j = i + d;
    float acc = 0.f, acc1 = 0.f;
    constexpr int MB = 8;
    // both sums read the slot in batches of MB terms, four batches in flight
    // (a batch's global loads are issued three batches before it is summed)
    if (isq) {
        // qmb: t = 0 .. N-j-5: Y(i, j+5+t) = YR[rowb(i) + d + 1 + t] (LDS),
        // qm1(j+1, j+5+t) on diagonal t+4 at position j (slot, coalesced)
        const int lim = N - j - 5;
        const int Tq = N - (1 + ls * WAVE + d) - 4;
        const int ta = (Tq * pi) / np, tb = (Tq * (pi + 1)) / np;
        const float *py = L.yr + rowb(i, N) + d + 1;
        auto ld = [&](float (&q)[MB], int t) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < MB; k++) q[k] = q1g[off(min(t + k, N - 5) + 4, N) + j];
        };
        auto use = [&](const float (&q)[MB], int t) __attribute__((always_inline)) {
            float yv[MB];
#pragma unroll
            for (int k = 0; k < MB; k++) yv[k] = py[t + k];
#pragma unroll
            for (int k = 0; k < MB; k += 2) {
                acc = fmaf((t + k <= lim && t + k < tb) ? yv[k] : 0.f, q[k], acc);
                acc1 = fmaf((t + k + 1 <= lim && t + k + 1 < tb) ? yv[k + 1] : 0.f, q[k + 1], acc1);
            }
        };
        float qa[MB], qb[MB], qc[MB], qd[MB];
        int t = ta;
        if (t < tb) ld(qa, t);
        if (t + MB < tb) ld(qb, t + MB);
        if (t + 2 * MB < tb) ld(qc, t + 2 * MB);
        while (t < tb) {
            if (t + 3 * MB < tb) ld(qd, t + 3 * MB);
            use(qa, t);
            t += MB;
            if (t >= tb) break;
            if (t + 3 * MB < tb) ld(qa, t + 3 * MB);
            use(qb, t);
            t += MB;
            if (t >= tb) break;
            if (t + 3 * MB < tb) ld(qb, t + 3 * MB);
            use(qc, t);
            t += MB;
            if (t >= tb) break;
            if (t + 3 * MB < tb) ld(qc, t + 3 * MB);
            use(qd, t);
            t += MB;
        }
    } else {
        // r2: u = 5 .. i-1 (ip = i - u): Y(i-u, j) = YR[rowb(i-u) + d + u - 4]
        // (LDS), qm(i-u, i-1) on diagonal u-1 at position i-u-1 (slot, coalesced)
        const int lim = i - 1;
        const int Tr = ilast - 5;
        const int ua = 5 + (Tr * pi) / np, ub = 5 + (Tr * (pi + 1)) / np;
        auto ld = [&](float (&q)[MB], int u) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < MB; k++) {
                const int uu = u + k;
                const bool ok = uu <= lim && uu < ub;
                q[k] = qmg[off(min(uu, N - 1) - 1, N) + (ok ? i - uu - 1 : 0)];
            }
        };
        auto use = [&](const float (&q)[MB], int u) __attribute__((always_inline)) {
            // Y(i-u-k, j): the row base moves by (i - u - k - N + 3) per term
            const int ip0 = max(i - u, 1);
            const int a0 = rowb(ip0, N) + d + u - 4;
            const int D0 = i - u - N + 3;
            float yv[MB];
#pragma unroll
            for (int k = 0; k < MB; k++) {
                const int uu = u + k;
                const bool ok = uu <= lim && uu < ub;
                const int a = a0 + k * D0 - (k * (k - 1)) / 2;
                yv[k] = L.yr[ok ? a : a0];
                yv[k] = ok ? yv[k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < MB; k += 2) {
                acc = fmaf(yv[k], q[k], acc);
                acc1 = fmaf(yv[k + 1], q[k + 1], acc1);
            }
        };
        float qa[MB], qb[MB], qc[MB], qd[MB];
        int u = ua;
        if (u < ub) ld(qa, u);
        if (u + MB < ub) ld(qb, u + MB);
        if (u + 2 * MB < ub) ld(qc, u + 2 * MB);
        while (u < ub) {
            if (u + 3 * MB < ub) ld(qd, u + 3 * MB);
            use(qa, u);
            u += MB;
            if (u >= ub) break;
            if (u + 3 * MB < ub) ld(qa, u + 3 * MB);
            use(qb, u);
            u += MB;
            if (u >= ub) break;
            if (u + 3 * MB < ub) ld(qb, u + 3 * MB);
            use(qc, u);
            u += MB;
            if (u >= ub) break;
            if (u + 3 * MB < ub) ld(qc, u + 3 * MB);
            use(qd, u);
            u += MB;
        }
    }
    return acc + acc1;
}

// One workgroup per (walker, outside variant).  pair_p: [W][n_pairs].
__global__ void __launch_bounds__(OX_NT, 1)
outside_ring_kernel(KArgs ka, const DevScaled *__restrict__ XS, const uint8_t *seqs, int W, const int *mask,
                    double *pair_p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int w = blockIdx.x / ka.n_bvars, bv = blockIdx.x % ka.n_bvars;
    if (w >= W) return;
    if (mask && mask[w] != 1) return;
    const int v = ka.bvars[bv];
    const DevVariant V = ka.variants[v];
    const int N = uni(V.N);
    const OxLay<OrK> Y(N);
    const OxL L = ox_view<OrK>(smem, Y);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = uni(tid / WAVE);
    OX_STAMP_LOCALS

    // ---- the proposal's inside tables (pf_ring_kernel's slot: qb, qm, qm1
    // diagonal-major, q5), at the variant's groups2 position
    const size_t B = 3 * size_t(ka.cells) + size_t(ka.Nmax) + 2;
    const size_t go = size_t(ka.bvar_slot[bv]) * B;
    const int cur = ka.cur_slot[w];
    const float *src = ka.tab + size_t(w) * 2 * ka.tab_slot + size_t(1 - cur) * ka.tab_slot + go;
    const size_t Cs = size_t(ka.cells);
    const float *qmg = src + Cs, *q1g = src + 2 * Cs;

    ox_setup(L, ka, XS, V, seqs, w, src + 3 * Cs, N, tid);
    const OxC c{N, src, XS, L.q5[N], XS->mlbase_sig, XS->mlclosing, XS->pwml[1],
                V.motif != 0 && XS->motif_len > 0, XS->motif_len};
    ox_pair_list(L, ka, bv, tid);
    // the exterior factors G(i, j) = qb(i,j) ext(i,j), column-major, in the Y
    // region (zeroed after the exterior adjoint)
    float *G = L.yr;
    for (int k = tid; k < Y.C + OrK::SLACK; k += OX_NT) {
        if (k >= Y.C) {
            G[k] = 0.f;
            continue;
        }
        const int jc = inv_colb(k), ic = k - colb(jc) + 1;
        G[k] = ox_ext_cell(L, src, N, ic, jc);
    }
    __syncthreads();
    OSTAMP(0);   // loads + the exterior-factor pass

    // ---- the exterior adjoint on wave 0 (three lane-sets of m), the motif sites
    // on wave 1, the window and the rank lists on the others
    if (wid == 0) ox_ext_adjoint<OR_SETS>(L, G, XS, N, lane);
    if (c.motif && wid == 1) ox_motif_sites(L, XS, N, c.mL, lane);
    if (wid >= 2) ox_window_ranks(L, N, wid, lane);
    __syncthreads();
    for (int k = tid; k < Y.C + OrK::SLACK; k += OX_NT) L.yr[k] = 0.f;   // G's region: Y from here on
    __syncthreads();
    OSTAMP(1);   // exterior adjoint, window, rank lists

    Pend<OR_SETS> pnext;   // the record wave's state (OxFin)
    Idx<OR_SETS> inext;
    pnext.cnt = 0;
    inext.cnt = 0;
    if (wid == OX_RW) rec_prime<OR_SETS>(L, *ka.T, N, lane, pnext, inext);
    __syncthreads();
    const OxFin<OrK> fin{L, c, *ka.T, lane, pnext, inext};

    if (wid < OR_NB) {
        switch (wid) {
            // loop sizes in blocks of about equal cost (a size >= 6: 3 reads for its
            // special shapes + one per 4 generic ones per lane-set; sizes <= 5 ~3 per
            // shape), a little less on the finalize (0-2) and record (7) waves
            case 0: b_sweep<OR_SETS, 28, 20, 13, 0, -1>(L, N, lane, std::integral_constant<int, 0>{}, fin OX_STP_ARGS); break;
            case 1: b_sweep<OR_SETS, 27, 21, 1, 7, -1>(L, N, lane, std::integral_constant<int, 1>{}, fin OX_STP_ARGS); break;
            case 2: b_sweep<OR_SETS, 26, 22, 12, 6, -1>(L, N, lane, std::integral_constant<int, 2>{}, fin OX_STP_ARGS); break;
            case 3: b_sweep<OR_SETS, 4, 19, 14, -1, -1>(L, N, lane, std::integral_constant<int, 3>{}, fin OX_STP_ARGS); break;
            case 4: b_sweep<OR_SETS, 3, 24, 16, 9, -1>(L, N, lane, std::integral_constant<int, 4>{}, fin OX_STP_ARGS); break;
            case 5: b_sweep<OR_SETS, 30, 25, 18, 11, -1>(L, N, lane, std::integral_constant<int, 5>{}, fin OX_STP_ARGS); break;
            case 6: b_sweep<OR_SETS, 5, 23, 15, 8, -1>(L, N, lane, std::integral_constant<int, 6>{}, fin OX_STP_ARGS); break;
            default: b_sweep<OR_SETS, 29, 2, 17, 10, -1>(L, N, lane, std::integral_constant<int, 7>{}, fin OX_STP_ARGS); break;   // wave 7
        }
    } else for (int d = N - 1; d >= 3; d--) {
        const int nls = d >= 4 ? (N - d + WAVE - 1) / WAVE : 0;
        const int par = d & 1;
        if (d >= 4) {
            // ---------------- M: the multiloop-sum parts of diagonal d on this wave
            const int m1 = massign(nls, wid);
            if (m1) L.mlp[(par * OX_NW + wid) * WAVE + lane] = or_mpart(L, q1g, qmg, N, lane, d, (m1 & 2) != 0, (m1 >> 2) & 3, (m1 >> 4) & 3, (m1 >> 6) + 1);
            const int m2 = massign(nls, wid - OR_NB);   // a second part, in the slot of B wave wid - 8
            if (m2) L.mlp[(par * OX_NW + wid - OR_NB) * WAVE + lane] = or_mpart(L, q1g, qmg, N, lane, d, (m2 & 2) != 0, (m2 >> 2) & 3, (m2 >> 4) & 3, (m2 >> 6) + 1);
        }
        OSTAMP(4);   // M sums
        lds_barrier();
        OSTAMP(6);   // barrier
    }
    OX_STAMP_FLUSH(g_stamps_or, wid, lane)
    ox_write_pairs(L, ka, c, pair_p + size_t(w) * ka.n_pairs, bv, tid);
}

}  // namespace

// LDS bytes of the ring outside kernel for this workload (0: not covered)
size_t outside_ring_lds(const KArgs &ka) {
    if (ka.Nmax < OR_NMIN || ka.Nmax > OR_NMAX || ka.n_pairs > OX_MAXP) return 0;
    return ox_lds_bytes<OrK>(ka.Nmax);
}

hipError_t launch_outside_ring(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, double *pair_p,
                               hipStream_t stream) {
    const size_t lds = outside_ring_lds(ka);
    if (lds == 0 || !ka.tab || !ka.bvar_slot) return hipErrorInvalidValue;
    hipError_t e = configure_dynamic_lds(outside_ring_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(outside_ring_kernel, dim3(W * ka.n_bvars), dim3(OX_NT), lds, stream, ka, ka.X, seqs, W, mask,
                       pair_p);
    return hipGetLastError();
}

}  // namespace adx
