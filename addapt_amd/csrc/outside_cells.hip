// gfx950 outside pass (base-pair probabilities, SURVEY.md A16 / BASELINE
// configs 3-4) with lanes = cells: the adjoint of the inside recursions of
// fold_rows.hip pf_group, in gather form and descending span order -- the same
// equations as fold_rows.hip outside() (oracle/fold.c orc_bppm is the scatter
// form of the sweep), mapped the way mfe_cells.hip maps the MFE:
//
//   * one workgroup (16 waves) per (walker, unconstrained fold with pair
//     terms); the fold's inside tables are NOT recomputed: score_kernel has
//     just written them to the walker's next incremental slot (KArgs::tab), and
//     they are loaded from there into LDS, all diagonal-major;
//   * one anti-diagonal per step, ONE barrier per step; a lane holds one cell
//     (i, i+d), so every interior-loop shape (n1, n2) is one LDS read per lane of
//     the outer cell (i-1-n1, j+1+n2) at a per-lane base plus an immediate
//     offset, no cross-lane reduction.  The 496 shapes are split by loop size
//     over 10 waves (B); waves 10-15 sum the multiloop adjoints (M) over row- /
//     column-major copies of Y, qm1 and qm (consecutive rows / columns of a
//     triangular table start in distinct banks, so a split point is one
//     conflict-free read per lane at an immediate offset); the next step
//     finalizes the cell (F).
//
//   q5b[m]    = sigma q5b[m+1] + sum_j q5b[j] qb(m+1,j) ext(m+1,j)   (before the sweep)
//   qmb(i,j)  = sum_{l >= j+5} Y(i,l) qm1(j+1,l)                      (M)
//   r2(i,j)   = sum_{ip <= i-5} Y(ip,j) qm(ip,i-1)                     (M)
//   R(i,j)    = pw1 (qmb(i-1,j) + R(i-1,j))     [= sum_ip qmb(ip,j) pw(i-ip); pw geometric]
//   qm1b(i,j) = qmb + R + r2 + expMLbase sigma qm1b(i,j+1)
//   qbb(i,j)  = sum_{outer (a,b), loop <= 30} qbb(a,b) F_int + q5b[j] q5[i-1] ext + qm1b stemM   (B, F)
//   Y(i,j)    = qmb(i,j) + X(i,j),  X(i+1,j-1) = qbb(i,j) MLclosing stemM(rev)
//   P(i,j)    = qb(i,j) qbb(i,j) / Z
//
// Covered: unconstrained folds (the pair terms' folds are the conditions'
// unconstrained folds, api_ctx.cpp), N <= 112 (LDS); everything else takes
// fold_rows.hip bppm_kernel.
//
// What it shares with outside_ring.hip is in outside_common.hpp; here: the
// traits (OcK), the table pass, the M role and the kernel (prologue, setup
// calls, the B switch, the M sweep, epilogue).
#include "outside_common.hpp"

OX_STAMP_TABLE(g_stamps_o, adx_debug_stamps_outside)

namespace adx {

namespace {

constexpr int OX_NMAX = 112;
constexpr int MS_CH = 4;   // terms per multiloop-sum read step (even; 16: 423k, 4: 430k, 2: 424k config-3 MC steps/s)

struct OcK {
    static constexpr int SETS = 2;          // lane-sets per diagonal (N - 4 <= 128 cells)
    static constexpr int FB = OX_NB;        // interior-loop block waves (0..9), summed in the finalize
    static constexpr int NMLP = OX_NM;      // mlp slots per parity: the M waves
    static constexpr int SLACK = 64;        // zeroed floats after each cell table
    static constexpr bool COLS = true;      // Y column-major, qm1 row-major, qm column-major in LDS
    __host__ __device__ static int row_len(int N) { return N + 2 * OX_PAD; }
    // the lane's qmb and r2 of lane-set fl from the M waves' parts (oc_m_role's
    // work items of a diagonal with nle lane-sets)
    __device__ __forceinline__ static void msums(const float *mp, int nle, int fl, float &qmbv, float &r2) {
        const bool te = nle == 2;
        qmbv = te ? (fl ? mp[2 * WAVE] : mp[0] + mp[WAVE]) : mp[0] + mp[WAVE] + mp[2 * WAVE];
        r2 = te ? (fl ? mp[4 * WAVE] + mp[5 * WAVE] : mp[3 * WAVE]) : mp[3 * WAVE] + mp[4 * WAVE] + mp[5 * WAVE];
    }
};

// Inside tables, one flat pass over the cells: qm1 row-major and qm
// column-major (transposed from the slot's column- / row-major), Y row-major
// zeroed; the exterior factors G(i, j) = qb(i,j) ext(i,j) column-major in the
// YC region (zeroed after the exterior adjoint)
__device__ __forceinline__ void oc_table_pass(const OxL &L, const float *src, size_t Cs, int N, int C, int tid) {
    float *G = L.yc;
#pragma unroll 2
    for (int k = tid; k < C + OcK::SLACK; k += OX_NT) {
        if (k >= C) {   // slack after each table: finite zeros for reads past a row end
            L.yr[k] = L.q1r[k] = L.qmc[k] = G[k] = 0.f;
            continue;
        }
        const int i = inv_off(k, N) - 3, l = i + 4 + (k - rowb(i, N));   // row-major cell (i, l): rowb == off(i + 3)
        L.q1r[k] = src[2 * Cs + colb(l) + i - 1];
        L.yr[k] = 0.f;
        const int jc = inv_colb(k), ic = k - colb(jc) + 1;                 // column-major cell (ic, jc)
        L.qmc[k] = src[Cs + rowb(ic, N) + jc - ic - 4];
        G[k] = ox_ext_cell(L, src, N, ic, jc);
    }
}

// sum_t y[t] q[t] over t = ta .. tl (the lane's own bound), MS_CH terms per
// step: the loop ends at the lane's range, so a lane reads at most MS_CH - 1
// terms past it (each a wasted LDS cycle on the chain the step waits on;
// pf_cells.hip qm items); even offsets into a0, odd into a1, in order --
// bit-identical to the 16-wide chunks
__device__ __forceinline__ void oc_msum(const float *py, const float *pq, int ta, int tl, float &a0, float &a1) {
    for (int t = ta; t <= tl; t += MS_CH) {
        float yv[MS_CH], qv[MS_CH];
#pragma unroll
        for (int k = 0; k < MS_CH; k++) { yv[k] = py[t + k]; qv[k] = pq[t + k]; }
#pragma unroll
        for (int k = 0; k < MS_CH; k += 2) {
            a0 = fmaf(t + k <= tl ? yv[k] : 0.f, qv[k], a0);
            a1 = fmaf(t + k + 1 <= tl ? yv[k + 1] : 0.f, qv[k + 1], a1);
        }
    }
}

// M: multiloop adjoint sums of diagonal d (nls lane-sets) on M wave mw.  Work
// items: two lane-sets: qmb ls0 (halves on waves 0, 1), qmb ls1, r2 ls0, r2 ls1
// (halves on 4, 5); one lane-set: qmb and r2 in thirds
__device__ __forceinline__ void oc_m_role(const OxL &L, int N, int d, int nls, int mw, int lane) {
    const bool two = nls == 2;
    const bool isq = mw < 3;
    const int ls = two ? ((mw == 2 || mw >= 4) ? 1 : 0) : 0;
    const int np = two ? ((mw <= 1 || mw >= 4) ? 2 : 1) : 3;                 // parts of the item
    const int pi = two ? (mw == 1 || mw == 5 ? 1 : 0) : (mw % 3);            // this wave's part
    int i = 1 + ls * WAVE + lane;
    const int ilast = min(N - d, (ls + 1) * WAVE);
    const bool valid = i <= N - d;
    if (!valid) i = N - d;
    const int j = i + d;
    float acc = 0.f, acc1 = 0.f;
    if (isq) {
        // qmb: t = 0 .. N-j-5: Y(i, j+5+t) = YR[rowb(i) + d + 1 + t],
        // qm1(j+1, j+5+t) = Q1R[rowb(j+1) + t]
        const int lim = N - j - 5;
        const int T = N - (1 + ls * WAVE + d) - 4;          // the lane-set's longest range
        const int ta = (T * pi) / np, tb = (T * (pi + 1)) / np;
        const float *py = L.yr + rowb(i, N) + d + 1, *pq = L.q1r + rowb(j + 1, N);
        oc_msum(py, pq, ta, min(lim, tb - 1), acc, acc1);
    } else {
        // r2: ip = 1 .. i-5: Y(ip, j) = YC[colb(j) + ip - 1], qm(ip, i-1) = QMC[colb(i-1) + ip - 1]
        const int lim = i - 5;
        const int T = ilast - 5;
        const int ta = 1 + (T * pi) / np, tb = 1 + (T * (pi + 1)) / np;
        const float *py = L.yc + colb(j) - 1, *pq = L.qmc + colb(i - 1) - 1;
        oc_msum(py, pq, ta, min(lim, tb - 1), acc, acc1);
    }
    L.mlp[((d & 1) * OX_NM + mw) * WAVE + lane] = acc + acc1;
}

// One workgroup per (walker, outside variant).  pair_p: [W][n_pairs].
__global__ void __launch_bounds__(OX_NT, 1)
outside_cells_kernel(KArgs ka, const DevScaled *__restrict__ XS, const uint8_t *seqs, int W, const int *mask,
                     double *pair_p, int sp_score) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int w = blockIdx.x / ka.n_bvars, bv = blockIdx.x % ka.n_bvars;
    if (w >= W) return;
    if (mask && mask[w] != 1) return;
    const int v = ka.bvars[bv];
    const DevVariant V = ka.variants[v];
    const int N = uni(V.N);
    const OxLay<OcK> Y(N);
    const OxL L = ox_view<OcK>(smem, Y);
    // physical wave -> role: the finalize roles (0, 1) run on waves 2, 3 and the
    // finalize-record roles (2, 3) on waves 0, 1, so the finalize shares its SIMDs
    // with fewer multiloop-sum waves (config 3 462.5k -> 470.3k MC steps/s,
    // profiles/r04zd_ab_wperm.txt)
    constexpr int wperm[OX_NW] = {2, 3, 0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = uni(wperm[tid / WAVE]);
    OX_STAMP_LOCALS

    // ---- the proposal's inside tables (score_kernel's P = sp_score layout, fold_rows.hip Inc)
    const size_t B = 3 * size_t(ka.cells) + size_t(ka.Nmax) + 2;
    const size_t go = (sp_score == 2 ? size_t(ka.bvar_slot[bv]) : size_t(v)) * B;
    const int cur = ka.cur_slot[w];
    const float *src = ka.tab + size_t(w) * 2 * ka.tab_slot + size_t(1 - cur) * ka.tab_slot + go;
    const size_t Cs = size_t(ka.cells);   // the slot's table stride (Nmax cells)

    ox_setup(L, ka, XS, V, seqs, w, src + 3 * Cs, N, tid);
    const OxC c{N, src, XS, L.q5[N], XS->mlbase_sig, XS->mlclosing, XS->pwml[1],
                V.motif != 0 && XS->motif_len > 0, XS->motif_len};
    ox_pair_list(L, ka, bv, tid);
    oc_table_pass(L, src, Cs, N, Y.C, tid);
    __syncthreads();

    OSTAMP(0);   // loads + table pass
    // ---- the exterior adjoint on wave 0, the motif sites on wave 1, the window
    // and the rank lists on the others
    if (wid == 0) ox_ext_adjoint<OcK::SETS>(L, L.yc, XS, N, lane);
    if (c.motif && wid == 1) ox_motif_sites(L, XS, N, c.mL, lane);
    if (wid >= 2) ox_window_ranks(L, N, wid, lane);
    __syncthreads();
    for (int k = tid; k < Y.C; k += OX_NT) L.yc[k] = 0.f;   // G's region: Y column-major from here on
    __syncthreads();

    OSTAMP(1);   // exterior adjoint + zeroing
    Pend<OcK::SETS> pnext;   // the record wave's state (OxFin)
    Idx<OcK::SETS> inext;
    pnext.cnt = 0;
    inext.cnt = 0;
    if (wid == OX_RW) rec_prime<OcK::SETS>(L, *ka.T, N, lane, pnext, inext);
    __syncthreads();
    const OxFin<OcK> fin{L, c, *ka.T, lane, pnext, inext};

    // ---- the sweep: step d runs B and M of diagonal d and F of diagonal d + 1.
    // B: loop sizes in blocks of about equal cost (generic shape ~2 instructions,
    // a special ~9); the 1x1..2x2 table shapes (u = 2, 3, 4) last in their blocks
    if (wid < OX_NB) {
        switch (wid) {
            // loop sizes spread so that every wave's B blocks plus its other role take
            // about the same time (stamps, tools/outside_stamps.py): the finalize
            // wave 0 one size and the record wave 7 none (a size >= 6 costs 3 reads for its
            // special shapes + one per 4 generic ones per lane-set, sizes <= 5 ~3 per shape)
            case 0: b_sweep<2, 19, -1, -1, -1, -1>(L, N, lane, std::integral_constant<int, 0>{}, fin OX_STP_ARGS); break;
            case 1: b_sweep<2, 5, 7, 15, -1, -1>(L, N, lane, std::integral_constant<int, 1>{}, fin OX_STP_ARGS); break;
            case 2: b_sweep<2, 4, 0, 23, -1, -1>(L, N, lane, std::integral_constant<int, 2>{}, fin OX_STP_ARGS); break;
            case 3: b_sweep<2, 3, 30, 6, 11, -1>(L, N, lane, std::integral_constant<int, 3>{}, fin OX_STP_ARGS); break;
            case 4: b_sweep<2, 29, 28, 27, 1, -1>(L, N, lane, std::integral_constant<int, 4>{}, fin OX_STP_ARGS); break;
            case 5: b_sweep<2, 26, 25, 24, 2, -1>(L, N, lane, std::integral_constant<int, 5>{}, fin OX_STP_ARGS); break;
            // (sizes 10 and 9 moved off blocks 8 / 9 measured within noise)
            case 6: b_sweep<2, 22, 21, 20, 8, -1>(L, N, lane, std::integral_constant<int, 6>{}, fin OX_STP_ARGS); break;
            case 7: b_sweep<2, -1, -1, -1, -1, -1>(L, N, lane, std::integral_constant<int, 7>{}, fin OX_STP_ARGS); break;
            case 8: b_sweep<2, 18, 17, 16, 10, -1>(L, N, lane, std::integral_constant<int, 8>{}, fin OX_STP_ARGS); break;
            default: b_sweep<2, 14, 13, 12, 9, -1>(L, N, lane, std::integral_constant<int, 9>{}, fin OX_STP_ARGS); break;   // wave 9
        }
    } else for (int d = N - 1; d >= 3; d--) {
        if (d >= 4) oc_m_role(L, N, d, (N - d + WAVE - 1) / WAVE, wid - OX_NB, lane);
        OSTAMP(4);   // M sums
        OSTAMP(5);   // F (M waves) / B tail
        lds_barrier();
        OSTAMP(6);   // barrier
    }
    OX_STAMP_FLUSH(g_stamps_o, wid, lane)
    ox_write_pairs(L, ka, c, pair_p + size_t(w) * ka.n_pairs, bv, tid);
}

}  // namespace

// LDS bytes of the lanes = cells outside kernel for this workload (0: not covered)
size_t outside_cells_lds(const KArgs &ka) {
    if (ka.Nmax > OX_NMAX || ka.Nmax < 8 || ka.n_pairs > OX_MAXP || !ka.tab) return 0;
    return ox_lds_bytes<OcK>(ka.Nmax);
}

hipError_t launch_outside_cells(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, double *pair_p,
                                int sp_score, hipStream_t stream) {
    const size_t lds = outside_cells_lds(ka);
    if (lds == 0) return hipErrorInvalidValue;
    hipError_t e = configure_dynamic_lds(outside_cells_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(outside_cells_kernel, dim3(W * ka.n_bvars), dim3(OX_NT), lds, stream, ka, ka.X, seqs, W, mask,
                       pair_p, sp_score);
    return hipGetLastError();
}

}  // namespace adx
