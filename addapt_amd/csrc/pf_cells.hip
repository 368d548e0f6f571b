// gfx950 McCaskill inside pass (the reference's scoring path, vrna_pf at
// scoring.cc:58,65; BASELINE configs 3-5 and the PF bench) with lanes = cells
// -- the same recursions, constraints, ligand motif and incremental folds as
// fold_rows.hip pf_group<…, 2, SumProd> (oracle/fold.c orc_pf_energy), mapped
// the way outside_cells.hip maps the outside pass:
//
//   * one workgroup (15 waves) per (walker, group of the apo and holo
//     variants of one (context, macrostate)), the two folds in lockstep as
//     float2 (ds_read_b64, v_pk_fma_f32: one instruction serves both);
//   * one anti-diagonal per step, ONE barrier per step.  Step s runs
//       B   the interior-loop sums of diagonal s (waves 0-7, loop sizes in
//           blocks of equal cost; four lanes per changed pairable cell, each
//           taking a quarter of a size's shapes; every shape one read of the
//           inner cell at a per-lane base plus an immediate offset);
//       F   the cells of diagonal s-1 (wave 8): qb, qbm, qm1;
//       Q   q5[s-1] (wave 9);
//       R   the setup records of diagonal s+2 (wave 10), built in four
//           stages a step apart;
//       M   the qm (fML) items of span s-2 (waves 11-14; K lanes per item so
//           that the few long items of late spans spread over the waves, the
//           split points read from the row-major qm and column-major qm1 at
//           immediate offsets).
//
// What it states identically to pf_ring.hip is in pf_common.hpp.
// Covered: N <= 100 (LDS); longer folds take pf_ring.hip.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"
#include "pf_common.hpp"

namespace adx {
namespace {

constexpr int PX_NB = 8;              // interior-loop blocks (waves 0 .. 7; round 6: +1.2 % PF over seven, A/B r06f)
constexpr int PX_M0 = PX_NB + 3;      // qm item waves PX_M0 .. PX_M0 + PF_NMW - 1
constexpr int PX_NW = PX_M0 + PF_NMW;
constexpr int PX_NT = PX_NW * WAVE;
// Roles of the waves after the blocks (F, Q, R, then four qm waves: the qm wave
// with the most items sets the step at a power-of-two lane split, so a fourth
// qm wave halves it at about half of the spans; measured +1 % over 8 + 3).
constexpr int PX_WF = PX_NB, PX_WQ = PX_NB + 1, PX_WR = PX_NB + 2;   // F, Q, R
__host__ __device__ constexpr int px_mw(int w) {   // M wave index (0 = most items) or -1
    return w == PX_M0 ? 0 : w == PX_M0 + 1 ? 1 : w == PX_M0 + 3 ? 2 : w == PX_M0 + 2 ? 3 : -1;
}
constexpr int PX_NMAX = 100;

// sum of v over the wave, both components (permlane32 swap folds x into lanes
// 0-31 and y into 32-63, one DPP chain finishes both; VALU only)
__device__ __forceinline__ f2 wave_sum_f2(f2 v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v.x), __float_as_uint(v.y), false, false);
    // lanes 0-31: x(l) + x(l+32); lanes 32-63: y(l-32) + y(l)
    float t = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    t += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0xb1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    t += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0x4e, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    t += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0x114, 0xf, 0xf, false));  // row_shr:4
    t += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0x118, 0xf, 0xf, false));  // row_shr:8
    t += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0x142, 0xa, 0xf, false));  // row_bcast:15
    return f2{__int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 31)),
              __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 63))};
}

struct PxLay {
    int C, NP;
    size_t QB, QM, Q1, CC, PART, REC, CL, MLA, UC, Q5, CT, DT, PW, BY, MT, FL, BYTES;
    __host__ __device__ static size_t a16(size_t b) { return (b + 15) & ~size_t(15); }
    __host__ __device__ explicit PxLay(int N) {
        C = ((N - 4) * (N - 3)) / 2;
        NP = N + 2;
        size_t o = 0;
        QB = o;   o += a16((size_t(C) + PF_SLACK) * 8);           // qb * mismatchI(inner), diagonal-major
        QM = o;   o += a16((size_t(C) + PF_SLACK) * 8);           // qm, row-major
        Q1 = o;   o += a16((size_t(C) + PF_SLACK) * 8);           // qm1, column-major
        CC = o;   o += a16(size_t(C) + PF_SLACK);                 // inner-pair code per cell
        PART = o; o += a16(size_t(2) * 2 * PX_NB * WAVE * 8);     // [parity][lane-set][block][lane]
        REC = o;  o += a16(size_t(3) * 2 * PF_RF * WAVE * 4 + 16); // [diagonal % 3][set][field][lane]; counts
        CL = o;   o += a16(size_t(C) + size_t(NP));               // rank lists of the changed pairable cells + counts
        MLA = o;  o += a16(size_t(2) * NP * 8);                   // split part of qm, by span parity
        UC = o;   o += a16(size_t(2) * NP * 8);                   // unpaired part U(i, j) of qm by column j, by span parity
        Q5 = o;   o += a16(size_t(NP) * 8);
        CT = o;   o += a16(size_t(CT_SIZE) * 4);
        DT = o;   o += a16(size_t(DT_HP) * 4);                    // (hairpin lengths: XS->hp, a register per wave)
        PW = o;   o += a16(size_t(N + 9) * 4);                    // (expMLbase sigma)^t
        BY = o;   o += a16(size_t(7) * NP);                       // S, up, dn, ptn, enc, flg, mat
        MT = o;   o += a16(size_t(MAX_SPECIAL_HP) * 8 + 2 * MAX_MOTIF);   // special hairpins, motif codes / partners
        FL = o;   o += 16;                                        // block_or word
        BYTES = o;
    }
};

// pf_common.hpp's traits of this kernel
struct PxK {
    using V = f2;
    static constexpr int NT = PX_NT, NW = PX_NW, NMAX = PX_NMAX;
    static constexpr int NB = PX_NB, SETS = 2;    // B blocks; lane-sets of a diagonal's records
    static constexpr int IB = 7;                  // bits of i in the record word
    static constexpr int REC_SLOTS = 3;           // record ring: B loads a step ahead of its use
    static constexpr bool HP_LDS = false, QBG = false;
    static constexpr bool REC_LAZY = true;        // record stages leave unused lane-sets unset (pf_common.hpp)
    static constexpr int ST_REC = 2, ST_SHAPES = 3;   // stamp slots (tools/pf_cells_stamps.py)
    __device__ static __forceinline__ int slot(int D) { return D % 3; }
    // first inner cell of diagonal D in qb / cc
    __device__ static __forceinline__ int inner(const PfL<f2> &L, int D) { return off(D, L.N); }
    // hairpin length factors of this wave's per-cell-pass diagonals D = 4 + wid + NW m
    // (lane m), a register: hp[D - 1] by readlane
    __device__ static __forceinline__ float hp_load(const DevScaled *XS, int tid, int lane, int wid, int N) {
        static_assert(4 + (WAVE - 1) * PX_NW > PX_NMAX, "hpl covers every diagonal");
        return XS->hp[min(3 + wid + PX_NW * lane, adx::NMAX)];   // the table's end (dev_types.hpp), not PxK::NMAX
    }
    __device__ static __forceinline__ float hp_len(const PfL<f2> &L, float hpl, int D, int wid) {
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hpl), (D - 4 - wid) / PX_NW));
    }
    // M: the split points t = 5..T interleaved over the K lanes (lane k: t = 5 + k +
    // K m), so an item's lanes read consecutive words of its qm1 column and qm row
    // (no bank conflicts inside an item); t in A, t + K in A1 (past T: 0, whatever
    // was read)
    __device__ static __forceinline__ f2 split_sum(const f2 *pq, const f2 *pr, int k, int K, int T) {
        const int nit = T >= 5 ? (T - 4 + 2 * K - 1) / (2 * K) : 0;
        f2 A = {0.f, 0.f}, A1 = {0.f, 0.f};
        const f2 z = {0.f, 0.f};
        for (int m = 0; m < nit; m++) {
            const int t = 5 + k + 2 * K * m, t2 = t + K;
            const f2 qa = pq[t], qn = pq[t2], ra = pr[t], rn = pr[t2];
            A = vfma(t <= T ? ra : z, t <= T ? qa : z, A);
            A1 = vfma(t2 <= T ? rn : z, t2 <= T ? qn : z, A1);
        }
        A += A1;
        return A;
    }
};
using PxL = PfL<f2>;

#ifdef ADX_STAMP
__device__ unsigned long long g_stamps_p[16][12];
#endif

// B: interior-loop sums of every diagonal for one block of loop sizes.  Lanes
// = (cell, phase r): four lanes per cell (16 cells per batch, pf_common.hpp
// pb_batch).  The first lane-set's records and the count of diagonal D are
// loaded a step ahead (the record wave writes them two steps ahead, slot D %
// 3): issued at the top of a step, they complete under its first reads
struct Pre {
    int n;
    BRec q;
};
template <bool H5, bool TB>
__device__ __forceinline__ Pre pre_load(const PxL &L, int D, int cq) {
    Pre p;
    const int sl = PxK::slot(D);
    p.n = (D <= L.N - 1 && D >= 6) ? L.rcnt[sl] : 0;
    p.q = brec_load<H5, TB>(brec_at<PxK>(L, sl, cq));
    return p;
}
template <int U0, int U1, int U2, int U3, int U4>
__device__ __forceinline__ void pb_sweep(const PxL &L, const DevScaled *XS, int N, int lane, int wid,
                                         bool constrained, int s_end PF_STP_PARAMS) {
    constexpr auto tb = [](int u) { return u >= 2 && u <= 4; };
    constexpr bool TB = tb(U0) || tb(U1) || tb(U2) || tb(U3) || tb(U4);
    constexpr bool H5 = U0 == 5 || U1 == 5 || U2 == 5 || U3 == 5 || U4 == 5;   // 2x3 loops (m23)
    const float eTAU = XS->ctab[CT_FSM + 6];
    const int r = lane & 3, cq = lane >> 2;
    typename PBlk<PxK, U0>::T s0;
    typename PBlk<PxK, U1>::T s1;
    typename PBlk<PxK, U2>::T s2;
    typename PBlk<PxK, U3>::T s3;
    typename PBlk<PxK, U4>::T s4;
    p_load<PxK, U0>(s0, XS, r);
    p_load<PxK, U1>(s1, XS, r);
    p_load<PxK, U2>(s2, XS, r);
    p_load<PxK, U3>(s3, XS, r);
    p_load<PxK, U4>(s4, XS, r);
    const int ctb = r < 2 ? CT_BUL : CT_ONEN;   // the lane's special-shape inner factor table
    Pre cur = pre_load<H5, TB>(L, 4, cq);
    for (int s = 4; s <= s_end; s++) {
        const Pre nxt = pre_load<H5, TB>(L, s + 1, cq);
        const int umax = min(30, s - 6);   // no interior loop fits a span below 6
        const int ncell = (s <= N - 1 && umax >= 0) ? uni(cur.n) : 0;
        for (int c0 = 0; c0 < ncell; c0 += WAVE / 4) {
            const int idx = c0 + cq;   // the lane's cell (records: set idx / 64, lane idx % 64)
            BRec q = cur.q;
            if (c0 > 0) q = brec_load<H5, TB>(brec_at<PxK>(L, PxK::slot(s), idx));
            pb_batch<PxK, U0, U1, U2, U3, U4>(L, s0, s1, s2, s3, s4, q, eTAU, s, umax, r, ctb, idx, ncell, wid,
                                              constrained PF_STP_ARGS);
        }
        cur = nxt;
        PF_STAMP(5);
        lds_barrier();
        PF_STAMP(6);
    }
}

// ---- refold restore: every table from the current slot (the changed cells are
// recomputed over it), two cells per lane and load, both folds interleaved.
// The loads are issued before the motif scan and stored to LDS after it, so their
// HBM latency overlaps the rest of the setup.  (HBM side dword-aligned only
// when cells or B1 are odd: fine for global loads.)
constexpr int PX_RS = 8;   // loads per lane: 3 * C / 2 <= PX_RS * PX_NT for N <= PX_NMAX
static_assert(3 * (((PX_NMAX - 4) * (PX_NMAX - 3) / 2) / 2) <= PX_RS * PX_NT, "restore loads fit PX_RS per lane");
static_assert(((PX_NMAX - 4) * (PX_NMAX - 3) / 2 + 15) / 16 <= PX_NT, "one code load per thread");
static_assert(PX_NMAX < PX_NT, "one q5 entry per thread");
struct PxRestore {
    float2 x[PX_RS], y[PX_RS];   // apo, holo
    uint4 cv;                    // the codes (round 6: the band's are recomputed)
    f2 od, r5;                   // the odd last cell of each table, q5's prefix
};
// src: the refold's slot (cc_src: its per-cell codes), or null: a fold from
// scratch zeroes qm (spans N-2, N-1 are never computed)
__device__ __forceinline__ PxRestore px_restore_load(const PxL &L, const float *src, const uint4 *cc_src, int C,
                                                     size_t Cs, size_t B1, int tid) {
    PxRestore R;
    R.cv = make_uint4(0, 0, 0, 0);
    R.od = R.r5 = f2{0.f, 0.f};
    if (src) {
        const int half = C >> 1;
#pragma unroll
        for (int t = 0; t < PX_RS; t++) {
            const int k = tid + t * PX_NT;
            const int kk = k < 3 * half ? k : 0;
            const int a = kk / half, c = kk - a * half;
            const float *sa = src + a * Cs + 2 * c;
            R.x[t] = *reinterpret_cast<const float2 *>(sa);
            R.y[t] = *reinterpret_cast<const float2 *>(sa + B1);
        }
        R.cv = cc_src[tid < ((C + 15) >> 4) ? tid : 0];
        const int ko = min(tid, 2);
        R.od = f2{src[ko * Cs + max(C - 1, 0)], src[B1 + ko * Cs + max(C - 1, 0)]};
        const int k5 = min(tid, L.N);
        R.r5 = f2{src[3 * Cs + k5], src[B1 + 3 * Cs + k5]};
    } else {
        for (int k = tid; k < C; k += PX_NT) L.qm[k] = f2{0.f, 0.f};
    }
    return R;
}
// ls4: the stride of qb, qm, q1 (contiguous) in float4; q5 up to the changed band
__device__ __forceinline__ void px_restore_store(const PxL &L, const PxRestore &R, int C, size_t ls4, int m_lo,
                                                 int tid) {
    float4 *qd = reinterpret_cast<float4 *>(L.qb);
    const int half = C >> 1;
#pragma unroll
    for (int t = 0; t < PX_RS; t++) {
        const int k = tid + t * PX_NT;
        if (k < 3 * half) {
            const int a = k / half, c = k - a * half;
            qd[a * ls4 + c] = float4{R.x[t].x, R.y[t].x, R.x[t].y, R.y[t].y};
        }
    }
    if ((C & 1) && tid < 3) L.qb[tid * (ls4 * 2) + C - 1] = R.od;
    if (tid < ((C + 15) >> 4)) reinterpret_cast<uint4 *>(L.cc)[tid] = R.cv;
    if (tid <= m_lo - 2 && tid <= L.N) L.q5[tid] = R.r5;
}

// Cells by diagonal (wave w: diagonals 4 + w, 4 + w + NW, ...; lanes = i), a
// refold's band rows only (every other cell was restored): the inner code; the
// hairpin (+ motif) initial value (pairable) or the mark, and the multiloop stem
// in qm1 (F reads both before it overwrites them); and the rank list of the
// changed pairable cells (the B lanes): cl[off(D) + rank] = i, cn[D] = count
__device__ __forceinline__ void px_cell_pass(const PxL &L, const Band &bd, float hpl, int mL, float mext, bool hol0,
                                             bool hol1, int lane, int wid) {
    const int N = L.N;
    const uint8_t *S = L.S;
    for (int D = 4 + wid; D <= N - 1; D += PX_NW) {
        const int od = off(D, N), lo = bd.clo(D), hi = bd.chi(D);
        int base = 0;
        for (int i0 = lo; i0 <= hi; i0 += WAVE) {
            const int i = i0 + lane;
            bool pr = false;
            if (i <= hi) {
                const int j = i + D;
                const int type = ptype(S[i], S[j]);
                L.cc[od + i - 1] = uint8_t(rtype(type) * 25 + S[j + 1] * 5 + S[i - 1]);
                pr = type != 0 && allowed(L, i, j);
                f2 init = f2{-0.f, -0.f};
                float m1 = 0.f;
                if (pr) {
                    init = pf_hairpin_init<PxK>(L, i, j, D, type, hpl, wid, mL, mext, hol0, hol1);
                    m1 = L.dt[DT_MLS + type * 25 + S[i - 1] * 5 + S[j + 1]];
                }
                L.qb[od + i - 1] = init;
                L.q1[colb(j) + i - 1] = f2{m1, m1};
            }
            base = pf_rank_push(L, od, base, pr, i);
        }
        if (lane == 0) L.cn[D] = uint8_t(base);
    }
}

// Q: exterior-stem factors of column j (cells (k, j), k <= j - 4, two lane-sets),
// static, gathered a step ahead of q5[j]
__device__ __forceinline__ void px_qfac(const PxL &L, int j, int lane, float (&qf)[2]) {
    const int N = L.N;
    if (j < 4 || j > N) return;
    const int sjp = (j < N) ? L.S[j + 1] : 5;
    const int sj = L.S[j];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int kk = 1 + h * WAVE + lane;
        const bool ok = kk <= j - 4;
        const int k = ok ? kk : 1;
        const float f = pf_ext_factor(L, k, ptype(L.S[k], sj), sjp, L.cc[off(j - k, N) + k - 1]);
        qf[h] = ok ? f : 0.f;
    }
}
// Q: q5[j] (column j is final; a refold: from the changed band on)
__device__ __forceinline__ void px_q5(const PxL &L, const Band &bd, int j, int lane, const float (&qf)[2],
                                      float sig1) {
    const int N = L.N;
    if (j >= 4 && j <= N && (!bd.incr || j >= bd.m_lo - 1)) {
        f2 acc = {0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h * WAVE >= j - 4) break;
            const int kk = 1 + h * WAVE + lane;
            const int k = kk <= j - 4 ? kk : 1;
            const int ix = off(j - k, N) + k - 1;
            acc = vfma(L.q5[k - 1] * L.qb[ix], splat<f2>(qf[h]), acc);
        }
        acc = wave_sum_f2(acc);
        if (lane == 0) L.q5[j] = (L.up[j] >= 1 ? L.q5[j - 1] * splat<f2>(sig1) : f2{0.f, 0.f}) + acc;
    }
}

// the proposal's tables (the next step's unchanged cells): apo and holo B1 apart
__device__ __forceinline__ void px_write_back(const PxL &L, float *dst, uint4 *cc_dst, int C, size_t Cs, size_t B1,
                                              int tid) {
    for (int k = tid; k < C; k += PX_NT) {
        const f2 a = L.qb[k], b = L.qm[k], c = L.q1[k];
        dst[k] = a.x;
        dst[B1 + k] = a.y;
        dst[Cs + k] = b.x;
        dst[B1 + Cs + k] = b.y;
        dst[2 * Cs + k] = c.x;
        dst[B1 + 2 * Cs + k] = c.y;
    }
    for (int k = tid; k <= L.N; k += PX_NT) {
        dst[3 * Cs + k] = L.q5[k].x;
        dst[B1 + 3 * Cs + k] = L.q5[k].y;
    }
    for (int k = tid; k < ((C + 15) >> 4); k += PX_NT) cc_dst[k] = reinterpret_cast<const uint4 *>(L.cc)[k];
}

// One workgroup per (walker, group).  gout: [W][n_variants] ensemble energies
// (kcal/mol, as score_sequence writes dG), the scores follow in combine_kernel.
__global__ void __launch_bounds__(PX_NT, 1)
pf_cells_kernel(KArgs ka, const DevScaled *__restrict__ XS, const uint8_t *seqs, int W, const int *mask,
                float *gout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef ADX_STAMP
    unsigned long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif
    const int wb = blockIdx.x / ka.n_groups2, grp = blockIdx.x % ka.n_groups2;
    if (wb >= W) return;
    const WalkerRef wr = walker_ref(ka, mask, wb);   // heaviest refolds first
    if (!wr.on) return;
    const int w = wr.w;
    const int vs0 = ka.groups2[2 * grp], vs1 = ka.groups2[2 * grp + 1];
    const DevVariant V = ka.variants[vs0];
    const bool hol0 = ka.variants[vs0].motif != 0, hol1 = ka.variants[vs1].motif != 0;
    const int N = uni(V.N);
    const PxLay Y(N);
    const PxL L = pf_carve<PxK>(smem, Y, N);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = uni(tid / WAVE);
    const int C = Y.C, NP = Y.NP;
    const DevTables &T = *ka.T;

    // ---- incremental fold state (fold_rows.hip score_sequence / Inc): this group's
    // tables of the current sequence (src) and the proposal's (dst)
    const size_t Cs = size_t(ka.cells), B1 = 3 * Cs + size_t(ka.Nmax) + 2;
    const float *src = nullptr;
    float *dst = nullptr;
    const uint4 *cc_src = nullptr;   // the slots' per-cell codes (dev_types.hpp inc_cc_offset_pf)
    uint4 *cc_dst = nullptr;
    int m_lo = 0, m_hi = 0;
    if (ka.tab) {
        const int cur = wr.cur;
        float *base = ka.tab + size_t(w) * 2 * ka.tab_slot;
        dst = base + size_t(1 - cur) * ka.tab_slot + size_t(grp) * 2 * B1;
        const size_t cco = inc_cc_offset_pf(ka.cells, ka.Nmax, ka.n_groups2, grp);
        cc_dst = reinterpret_cast<uint4 *>(base + size_t(1 - cur) * ka.tab_slot + cco);
        if (wr.valid && wr.c0 >= 0) {
            src = base + size_t(cur) * ka.tab_slot + size_t(grp) * 2 * B1;
            cc_src = reinterpret_cast<const uint4 *>(base + size_t(cur) * ka.tab_slot + cco);
            m_lo = wr.c0 + 1 + V.before_len;
            m_hi = wr.c1 + 1 + V.before_len;
        }
    }
    const bool incr = src != nullptr;
    if (tid == 0) *reinterpret_cast<int *>(smem + Y.FL) = 0;   // block_or word (read after two barriers)
    const Band bd{incr, N, uni(m_lo), uni(m_hi)};

    PF_STAMP(8);   // the prologue (walker, slot, variant words)
    // ---- setup (round 6): every load of the tables and the sequence / constraint
    // arrays in flight at once and stored before the restore's loads are issued
    // (the first table load waited behind the restore's: stamps r06p "tables")
    const auto su = pf_setup_load<PxK>(ka, XS, V, seqs, w, tid, lane, wid, N, NP);
    const bool cst = pf_setup_store<PxK>(L, su, tid, N, NP);
    PF_STAMP(9);   // setup loads and stores
    const PxRestore rs = px_restore_load(L, src, cc_src, C, Cs, B1, tid);
    for (int k = tid; k < 2 * NP; k += PX_NT) L.mla[k] = f2{0.f, 0.f};
    for (int k = C + tid; k < C + PF_SLACK; k += PX_NT) L.qb[k] = L.qm[k] = L.q1[k] = f2{0.f, 0.f};
    PF_STAMP(10);   // the restore's loads issued
    __syncthreads();   // orders tid 0's zeroing of the block_or word before the ORs
    const bool constrained = block_or(reinterpret_cast<int *>(smem + Y.FL), cst);
    PF_STAMP(1);
    const int mL = XS->motif_len;
    pf_motif_sites<PxK>(L, (hol0 || hol1) && mL > 0, mL, tid, lane, wid);
    if (incr) px_restore_store(L, rs, C, (Y.QM - Y.QB) >> 4, bd.m_lo, tid);
    __syncthreads();
    PF_STAMP(7);   // motif sites + the restore's stores (the wait for its loads)
    const float sig1 = XS->sig[1], mlbase_sig = XS->mlbase_sig, mlclosing = XS->mlclosing;
    px_cell_pass(L, bd, su.hp, mL, XS->motif_extra, hol0, hol1, lane, wid);
    pf_q5_prefix<PxK>(L, sig1, tid);
    __syncthreads();
    PF_STAMP(0);

    // ---- records (wave R, pf_common.hpp): gathered at step D - 2 (rec_load) and
    // written at step D - 1 (rec_store)
    Pend<2> pend;
    Seq<2> seqp;
    Idx<2> idxp;
    if (wid == PX_WR) {   // the records run two steps ahead of B (which loads them one step ahead)
        // the sweep's first B diagonals (no loop fits: count 0)
        rec_store<PxK>(L, 4, rec_load<PxK>(L, T, 4, seq_load<PxK>(L, 4, idx_load<PxK>(L, 4, lane)), lane), lane);
        rec_store<PxK>(L, 5, rec_load<PxK>(L, T, 5, seq_load<PxK>(L, 5, idx_load<PxK>(L, 5, lane)), lane), lane);
        pend = rec_load<PxK>(L, T, 6, seq_load<PxK>(L, 6, idx_load<PxK>(L, 6, lane)), lane);
        seqp = seq_load<PxK>(L, 7, idx_load<PxK>(L, 7, lane));
        idxp = idx_load<PxK>(L, 8, lane);
    }
    __syncthreads();

    float qf[2] = {0.f, 0.f};   // Q: the exterior factors of the next column
    if (wid == PX_WQ) px_qfac(L, 4, lane, qf);
    const int s_end = N + 1;
    if (wid < PX_NB) {
        // eight blocks (round 6, A/B r06f: +1.2 % PF over seven): sizes 9, 14, 6 of
        // the blocks the stamps showed busiest (profiles/r06e_pf_cells_stamps.txt)
        // on an eighth wave.  The other sizes are hand-placed from the stamps:
        // against blocks of about equal LDS cost, 16 sits on block 3, 15 on block
        // 5, 0 on block 1 and 13 on block 2 (+2.4 % PF r07g,
        // +1.0 % r07i; moving sizes back onto block 4 was no faster, A/B r07n)
        switch (wid) {
            case 0: pb_sweep<5, 22, 12, 11, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 1: pb_sweep<4, 21, 19, 10, 0>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 2: pb_sweep<3, 20, 18, 8, 13>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 3: pb_sweep<28, 26, 1, 7, 16>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 4: pb_sweep<29, 27, -1, -1, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 5: pb_sweep<30, 2, 17, 15, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 6: pb_sweep<24, 25, 23, -1, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            default: pb_sweep<9, 14, 6, -1, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
        }
    } else {
        // the M / F / Q / R chains set the step time; issue arbitration favours the
        // older (B) waves of the workgroup, so these run at a higher priority
        __builtin_amdgcn_s_setprio(2);
        // one sweep instance per role (round 6): each holds only its own role's
        // registers (the shared loop kept every role's values live: 38 SGPR spills)
        auto sweep = [&](auto role_c) __attribute__((always_inline)) {
            constexpr int ROLE = decltype(role_c)::value;   // 0 M, 1 F, 2 Q, 3 R
            for (int s = 4; s <= s_end; s++) {
                if constexpr (ROLE == 0) {          // M: qm items of span s - 2
                    pf_m_role<PxK>(L, bd, s - 2, px_mw(wid), lane, constrained, mlbase_sig);
                } else if constexpr (ROLE == 1) {   // F: the changed cells of diagonal s - 1
                    pf_f_role<PxK>(L, bd, s - 1, lane, mlclosing, mlbase_sig, nullptr);
                } else if constexpr (ROLE == 2) {   // Q: q5[s - 1], U of span s - 2, the next column's factors
                    px_q5(L, bd, s - 1, lane, qf, sig1);
                    pf_uc_update(L, s - 2, lane, constrained, mlbase_sig);
                    px_qfac(L, s, lane, qf);
                } else {
                    // R: records of diagonal s + 2 (B loads them next step for the step
                    // after), tables of s + 3, bases of s + 4, rank list of s + 5
                    rec_store<PxK>(L, s + 2, pend, lane);
                    pend = rec_load<PxK>(L, T, s + 3, seqp, lane);
                    seqp = seq_load<PxK>(L, s + 4, idxp);
                    idxp = idx_load<PxK>(L, s + 5, lane);
                }
                PF_STAMP(4);
                lds_barrier();
                PF_STAMP(6);
            }
        };
        if (px_mw(wid) >= 0) sweep(std::integral_constant<int, 0>{});
        else if (wid == PX_WF) sweep(std::integral_constant<int, 1>{});
        else if (wid == PX_WQ) sweep(std::integral_constant<int, 2>{});
        else sweep(std::integral_constant<int, 3>{});   // PX_WR
    }
#ifdef ADX_STAMP
    if (lane == 0)
        for (int k = 0; k < 12; k++) atomicAdd(&g_stamps_p[wid][k], st_acc[k]);
#endif
    __syncthreads();
    // ---- the proposal's tables and the energies
    if (dst) px_write_back(L, dst, cc_dst, C, Cs, B1, tid);
    if (tid == 0) {
        const f2 z = L.q5[N];
        gout[size_t(w) * ka.n_variants + vs0] = pf_energy(XS, z.x, N);
        gout[size_t(w) * ka.n_variants + vs1] = pf_energy(XS, z.y, N);
    }
}

}  // namespace

// LDS bytes of the lanes = cells PF kernel for this workload (0: not covered)
size_t pf_cells_lds(const KArgs &ka) {
    if (ka.mode != 0 || ka.Nmax > PX_NMAX || ka.Nmax < 8) return 0;
    const size_t b = PxLay(ka.Nmax).BYTES;   // no static LDS (block_or, not __syncthreads_or; checked at launch)
    return b <= size_t(LDS_LIMIT) ? b : 0;
}

hipError_t launch_pf_cells(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, float *gout,
                           hipStream_t stream) {
    const size_t lds = pf_cells_lds(ka);
    if (lds == 0) return hipErrorInvalidValue;
    // the carve addresses LDS from 0: no static LDS may precede the block
    hipError_t e = configure_dynamic_lds(pf_cells_kernel, lds, true);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pf_cells_kernel, dim3(W * ka.n_groups2), dim3(PX_NT), lds, stream, ka, ka.X, seqs, W, mask,
                       gout);
    return hipGetLastError();
}

}  // namespace adx

#ifdef ADX_STAMP
extern "C" int adx_debug_stamps_pf(unsigned long long *out, int reset) {  // [16][12]
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(adx::g_stamps_p), sizeof(adx::g_stamps_p)) != hipSuccess) return 1;
    if (reset) {
        static unsigned long long z[16][12] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(adx::g_stamps_p), z, sizeof(z)) != hipSuccess) return 2;
    }
    return 0;
}
#endif
