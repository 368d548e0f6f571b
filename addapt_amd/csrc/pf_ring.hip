// gfx950 McCaskill inside pass for folds longer than pf_cells.hip covers
// (BASELINE config 4: N = 150, the reference's vrna_pf at scoring.cc:58,65),
// lanes = cells like pf_cells_kernel, with the LDS carved for ONE fold:
//
//   * one workgroup (14 waves) per (walker, variant): FP32 values (pf_cells
//     keeps apo|holo as float2, which at N = 150 would need 257 KB);
//   * qm (row-major) and qm1 (column-major) stay whole in LDS (2 x 43 KB);
//   * qb and the inner codes live in a RING of the last 34 diagonals: an
//     interior loop (<= 30 unpaired) reaches 32 diagonals back, F writes the
//     previous one and the prep stage the next;
//   * the exterior recursion q5[j] needs whole columns of qb: F stores every
//     finalised cell to the walker's table slot (diagonal-major, as pf_cells),
//     the prep stage stores the restored and non-pairable cells, and Q reads
//     column j from there two steps after it is final (a global read per lane
//     and lane-set, issued a step ahead; every writer drains its stores at the
//     start of its next step, so no wave waits on a store on its way to the
//     barrier);
//   * the slot keeps qm and qm1 DIAGONAL-major (not row- / column-major as
//     pf_cells): the outside pass for these lengths (outside_ring.hip) reads
//     them from the slot with lanes = cells, where a diagonal-major table makes
//     every read one coalesced line.
//
// One step = one anti-diagonal, ONE barrier:
//   B  (waves 0-6)  interior-loop sums of diagonal s
//   F  (wave 7)     cells of diagonal s-1: qb, qm1, the slot store
//   Q  (wave 8)     q5[s-3] from column s-3 (loaded last step), the load of
//                   column s-2
//   R  (wave 9)     setup records of the B lanes, four stages a step apart
//   prep            of diagonal s+1, one lane-set each on M waves 12, 13 and R: inner
//                   codes, hairpin (+ motif) initial values of the changed
//                   cells, restored values of the others (loaded a step ahead)
//   M  (waves 10-13) qm items of span s-2
//
// What it states identically to pf_cells.hip is in pf_common.hpp.
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

constexpr int RG_NW = 14;
constexpr int RG_NT = RG_NW * WAVE;
constexpr int RG_NB = 7;              // interior-loop blocks (waves 0..6)
constexpr int RG_WF = 7, RG_WQ = 8, RG_WR = 9;
__host__ __device__ constexpr int rg_mw(int w) {   // M wave index (0 = most items) or -1
    return w == 10 ? 0 : w == 11 ? 1 : w == 13 ? 2 : w == 12 ? 3 : -1;
}
constexpr int RG_NMIN = 101;          // pf_cells_kernel covers N <= 100
constexpr int RG_NMAX = 190;          // lane-sets of a diagonal: N - 4 <= RG_SETS * 64
constexpr int RG_SETS = 3;
constexpr int RG_RING = 34;           // diagonals s-32 .. s+1

struct RgLay {
    int C, NP, RS;
    size_t QM, Q1, QB, CC, PART, REC, CL, MLA, UC, Q5, CT, DT, PW, BY, MT, BYTES;
    __host__ __device__ static size_t a16(size_t b) { return (b + 15) & ~size_t(15); }
    __host__ __device__ explicit RgLay(int N) {
        C = ((N - 4) * (N - 3)) / 2;
        NP = N + 2;
        RS = ((N - 4) + 3) & ~3;                                   // ring row: the longest diagonal
        size_t o = 0;
        QM = o;   o += a16((size_t(C) + PF_SLACK) * 4);           // qm, row-major
        Q1 = o;   o += a16((size_t(C) + PF_SLACK) * 4);           // qm1, column-major
        QB = o;   o += a16(size_t(RG_RING) * RS * 4);             // qb * mismatchI(inner) ring
        CC = o;   o += a16(size_t(RG_RING) * RS);                 // inner-pair code ring
        PART = o; o += a16(size_t(2) * RG_SETS * RG_NB * WAVE * 4);   // [parity][lane-set][block][lane]
        REC = o;  o += a16(size_t(2) * RG_SETS * PF_RF * WAVE * 4 + 16);   // [parity][set][field][lane]; counts
        CL = o;   o += a16(size_t(C) + size_t(NP));               // rank lists of the changed pairable cells + counts
        MLA = o;  o += a16(size_t(2) * NP * 4);                   // split part of qm, by span parity
        UC = o;   o += a16(size_t(2) * NP * 4);                   // unpaired part U(i, j) of qm by column j, by span parity
        Q5 = o;   o += a16(size_t(NP) * 4);
        CT = o;   o += a16(size_t(CT_SIZE) * 4);
        DT = o;   o += a16(size_t(DT_HP + N + 1) * 4);
        PW = o;   o += a16(size_t(N + 9) * 4);                    // (expMLbase sigma)^t
        BY = o;   o += a16(size_t(7) * NP);                       // S, up, dn, ptn, enc, flg, mat
        MT = o;   o += a16(size_t(MAX_SPECIAL_HP) * 8 + 2 * MAX_MOTIF);
        BYTES = o;
    }
};

// ring position of diagonal D's first cell
__device__ __forceinline__ int rgo(int D, int RS) { return (D % RG_RING) * RS; }

// pf_common.hpp's traits of this kernel
struct RgK {
    using V = float;
    static constexpr int NT = RG_NT, NW = RG_NW, NMAX = RG_NMAX;
    static constexpr int NB = RG_NB, SETS = RG_SETS;   // B blocks; lane-sets of a diagonal's records
    static constexpr int IB = 8;                       // bits of i in the record word
    static constexpr int REC_SLOTS = 2;                // records by diagonal parity
    static constexpr bool HP_LDS = true, QBG = true;   // hp in dt[DT_HP]; F copies qb to the slot
    static constexpr bool REC_LAZY = false;            // record stages zero unused lane-sets (pf_common.hpp)
    static constexpr int ST_REC = 1, ST_SHAPES = 2;    // stamp slots (tools/ring_stamps.py)
    __device__ static __forceinline__ int slot(int D) { return D & 1; }
    // first inner cell of diagonal D in the qb / cc ring
    __device__ static __forceinline__ int inner(const PfL<float> &L, int D) { return rgo(D, L.RS); }
    __device__ static __forceinline__ float hp_load(const DevScaled *XS, int tid, int lane, int wid, int N) {
        return XS->hp[min(tid, N)];
    }
    __device__ static __forceinline__ float hp_len(const PfL<float> &L, float, int D, int wid) {
        return L.dt[DT_HP + D - 1];
    }
    // M: the split points t = 5..T in one contiguous chunk per lane (K lanes),
    // pairs: even offsets in A, odd in A1
    __device__ static __forceinline__ float split_sum(const float *pq, const float *pr, int k, int K, int T) {
        const int nb = T - 4;
        const int tch = nb > 0 ? (nb + K - 1) / K : 0;
        const int t0 = 5 + k * tch, t1 = min(T, t0 + tch - 1);
        float A = 0.f, A1 = 0.f;
        for (int t = t0; t <= t1; t += 2) {
            const float qa = pq[t], qn = pq[t + 1], ra = pr[t], rn = pr[t + 1];
            A = fmaf(ra, qa, A);
            A1 = fmaf(rn, t + 1 <= t1 ? qn : 0.f, A1);
        }
        A += A1;
        return A;
    }
};
using RgL = PfL<float>;

// sum over the wave, uniform result: DPP row sums, then the four rows' totals
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = dpp_add<0xb1>(v);    // quad_perm [1,0,3,2]
    v = dpp_add<0x4e>(v);    // quad_perm [2,3,0,1]
    v = dpp_add<0x114>(v);   // row_shr:4
    v = dpp_add<0x118>(v);   // row_shr:8 -> lane 15 of each row holds the row sum
    const int b = __float_as_int(v);
    return __int_as_float(__builtin_amdgcn_readlane(b, 15)) + __int_as_float(__builtin_amdgcn_readlane(b, 31)) +
           __int_as_float(__builtin_amdgcn_readlane(b, 47)) + __int_as_float(__builtin_amdgcn_readlane(b, 63));
}
#ifdef ADX_STAMP
// Diagnostic build only: per-wave cycle sums of the phases (s_memtime), read
// back through adx_debug_stamps_ring().  Never in the product.
__device__ unsigned long long g_stamps_r[16][8];
#endif

// global stores of this wave complete before the step's barrier (the slot is
// read back by Q within the workgroup)
__device__ __forceinline__ void vm_drain() { __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// B: interior-loop sums of every diagonal for one block of loop sizes (lanes =
// (cell, phase): pf_common.hpp pb_batch), the records of the step's parity
template <int U0, int U1, int U2, int U3, int U4>
__device__ __forceinline__ void rb_sweep(const RgL &L, const DevScaled *XS, int N, int lane, int wid,
                                         bool constrained, int s_end PF_STP_PARAMS) {
    constexpr auto tb = [](int u) { return u >= 2 && u <= 4; };
    constexpr bool TB = tb(U0) || tb(U1) || tb(U2) || tb(U3) || tb(U4);
    constexpr bool H5 = U0 == 5 || U1 == 5 || U2 == 5 || U3 == 5 || U4 == 5;
    const float eTAU = XS->ctab[CT_FSM + 6];
    const int r = lane & 3, cq = lane >> 2;
    typename PBlk<RgK, U0>::T s0;
    typename PBlk<RgK, U1>::T s1;
    typename PBlk<RgK, U2>::T s2;
    typename PBlk<RgK, U3>::T s3;
    typename PBlk<RgK, U4>::T s4;
    p_load<RgK, U0>(s0, XS, r);
    p_load<RgK, U1>(s1, XS, r);
    p_load<RgK, U2>(s2, XS, r);
    p_load<RgK, U3>(s3, XS, r);
    p_load<RgK, U4>(s4, XS, r);
    const int ctb = r < 2 ? CT_BUL : CT_ONEN;
    for (int s = 4; s <= s_end; s++) {
        const int umax = min(30, s - 6);
        const int ncell = (s <= N - 1 && umax >= 0) ? uni(L.rcnt[RgK::slot(s)]) : 0;
        for (int c0 = 0; c0 < ncell; c0 += WAVE / 4) {
            const int idx = c0 + cq;
            const BRec q = brec_load<H5, TB>(brec_at<RgK>(L, RgK::slot(s), idx));
            pb_batch<RgK, U0, U1, U2, U3, U4>(L, s0, s1, s2, s3, s4, q, eTAU, s, umax, r, ctb, idx, ncell, wid,
                                              constrained PF_STP_ARGS);
        }
        PF_STAMP(3);
        lds_barrier();
        PF_STAMP(7);   // barrier
    }
}

// ---- refold restore of qm (row-major) and qm1 (column-major) from the slot's
// diagonal-major tables, one diagonal per wave, lanes = cells, and of q5 up to
// the changed band.  A wave's (diagonal, lane-set) items go in batches of RB:
// every load of a batch in flight before its stores (round 6; a load -> store
// pair per item waited on HBM once per item)
__device__ __forceinline__ void rg_restore(const RgL &L, const float *src, size_t Cs, int m_lo, int tid, int lane,
                                           int wid) {
    const int N = L.N;
    constexpr int RB = 8;
    int D = 4 + wid, i0 = 1;
    const float q5v = src[3 * Cs + min(tid, N)];
    while (D <= N - 1) {
        float va[RB], vb[RB];
        int ia[RB], ib[RB];
#pragma unroll
        for (int k = 0; k < RB; k++) {
            const int i = i0 + lane;
            const bool ok = D <= N - 1 && i <= N - D;
            const int c = ok ? off(D, N) + i - 1 : 0;
            va[k] = src[Cs + c];
            vb[k] = src[2 * Cs + c];
            ia[k] = ok ? rowb(i, N) + D - 4 : -1;
            ib[k] = colb(i + D) + i - 1;
            if (D <= N - 1) {   // next item (uniform)
                i0 += WAVE;
                if (i0 > N - D) {
                    D += RG_NW;
                    i0 = 1;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RB; k++)
            if (ia[k] >= 0) {
                L.qm[ia[k]] = va[k];
                L.q1[ib[k]] = vb[k];
            }
    }
    if (tid <= m_lo - 2 && tid <= N) L.q5[tid] = q5v;
}

// The changed cells' multiloop stems in qm1 (F reads them before it overwrites
// them) and the rank lists of the changed pairable cells (the B lanes):
// cl[off(D) + rank] = i, cn[D] = count; wave w: diagonals 4 + w, 4 + w + NW, ...
__device__ __forceinline__ void rg_stem_pass(const RgL &L, const Band &bd, int lane, int wid) {
    const int N = L.N;
    const uint8_t *S = L.S;
    for (int D = 4 + wid; D <= N - 1; D += RG_NW) {
        const int od = off(D, N), lo = bd.clo(D), hi = bd.chi(D);
        int base = 0;
        for (int i0 = lo; i0 <= hi; i0 += WAVE) {   // the changed band's rows (round 6: every row before)
            const int i = i0 + lane;
            bool pr = false;
            if (i <= hi) {
                const int j = i + D;
                const int type = ptype(S[i], S[j]);
                pr = type != 0 && allowed(L, i, j);
                L.q1[colb(j) + i - 1] = pr ? L.dt[DT_MLS + type * 25 + S[i - 1] * 5 + S[j + 1]] : 0.f;
            }
            base = pf_rank_push(L, od, base, pr, i);
        }
        if (lane == 0) L.cn[D] = uint8_t(base);
    }
}

// ---- prep of lane-set h of diagonal D into the ring (lane-sets 0, 1, 2 on
// waves 12, 13 and R): inner codes; the changed cells' hairpin (+ motif)
// initial values or the non-pairable mark (-0, also stored to the slot qbg);
// the restored values of the others (rsv, loaded one step ahead: rg_rload) and
// their slot copies
__device__ __forceinline__ void rg_rload(const RgL &L, const Band &bd, const float *src, int D, int h, int lane,
                                         float &rsv) {
    const int N = L.N;
    if (!src || D < 4 || D > N - 1) return;
    const int od = off(D, N), lo = bd.clo(D), hi = bd.chi(D);
    const int i = 1 + h * WAVE + lane;
    if (h * WAVE < N - D && i <= N - D && (i < lo || i > hi)) rsv = src[od + i - 1];
}
__device__ __forceinline__ void rg_prep(const RgL &L, const Band &bd, float *qbg, int D, int h, int lane, float rsv,
                                        int mL, float mext, bool hol) {
    const int N = L.N;
    const uint8_t *S = L.S;
    if (D < 4 || D > N - 1) return;
    const int od = off(D, N), ro = rgo(D, L.RS), lo = bd.clo(D), hi = bd.chi(D);
    const int i = 1 + h * WAVE + lane;
    if (h * WAVE >= N - D || i > N - D) return;
    const int j = i + D;
    const int type = ptype(S[i], S[j]);
    L.cc[ro + i - 1] = uint8_t(rtype(type) * 25 + S[j + 1] * 5 + S[i - 1]);
    if (i >= lo && i <= hi) {
        float init = -0.f;
        if (type != 0 && allowed(L, i, j))
            init = pf_hairpin_init<RgK>(L, i, j, D, type, 0.f, 0, mL, mext, hol, hol);
        else
            qbg[od + i - 1] = -0.f;   // non-pairable: the mark, final
        L.qb[ro + i - 1] = init;
    } else {   // restored (final)
        L.qb[ro + i - 1] = rsv;
        qbg[od + i - 1] = rsv;
    }
}

// Q: column `col` of qb (qv, from the slot / scratch qbg) and its exterior-stem
// factors (qf), cells (k, col), k <= col - 4, three lane-sets; gathered a step
// ahead of q5[col]
struct RgCol {
    float qf[RG_SETS], qv[RG_SETS];
    int col;
};
__device__ __forceinline__ void rg_qload(const RgL &L, const Band &bd, const float *qbg, int j, int lane, RgCol &c) {
    const int N = L.N;
    const uint8_t *S = L.S;
    c.col = -1;
    if (j < 5 || j > N || (bd.incr && j < bd.m_lo - 1)) return;
    c.col = j;
    const int sjp = (j < N) ? S[j + 1] : 5;
    const int sj = S[j];
#pragma unroll
    for (int h = 0; h < RG_SETS; h++) {
        const int kk = 1 + h * WAVE + lane;
        const bool ok = kk <= j - 4;
        const int k = ok ? kk : 1;
        const int ty = ptype(S[k], sj);
        const int code = rtype(ty) * 25 + S[j + 1] * 5 + S[k - 1];   // the cell's inner code (S wraps)
        const float f = pf_ext_factor(L, k, ty, sjp, code);
        c.qf[h] = ok ? f : 0.f;
        c.qv[h] = ok && h * WAVE < j - 4 ? qbg[off(j - k, N) + k - 1] : 0.f;
    }
}
// Q: q5[j] from the column loaded last step
__device__ __forceinline__ void rg_q5(const RgL &L, const Band &bd, int j, int lane, const RgCol &c, float sig1) {
    if (j >= 4 && j <= L.N && (!bd.incr || j >= bd.m_lo - 1)) {
        float acc = 0.f;
        if (c.col == j) {
#pragma unroll
            for (int h = 0; h < RG_SETS; h++) {
                if (h * WAVE >= j - 4) break;
                const int kk = 1 + h * WAVE + lane;
                const int k = kk <= j - 4 ? kk : 1;
                acc = fmaf(L.q5[k - 1] * c.qv[h], c.qf[h], acc);
            }
        }
        acc = wave_sum_dpp(acc);
        if (lane == 0) L.q5[j] = (L.up[j] >= 1 ? L.q5[j - 1] * sig1 : 0.f) + acc;
    }
}

// the proposal's qm / qm1 to the slot, diagonal-major (qb is there already), and q5
__device__ __forceinline__ void rg_write_back(const RgL &L, float *dst, size_t Cs, int tid, int lane, int wid) {
    const int N = L.N;
    for (int D = 4 + wid; D <= N - 1; D += RG_NW) {
        const int od = off(D, N);
        for (int i = 1 + lane; i <= N - D; i += WAVE) {
            dst[Cs + od + i - 1] = L.qm[rowb(i, N) + D - 4];
            dst[2 * Cs + od + i - 1] = L.q1[colb(i + D) + i - 1];
        }
    }
    for (int k = tid; k <= N; k += RG_NT) dst[3 * Cs + k] = L.q5[k];
}

// One workgroup per (walker, variant of a groups2 pair).  gout: [W][n_variants]
// ensemble energies (kcal/mol); qscr: per workgroup C floats of qb when the fold
// keeps no state (adx_score_batch), else null (the slot holds qb).
__global__ void __launch_bounds__(RG_NT, 1)
pf_ring_kernel(KArgs ka, const DevScaled *__restrict__ XS, const uint8_t *seqs, int W, const int *mask,
               float *gout, float *qscr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ng = 2 * ka.n_groups2;
    const int wb = blockIdx.x / ng, rem = blockIdx.x % ng;
    const int grp = rem >> 1, half = rem & 1;
    if (wb >= W) return;
    const WalkerRef wr = walker_ref(ka, mask, wb);   // heaviest refolds first
    if (!wr.on) return;
    const int w = wr.w;
    const int v0 = ka.groups2[2 * grp], vh = ka.groups2[2 * grp + half];
    if (half == 1 && vh == v0) return;   // a lone variant: one fold
    const DevVariant V = ka.variants[vh];
    const bool hol = V.motif != 0;
    const int N = uni(V.N);
    const RgLay Y(N);
    RgL L = pf_carve<RgK>(smem, Y, N);
    L.RS = Y.RS;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = uni(tid / WAVE);
    const int C = Y.C, NP = Y.NP, RS = Y.RS;
    const DevTables &T = *ka.T;
#ifdef ADX_STAMP
    unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif

    // ---- incremental fold state (as pf_cells.hip): this variant's tables of the
    // current sequence (src) and the proposal's (dst), diagonal-major
    const size_t Cs = size_t(ka.cells), B1 = 3 * Cs + size_t(ka.Nmax) + 2;
    const float *src = nullptr;
    float *dst = nullptr;
    int m_lo = 0, m_hi = 0;
    if (ka.tab) {
        const int cur = wr.cur;
        float *base = ka.tab + size_t(w) * 2 * ka.tab_slot;
        dst = base + size_t(1 - cur) * ka.tab_slot + size_t(grp) * 2 * B1 + size_t(half) * B1;
        if (wr.valid && wr.c0 >= 0) {
            src = base + size_t(cur) * ka.tab_slot + size_t(grp) * 2 * B1 + size_t(half) * B1;
            m_lo = wr.c0 + 1 + V.before_len;
            m_hi = wr.c1 + 1 + V.before_len;
        }
    }
    // qb of every cell, read back by Q: the slot, or this workgroup's scratch
    float *qbg = dst ? dst : qscr + size_t(blockIdx.x) * Cs;
    const bool incr = src != nullptr;
    const Band bd{incr, N, uni(m_lo), uni(m_hi)};

    // ---- setup (round 6, as pf_cells.hip): every load in flight at once, then the stores
    const auto su = pf_setup_load<RgK>(ka, XS, V, seqs, w, tid, lane, wid, N, NP);
    const bool cst = pf_setup_store<RgK>(L, su, tid, N, NP);
    for (int k = tid; k < 2 * NP; k += RG_NT) L.mla[k] = 0.f;
    for (int k = C + tid; k < C + PF_SLACK; k += RG_NT) L.qm[k] = L.q1[k] = 0.f;
    for (int k = tid; k < RG_RING * RS; k += RG_NT) {
        L.qb[k] = 0.f;
        L.cc[k] = 0;
    }
    const bool constrained = __syncthreads_or(cst);
    const int mL = XS->motif_len;
    pf_motif_sites<RgK>(L, hol && mL > 0, mL, tid, lane, wid);
    if (incr) {
        rg_restore(L, src, Cs, bd.m_lo, tid, lane, wid);
    } else {
        for (int k = tid; k < C; k += RG_NT) L.qm[k] = 0.f;   // spans N-2, N-1 are never computed
    }
    __syncthreads();
    const float sig1 = XS->sig[1], mlbase_sig = XS->mlbase_sig, mlclosing = XS->mlclosing;
    const float mext = XS->motif_extra;
    rg_stem_pass(L, bd, lane, wid);
    pf_q5_prefix<RgK>(L, sig1, tid);
    __syncthreads();

    // this wave's prep lane-set: the two M waves with the fewest items and R
    const int ph = wid == 12 ? 0 : wid == 13 ? 1 : wid == RG_WR ? 2 : -1;
    float rsv = 0.f;   // the lane's restored value of the next prep
    // ---- records (wave R, pf_common.hpp), three lane-sets
    Pend<RG_SETS> pend;
    Seq<RG_SETS> seqp;
    Idx<RG_SETS> idxp;
    if (wid == RG_WR) {
        rec_store<RgK>(L, 4, rec_load<RgK>(L, T, 4, seq_load<RgK>(L, 4, idx_load<RgK>(L, 4, lane)), lane), lane);
        pend = rec_load<RgK>(L, T, 5, seq_load<RgK>(L, 5, idx_load<RgK>(L, 5, lane)), lane);
        seqp = seq_load<RgK>(L, 6, idx_load<RgK>(L, 6, lane));
        idxp = idx_load<RgK>(L, 7, lane);
    }
    if (ph >= 0) {   // diagonal 4 before the sweep, diagonal 5's restored values in flight
        rg_rload(L, bd, src, 4, ph, lane, rsv);
        rg_prep(L, bd, qbg, 4, ph, lane, rsv, mL, mext, hol);
        vm_drain();
        rg_rload(L, bd, src, 5, ph, lane, rsv);
    }
    __syncthreads();

    RgCol qc = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, -1};   // Q: the column loaded for the next q5
    const int s_end = N + 3;   // Q finishes q5[N] three steps after column N is final
    PF_STAMP(0);   // setup
    if (wid < RG_NB) {
        // (moving 16, 13 or 0 off block 4, the busiest in the stamps, was no faster:
        // profiles/r06u_pf_ring_stamps.txt)
        switch (wid) {
            case 0: rb_sweep<5, 22, 12, 11, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 1: rb_sweep<4, 21, 19, 10, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 2: rb_sweep<3, 20, 18, 8, 6>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 3: rb_sweep<28, 26, 1, 9, 7>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 4: rb_sweep<29, 27, 16, 13, 0>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            case 5: rb_sweep<30, 2, 17, 14, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
            default: rb_sweep<24, 25, 23, 15, -1>(L, XS, N, lane, wid, constrained, s_end PF_STP_ARGS); break;
        }
    } else {
        __builtin_amdgcn_s_setprio(2);
        // one sweep instance per role (round 6, as pf_cells.hip): the shared loop
        // kept every role's values live (65 SGPR spill reads / writes per step)
        auto sweep = [&](auto role_c) __attribute__((always_inline)) {
            constexpr int ROLE = decltype(role_c)::value;   // 0 M, 1 F, 2 Q, 3 R
            for (int s = 4; s <= s_end; s++) {
                if constexpr (ROLE == 0) {          // M: qm items of span s - 2
                    pf_m_role<RgK>(L, bd, s - 2, rg_mw(wid), lane, constrained, mlbase_sig);
                    if (ph >= 0) {
                        // the prep of lane-set ph of diagonal s + 1 (its restored values were
                        // loaded last step); the drain first completes last step's prep
                        // stores (read by Q two steps on) and loads, a step old by now
                        PF_STAMP(5);
                        vm_drain();
                        rg_prep(L, bd, qbg, s + 1, ph, lane, rsv, mL, mext, hol);
                        PF_STAMP(6);
                        rg_rload(L, bd, src, s + 2, ph, lane, rsv);   // in flight across the barrier
                    }
                } else if constexpr (ROLE == 1) {   // F: the changed cells of diagonal s - 1
                    vm_drain();        // last step's finalised cells (Q loads them this step)
                    pf_f_role<RgK>(L, bd, s - 1, lane, mlclosing, mlbase_sig, qbg);
                } else if constexpr (ROLE == 2) {   // Q: q5[s - 3] from the column loaded last step
                    rg_q5(L, bd, s - 3, lane, qc, sig1);
                    PF_STAMP(5);       // q5
                    pf_uc_update(L, s - 2, lane, constrained, mlbase_sig);
                    // column s - 2 is final: its last cell, (1, s-2), was finalised two steps
                    // ago and its store drained by F at the start of the last step
                    rg_qload(L, bd, qbg, s - 2, lane, qc);
                } else {               // R: its prep lane-set, then the record stages
                    vm_drain();        // last step's prep stores and loads (the record loads are a step old)
                    rg_prep(L, bd, qbg, s + 1, 2, lane, rsv, mL, mext, hol);
                    rg_rload(L, bd, src, s + 2, 2, lane, rsv);
                    rec_store<RgK>(L, s + 1, pend, lane);
                    pend = rec_load<RgK>(L, T, s + 2, seqp, lane);
                    seqp = seq_load<RgK>(L, s + 3, idxp);
                    idxp = idx_load<RgK>(L, s + 4, lane);
                }
                PF_STAMP(3);   // the role's step work
                lds_barrier();
                PF_STAMP(7);   // barrier
            }
        };
        if (rg_mw(wid) >= 0) sweep(std::integral_constant<int, 0>{});
        else if (wid == RG_WF) sweep(std::integral_constant<int, 1>{});
        else if (wid == RG_WQ) sweep(std::integral_constant<int, 2>{});
        else sweep(std::integral_constant<int, 3>{});   // RG_WR
    }
    __syncthreads();
    PF_STAMP(4);
#ifdef ADX_STAMP
    if (lane == 0)
        for (int k = 0; k < 8; k++) atomicAdd(&g_stamps_r[wid][k], st_acc[k]);
#endif
    if (dst) rg_write_back(L, dst, Cs, tid, lane, wid);
    if (tid == 0) gout[size_t(w) * ka.n_variants + vh] = pf_energy(XS, L.q5[N], N);
}

}  // namespace

// LDS bytes of the ring PF kernel for this workload (0: not covered)
size_t pf_ring_lds(const KArgs &ka) {
    if (ka.mode != 0 || ka.Nmax < RG_NMIN || ka.Nmax > RG_NMAX) return 0;
    const size_t b = RgLay(ka.Nmax).BYTES;
    return b + 256 <= size_t(LDS_LIMIT) ? b : 0;
}
// floats of per-workgroup qb scratch a stateless launch needs
size_t pf_ring_scratch_floats(const KArgs &ka, int W) {
    return size_t(W) * 2 * ka.n_groups2 * size_t(ka.cells);
}

hipError_t launch_pf_ring(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, float *gout,
                          float *qscr, hipStream_t stream) {
    const size_t lds = pf_ring_lds(ka);
    if (lds == 0 || (!ka.tab && !qscr)) return hipErrorInvalidValue;
    hipError_t e = configure_dynamic_lds(pf_ring_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pf_ring_kernel, dim3(W * 2 * ka.n_groups2), dim3(RG_NT), lds, stream, ka, ka.X, seqs, W, mask,
                       gout, qscr);
    return hipGetLastError();
}

}  // namespace adx

#ifdef ADX_STAMP
extern "C" int adx_debug_stamps_ring(unsigned long long *out, int reset) {  // [16][8]
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(adx::g_stamps_r), sizeof(adx::g_stamps_r)) != hipSuccess) return 1;
    if (reset) {
        static unsigned long long z[16][8] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(adx::g_stamps_r), z, sizeof(z)) != hipSuccess) return 2;
    }
    return 0;
}
#endif
