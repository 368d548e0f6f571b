// What the lanes = cells PF inside kernels share (pf_cells.hip: the apo | holo
// pair of a group as float2, every table whole in LDS; pf_ring.hip: one fold
// in FP32, qb and the inner codes in a ring of diagonals): the value helpers
// for float / float2, the LDS view and its carve, the interior-loop shapes and
// a B batch of 16 cells, a refold's setup pieces (table and sequence loads,
// motif sites, hairpin initial values, rank lists), the four record stages,
// the M and F roles, the column recursion of Q, the exterior factor and the
// ensemble energy.  The helpers take the kernel's traits K (PxK, RgK: value
// type, block / lane-set / slot counts, record word width, the inner cells'
// base address, the M split loop, the hairpin length factor's home, stamp
// slots).  Where the kernels differ in substance -- the B loop around a batch,
// the exterior sums, restore and write-back, the ring's prep -- the code stays
// in the kernel's file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "dev_types.hpp"
#include "fold_common.hpp"

namespace adx {
namespace {

constexpr int PF_NMW = 4;     // qm item waves
constexpr int PF_RF = 8;      // record fields (rec_store): word, mmo, mo, m23, 1x1..2x2 factors
constexpr int PF_SLACK = 16;

// ---------------------------------------------------------------- values: float or f2
template <class V> __device__ __forceinline__ V splat(float x);
template <> __device__ __forceinline__ float splat<float>(float x) { return x; }
template <> __device__ __forceinline__ f2 splat<f2>(float x) { return f2{x, x}; }
template <class V> __device__ __forceinline__ V vzero() { return splat<V>(0.f); }
// one value per variant of the group (the ring folds one: the first)
template <class V> __device__ __forceinline__ V per_variant(float a, float b);
template <> __device__ __forceinline__ float per_variant<float>(float a, float) { return a; }
template <> __device__ __forceinline__ f2 per_variant<f2>(float a, float b) { return f2{a, b}; }
__device__ __forceinline__ float vfma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ f2 vfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
// g + v * f, f one factor: scalar FMAs (a packed one wants the factor duplicated in a register pair)
__device__ __forceinline__ float vfma_s(float v, float f, float g) { return fmaf(v, f, g); }
__device__ __forceinline__ f2 vfma_s(f2 v, float f, f2 g) { return f2{fmaf(v.x, f, g.x), fmaf(v.y, f, g.y)}; }
// the non-pairable mark (-0; a finished cell never takes it)
__device__ __forceinline__ bool is_mark(float v) { return __float_as_uint(v) == 0x80000000u; }
__device__ __forceinline__ bool is_mark(f2 v) { return __float_as_uint(v.x) == 0x80000000u; }

// Diagnostic builds (-DADX_STAMP): the kernel's stamp locals, handed to the helpers that stamp
#ifdef ADX_STAMP
#define PF_STAMP(k) ADX_STAMP_AT(k)   // fold_common.hpp
#define PF_STP_PARAMS , unsigned long long *st_acc, unsigned long long &st_last
#define PF_STP_ARGS , st_acc, st_last
#else
#define PF_STAMP(k) ((void)(k))
#define PF_STP_PARAMS
#define PF_STP_ARGS
#endif

// ---------------------------------------------------------------- LDS view
template <class V>
struct PfL {
    V *qb, *qm, *q1, *part, *mla, *uc, *q5;
    float *rec, *ct, *dt, *pw;
    int *rcnt;
    uint8_t *cc, *cl, *cn, *S, *up, *dn, *ptn, *enc, *flg, *mat;
    uint32_t *spk;     // special-hairpin keys (padded: no match)
    float *spv;
    uint8_t *mcode;    // motif codes / partners
    int8_t *mpt;
    int N, NP, RS;     // RS: ring row (pf_ring.hip)
};
// Y: the kernel's layout (PxLay, RgLay: byte offsets by the same names)
template <class K, class Lay>
__device__ __forceinline__ PfL<typename K::V> pf_carve(char *smem, const Lay &Y, int N) {
    using V = typename K::V;
    PfL<V> L;
    L.qb = reinterpret_cast<V *>(smem + Y.QB);
    L.qm = reinterpret_cast<V *>(smem + Y.QM);
    L.q1 = reinterpret_cast<V *>(smem + Y.Q1);
    L.cc = reinterpret_cast<uint8_t *>(smem + Y.CC);
    L.part = reinterpret_cast<V *>(smem + Y.PART);
    L.rec = reinterpret_cast<float *>(smem + Y.REC);
    L.rcnt = reinterpret_cast<int *>(smem + Y.REC + size_t(K::REC_SLOTS) * K::SETS * PF_RF * WAVE * 4);
    L.cl = reinterpret_cast<uint8_t *>(smem + Y.CL);       // cl[off(D) + rank] = i
    L.cn = L.cl + Y.C;                                      // cn[D] = count
    L.mla = reinterpret_cast<V *>(smem + Y.MLA);
    L.uc = reinterpret_cast<V *>(smem + Y.UC);
    L.q5 = reinterpret_cast<V *>(smem + Y.Q5);
    L.ct = reinterpret_cast<float *>(smem + Y.CT);
    L.dt = reinterpret_cast<float *>(smem + Y.DT);
    L.pw = reinterpret_cast<float *>(smem + Y.PW);
    uint8_t *by = reinterpret_cast<uint8_t *>(smem + Y.BY);
    L.S = by;
    L.up = by + Y.NP;
    L.dn = by + 2 * Y.NP;
    L.ptn = by + 3 * Y.NP;
    L.enc = by + 4 * Y.NP;
    L.flg = by + 5 * Y.NP;
    L.mat = by + 6 * Y.NP;
    L.spk = reinterpret_cast<uint32_t *>(smem + Y.MT);
    L.spv = reinterpret_cast<float *>(smem + Y.MT + MAX_SPECIAL_HP * 4);
    L.mcode = reinterpret_cast<uint8_t *>(smem + Y.MT + MAX_SPECIAL_HP * 8);
    L.mpt = reinterpret_cast<int8_t *>(L.mcode + MAX_MOTIF);
    L.N = N;
    L.NP = Y.NP;
    L.RS = 0;
    return L;
}

// ---------------------------------------------------------------- interior-loop shapes
struct PfCell {              // per lane: the closing pair (i, i+s)
    int i, ty8, A, B;
    float tau, mo, m23;
    float t11, t12, t21, t22;
};

// shapes n1 = lo .. hi of a constrained cell's size U are allowed (n1 <= A and U - n1 <= B)
__device__ __forceinline__ uint32_t shape_bits(const PfCell &c, int U) {
    const int lo = max(0, U - c.B), hi = min(U, c.A);
    return hi < lo ? 0u : ((2u << hi) - 1u) & ~((1u << lo) - 1u);
}

// One shape (N1, U - N1): the inner cell (i+1+N1, j-1-U+N1) on diagonal s-2-U
// at qb / cc row base + N1 (qb + o, cc + o: this lane's bases).
template <int U, int N1, bool MK, class V>
__device__ __forceinline__ void pshape1(const PfL<V> &L, const PfCell &c, const float *fv, const V *qb,
                                        const uint8_t *cc, uint32_t bits, V &g, V &sp) {
    constexpr int k = loop_kind(N1, U - N1);
    constexpr int FI = N1 < U - N1 ? N1 : U - N1;
    V v = qb[N1];
    // constrained cell: shapes past its unpaired runs count 0 (bit N1 of the size's
    // allowed-n1 mask as a factor: a compare-select becomes a branch around the load)
    if constexpr (MK) v *= splat<V>(float((bits >> N1) & 1u));
    if constexpr (k < 0) {
        g = vfma_s(v, fv[FI], g);
    } else {
        const float *ct = L.ct;
        const int ci = cc[N1];
        float f;
        if constexpr (k == TK_STK || k == TK_B1) {
            f = ct[CT_INVMM + ci] * ct[CT_STK + c.ty8 + ((ci * 41) >> 10)] * fv[FI];
        } else if constexpr (k == TK_BUL) {
            f = ct[CT_BUL + ci] * (c.tau * fv[FI]);
        } else if constexpr (k == TK_1N) {
            f = ct[CT_ONEN + ci] * (c.mo * fv[FI]);
        } else if constexpr (k == TK_M23) {
            f = ct[CT_INVMM + ci] * ct[CT_M23O + ci] * (c.m23 * fv[FI]);
        } else {
            const float tv = k == TK_I11 ? c.t11 : k == TK_I12 ? c.t12 : k == TK_I21 ? c.t21 : c.t22;
            f = ct[CT_INVMM + ci] * (tv * fv[FI]);
        }
        sp = vfma(v, splat<V>(f), sp);
    }
}
template <int U, bool MK, class V, int... N1s>
__device__ __forceinline__ void pshape_seq(std::integer_sequence<int, N1s...>, const PfL<V> &L, const PfCell &c,
                                           const float *fv, const V *qb, const uint8_t *cc, uint32_t bits, V &g,
                                           V &sp) {
    (pshape1<U, N1s, MK>(L, c, fv, qb, cc, bits, g, sp), ...);
}
// A size <= 5 (the stack, 1x1..2x3 table loops), every shape by one lane.  Every
// shape factor is symmetric in (n1, n2) (setup_core.hpp build_scaled): a size keeps
// U/2 + 1 of them, shape n1 reads fv[min(n1, U - n1)]
template <class K, int U>
struct PSize {
    using V = typename K::V;
    float fv[U < 0 ? 1 : U / 2 + 1];
    __device__ __forceinline__ void load(const DevScaled *XS) {
        if constexpr (U >= 0)
#pragma unroll
            for (int n1 = 0; n1 <= U / 2; n1++) fv[n1] = shape_factor(XS, U, n1);   // uniform: SGPRs
    }
    template <bool MK>
    __device__ __forceinline__ void run(const PfL<V> &L, const PfCell &c, int s, int umax, V &g, V &sp) const {
        if constexpr (U >= 0) {
            if (U <= umax) {
                const int o = K::inner(L, s - 2 - U) + c.i;   // inner cell (i+1+n1, ...) at o + n1
                const uint32_t bits = MK ? shape_bits(c, U) : 0u;
                pshape_seq<U, MK>(std::make_integer_sequence<int, U + 1>{}, L, c, fv, L.qb + o, L.cc + o, bits, g,
                                  sp);
            }
        }
    }
};

// Loop size U >= 6 over the four lanes of a cell (phase r = lane & 3): lane r
// takes one of the four special shapes -- bulges (0,U) (U,0), 1 x n loops
// (1,U-1) (U-1,1) -- and the generic shapes n1 = 2 + r, 6 + r, ... <= U - 2
// (one read at a per-lane base + immediate offset 4m, its factor in a VGPR;
// 0 past the size, so the last round needs no mask).  Every lane runs the same
// code; the four lanes' sums are added in a fixed order (bit-identical refolds).
template <class K, int U>
struct PSizeQ {
    using V = typename K::V;
    static constexpr int NR = U >= 6 ? (U - 3 + 3) / 4 : 1;   // generic rounds
    float gf[NR];
    float fsp;      // the lane's special-shape factor (bulge FB[U] or 1 x n F1N[U-1])
    int n1sp;       // the lane's special shape
    __device__ __forceinline__ void load(const DevScaled *XS, int r) {
#pragma unroll
        for (int m = 0; m < NR; m++) {
            const int n1 = 2 + 4 * m + r;
            gf[m] = n1 <= U - 2 ? XS->fgen[(U - 6) * FG_ROW + n1 - 2] : 0.f;
        }
        n1sp = r == 0 ? 0 : r == 1 ? U : r == 2 ? 1 : U - 1;
        fsp = r < 2 ? XS->ctab[CT_FB + U] : XS->ctab[CT_F1N + U - 1];
    }
    template <bool MK>
    __device__ __forceinline__ void run(const PfL<V> &L, const PfCell &c, int s, int umax, int r, int ctb,
                                        float outer, V &g, V &sp) const {
        if (U <= umax) {
            const int o = K::inner(L, s - 2 - U) + c.i;   // inner cell (i+1+n1, ...) at o + n1
            const uint32_t bits = MK ? shape_bits(c, U) : ~0u;
            // special shape of this lane
            {
                V v = L.qb[o + n1sp];
                if constexpr (MK) v *= splat<V>(float((bits >> n1sp) & 1u));
                const int ci = L.cc[o + n1sp];
                sp = vfma(v, splat<V>(L.ct[ctb + ci] * (outer * fsp)), sp);
            }
            // generic shapes n1 = 2 + r + 4m
            const V *q = L.qb + o + 2 + r;
            const uint32_t bm = bits >> (2 + r);
#pragma unroll
            for (int m = 0; m < NR; m++) {
                V v = q[4 * m];
                if constexpr (MK) v *= splat<V>(float((bm >> (4 * m)) & 1u));
                g = vfma_s(v, gf[m], g);
            }
        }
    }
};

template <class K, int U>
struct PBlk {   // the size's state in a B wave
    using T = typename std::conditional<(U < 0), PSize<K, -1>,
                                        typename std::conditional<(U <= 5), PSize<K, U>, PSizeQ<K, U>>::type>::type;
};
template <class K, int U, bool MK>
__device__ __forceinline__ void p_run(const typename PBlk<K, U>::T &z, const PfL<typename K::V> &L, const PfCell &c,
                                      int s, int umax, int r, int ctb, float outer, typename K::V &g,
                                      typename K::V &sp, typename K::V &gs, typename K::V &sps) {
    if constexpr (U < 0) {
    } else if constexpr (U <= 5) {
        // counted on phase 0 only: the other phases skip the reads (LDS cycles)
        if (!ADX_SMALL_R0 || r == 0) z.template run<MK>(L, c, s, umax, gs, sps);
    } else {
        z.template run<MK>(L, c, s, umax, r, ctb, outer, g, sp);
    }
}
template <class K, int U>
__device__ __forceinline__ void p_load(typename PBlk<K, U>::T &z, const DevScaled *XS, int r) {
    if constexpr (U < 0) {
    } else if constexpr (U <= 5) {
        z.load(XS);
    } else {
        z.load(XS, r);
    }
}

// ---------------------------------------------------------------- B: one batch of 16 cells
// A cell's record (rec_store), read by the four lanes of the cell.  Word: i |
// ty << IB | A << IB+3 | B << IB+11 | masked << IB+19 | real << IB+20 (IB: the
// width of i).  A block reads only the fields its sizes use (H5: the 2x3 loops'
// m23; TB: the 1x1..2x2 table factors)
struct BRec {
    int fl;
    float mmo, mo, m23, t11, t12, t21, t22;
};
// the records of slot sl (a diagonal's, K::slot), cell idx of the diagonal's rank list
template <class K>
__device__ __forceinline__ const float *brec_at(const PfL<typename K::V> &L, int sl, int idx) {
    return L.rec + ((sl * K::SETS + (idx >> 6)) * PF_RF) * WAVE + (idx & (WAVE - 1));
}
template <bool H5, bool TB>
__device__ __forceinline__ BRec brec_load(const float *rr) {
    BRec q;
    q.fl = __float_as_int(rr[0]);
    q.mmo = rr[WAVE];
    q.mo = rr[2 * WAVE];
    q.m23 = H5 ? rr[3 * WAVE] : 0.f;
    q.t11 = q.t12 = q.t21 = q.t22 = 0.f;
    if constexpr (TB) {
        q.t11 = rr[4 * WAVE];
        q.t12 = rr[5 * WAVE];
        q.t21 = rr[6 * WAVE];
        q.t22 = rr[7 * WAVE];
    }
    return q;
}
// The five sizes of block wid on the lane's cell (record q, cell idx of ncell
// on diagonal s): sizes >= 6 as PSizeQ (shapes spread over the phases), sizes
// <= 5 computed whole and counted once (phase 0).  The four partials are summed
// by DPP and phase 0 writes the cell's natural slot of the step's parity.
template <class K, int U0, int U1, int U2, int U3, int U4>
__device__ __forceinline__ void pb_batch(const PfL<typename K::V> &L, const typename PBlk<K, U0>::T &s0,
                                         const typename PBlk<K, U1>::T &s1, const typename PBlk<K, U2>::T &s2,
                                         const typename PBlk<K, U3>::T &s3, const typename PBlk<K, U4>::T &s4,
                                         const BRec &q, float eTAU, int s, int umax, int r, int ctb, int idx,
                                         int ncell, int wid, bool constrained PF_STP_PARAMS) {
    using V = typename K::V;
    const int fl = q.fl;
    PfCell c;
    c.i = fl & ((1 << K::IB) - 1);
    const int ty = (fl >> K::IB) & 7;
    c.ty8 = ty * 8;
    c.A = (fl >> (K::IB + 3)) & 255;
    c.B = (fl >> (K::IB + 11)) & 255;
    const float mmo = q.mmo;
    c.tau = ty > 2 ? eTAU : 1.f;
    c.mo = q.mo;
    c.m23 = q.m23;
    c.t11 = q.t11;
    c.t12 = q.t12;
    c.t21 = q.t21;
    c.t22 = q.t22;
    const float outer = r < 2 ? c.tau : c.mo;
    V g = vzero<V>(), sp = vzero<V>(), gs = vzero<V>(), sps = vzero<V>();
    PF_STAMP(K::ST_REC);   // B cell records
    // shapes past a cell's allowed unpaired runs (constraints) are masked
    const bool mk = constrained && __ballot((fl >> (K::IB + 19)) & 1) != 0;
    if (mk) {
        p_run<K, U0, true>(s0, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
        p_run<K, U1, true>(s1, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
        p_run<K, U2, true>(s2, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
        p_run<K, U3, true>(s3, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
        p_run<K, U4, true>(s4, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
    } else {
        p_run<K, U0, false>(s0, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
        p_run<K, U1, false>(s1, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
        p_run<K, U2, false>(s2, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
        p_run<K, U3, false>(s3, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
        p_run<K, U4, false>(s4, L, c, s, umax, r, ctb, outer, g, sp, gs, sps);
    }
    // small sizes count once (phase 0), then the cell's total over its four lanes
    const V part = quad_sum(vfma(g, splat<V>(mmo), sp) + (r == 0 ? vfma(gs, splat<V>(mmo), sps) : vzero<V>()));
    if (r == 0 && idx < ncell && ((fl >> (K::IB + 20)) & 1))
        L.part[(((s & 1) * K::SETS + ((c.i - 1) >> 6)) * K::NB + wid) * WAVE + ((c.i - 1) & (WAVE - 1))] = part;
    PF_STAMP(K::ST_SHAPES);   // B shapes
}

// ---------------------------------------------------------------- setup
// The one element (ct: NCT) of every table and of the sequence / constraint
// arrays a thread stores, all loads in flight at once (a loop per table waited
// on each load in turn: ~14k cycles per group), then the stores.  hp: the
// kernel's hairpin length factor (K::hp_load: a register of pf_cells, dt[DT_HP]
// of the ring)
template <int NCT>
struct PfSetup {
    float ct[NCT], mh, mi, ms, ex, tau, pw, hp, spv;
    uint32_t spk;
    int n_sp;
    uint8_t mc, s, up, dn, pt, en, fl;
    int8_t mp;
};
template <class K>
constexpr int pf_nct() { return (CT_SIZE + K::NT - 1) / K::NT; }

template <class K>
__device__ __forceinline__ PfSetup<pf_nct<K>()> pf_setup_load(const KArgs &ka, const DevScaled *XS,
                                                              const DevVariant &V, const uint8_t *seqs, int w, int tid,
                                                              int lane, int wid, int N, int NP) {
    static_assert(288 <= K::NT && K::NMAX + 9 <= K::NT && MAX_SPECIAL_HP <= K::NT && MAX_MOTIF <= K::NT &&
                  K::NMAX + 2 <= K::NT, "one setup element per thread");
    const DevTables &T = *ka.T;
    PfSetup<pf_nct<K>()> u;
#pragma unroll
    for (int t = 0; t < pf_nct<K>(); t++) u.ct[t] = XS->ctab[min(tid + t * K::NT, CT_SIZE - 1)];
    u.mh = (&T.mmH[0][0][0])[min(tid, 199)];
    u.mi = (&T.mmI[0][0][0])[min(tid, 199)];
    u.ms = (&T.mlstem[0][0][0])[min(tid, 199)];
    u.ex = (&T.ext[0][0][0])[min(tid, 287)];
    u.tau = T.termAU[tid & 7];
    u.hp = K::hp_load(XS, tid, lane, wid, N);
    u.pw = XS->pwml[min(tid, N + 8)];
    u.n_sp = XS->n_special;
    u.spk = XS->sp_key[min(tid, MAX_SPECIAL_HP - 1)];
    u.spv = XS->sp_val[min(tid, MAX_SPECIAL_HP - 1)];
    u.mc = XS->motif_code[min(tid, MAX_MOTIF - 1)];
    u.mp = XS->motif_pt[min(tid, MAX_MOTIF - 1)];
    const uint8_t *cons = ka.cons + V.cons_off;
    const int kp = min(tid, NP - 1);   // this thread's position
    const SeqSrc src = seq_src(ka, V, seqs + size_t(w) * ka.Nraw);
    u.s = *src.at(kp >= 1 && kp <= N ? kp - 1 : src.blen);   // outside 1..N: a valid byte, discarded
    u.up = cons[kp];
    u.dn = cons[NP + kp];
    u.pt = cons[2 * NP + kp];
    u.en = cons[3 * NP + kp];
    u.fl = cons[4 * NP + kp];
    return u;
}
// the stores (fold_rows.hip pf_group setup); true when this thread's position is constrained
template <class K>
__device__ __forceinline__ bool pf_setup_store(const PfL<typename K::V> &L, const PfSetup<pf_nct<K>()> &u, int tid,
                                               int N, int NP) {
    if (tid < NP) {
        L.S[tid] = (tid >= 1 && tid <= N) ? u.s : 0;
        L.up[tid] = u.up;
        L.dn[tid] = u.dn;
        L.ptn[tid] = u.pt;
        L.enc[tid] = u.en;
        L.flg[tid] = u.fl;
        L.mat[tid] = 0;
    }
#pragma unroll
    for (int t = 0; t < pf_nct<K>(); t++)
        if (tid + t * K::NT < CT_SIZE) L.ct[tid + t * K::NT] = u.ct[t];
    if (tid < 200) {
        L.dt[DT_MMH + tid] = u.mh;
        L.dt[DT_MMI + tid] = u.mi;
        L.dt[DT_MLS + tid] = u.ms;
    }
    if (tid < 288) L.dt[DT_EXT + tid] = u.ex;
    if (tid < 8) L.dt[DT_TAU + tid] = u.tau;
    if constexpr (K::HP_LDS)
        if (tid <= N) L.dt[DT_HP + tid] = u.hp;
    if (tid < N + 9) L.pw[tid] = u.pw;
    if (tid < MAX_SPECIAL_HP) {
        const bool on = tid < u.n_sp;
        L.spk[tid] = on ? u.spk : 0xFFFFFFFFu;   // hp_key never sets the top bits
        L.spv[tid] = on ? u.spv : 0.f;
    }
    if (tid < MAX_MOTIF) {
        L.mcode[tid] = u.mc;
        L.mpt[tid] = u.mp;
    }
    return tid >= 1 && tid <= N && (u.fl | u.pt) != 0;
}

// ViennaRNA's S1 wrap-around, then the motif sites: the sequence (one lane per
// start), then the constraints of each matching start (one wave per start,
// lanes = motif positions).  Every thread of the workgroup calls it (barriers)
template <class K>
__device__ __forceinline__ void pf_motif_sites(const PfL<typename K::V> &L, bool any_motif, int mL, int tid, int lane,
                                               int wid) {
    const int N = L.N;
    if (tid == 0) wrap_ends(L, N);
    __syncthreads();
    if (any_motif) {
        motif_scan<K::NT>(L, L.mcode, mL, N, tid);
        __syncthreads();
        motif_constraints<K::NW>(L, L.mpt, mL, N, wid, lane);
    }
}

// Hairpin (+ motif) initial value of the changed pairable cell (i, j), j - i =
// D, of pair type `type`; hpl, wid: where K::hp_len finds the length factor
// hp[D - 1]; hol0 / hol1: the group's variants that carry the motif (the ring
// folds one)
template <class K>
__device__ __forceinline__ typename K::V pf_hairpin_init(const PfL<typename K::V> &L, int i, int j, int D, int type,
                                                         float hpl, int wid, int mL, float mext, bool hol0,
                                                         bool hol1) {
    using V = typename K::V;
    const uint8_t *S = L.S;
    const int u = D - 1;
    float h = 0.f;
    if (L.up[i + 1] >= u) {
        bool special = false;
        if (u == 3 || u == 4 || u == 6) {
            const int sh = special_hp(L.spk, hp_key(S, i, u + 2));
            if (sh >= 0) {
                h = L.spv[sh];
                special = true;
            }
        }
        if (!special)
            // L.dt[hairpin_dt_index(u, type, S[i+1], S[j-1])], open-coded as a select between two
            // loads (the index form cost pf_cells_kernel 0.3 %, profiles/fold_setup_ab.txt)
            h = K::hp_len(L, hpl, D, wid) *
                ((u == 3) ? L.dt[DT_TAU + type] : L.dt[DT_MMH + type * 25 + S[i + 1] * 5 + S[j - 1]]);
    }
    const bool mx = (hol0 || hol1) && D == mL - 1 && mL > 0 && L.mat[i];
    return per_variant<V>((mx && hol0) ? h + mext : h, (mx && hol1) ? h + mext : h);
}

// Rank list of the changed pairable cells of a diagonal (the B lanes): the
// wave's lanes with pr append their i to cl[od + base ...]; the new base
template <class V>
__device__ __forceinline__ int pf_rank_push(const PfL<V> &L, int od, int base, bool pr, int i) {
    const uint64_t m = __ballot(pr);
    const int slot = base + __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
    if (pr) L.cl[od + slot] = uint8_t(i);
    return base + __popcll(m);
}

// q5[0..3] (pf_group: unpaired prefix)
template <class K>
__device__ __forceinline__ void pf_q5_prefix(const PfL<typename K::V> &L, float sig1, int tid) {
    for (int k = tid; k <= 3 && k <= L.N; k += K::NT) {
        float q = 1.f;
        bool ok = true;
        for (int t = 1; t <= k; t++) {
            ok = ok && L.up[t] >= 1;
            q *= sig1;
        }
        L.q5[k] = ok ? splat<typename K::V>(q) : vzero<typename K::V>();
    }
}

// ---------------------------------------------------------------- R: records
// The changed pairable cells of diagonal D (rank lists) and their setup values
// -- outer factors of the closing pair, the unpaired runs, the 1x1..2x2 table
// factors (HBM/L2 loads) -- in four stages a step apart, one LDS round trip
// each: idx_load (rank list), seq_load (bases), rec_load (tables: LDS factors,
// HBM/L2 1x1..2x2 factors), rec_store, so the table loads complete in the
// shadow of a step.  Per lane-set k (SETS of them): lane l holds cell k * 64 + l
// K::REC_LAZY: seq_load and rec_load leave the lane-sets past the count unset
// (no stage reads them) instead of zeroed.  The R wave runs at a raised
// priority beside B waves, so its instructions cost them issue slots, and the
// form is per kernel because it measured opposite ways (profiles/pfcommon_ab.txt):
// zeroed on pf_cells -0.74 % PF against the parent and unset -0.19 %; unset on
// pf_ring -0.93 % config 4 and zeroed -0.38 %
template <int SETS>
struct Idx {                     // i of the lane's cell (the first cell on idle lanes)
    int n;
    int i[SETS];
};
template <int SETS>
struct Seq {                     // i and the bases around the closing pair
    int n;
    int i[SETS], sq[SETS];       // sq: ty | si1 << 4 | sj1 << 8 | si2 << 12 | sj2 << 16
    int ab[SETS];                // A | B << 8
};
template <int SETS>
struct Pend {
    int n;                       // cells
    int w1[SETS];                // the record word (BRec)
    float mmo[SETS], mo[SETS], m23[SETS], t11[SETS], t12[SETS], t21[SETS], t22[SETS];
};
template <class K>
__device__ __forceinline__ Idx<K::SETS> idx_load(const PfL<typename K::V> &L, int D, int lane) {
    const int N = L.N;
    Idx<K::SETS> X;
    X.n = 0;
#pragma unroll
    for (int k = 0; k < K::SETS; k++) X.i[k] = 1;
    if (D < 6 || D > N - 1) return X;
    const int od = off(D, N);
    X.n = uni(L.cn[D]);
    const int i0 = L.cl[od];
#pragma unroll
    for (int k = 0; k < K::SETS; k++) {
        const int idx = k * WAVE + lane;
        const int ir = L.cl[od + min(idx, N - D - 1)];
        X.i[k] = idx < X.n ? ir : i0;
    }
    return X;
}
template <class K>
__device__ __forceinline__ Seq<K::SETS> seq_load(const PfL<typename K::V> &L, int D, const Idx<K::SETS> &X) {
    const uint8_t *S = L.S;
    Seq<K::SETS> Q;
    Q.n = X.n;
#pragma unroll
    for (int k = 0; k < K::SETS; k++) {
        if (K::REC_LAZY && k * WAVE >= Q.n) break;
        Q.i[k] = X.i[k];
        Q.sq[k] = 0;
        Q.ab[k] = 0;
        if (k * WAVE >= Q.n) continue;
        const int i = X.i[k], j = i + D;
        Q.sq[k] = ptype(S[i], S[j]) | (S[i + 1] << 4) | (S[j - 1] << 8) | (S[i + 2] << 12) | (S[j - 2] << 16);
        Q.ab[k] = L.up[i + 1] | (L.dn[j - 1] << 8);
    }
    return Q;
}
template <class K>
__device__ __forceinline__ Pend<K::SETS> rec_load(const PfL<typename K::V> &L, const DevTables &T, int D,
                                                  const Seq<K::SETS> &Q, int lane) {
    const float *ct = L.ct;
    Pend<K::SETS> P;
    P.n = Q.n;
    const int umax = min(30, D - 6);
#pragma unroll
    for (int k = 0; k < K::SETS; k++) {
        if (K::REC_LAZY && k * WAVE >= Q.n) break;
        P.w1[k] = 0;
        P.mmo[k] = P.mo[k] = P.m23[k] = P.t11[k] = P.t12[k] = P.t21[k] = P.t22[k] = 0.f;
        if (k * WAVE >= Q.n) continue;
        const bool v = k * WAVE + lane < Q.n;
        const int i = Q.i[k], sqk = Q.sq[k];
        const int ty = sqk & 15, si1 = (sqk >> 4) & 15, sj1 = (sqk >> 8) & 15, si2 = (sqk >> 12) & 15,
                  sj2 = (sqk >> 16) & 15;
        const int oc = ty * 25 + si1 * 5 + sj1;
        const int A = Q.ab[k] & 255, Bq = Q.ab[k] >> 8;
        // fold_rows.hip load_chunk: the table factors of the 1x1..2x2 loops (their
        // inner codes: diagonals D-4 .. D-6)
        auto t2of = [&](int n1, int n2) { return (L.cc[K::inner(L, D - 2 - n1 - n2) + i + n1] * 41) >> 10; };
        if (umax >= 2) P.t11[k] = T.int11[ty][t2of(1, 1)][si1][sj1];
        if (umax >= 3) {
            P.t12[k] = T.int21[ty][t2of(1, 2)][si1][sj2][sj1];
            P.t21[k] = T.int21[t2of(2, 1)][ty][sj1][si1][si2];
        }
        if (umax >= 4) P.t22[k] = T.int22[ty][t2of(2, 2)][si1][si2][sj2][sj1];
        const bool mkc = A < umax || Bq < umax;
        P.w1[k] = i | (ty << K::IB) | (A << (K::IB + 3)) | (Bq << (K::IB + 11)) | (mkc ? (1 << (K::IB + 19)) : 0) |
                  (v ? (1 << (K::IB + 20)) : 0);
        P.mmo[k] = L.dt[DT_MMI + oc];
        P.mo[k] = ct[CT_ONEN + oc] * P.mmo[k];
        P.m23[k] = ct[CT_M23O + oc];
    }
    return P;
}
template <class K>
__device__ __forceinline__ void rec_store(const PfL<typename K::V> &L, int D, const Pend<K::SETS> &P, int lane) {
#pragma unroll
    for (int k = 0; k < K::SETS; k++) {
        if (k * WAVE >= P.n) break;
        float *r = L.rec + ((K::slot(D) * K::SETS + k) * PF_RF) * WAVE + lane;
        r[0] = __int_as_float(P.w1[k]);
        r[WAVE] = P.mmo[k];
        r[2 * WAVE] = P.mo[k];
        r[3 * WAVE] = P.m23[k];
        r[4 * WAVE] = P.t11[k];
        r[5 * WAVE] = P.t12[k];
        r[6 * WAVE] = P.t21[k];
        r[7 * WAVE] = P.t22[k];
    }
    if (lane == 0) L.rcnt[K::slot(D)] = P.n;
}

// ---------------------------------------------------------------- M: qm items of span sq
// K lanes per item (a power of two <= 16, one DPP row), summed over the K lanes:
//   qm(i, jb)  = U(i, jb) + sum_{t >= 5} qm(i, i+t-1) qm1(i+t, jb)
//   mla(i, sq) = the split part
// with the unpaired part sum_t [t <= up_i] pw(t) qm1(i+t, jb) as the column
// recursion U(i, jb) = qm1(i, jb) + [up_i >= 1] (expMLbase sigma) U(i+1, jb), U of
// span sq - 1 kept by the Q wave (split points t = 0..4 read no more).  K and
// the split ranges follow the full fold's item count N - sq, so a refold sums
// every item in the order a fold from scratch does (bit-identical tables; n <=
// N - sq <= PF_NMW * WAVE / K: one round).  The split points t = 5..T are the
// kernel's to spread over the K lanes (K::split_sum: summation order).
// mw: the wave's M index (0 = most items)
template <class K>
__device__ __forceinline__ void pf_m_role(const PfL<typename K::V> &L, const Band &bd, int sq, int mw, int lane,
                                          bool constrained, float mlbase_sig) {
    using V = typename K::V;
    const int N = L.N, NP = L.NP;
    if (sq >= 4 && sq <= N - 3) {
        const int lo = bd.qlo(sq), n = bd.qhi(sq) - lo + 1;
        int KL = 16;
        while (KL > 1 && (N - sq) * KL > PF_NMW * WAVE) KL >>= 1;
        const int ipw = WAVE / KL;                 // items per wave
        const int k = lane & (KL - 1);
        const int item = mw * ipw + lane / KL;
        if (mw * ipw < n) {
            const bool valid = item < n;
            const int i = lo + (valid ? item : n - 1);
            const int jb = i + sq, T = sq - 4;
            const V *pq = L.q1 + colb(jb) + i - 1;   // qm1(i+t, jb) at +t
            const V *pr = L.qm + rowb(i, N) - 5;      // qm(i, i+t-1) at +t (t >= 5)
            const bool up1 = sq >= 5 && (!constrained || L.up[i] >= 1);
            const V u1 = up1 ? L.uc[((sq - 1) & 1) * NP + jb] : vzero<V>();
            const V q0 = pq[0];
            V A = K::split_sum(pq, pr, k, KL, T);
            if (KL >= 2) A = dpp_add<0xb1>(A);     // quad_perm [1,0,3,2]
            if (KL >= 4) A = dpp_add<0x4e>(A);     // quad_perm [2,3,0,1]
            if (KL >= 8) A = dpp_add<0x114>(A);    // row_shr:4
            if (KL >= 16) A = dpp_add<0x118>(A);   // row_shr:8
            if (valid && k == (KL >= 8 ? KL - 1 : 0)) {
                L.qm[rowb(i, N) + sq - 4] = A + vfma(splat<V>(mlbase_sig), u1, q0);
                L.mla[(sq & 1) * NP + i] = A;
            }
        }
    }
}

// ---------------------------------------------------------------- F: the changed cells of diagonal e
// qb (times the inner mismatch) and qm1 from the B partials, the hairpin
// initial value and the multiloop split part; qbg: the ring's slot copy of qb
// (K::QBG), else unused
template <class K>
__device__ __forceinline__ void pf_f_role(const PfL<typename K::V> &L, const Band &bd, int e, int lane,
                                          float mlclosing, float mlbase_sig, float *qbg) {
    using V = typename K::V;
    const int N = L.N, NP = L.NP;
    const uint8_t *S = L.S;
    if (e >= 4 && e <= N - 1) {
        const int lo = bd.clo(e), hi = bd.chi(e);
        const int ro = K::inner(L, e), od = off(e, N);
        for (int i0 = lo; i0 <= hi; i0 += WAVE) {
            const int i = i0 + lane;
            if (i > hi) break;
            const int j = i + e;
            const int ce = ro + i - 1, c1 = colb(j) + i - 1;
            const V init = L.qb[ce];
            const V stem = L.q1[c1];
            const bool upj = e >= 5 && L.up[j] >= 1;
            const V prev = upj ? L.q1[colb(j - 1) + i - 1] : vzero<V>();
            if (!is_mark(init)) {
                const int ty = ptype(S[i], S[j]);
                const float mlcl = mlclosing * L.dt[DT_MLS + rtype(ty) * 25 + S[j - 1] * 5 + S[i + 1]];
                V a_int = vzero<V>();
                if (e >= 6) {
                    const V *pp = L.part + ((e & 1) * K::SETS + ((i - 1) >> 6)) * K::NB * WAVE + ((i - 1) & (WAVE - 1));
#pragma unroll
                    for (int b = 0; b < K::NB; b++) a_int += pp[b * WAVE];
                }
                const V ml = e - 2 >= 4 ? L.mla[((e - 2) & 1) * NP + i + 1] : vzero<V>();
                const V qb = a_int + init + ml * splat<V>(mlcl);
                const float mmc = L.dt[DT_MMI + L.cc[ce]];
                const V fin = qb * splat<V>(mmc) + vzero<V>();   // never the mark (-0)
                L.qb[ce] = fin;
                if constexpr (K::QBG) qbg[od + i - 1] = fin;
                L.q1[c1] = vfma(qb, stem, prev * splat<V>(mlbase_sig));
            } else {
                L.q1[c1] = prev * splat<V>(mlbase_sig);
            }
        }
    }
}

// ---------------------------------------------------------------- Q
// U(i, jb) of span sq for every cell (M reads it next step)
template <class V>
__device__ __forceinline__ void pf_uc_update(const PfL<V> &L, int sq, int lane, bool constrained, float mlbase_sig) {
    const int N = L.N, NP = L.NP;
    if (sq >= 4 && sq <= N - 4) {
        for (int i = 1 + lane; i <= N - sq; i += WAVE) {
            const int jb = i + sq;
            const bool up1 = sq >= 5 && (!constrained || L.up[i] >= 1);
            const V u1 = up1 ? L.uc[((sq - 1) & 1) * NP + jb] : vzero<V>();
            L.uc[(sq & 1) * NP + jb] = vfma(splat<V>(mlbase_sig), u1, L.q1[colb(jb) + i - 1]);
        }
    }
}
// exterior-stem factor of the column cell (k, j) of pair type ty and inner code
// `code`: INVMM(code) * ext(type, S[k-1], S[j+1]); sjp: S[j+1], 5 past the end
template <class V>
__device__ __forceinline__ float pf_ext_factor(const PfL<V> &L, int k, int ty, int sjp, int code) {
    const float e = L.dt[DT_EXT + ty * 36 + ((k > 1) ? L.S[k - 1] : 5) * 6 + sjp];
    return L.ct[CT_INVMM + code] * e;
}

// ensemble energy -kT (ln Z_scaled - N ln sigma), as vrna_pf (float)
__device__ __forceinline__ float pf_energy(const DevScaled *XS, float z, int N) {
    return float(-XS->kT * (log(double(z)) - N * XS->log_sigma));
}

}  // namespace
}  // namespace adx
