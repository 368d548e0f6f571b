// What the lanes = cells outside kernels share (outside_cells.hip for N <= 112:
// Y row- and column-major and the inside qm1 / qm whole in LDS; outside_ring.hip
// beyond: Y row-major only, qm1 / qm read from the slot): the LDS carve and its
// view, the interior-loop shape machinery of the B waves (one window read per
// shape at a per-lane base + immediate offset) and the B sweep, the setup
// pieces (sequence and table loads, shape factors, requested pairs, exterior
// factor, exterior adjoint, motif sites, window zeroing and rank lists), the
// record stages, the finalize, the pair epilogue and the stamp table.  The
// helpers take the kernel's traits K (OcK, OrK: lane-sets per diagonal,
// interior-loop block waves summed in the finalize, mlp slots per parity, the
// window row length, the slack, whether the column copies exist, the two
// multiloop sums of the finalize).  Where the kernels differ in substance --
// the table pass, the multiloop sums, the block partitions of the B sweep,
// the wave permutation, the launchers -- the code stays in the kernel's file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"

#define OSTAMP(k) ADX_STAMP_AT(k)   // fold_common.hpp

// Diagnostic builds (-DADX_STAMP) only, never the product: per-wave cycle sums
// of the phases (s_memtime).  OX_STAMP_TABLE (at file scope): the kernel's
// table and the export that reads it back; OX_STAMP_LOCALS / OX_STAMP_FLUSH:
// the kernel's stamp locals and their accumulation into the table.
#ifdef ADX_STAMP
#define OX_STAMP_TABLE(sym, reader)                                                                             \
    namespace adx {                                                                                             \
    __device__ unsigned long long sym[16][8];                                                                   \
    }                                                                                                           \
    extern "C" int reader(unsigned long long *out, int reset) { /* [16][8] */                                   \
        if (hipMemcpyFromSymbol(out, HIP_SYMBOL(adx::sym), sizeof(adx::sym)) != hipSuccess) return 1;           \
        if (reset) {                                                                                            \
            static unsigned long long z[16][8] = {};                                                            \
            if (hipMemcpyToSymbol(HIP_SYMBOL(adx::sym), z, sizeof(z)) != hipSuccess) return 2;                  \
        }                                                                                                       \
        return 0;                                                                                               \
    }
#define OX_STAMP_LOCALS                                          \
    unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};     \
    unsigned long long st_last = __builtin_amdgcn_s_memtime();
#define OX_STAMP_FLUSH(sym, wid, lane) \
    if ((lane) == 0)                   \
        for (int k = 0; k < 8; k++) atomicAdd(&sym[wid][k], st_acc[k]);
#define OX_STP_PARAMS , unsigned long long *st_acc, unsigned long long &st_last
#define OX_STP_ARGS , st_acc, st_last
#else
#define OX_STAMP_TABLE(sym, reader)
#define OX_STAMP_LOCALS
#define OX_STAMP_FLUSH(sym, wid, lane)
#define OX_STP_PARAMS
#define OX_STP_ARGS
#endif

namespace adx {
namespace {

constexpr int OX_NW = 16;             // waves per workgroup
constexpr int OX_NT = OX_NW * WAVE;
constexpr int OX_NB = 10;             // interior-loop block slots of a cell's partials (outside_cells: waves 0..9)
constexpr int OX_NM = OX_NW - OX_NB;  // outside_cells' multiloop-sum waves (10..15)
constexpr int OX_WIN = 32;            // qbb window: spans d+2 .. d+32 are read at step d
constexpr int OX_PAD = 32;            // zero cells in front of each window row (outer a >= i-31)
constexpr int OX_MAXP = 64;           // requested pairs of one fold kept in LDS
constexpr int OX_FF = 5;              // finalize record fields (see frec_write)
constexpr int OX_RF = 8;              // cell setup record fields (see rec_write)
constexpr int OX_RW = 7;              // B wave OX_RW: setup records (every lane-set)

// ---------------------------------------------------------------- LDS carve and view
struct OxL {
    float *yr, *yc, *q1r, *qmc, *qw, *part, *mlp, *rec, *fr, *sf, *rq, *rr, *r1, *q5, *q5b, *pm, *ct, *dt;
    int *pl;
    uint8_t *ow, *S, *mat, *cl, *cn;   // cn[D]: pairable cells of diagonal D
    int *rcnt;
    double *pd;
    int RL, NP;
};

// LDS carve for folded length N (runtime; the host sizes the launch with it).
// The kernel's part is the cell tables: K::COLS adds Y column-major and the
// inside qm1 / qm to Y row-major
template <class K>
struct OxLay {
    int C, NP, RL;
    size_t YR, YC, Q1R, QMC, QW, OW, PART, MLP, REC, CL, FR, SF, RQ, RR, R1, Q5, Q5B, PM, CT, DT, PD, PL, S, MT, BYTES;
    __host__ __device__ static size_t a16(size_t b) { return (b + 15) & ~size_t(15); }
    __host__ __device__ explicit OxLay(int N) {
        C = ((N - 4) * (N - 3)) / 2;
        NP = N + 2;
        RL = K::row_len(N);
        size_t o = 0;
        const size_t T = a16((size_t(C) + K::SLACK) * 4);       // K::SLACK zeroed floats after each cell table (reads past a row end)
        YR = o;   o += T;                                        // Y row-major (qmb sums; the ring: G column-major before the sweep)
        YC = Q1R = QMC = 0;
        if (K::COLS) {
            YC = o;   o += T;                                    // Y column-major (r2 sums; G before the sweep)
            Q1R = o;  o += T;                                    // inside qm1, row-major
            QMC = o;  o += T;                                    // inside qm, column-major
        }
        QW = o;   o += a16(size_t(OX_WIN) * RL * 4);             // qbb * mismatchI(outer) window
        OW = o;   o += a16(size_t(OX_WIN) * RL);                 // outer codes window
        PART = o; o += a16(size_t(2) * K::SETS * OX_NB * WAVE * 4);   // [parity][lane-set][block][lane]
        MLP = o;  o += a16(size_t(2) * K::NMLP * WAVE * 4);      // M parts: [parity][slot][lane]
        REC = o;  o += a16(size_t(2) * K::SETS * OX_RF * WAVE * 4 + 16);   // cell setup records [parity][lane-set][field][lane]; counts [parity]
        CL = o;   o += a16(size_t(C) + size_t(NP));              // pairable cells per diagonal: cl[off(D) + rank] = i; counts
        FR = o;   o += a16(size_t(2) * K::SETS * OX_FF * WAVE * 4);   // finalize records [parity][lane-set][field][lane]
        SF = o;   o += a16(size_t(31) * 32 * 4);                 // constant factor of shape (u, n1): [u][n1]
        RQ = o;   o += a16(size_t(2) * NP * 4);                  // qmb ring [parity][i]
        RR = o;   o += a16(size_t(2) * NP * 4);                  // R ring
        R1 = o;   o += a16(size_t(2) * NP * 4);                  // qm1b ring
        Q5 = o;   o += a16(size_t(NP) * 4);
        Q5B = o;  o += a16(size_t(NP) * 4);
        PM = o;   o += a16(size_t(NP) * 4);                      // motif site weights
        CT = o;   o += a16(size_t(CT_SIZE) * 4);
        DT = o;   o += a16(size_t(DT_EXT + 288) * 4);            // MMI, MLS, EXT
        PD = o;   o += a16(size_t(OX_MAXP) * 8);                 // requested pairs: qb qbb / Z
        PL = o;   o += a16(size_t(OX_MAXP) * 4 + 4);             // this fold's pairs: t | i << 8 | j << 16; count
        S = o;    o += a16(size_t(NP) + 8);
        MT = o;   o += a16(size_t(NP));                          // motif site flags
        BYTES = o;
    }
};

template <class K>
__device__ __forceinline__ OxL ox_view(char *smem, const OxLay<K> &Y) {
    OxL L;
    L.yr = reinterpret_cast<float *>(smem + Y.YR);
    L.yc = K::COLS ? reinterpret_cast<float *>(smem + Y.YC) : nullptr;
    L.q1r = K::COLS ? reinterpret_cast<float *>(smem + Y.Q1R) : nullptr;
    L.qmc = K::COLS ? reinterpret_cast<float *>(smem + Y.QMC) : nullptr;
    L.pl = reinterpret_cast<int *>(smem + Y.PL);
    L.qw = reinterpret_cast<float *>(smem + Y.QW);
    L.ow = reinterpret_cast<uint8_t *>(smem + Y.OW);
    L.part = reinterpret_cast<float *>(smem + Y.PART);
    L.mlp = reinterpret_cast<float *>(smem + Y.MLP);
    L.rec = reinterpret_cast<float *>(smem + Y.REC);
    L.rcnt = reinterpret_cast<int *>(smem + Y.REC + size_t(2) * K::SETS * OX_RF * WAVE * 4);
    L.cl = reinterpret_cast<uint8_t *>(smem + Y.CL);
    L.cn = L.cl + Y.C;
    L.sf = reinterpret_cast<float *>(smem + Y.SF);
    L.fr = reinterpret_cast<float *>(smem + Y.FR);
    L.rq = reinterpret_cast<float *>(smem + Y.RQ);
    L.rr = reinterpret_cast<float *>(smem + Y.RR);
    L.r1 = reinterpret_cast<float *>(smem + Y.R1);
    L.q5 = reinterpret_cast<float *>(smem + Y.Q5);
    L.q5b = reinterpret_cast<float *>(smem + Y.Q5B);
    L.pm = reinterpret_cast<float *>(smem + Y.PM);
    L.ct = reinterpret_cast<float *>(smem + Y.CT);
    L.dt = reinterpret_cast<float *>(smem + Y.DT);
    L.pd = reinterpret_cast<double *>(smem + Y.PD);
    L.S = reinterpret_cast<uint8_t *>(smem + Y.S);
    L.mat = reinterpret_cast<uint8_t *>(smem + Y.MT);
    L.RL = Y.RL;
    L.NP = Y.NP;
    return L;
}

// LDS bytes of kernel K's carve for folded length Nmax (0: does not fit)
template <class K>
inline size_t ox_lds_bytes(int Nmax) {
    const OxLay<K> y(Nmax);
    return y.BYTES + 256 <= size_t(LDS_LIMIT) ? y.BYTES : 0;
}

// The fold's uniform values, as the finalize and the epilogue use them
struct OxC {
    int N;
    const float *src;        // the fold's inside tables in the walker's slot (qb first)
    const DevScaled *XS;
    float Z, mlbase_sig, mlclosing, pw1;
    bool motif;
    int mL;
};

__device__ __forceinline__ int wslot(int D) { return D & (OX_WIN - 1); }

// diagonal D of the diagonal-major cell index k: off(D) <= k < off(D + 1)
__device__ __forceinline__ int inv_off(int k, int N) {
    const float b = float(2 * N - 7);
    int D = 4 + int((b - sqrtf(fmaxf(b * b - 8.f * float(k), 0.f))) * 0.5f);
    D = D < 4 ? 4 : D;
    while (D < N - 1 && off(D + 1, N) <= k) D++;
    while (D > 4 && off(D, N) > k) D--;
    return D;
}
// column j of the column-major cell index k: colb(j) <= k < colb(j + 1)
__device__ __forceinline__ int inv_colb(int k) {
    int j = 5 + int((sqrtf(8.f * float(k) + 1.f) - 1.f) * 0.5f);
    while (colb(j + 1) <= k) j++;
    while (colb(j) > k) j--;
    return j;
}

// ---------------------------------------------------------------- interior-loop shapes
struct OxCell {                 // per lane: the inner pair (i, j) of every shape
    int i;
    float mmin, tau_in, mo_in, m23_in;
    float t11, t12, t21, t22;   // 1x1 / 1x2 / 2x1 / 2x2 table factors (HBM, issued at the block start)
};

// One shape (N1, U - N1) of the lane's cell; qw / ow: this lane's window row of
// the outer span d + 2 + U at outer a = i - 1 - U (n1 = U), so shape N1 reads
// offset U - N1; fv: the shapes' constant factors (OxL::sf row U, in registers).
// Compile-time shape: the kind and every table offset fold.
template <int U, int N1>
__device__ __forceinline__ void oshape1(const OxL &L, const OxCell &c, const float *fv, const float *qw,
                                        const uint8_t *ow, int ty2, float &g, float &sp) {
    constexpr int k = loop_kind(N1, U - N1);
    const float v = qw[U - N1];
    if constexpr (k < 0) {
        g = fmaf(v, fv[N1], g);
    } else {
        const float *ct = L.ct;
        const int oc = ow[U - N1];
        float f;
        if constexpr (k == TK_STK || k == TK_B1) {
            f = ct[CT_INVMM + oc] * ct[CT_STK + ((oc * 41) >> 10) * 8 + ty2] * fv[N1];
        } else if constexpr (k == TK_BUL) {
            f = ct[CT_BUL + oc] * (c.tau_in * fv[N1]);
        } else if constexpr (k == TK_1N) {
            f = ct[CT_ONEN + oc] * (c.mo_in * fv[N1]);
        } else if constexpr (k == TK_M23) {
            f = ct[CT_INVMM + oc] * ct[CT_M23O + oc] * (c.m23_in * fv[N1]);
        } else {
            const float tv = k == TK_I11 ? c.t11 : k == TK_I12 ? c.t12 : k == TK_I21 ? c.t21 : c.t22;
            f = ct[CT_INVMM + oc] * (tv * fv[N1]);
        }
        sp = fmaf(v, f, sp);
    }
}
template <int U, int... N1s>
__device__ __forceinline__ void oshape_seq(std::integer_sequence<int, N1s...>, const OxL &L, const OxCell &c,
                                           const float *fv, const float *qw, const uint8_t *ow, int ty2, float &g,
                                           float &sp) {
    (oshape1<U, N1s>(L, c, fv, qw, ow, ty2, g, sp), ...);
}
// the shapes of loop size U (skipped past the step's umax: uniform)
template <int U>
struct OxSize {
    float fv[U < 0 ? 1 : U + 1];
    __device__ __forceinline__ void load(const OxL &L) {
        if constexpr (U >= 0)
#pragma unroll
            for (int n1 = 0; n1 <= U; n1++) fv[n1] = L.sf[U * 32 + n1];
    }
    __device__ __forceinline__ void run(const OxL &L, const OxCell &c, int d, int umax, int ty2, float &g,
                                        float &sp) const {
        if constexpr (U >= 0) {
            if (U <= umax) {
                const int o = wslot(d + 2 + U) * L.RL + OX_PAD + c.i - 2 - U;
                oshape_seq<U>(std::make_integer_sequence<int, U + 1>{}, L, c, fv, L.qw + o, L.ow + o, ty2, g, sp);
            }
        }
    }
};

// Loop size U >= 6 over the four lanes of an inner cell (phase r = lane & 3),
// as pf_common.hpp PSizeQ: lane r takes one special shape -- the bulges (0,U)
// (U,0) and 1 x n loops (1,U-1) (U-1,1), a window read, an outer-code read and
// a factor gather -- and the generic shapes n1 = 2 + r + 4m <= U - 2 (one
// window read at a per-lane base + immediate offset, its factor in a VGPR; 0
// past the size).  The four lanes' sums are added in a fixed order.
template <int U>
struct OxSizeQ {
    static constexpr int NR = U >= 6 ? (U - 3 + 3) / 4 : 1;
    float gf[NR];
    float fsp;
    int n1sp;
    __device__ __forceinline__ void load(const OxL &L, int r) {
#pragma unroll
        for (int m = 0; m < NR; m++) {
            const int n1 = 2 + 4 * m + r;
            gf[m] = n1 <= U - 2 ? L.sf[U * 32 + n1] : 0.f;
        }
        n1sp = r == 0 ? 0 : r == 1 ? U : r == 2 ? 1 : U - 1;
        fsp = L.sf[U * 32 + n1sp];
    }
    __device__ __forceinline__ void run(const OxL &L, const OxCell &c, int d, int umax, int ctb, float outer,
                                        float &g, float &sp) const {
        if (U <= umax) {
            const int o = wslot(d + 2 + U) * L.RL + OX_PAD + c.i - 2 - U;   // shape n1 at o + U - n1
            {
                const float v = L.qw[o + U - n1sp];
                const int oc = L.ow[o + U - n1sp];
                sp = fmaf(v, L.ct[ctb + oc] * (outer * fsp), sp);
            }
            const float *q = L.qw + o + U - 2 - (threadIdx.x & 3);
#pragma unroll
            for (int m = 0; m < NR; m++) g = fmaf(q[-4 * m], gf[m], g);
        }
    }
};
template <int U>
struct OxBlk {   // the size's state in a B wave (sizes <= 5 whole in every lane)
    using T = typename std::conditional<(U <= 5), OxSize<U>, OxSizeQ<U>>::type;
};
template <int U>
__device__ __forceinline__ void ox_load(typename OxBlk<U>::T &z, const OxL &L, int r) {
    if constexpr (U <= 5) z.load(L);
    else z.load(L, r);
}
template <int U>
__device__ __forceinline__ void ox_run(const typename OxBlk<U>::T &z, const OxL &L, const OxCell &c, int d, int umax,
                                       int ty2, int ctb, float outer, float &g, float &sp, float &gs, float &sps,
                                       int r) {
    if constexpr (U < 0) {
    } else if constexpr (U <= 5) {
        if (!ADX_SMALL_R0 || r == 0) z.run(L, c, d, umax, ty2, gs, sps);   // counted on phase 0 only
    } else {
        z.run(L, c, d, umax, ctb, outer, g, sp);
    }
}

// B: the interior-loop gather of every diagonal for one block of loop sizes
// (-1 = none), the block's shape factors held in registers for the whole sweep;
// four lanes per inner cell (16 cells per lane-set; OxSizeQ), one barrier per
// diagonal, as the M / F waves.
// wid: the wave as a compile-time constant (std::integral_constant; round 6), so
// the role fin(d, wid) runs on this wave is resolved per instance
template <int NSETS, int U0, int U1, int U2, int U3, int U4, class Fin, class Wid>
__device__ __forceinline__ void b_sweep(const OxL &L, int N, int lane, Wid wid, const Fin &fin OX_STP_PARAMS) {
    constexpr auto tb = [](int u) { return u >= 2 && u <= 4; };
    constexpr bool TB = tb(U0) || tb(U1) || tb(U2) || tb(U3) || tb(U4);
    constexpr bool H5 = U0 == 5 || U1 == 5 || U2 == 5 || U3 == 5 || U4 == 5;   // 2x3 loops (m23)
    const int r = lane & 3, cq = lane >> 2;
    typename OxBlk<U0>::T s0;
    typename OxBlk<U1>::T s1;
    typename OxBlk<U2>::T s2;
    typename OxBlk<U3>::T s3;
    typename OxBlk<U4>::T s4;
    ox_load<U0>(s0, L, r);
    ox_load<U1>(s1, L, r);
    ox_load<U2>(s2, L, r);
    ox_load<U3>(s3, L, r);
    ox_load<U4>(s4, L, r);
    const int ctb = r < 2 ? CT_BUL : CT_ONEN;   // the lane's special-shape outer factor table
    const float eTAU = L.ct[CT_FSM + 6];
    for (int d = N - 1; d >= 3; d--) {
        const int par = d & 1;
        const int umax = min(30, N - 3 - d);                      // outer spans d+2 .. d+2+umax
        // lanes = the pairable cells of diagonal d, compacted (records one step ahead)
        const int ncell = (d >= 4 && umax >= 0) ? uni(L.rcnt[par]) : 0;
        for (int c0 = 0; c0 < ncell; c0 += WAVE / 4) {
            const int idx = c0 + cq;   // the lane's cell (records: set idx / 64, lane idx % 64)
            const float *rr = L.rec + ((par * NSETS + (idx >> 6)) * OX_RF) * WAVE + (idx & (WAVE - 1));
            // word: i | ty2 << 8 | real << 16; a block reads only the fields its sizes use
            const int tp = __float_as_int(rr[0]);
            const int i = tp & 255;
            OxCell c;
            c.i = i;
            const int ty2 = (tp >> 8) & 255;
            c.mmin = rr[WAVE];
            c.tau_in = ty2 > 2 ? eTAU : 1.f;
            c.mo_in = rr[2 * WAVE];
            c.m23_in = H5 ? rr[3 * WAVE] : 0.f;
            c.t11 = c.t12 = c.t21 = c.t22 = 0.f;
            if constexpr (TB) {
                c.t11 = rr[4 * WAVE];
                c.t12 = rr[5 * WAVE];
                c.t21 = rr[6 * WAVE];
                c.t22 = rr[7 * WAVE];
            }
            const float outer = r < 2 ? c.tau_in : c.mo_in;
            float g = 0.f, sp = 0.f, gs = 0.f, sps = 0.f;
            OSTAMP(2);   // B cell setup
            ox_run<U0>(s0, L, c, d, umax, ty2, ctb, outer, g, sp, gs, sps, r);
            ox_run<U1>(s1, L, c, d, umax, ty2, ctb, outer, g, sp, gs, sps, r);
            ox_run<U2>(s2, L, c, d, umax, ty2, ctb, outer, g, sp, gs, sps, r);
            ox_run<U3>(s3, L, c, d, umax, ty2, ctb, outer, g, sp, gs, sps, r);
            ox_run<U4>(s4, L, c, d, umax, ty2, ctb, outer, g, sp, gs, sps, r);
            OSTAMP(3);   // B shapes
            // small sizes count once (phase 0), then the cell's total over its four lanes
            const float part = quad_sum(fmaf(g, c.mmin, sp) + (r == 0 ? fmaf(gs, c.mmin, sps) : 0.f));
            if (r == 0 && idx < ncell && (tp >> 16))   // the cell's natural slot (F reads lane = cell)
                L.part[((par * NSETS + ((i - 1) >> 6)) * OX_NB + wid) * WAVE + ((i - 1) & (WAVE - 1))] = part;
        }
        fin(d, wid);   // F of diagonal d + 1 on the first waves
        OSTAMP(5);
        lds_barrier();
        OSTAMP(6);   // barrier
    }
}

// ---------------------------------------------------------------- setup
// The sequence with its contexts (fold_rows.hip pf_group; ViennaRNA S1 wrap),
// the ct / dt tables, the constant factor of each shape (u, n1) -- generic
// fgen, bulge / 1xn length factors, the sigma powers of the tabulated loops
// (setup_core.hpp addS) -- q5 from the slot (q5g) and the zeroed rings, site
// weights and pair values.  Every thread of the workgroup calls it (barriers)
__device__ __forceinline__ void ox_setup(const OxL &L, const KArgs &ka, const DevScaled *XS, const DevVariant &V,
                                         const uint8_t *seqs, int w, const float *q5g, int N, int tid) {
    const DevTables &T = *ka.T;
    const int NP = L.NP;
    const SeqSrc src = seq_src(ka, V, seqs + size_t(w) * ka.Nraw);
    for (int k = tid; k < NP; k += OX_NT) L.S[k] = src.code(k, N);
    for (int k = tid; k < CT_SIZE; k += OX_NT) L.ct[k] = XS->ctab[k];
    for (int k = tid; k < 200; k += OX_NT) {
        L.dt[DT_MMI + k] = (&T.mmI[0][0][0])[k];
        L.dt[DT_MLS + k] = (&T.mlstem[0][0][0])[k];
    }
    for (int k = tid; k < 288; k += OX_NT) L.dt[DT_EXT + k] = (&T.ext[0][0][0])[k];
    for (int k = tid; k < 31 * 32; k += OX_NT) {
        const int u = k >> 5, n1 = k & 31;
        L.sf[k] = n1 <= u ? shape_factor(XS, u, n1) : 0.f;
    }
    for (int k = tid; k <= N; k += OX_NT) L.q5[k] = q5g[k];
    for (int k = tid; k < 2 * NP; k += OX_NT) L.rq[k] = L.rr[k] = L.r1[k] = 0.f;
    for (int k = tid; k < NP; k += OX_NT) { L.q5b[k] = 0.f; L.pm[k] = 0.f; L.mat[k] = 0; }
    for (int k = tid; k < OX_MAXP; k += OX_NT) L.pd[k] = 0.0;
    __syncthreads();
    if (tid == 0) wrap_ends(L, N);
    __syncthreads();
}

// this fold's requested pairs (score terms), kept in LDS for the finalize
__device__ __forceinline__ void ox_pair_list(const OxL &L, const KArgs &ka, int bv, int tid) {
    if (tid == 0) {
        int n = 0;
        for (int t = 0; t < ka.n_pairs && t < OX_MAXP; t++)
            if (ka.pairs[3 * t] == bv) L.pl[n++] = t | (ka.pairs[3 * t + 1] << 8) | (ka.pairs[3 * t + 2] << 16);
        L.pl[OX_MAXP] = n;
    }
}

// the exterior factor G(ic, jc) = qb(ic,jc) ext(ic,jc) of a column-major cell (qb: the slot's, src)
__device__ __forceinline__ float ox_ext_cell(const OxL &L, const float *src, int N, int ic, int jc) {
    const uint8_t *S = L.S;
    const int ty = ptype(S[ic], S[jc]);
    const int cc = rtype(ty) * 25 + S[jc + 1] * 5 + S[ic - 1];
    const float e = L.dt[DT_EXT + ty * 36 + ((ic > 1) ? S[ic - 1] : 5) * 6 + ((jc < N) ? S[jc + 1] : 5)];
    return src[off(jc - ic, N) + ic - 1] * (L.ct[CT_INVMM + cc] * e);   // non-pairable: -0 * x = 0
}

// a[hs] of a per-lane-set value (hs uniform): hs == 0 ? a[0] : hs == 1 ? a[1] : ... a[SETS - 1]
template <int SETS, int H = 0>
__device__ __forceinline__ float ox_pick_set(const float (&a)[SETS], int hs) {
    if constexpr (H == SETS - 1) return a[H];
    else return hs == H ? a[H] : ox_pick_set<SETS, H + 1>(a, hs);
}

// Exterior adjoint (fold_rows.hip outside(), push form, one wave, lanes = m in
// SETS lane-sets; G: the exterior factors, column-major): once q5b[j] is known
// every m <= j-5 takes q5b[j] G(m+1, j).  acc[j-5] is final after the push of
// j, and q5b[j-5] needs it four steps later, so the loop-carried chain is one
// FMA: q5b[j-1] = sigma q5b[j] + acc[j-1], acc[j-1] read (readlane) four
// iterations ahead; the next column of G is loaded during the current push.
template <int SETS>
__device__ __forceinline__ void ox_ext_adjoint(const OxL &L, const float *G, const DevScaled *XS, int N, int lane) {
    const float sig1 = XS->sig[1];
    float acc[SETS], g[SETS];   // m = h * 64 + lane: the sum, G column j
#pragma unroll
    for (int h = 0; h < SETS; h++) acc[h] = g[h] = 0.f;
    float val = 1.f;            // q5b[N]
    float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;   // acc[j-1], acc[j-2], acc[j-3], acc[j-4]
    if (lane == 0) L.q5b[N] = 1.f;
    if (N >= 5) {
        const int cb = colb(N);
#pragma unroll
        for (int h = 0; h < SETS; h++) g[h] = G[cb + min(h * WAVE + lane, N - 5)];
    }
    for (int j = N; j >= 1; j--) {
        float nx[SETS];         // prefetch: column j - 1
#pragma unroll
        for (int h = 0; h < SETS; h++) nx[h] = 0.f;
        if (j - 1 >= 5) {
            const int cb = colb(j - 1);
#pragma unroll
            for (int h = 0; h < SETS; h++) nx[h] = G[cb + min(h * WAVE + lane, j - 6)];
        }
        float a5 = 0.f;
        if (j >= 5) {
            const int m5 = j - 5;
#pragma unroll
            for (int h = 0; h < SETS; h++)
                if (h * WAVE + lane <= m5) acc[h] = fmaf(val, g[h], acc[h]);
            // acc[j-5] is final now
            const int hs = m5 / WAVE, ls = m5 - hs * WAVE;
            a5 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ox_pick_set<SETS>(acc, hs)), ls));
        }
        val = fmaf(sig1, val, q0);   // q5b[j-1]
        if (lane == 0) L.q5b[j - 1] = val;
        q0 = q1;
        q1 = q2;
        q2 = q3;
        q3 = a5;
#pragma unroll
        for (int h = 0; h < SETS; h++) g[h] = nx[h];
    }
}

// motif sites (unconstrained: the sequence alone decides), one wave
__device__ __forceinline__ void ox_motif_sites(const OxL &L, const DevScaled *XS, int N, int mL, int lane) {
    motif_scan<WAVE>(L, XS->motif_code, mL, N, lane);
}

// While wave 0 runs the exterior adjoint: the window zeroed and the pairable
// cells of every diagonal in rank order (the B lanes; an unconstrained fold:
// the pair type alone decides), on waves 2.. (neither touches G)
__device__ __forceinline__ void ox_window_ranks(const OxL &L, int N, int wid, int lane) {
    const uint8_t *S = L.S;
    const int t2 = (wid - 2) * WAVE + lane, n2 = OX_NT - 2 * WAVE;
    for (int k = t2; k < OX_WIN * L.RL; k += n2) {
        L.qw[k] = 0.f;
        L.ow[k] = 0;
    }
    for (int D = 4 + wid - 2; D <= N - 1; D += OX_NW - 2) {
        const int od = off(D, N);
        int base = 0;
        for (int i0 = 1; i0 <= N - D; i0 += WAVE) {
            const int i = i0 + lane;
            const bool pr = i <= N - D && ptype(S[i], S[i + D]) != 0;
            const uint64_t m = __ballot(pr);
            const int slot = base + __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
            if (pr) L.cl[od + slot] = uint8_t(i);
            base += __popcll(m);
        }
        if (lane == 0) L.cn[D] = uint8_t(base);
    }
}

// ---------------------------------------------------------------- records
// the lane's cell (i, j) of lane-set ls of diagonal D (the last cell past the end); false past the end
__device__ __forceinline__ bool cell_of(int N, int D, int ls, int lane, int &i, int &j) {
    i = 1 + ls * WAVE + lane;
    const bool valid = i <= N - D;
    if (!valid) i = N - D;
    j = i + D;
    return valid;
}

// The setup records of diagonal D's pairable cells (rank lists built in
// setup), written one step before B reads them: inner mismatch, TermAU, 1xn /
// 2x3 factors of the cell as the inner pair, the four 1x1..2x2 table factors,
// type | pairable.  Three stages a step apart, one LDS round trip each:
// idx_load (rank list), tab_load (bases, the cell's LDS factors, the 1x1..2x2
// table factors from HBM/L2), rec_write (stores only).  Per lane-set k (SETS of
// them): lane l holds cell k * 64 + l of the rank list
template <int SETS>
struct Idx {
    int cnt;
    int i[SETS];   // the lane's cell (cell 1 on idle lanes: its shapes are read and discarded)
};
template <int SETS>
struct Pend {
    int cnt;
    int i[SETS], ty2[SETS];
    float mmin[SETS], mo[SETS], m23[SETS];
    float4 t[SETS];
};
template <int SETS>
__device__ __forceinline__ Idx<SETS> idx_load(const OxL &L, int N, int D, int lane) {
    Idx<SETS> X;
    X.cnt = 0;
#pragma unroll
    for (int k = 0; k < SETS; k++) X.i[k] = 1;
    if (D < 4) return X;
    const int od = off(D, N);
    X.cnt = uni(L.cn[D]);
#pragma unroll
    for (int k = 0; k < SETS; k++) {
        const int idx = k * WAVE + lane;
        const int ir = L.cl[od + min(idx, N - D - 1)];
        X.i[k] = idx < X.cnt ? ir : 1;
    }
    return X;
}
template <int SETS>
__device__ __forceinline__ Pend<SETS> tab_load(const OxL &L, const DevTables &T, int N, int D, const Idx<SETS> &X) {
    Pend<SETS> P;
    P.cnt = X.cnt;
    const uint8_t *S = L.S;
    const int umax = min(30, N - 3 - D);
    auto Sc = [&](int x) { return int(S[x < 0 ? 0 : (x > N + 1 ? N + 1 : x)]); };
#pragma unroll
    for (int k = 0; k < SETS; k++) {
        P.i[k] = X.i[k];
        P.ty2[k] = 0;
        P.mmin[k] = P.mo[k] = P.m23[k] = 0.f;
        P.t[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k * WAVE >= X.cnt) continue;
        const int i = X.i[k], j = i + D;
        const int ty2 = rtype(ptype(S[i], S[j]));
        const int cc = ty2 * 25 + S[j + 1] * 5 + S[i - 1];
        P.ty2[k] = ty2;
        P.mmin[k] = L.dt[DT_MMI + cc];
        P.mo[k] = L.ct[CT_ONEN + cc] * P.mmin[k];
        P.m23[k] = L.ct[CT_M23O + cc];
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (umax >= 2) t.x = T.int11[ptype(Sc(i - 2), Sc(j + 2))][ty2][Sc(i - 1)][Sc(j + 1)];
        if (umax >= 3) {
            t.y = T.int21[ptype(Sc(i - 2), Sc(j + 3))][ty2][Sc(i - 1)][Sc(j + 1)][Sc(j + 2)];
            t.z = T.int21[ty2][ptype(Sc(i - 3), Sc(j + 2))][Sc(j + 1)][Sc(i - 2)][Sc(i - 1)];
        }
        if (umax >= 4) t.w = T.int22[ptype(Sc(i - 3), Sc(j + 3))][ty2][Sc(i - 2)][Sc(i - 1)][Sc(j + 1)][Sc(j + 2)];
        P.t[k] = t;
    }
    return P;
}
// records of diagonal D's compacted pairable cells (read by B at step D)
template <int SETS>
__device__ __forceinline__ void rec_write(const OxL &L, int D, const Pend<SETS> &P, int lane) {
    if (D < 4) return;
    if (lane == 0) L.rcnt[D & 1] = P.cnt;
#pragma unroll
    for (int k = 0; k < SETS; k++) {
        const int idx = k * WAVE + lane;
        if (k * WAVE >= P.cnt) break;
        const bool v = idx < P.cnt;
        float *r = L.rec + (((D & 1) * SETS + k) * OX_RF) * WAVE + lane;
        // an idle lane reads cell 1's shapes (discarded)
        r[0 * WAVE] = __int_as_float(P.i[k] | (P.ty2[k] << 8) | (v ? (1 << 16) : 0));
        r[1 * WAVE] = P.mmin[k];
        r[2 * WAVE] = P.mo[k];
        r[3 * WAVE] = P.m23[k];
        r[4 * WAVE] = P.t[k].x;
        r[5 * WAVE] = P.t[k].y;
        r[6 * WAVE] = P.t[k].z;
        r[7 * WAVE] = P.t[k].w;
    }
}
// the record wave before the sweep: the records of diagonal N - 1, the factors
// of N - 2 (pnext), the rank list of N - 3 (inext)
template <int SETS>
__device__ __forceinline__ void rec_prime(const OxL &L, const DevTables &T, int N, int lane, Pend<SETS> &pnext,
                                          Idx<SETS> &inext) {
    rec_write<SETS>(L, N - 1, tab_load<SETS>(L, T, N, N - 1, idx_load<SETS>(L, N, N - 1, lane)), lane);
    pnext = tab_load<SETS>(L, T, N, N - 2, idx_load<SETS>(L, N, N - 2, lane));
    inext = idx_load<SETS>(L, N, N - 3, lane);
}

// Finalize record of lane-set ls of diagonal e (written at step e, read by F
// at step e - 1): the cell's exterior term q5b[j] q5[i-1] ext, multiloop stem,
// outer mismatch, multiloop-closing factor of the pair, type | code | pairable.
template <int SETS>
__device__ __forceinline__ void frec_write(const OxL &L, int N, int e, int ls, int lane, float mlclosing) {
    if (e < 4 || ls >= (N - e + WAVE - 1) / WAVE) return;
    const uint8_t *S = L.S;
    int i, j;
    const bool valid = cell_of(N, e, ls, lane, i, j);
    const int ty = ptype(S[i], S[j]);
    const int oc = ty * 25 + S[i + 1] * 5 + S[j - 1];
    float *r = L.fr + (((e & 1) * SETS + ls) * OX_FF) * WAVE + lane;
    r[0] = L.q5b[j] * L.q5[i - 1] * L.dt[DT_EXT + ty * 36 + ((i > 1) ? S[i - 1] : 5) * 6 + ((j < N) ? S[j + 1] : 5)];
    r[WAVE] = L.dt[DT_MLS + ty * 25 + S[i - 1] * 5 + S[j + 1]];
    r[2 * WAVE] = L.dt[DT_MMI + oc];
    r[3 * WAVE] = mlclosing * L.dt[DT_MLS + rtype(ty) * 25 + S[j - 1] * 5 + S[i + 1]];
    r[4 * WAVE] = __int_as_float(ty | (oc << 8) | ((valid && ty != 0) ? (1 << 16) : 0));
}

// ---------------------------------------------------------------- F: finalize diagonal e = d + 1, lane-set fl
// (after the step's B work, on the first K::SETS B waves): one batch of
// independent reads.  K::msums: the lane's qmb and r2 from the M waves' parts
// of parity pe (mp: this lane's first slot), summed in the kernel's own order;
// K::FB: the B waves whose partials are summed; K::COLS: Y's column copy
template <class K>
__device__ __forceinline__ void ox_finalize(const OxL &L, const OxC &c, int d, int fl, int lane) {
    const int N = c.N, NP = L.NP;
    const int e = d + 1;
    const int nle = (N - e + WAVE - 1) / WAVE;
    if (e > N - 1 || fl >= nle) return;
    const int pe = e & 1, pn = (e + 1) & 1;
    const int i = 1 + fl * WAVE + lane;
    if (i > N - e) return;
    const int j = i + e;
    float qmbv, r2;
    K::msums(L.mlp + pe * K::NMLP * WAVE + lane, nle, fl, qmbv, r2);
    const float R = i >= 2 ? c.pw1 * (L.rq[pn * NP + i - 1] + L.rr[pn * NP + i - 1]) : 0.f;
    const float chain = j < N ? c.mlbase_sig * L.r1[pn * NP + i] : 0.f;
    const float qm1b = qmbv + R + r2 + chain;
    const float *fr = L.fr + ((pe * K::SETS + fl) * OX_FF) * WAVE + lane;
    const int tp = __float_as_int(fr[4 * WAVE]);
    float a_int = 0.f;   // B wrote the partials of every pairable cell when an outer loop fits
    const float *pp = L.part + (pe * K::SETS + fl) * OX_NB * WAVE + lane;
#pragma unroll
    for (int b = 0; b < K::FB; b++) a_int += pp[b * WAVE];
    if (N - 3 - e < 0) a_int = 0.f;
    L.rq[pe * NP + i] = qmbv;
    L.rr[pe * NP + i] = R;
    L.r1[pe * NP + i] = qm1b;
    L.yr[rowb(i, N) + e - 4] += qmbv;   // Y(i, j): X(i, j) was stored two diagonals ago
    if constexpr (K::COLS) L.yc[colb(j) + i - 1] += qmbv;
    float qbbm = 0.f;
    if (tp >> 16) {
        const float qbb = a_int + fr[0] + qm1b * fr[WAVE];
        qbbm = qbb * fr[2 * WAVE];
        if (e - 2 >= 4) {   // X(i+1, j-1): this pair closing a multiloop
            const float x = qbb * fr[3 * WAVE];
            L.yr[rowb(i + 1, N) + e - 6] = x;
            if constexpr (K::COLS) L.yc[colb(j - 1) + i] = x;
        }
        if (c.motif && e == c.mL - 1 && L.mat[i]) L.pm[i] = float(double(qbb) * c.XS->motif_extra / c.Z);
        const int npl = L.pl[OX_MAXP];
        for (int q = 0; q < npl; q++) {
            const int pk = L.pl[q];
            if (((pk >> 8) & 255) == i && (pk >> 16) == j) {
                const int cc = rtype(tp & 255) * 25 + L.S[j + 1] * 5 + L.S[i - 1];
                const double qb = double(c.src[off(e, N) + i - 1]) * double(L.ct[CT_INVMM + cc]);
                L.pd[pk & 255] = qb * double(qbb) / double(c.Z);
            }
        }
    }
    const int wo = wslot(e) * L.RL + OX_PAD + i - 1;
    L.qw[wo] = qbbm;
    L.ow[wo] = uint8_t((tp >> 8) & 255);
}

// What a B wave runs after its blocks at step d (b_sweep's fin), by the wave as
// a compile-time constant: the finalize of diagonal d + 1 on waves 0 ..
// SETS-1, the finalize records of diagonal d on the next SETS, and on wave
// OX_RW the setup records of diagonal d - 1 (next step's B) from the factors
// made last step, the factors of diagonal d - 2, the rank list of d - 3
template <class K>
struct OxFin {
    const OxL &L;
    const OxC &c;
    const DevTables &T;
    int lane;
    Pend<K::SETS> &pnext;   // the record wave's: the factors of the diagonal after the next
    Idx<K::SETS> &inext;    // and the rank list of the one after that
    template <class Wid>
    __device__ __forceinline__ void operator()(int d, Wid) const {
        constexpr int w = Wid::value;
        if constexpr (w < K::SETS) {
            ox_finalize<K>(L, c, d, w, lane);
        } else if constexpr (w < 2 * K::SETS) {
            frec_write<K::SETS>(L, c.N, d, w - K::SETS, lane, c.mlclosing);   // diagonal d, finalized next step
        } else if constexpr (w == OX_RW) {
            rec_write<K::SETS>(L, d - 1, pnext, lane);
            pnext = tab_load<K::SETS>(L, T, c.N, d - 2, inext);
            inext = idx_load<K::SETS>(L, c.N, d - 3, lane);
        }
    }
};

// ---------------------------------------------------------------- epilogue
// The requested pairs of fold bv (score terms) to pp = the walker's row of
// pair_p, the motif's inner pairs credited from its closing cell (fold_rows.hip
// outside())
__device__ __forceinline__ void ox_write_pairs(const OxL &L, const KArgs &ka, const OxC &c, double *pp, int bv,
                                               int tid) {
    const int N = c.N, mL = c.mL;
    for (int t = tid; t < ka.n_pairs; t += OX_NT) {
        if (ka.pairs[3 * t] != bv) continue;
        const int i = ka.pairs[3 * t + 1], j = ka.pairs[3 * t + 2];
        double pij = 0.0;
        if (i >= 1 && j <= N && j - i >= 4) {
            pij = t < OX_MAXP ? L.pd[t] : 0.0;
            if (c.motif)
                for (int o = 1; o + mL - 1 <= N; o++) {
                    if (o + mL - 1 < j || i < o) continue;
                    const float pmo = L.pm[o];
                    if (pmo == 0.f) continue;
                    const int pk = c.XS->motif_pt[i - o];
                    if (i - o >= 1 && pk == j - o) pij += pmo;
                }
        }
        pp[t] = pij;
    }
}

}  // namespace
}  // namespace adx
