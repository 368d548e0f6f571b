// What the lanes = cells MFE kernels share (mfe_cells.hip: one anti-diagonal
// per barrier; mfe_pair.hip: two): the packed 16-bit min-plus encoding (apo |
// holo halves), wave reductions, the LDS address of an object, the state the
// generated interior-loop blocks (mfe_blocks.inc, mfe_pair_blocks.inc;
// tools/gen_mfe_blocks.py) read and a B cell's setup for them, the carve
// constants and byte arrays, a refold's band and slots, and the pieces of the
// setup, write-back and epilogue that are the same in both.  The helpers take
// either carve (CL, CP) as a template argument: the member names agree.  Where
// the kernels differ in substance the code stays in the kernel's file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "loop_codetab_core.hpp"

namespace adx {
namespace {

using u32 = uint32_t;
constexpr u32 INF16 = 0x7FFF7FFFu;
constexpr u32 MARK16 = 0x7FFE7FFEu;   // non-pairable cell (setup value; a finished cell never takes it)

__device__ __forceinline__ s16x2 sv(u32 x) { return __builtin_bit_cast(s16x2, x); }
__device__ __forceinline__ u32 su(s16x2 x) { return __builtin_bit_cast(u32, x); }
__device__ __forceinline__ u32 pmin(u32 a, u32 b) { return su(__builtin_elementwise_min(sv(a), sv(b))); }
__device__ __forceinline__ u32 padd(u32 a, u32 b) { return su(__builtin_elementwise_add_sat(sv(a), sv(b))); }
__device__ __forceinline__ u32 pfin(u32 u) {   // halves in [0x4000, 0x7FFF] -> 0x7FFF
    const u32 imp = (u & ~(u >> 1)) & 0x40004000u;
    return u | ((imp >> 14) * 0x7FFFu);
}

template <int CTRL, int ROWS>
__device__ __forceinline__ u32 dpp_min(u32 v) {
    const int moved = __builtin_amdgcn_update_dpp(int(INF16), int(v), CTRL, ROWS, 0xf, false);
    return pmin(v, u32(moved));
}
__device__ __forceinline__ u32 wave_min(u32 v) {   // full-wave min, result uniform
    v = dpp_min<0xb1, 0xf>(v);    // quad_perm [1,0,3,2]
    v = dpp_min<0x4e, 0xf>(v);    // quad_perm [2,3,0,1]
    v = dpp_min<0x114, 0xf>(v);   // row_shr:4
    v = dpp_min<0x118, 0xf>(v);   // row_shr:8
    v = dpp_min<0x142, 0xa>(v);   // row_bcast:15
    v = dpp_min<0x143, 0xc>(v);   // row_bcast:31
    return u32(__builtin_amdgcn_readlane(int(v), 63));
}

// min across lane halves / 16-lane rows (lanes l, l^32 / l, l^16 end equal; no LDS)
__device__ __forceinline__ u32 fold_halves(u32 v) {
    const auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return pmin(u32(p[0]), u32(p[1]));
}
__device__ __forceinline__ u32 fold_rows16(u32 v) {
    const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return pmin(u32(p[0]), u32(p[1]));
}

// LDS byte address of an LDS object (the inline-asm read batches address LDS directly)
typedef __attribute__((address_space(3))) char lds_char;
template <class T>
__device__ __forceinline__ uint32_t lds_addr(T *p) {
    return uint32_t(uintptr_t((lds_char *)(p)));   // generic -> LDS address space
}

// A pointer to LDS byte address a: kernels without static LDS (no __shared__
// variables, no library code that declares any -- fold_common.hpp block_or)
// get their dynamic block at address 0, so a carve of literal addresses needs
// no SGPR per region (the launcher checks the static size is 0)
template <class T>
__device__ __forceinline__ T *lds_at(size_t a) {
    return (T *)((__attribute__((address_space(3))) char *)(uint32_t(a)));
}

// The per-size energy records (DevScaled::ku16) through the constant address
// space: uniform loads from it are scalar (s_load, lgkmcnt).  Through a generic
// pointer they were flat loads, which count on vmcnt too, so the first record
// use of a block waited for the block's 1x1..2x2 table prefetches from L2.
typedef __attribute__((address_space(4))) const uint32_t kc_u32;
__device__ __forceinline__ const kc_u32 *kconst(const uint4 *p) { return (const kc_u32 *)(uintptr_t)p; }
__device__ __forceinline__ uint4 kload(const kc_u32 *p, int k) {   // record k (4 words)
    return make_uint4(p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]);
}

// ---------------------------------------------------------------- interior-loop shapes
struct BUni {                 // wave-uniform
    uint32_t aq, ac, act;     // LDS byte addresses of qbm, cc, ct (inline-asm batches)
    const u32 *qbm;           // LDS
    const uint8_t *cc;        // LDS
    const u32 *ct;            // LDS (per-lane indexed factors)
    const uint4 *kg;          // per loop size u: {il[u] + nin[k] (k = 0..5), bulge[u], 1 x (u-1)}
                              // (DevScaled::ku16, uniform: scalar loads)
    const u32 *gct;           // HBM ctab (uniform entries, runtime path only)
    const u32 *il, *nin;      // HBM generic interior energy parts (runtime path only)
    u32 fs1;                  // bulge of size 1
    int d, N, umax;
    bool mk;                  // some lane's unpaired runs cut loop sizes <= umax: mask shapes
    __device__ __forceinline__ int offu(int u) const { return off(d - 2 - u, N); }
};
struct BCell {                // per lane: the closing pair (i, i+d)
    int i, ty8, A, B;
    uint32_t rs;              // 4 * lane slice (sliced blocks: first generic shape offset)
    uint32_t ee;              // 4 lanes per cell: LDS byte address of the slice's column of CL::e4
    bool r1, r2;              // lane slice bits
    int hb;                   // pair kernel (mfe_pair.hip): 1 on the lanes of the step's second diagonal
    int ea, eb, ctb;          // sliced blocks: the slice's edge shapes n1 = ea + eb * u, their factor table
    u32 m23f;                 // 2x3: interior[5] + ninio + outer mismatch23
    u32 t11, t12, t21, t22;   // prefetched 1x1 / 1x2 / 2x1 / 2x2 table energies (mfe_pair.hip: the low half)
};
struct Acc {
    u32 s, g0, g1, b, n;      // specials; generic (+ outer mismatchI, even / odd u1); bulges (+ TermAU); 1xn (+ mismatch1n)
    u32 e;                    // 4 lanes per cell: the slice's edge shapes (+ TermAU on slices 0, 1, mismatch1n on 2, 3)
};

#define MFE_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)

// wave-uniform part of the blocks' state (d, umax, mk: per step / lane-set)
template <class LT>
__device__ __forceinline__ BUni buni(const LT &L, const DevScaled *XS, int N) {
    const u32 *gct = reinterpret_cast<const u32 *>(XS->ctab);
    BUni U;
    U.qbm = L.qbm;
    U.cc = L.cc;
    U.ct = L.ct;
    U.gct = gct;
    U.kg = reinterpret_cast<const uint4 *>(XS->ku16);
    U.aq = lds_addr(L.qbm);
    U.ac = lds_addr(L.cc);
    U.act = lds_addr(L.ct);
    U.fs1 = gld(gct + CT_FSM + 1);
    U.il = reinterpret_cast<const u32 *>(XS->il);
    U.nin = reinterpret_cast<const u32 *>(XS->nin);
    U.N = N;
    return U;
}

// A B cell's setup: the closing pair's row, its code oc = type * 25 + S[i+1] * 5
// + S[j-1], the unpaired runs inside it, mismatchI(oc) and mismatch1n(oc) +
// mismatchI(oc).  The list role records it for the ranks < 64 (brec_word; the
// kernels store the two energies their own way: three words a record in
// mfe_cells.hip, two in mfe_pair.hip, which packs one half of each)
struct BRec {
    int i, oc, A, B;
    u32 mmo, mo;
};
__device__ __forceinline__ u32 brec_word(int i, int oc, int A, int B) {   // the record's first word
    return uint32_t(i) | (uint32_t(oc) << 8) | (uint32_t(A) << 16) | (uint32_t(B) << 24);
}
__device__ __forceinline__ BRec brec_unpack(u32 wd, u32 mmo, u32 mo) {
    return BRec{int(wd & 255), int((wd >> 8) & 255), int((wd >> 16) & 255), int(wd >> 24), mmo, mo};
}
template <class LT>
__device__ __forceinline__ int brec_code(const LT &L, int i, int j) {
    return ptype(L.S[i], L.S[j]) * 25 + L.S[i + 1] * 5 + L.S[j - 1];
}
template <class LT>
__device__ __forceinline__ BRec brec_of(const LT &L, int i, int j) {   // from the tables (ranks >= 64)
    BRec r;
    r.i = i;
    r.oc = brec_code(L, i, j);
    r.A = L.up[i + 1];
    r.B = L.dn[j - 1];
    r.mmo = L.dt[DT_MMI + r.oc];
    r.mo = padd(L.ct[CT_ONEN + r.oc], r.mmo);
    return r;
}

// lane slice r of 1 << sh per cell.  Edge shapes (gen_mfe_blocks.py
// sliced_parts): 4 slices -> bulge (0,u), (u,0), 1 x n (1,u-1), (u-1,1);
// 2 slices -> bulge (0,u) + 1 x n (1,u-1) or bulge (u,0) + 1 x n (u-1,1)
__device__ __forceinline__ void bcell_slice(BCell &C, int r, int sh, uint32_t ae4) {
    C.rs = uint32_t(r) * 4u;
    C.ee = ae4 + uint32_t(r) * 4u;
    C.r1 = (r & 1) != 0;
    C.r2 = (r & 2) != 0;
    C.eb = r & 1;
    C.ea = sh == 2 ? ((r & 1) ? -(r >> 1) : (r >> 1)) : ((r & 1) ? -1 : 1);
    C.ctb = (r & 2) ? CT_ONEN : CT_BUL;
}

// the two 16-bit energies of a word, each to a packed apo | holo word
__device__ __forceinline__ u32 lo2(u32 x) { return __builtin_amdgcn_perm(x, x, 0x05040504u); }
__device__ __forceinline__ u32 hi2(u32 x) { return __builtin_amdgcn_perm(x, x, 0x07060706u); }

// 1x1 .. 2x2 energies of cell (i, i + dd) from HBM (L2), used at the block end (the caller starts
// them at INF16), 16 bits wide as loaded: the block widens them with lo2() where it uses them
// (widened here, each load was waited for at once); p2, p3, p4: this wave's block reads loop size 2, 3, 4, um: the cell's largest.
// E: the energies by code pair (loop_codetab_core.hpp, KArgs::loop16), E[k][oc][c] with the cell's
// code oc and the inner pair's c as they stand: one multiply-add and one load per energy (indexing
// int11 / int21 / int22 by the types and bases took the codes apart with / 5 and % 5, 50 VALU
// instructions a step on the size-3 wave).
// mfe_pair.hip only: mfe_cells.hip tests one bit per block and keeps its copy (this form: -1.9 % at N = 150)
template <class LT>
__device__ __forceinline__ void bcell_tables(BCell &C, const LT &L, const uint16_t *E, int N, int dd, int i, int oc,
                                             int um, bool p2, bool p3, bool p4) {
    // byte offsets in 32 bits off the one uniform base: row oc by a 24-bit multiply, once per cell
    const uint32_t ob = __umul24(uint32_t(oc), uint32_t(sizeof(uint16_t)) * LCT_CODES);
    auto at = [&](int k, int c) {
        const uint32_t o = ob + uint32_t(sizeof(uint16_t)) * uint32_t(loop_codetab_index(k, 0, c));
        return u32(gld(reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(E) + o)));
    };
    if (p2 && um >= 2) C.t11 = at(LCT_11, L.cc[off(dd - 4, N) + i + 1]);
    if (p3 && um >= 3) {
        const int o3 = off(dd - 5, N) + i;
        const int a2 = L.cc[o3 + 1], b2 = L.cc[o3 + 2];
        C.t12 = at(LCT_12, a2);
        C.t21 = at(LCT_21, b2);
    }
    if (p4 && um >= 4) C.t22 = at(LCT_22, L.cc[off(dd - 6, N) + i + 2]);
}

// a block's accumulators to the cell's partial minimum: the outer pair's terms,
// then the minimum over the cell's lane slices
__device__ __forceinline__ u32 acc_fold(const Acc &a, const BCell &C, int sh, u32 mmo, u32 mo, u32 tau) {
    u32 acc = pmin(pmin(a.s, padd(pmin(a.g0, a.g1), mmo)), pmin(padd(a.b, tau), padd(a.n, mo)));
    if (sh == 2) acc = pmin(acc, padd(a.e, C.r2 ? mo : tau));
    if (sh == 2) acc = fold_rows16(acc);
    if (sh >= 1) acc = fold_halves(acc);
    return acc;
}

// ---------------------------------------------------------------- shared by both carves
constexpr int NWV = 8;            // waves per walker
constexpr int MFE_WPE = (2 * NWV + 3) / 4;   // waves per SIMD the register budget is cut for (2 workgroups)
constexpr int MFE_E4_MAX = 64;    // slots of e4 the carves hold (MFE_E4_SLOTS of the generated blocks)
constexpr size_t al16(size_t b) { return (b + 15) & ~size_t(15); }
__device__ __forceinline__ int lanesets(int n) { return (n + 63) >> 6; }   // of a diagonal with n cells

// The eight byte arrays, NP bytes apart from y in this order.  Role F's read
// batch in mfe_pair.hip relies on the spacing: it reads up and dn at offsets
// NP and 2 NP from an address in S
template <class LT>
__device__ __forceinline__ void carve_bytes(LT &l, uint8_t *y, int NP) {
    l.S = y;
    l.up = y + NP;
    l.dn = y + 2 * NP;
    l.ptn = y + 3 * NP;
    l.enc = y + 4 * NP;
    l.flg = y + 5 * NP;
    l.mat = y + 6 * NP;
    l.raw = y + 7 * NP;
}

// A fold's incremental state (KArgs::tab): the slot it writes and, for a
// refold, the slot it restores and the changed positions in the folded sequence
struct IncM {
    const u32 *src;
    u32 *dst;
    int m_lo, m_hi;
    const uint4 *cc_src;   // the slots' per-cell codes (dev_types.hpp inc_cc_offset); mfe_cells.hip
    uint4 *cc_dst;         // recomputes the codes and leaves cc_src null
    __device__ __forceinline__ Band band(int N) const { return Band{src != nullptr, N, uni(m_lo), uni(m_hi)}; }
};
// walker w's fold group g writes slot 1 - cur ...
__device__ __forceinline__ IncM inc_slots(const KArgs &ka, int w, int g, int cur) {
    const size_t Gf = inc_group_floats(ka.cells, ka.Nmax, 1);
    float *to = ka.tab + size_t(w) * 2 * ka.tab_slot + size_t(1 - cur) * ka.tab_slot;
    return IncM{nullptr, reinterpret_cast<u32 *>(to + size_t(g) * Gf), 0, 0, nullptr,
                reinterpret_cast<uint4 *>(to + inc_cc_offset(ka.cells, ka.Nmax, ka.n_groups2, g))};
}
// ... and a refold restores slot cur; c0 .. c1: the changed raw positions, lb: the context before them
__device__ __forceinline__ void inc_refold(IncM &inc, const KArgs &ka, int w, int g, int cur, int c0, int c1, int lb) {
    const size_t Gf = inc_group_floats(ka.cells, ka.Nmax, 1);
    const float *from = ka.tab + size_t(w) * 2 * ka.tab_slot + size_t(cur) * ka.tab_slot;
    inc.src = reinterpret_cast<const u32 *>(from + size_t(g) * Gf);
    inc.cc_src = reinterpret_cast<const uint4 *>(from + inc_cc_offset(ka.cells, ka.Nmax, ka.n_groups2, g));
    inc.m_lo = c0 + 1 + lb;
    inc.m_hi = c1 + 1 + lb;
}

// ---------------------------------------------------------------- setup and finish pieces
// q5[0..4]: no pair fits (one thread)
template <class LT>
__device__ __forceinline__ void q5_start(const LT &L, int N) {
    L.q5[0] = 0u;
    for (int j = 1; j <= 4 && j <= N; j++) L.q5[j] = (L.up[j] >= 1) ? L.q5[j - 1] : INF16;
}

// fold_writeback_once's pass over the fold's whole vectors of V (n words each) of the
// three tables: every element read from LDS once, checked and, with a slot to
// write (dp; Cs words between its tables), stored.  Returns the cells done
template <class V, int NT, class LT>
__device__ __forceinline__ int writeback_vectors(const LT &L, u32 *dp, size_t Cs, int C, int tid, bool &low) {
    constexpr int n = int(sizeof(V) / sizeof(u32));
    const int nv = C / n;   // n = 1, 2, 4: a shift
    const uint32_t cs = uint32_t(Cs) / n;   // (the caller checked that Cs is a multiple of n)
    for (int k = tid; k < nv; k += NT) {
        const V a = reinterpret_cast<const V *>(L.qbm)[k];
        const V b = reinterpret_cast<const V *>(L.qm)[k];
        const V c = reinterpret_cast<const V *>(L.qm1)[k];
        u32 e[3 * n];
        __builtin_memcpy(e, &a, sizeof a);
        __builtin_memcpy(e + n, &b, sizeof b);
        __builtin_memcpy(e + 2 * n, &c, sizeof c);
#pragma unroll
        for (int t = 0; t < 3 * n; t++) low |= mfe16_inexact(sv(e[t]));
        if (dp) {
            // (32-bit offsets from the slot: one base address for the three tables)
            gst(reinterpret_cast<V *>(dp) + uint32_t(k), a);
            gst(reinterpret_cast<V *>(dp) + (cs + uint32_t(k)), b);
            gst(reinterpret_cast<V *>(dp) + (2 * cs + uint32_t(k)), c);
        }
    }
    return nv * n;
}

// mfe_pair.hip's write-back (tid: the thread's index).  The fold's cells of the
// three tables, q5 and the codes to the slot the fold writes (the next proposal's
// unchanged cells; a restore reads no cell past the fold's own), and the
// exactness guard, as fold_writeback below, in one pass: each element
// is read from LDS once, checked and stored, in the widest vectors that the LDS
// tables, the slot and its table stride (ka.cells) are all aligned for -- 16
// bytes at Nmax = 100 for a walker's even fold groups, 8 for the odd ones, whose
// slot starts 3 cells + Nmax + 2 words later; the cells past the last whole
// vector, and every cell of a layout aligned to 4 bytes only, go one by one.
// (Two passes with 4-byte accesses before; a merged pass that found each
// element's table by a division measured -1.2 % in round 6.)  mfe_cells.hip keeps
// the two passes: at Nmax = 150 the slot's tables are aligned to 4 bytes only
// (10731 cells), and this function's one-by-one loop measured -3.2 % on the
// 150-nt bench line.  Returns this thread's part of the guard; the caller ORs it
// over the workgroup
template <int NT, class LT>
__device__ __forceinline__ bool fold_writeback_once(const KArgs &ka, const LT &L, const IncM &inc, int N, int tid) {
    const int C = ((N - 4) * (N - 3)) >> 1;
    const size_t Cs = size_t(ka.cells);
    u32 *dp = inc.dst;
    bool low = false;
    const uint32_t al = uni(int(uint32_t(uintptr_t(dp)) | uint32_t(Cs * 4) | lds_addr(L.qbm) | lds_addr(L.qm) |
                                lds_addr(L.qm1)));
    int done = 0;
    if ((al & 15u) == 0) done = writeback_vectors<uint4, NT>(L, dp, Cs, C, tid, low);
    else if ((al & 7u) == 0) done = writeback_vectors<uint2, NT>(L, dp, Cs, C, tid, low);
    for (int k = done + tid; k < C; k += NT) {
        const u32 a = L.qbm[k], b = L.qm[k], c = L.qm1[k];
        low |= mfe16_inexact(sv(a)) || mfe16_inexact(sv(b)) || mfe16_inexact(sv(c));
        if (dp) {
            gst(dp + uint32_t(k), a);
            gst(dp + (uint32_t(Cs) + uint32_t(k)), b);
            gst(dp + (2 * uint32_t(Cs) + uint32_t(k)), c);
        }
    }
    for (int k = tid; k <= N; k += NT) {
        const u32 q = L.q5[k];
        low |= mfe16_inexact(sv(q));
        if (dp) gst(dp + (3 * uint32_t(Cs) + uint32_t(k)), q);
    }
    if (dp) {
        const int C16 = (C + 15) >> 4;
        for (int k = tid; k < C16; k += NT) gst(inc.cc_dst + uint32_t(k), reinterpret_cast<const uint4 *>(L.cc)[k]);
    }
    return low;
}

// After the sweep: the three tables, q5 and the codes to the slot the fold
// writes (the next proposal's unchanged cells), and the exactness guard of the
// 16-bit encoding, every stored value >= floor.  Returns this thread's part of
// the guard; the caller ORs it over the workgroup
template <int NT, class LT>
__device__ __forceinline__ bool fold_writeback(const KArgs &ka, const LT &L, const IncM &inc, int N) {
    const int tid = threadIdx.x;
    if (inc.dst) {
        const size_t C = size_t(ka.cells);
        u32 *dp = inc.dst;
        for (int k = tid; k < int(C); k += NT) {
            dp[k] = L.qbm[k];
            dp[C + k] = L.qm[k];
            dp[2 * C + k] = L.qm1[k];
        }
        for (int k = tid; k <= N; k += NT) dp[3 * C + k] = L.q5[k];
        const int C16 = (((N - 4) * (N - 3)) / 2 + 15) >> 4;
        for (int k = tid; k < C16; k += NT) inc.cc_dst[k] = reinterpret_cast<const uint4 *>(L.cc)[k];
    }
    bool low = false;
    const int C = ((N - 4) * (N - 3)) >> 1;
    auto chk = [&](u32 x) { low |= mfe16_inexact(sv(x)); };
    for (int k = tid; k < C; k += NT) {
        chk(L.qbm[k]);
        chk(L.qm[k]);
        chk(L.qm1[k]);
    }
    for (int k = tid; k <= N; k += NT) chk(L.q5[k]);
    return low;
}

// One thread: f5[N] = z of the group's two variants to gout (dcal/mol; a half of
// 0x4000 and above = no structure); bad: a value left the exact range, so the
// walker is re-folded by the FP32 MinPlus kernel and from scratch next time
__device__ __forceinline__ void fold_result(const KArgs &ka, int w, const int *vs, float *gout, u32 z, bool bad) {
    const s16x2 q = sv(z);
    const int hv[2] = {q.x, q.y};
    for (int h = 0; h < 2; h++) {
        const double e = hv[h] >= 0x4000 ? double(INFINITY) : static_cast<double>(hv[h]) / 100.0;
        gst(gout + size_t(w) * ka.n_variants + vs[h], static_cast<float>(e));
    }
    if (bad && ka.ovf) {
        gst(ka.ovf + w, 1);
        if (ka.tab) gst(ka.tab_valid + w, 0);
    }
}

}  // namespace
}  // namespace adx
