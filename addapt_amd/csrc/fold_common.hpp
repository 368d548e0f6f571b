// Helpers shared by the fold kernels (fold_rows.hip, mfe_cells.hip, ...) that
// need HIP: global-address-space loads and stores, the LDS-only barrier and the
// workgroup OR, a fold workgroup's walker words, the packed 16-bit min-plus
// range, the special-hairpin lookup, a refold's band, the motif sites by wave
// (motif_scan, motif_constraints) and the quad sum over four DPP lanes.  The
// pure index arithmetic -- cell indexing, pair types, loop kinds, allowed(), the
// folded sequence in its context, the scalar motif site, the per-cell table
// block layout -- is fold_setup_core.hpp, included here for every kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_types.hpp"

#define FS_FN __device__ __forceinline__
#include "fold_setup_core.hpp"

// Diagnostic builds (-DADX_STAMP) only, never the product: add the cycles
// (s_memtime) since the wave's last stamp to its phase counter k.  st_acc and
// st_last are the kernel's locals; each kernel copies st_acc to its own
// g_stamps_* array, read back through its adx_debug_stamps*() export.
#ifdef ADX_STAMP
#define ADX_STAMP_AT(k) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[k] += t_ - st_last; st_last = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define ADX_STAMP_AT(k) do { } while (0)
#endif

// The four-lanes-per-cell interior-loop sweeps (pf_cells.hip, pf_ring.hip,
// outside_common.hpp) compute the sizes <= 5 on phase 0 only (the other
// phases' copies are discarded); 0: on every phase
#ifndef ADX_SMALL_R0
#define ADX_SMALL_R0 1
#endif

namespace adx {
namespace {

constexpr int WAVE = 64;

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

// Loads and stores of device memory through a pointer typed to the global
// address space at the dereference: global_load / global_store, which count on
// vmcnt alone.  A pointer the compiler cannot trace to a kernel argument (one
// rebuilt from words that mfe_pair.hip's loop reads again from the argument
// segment) is a generic pointer, and an access through it is a flat
// instruction, which counts on lgkmcnt as well: every `s_waitcnt lgkmcnt(0)`
// after an LDS batch then also waits for the loads from L2 / HBM still in flight.
// Where the compiler already knows the address space the code is the same.
// (uint2 / uint4 go as vectors of words: 8- and 16-byte accesses)
template <class T>
struct gmem_word {
    using type = T;
};
template <>
struct gmem_word<uint2> {
    typedef uint32_t type __attribute__((ext_vector_type(2)));
};
template <>
struct gmem_word<uint4> {
    typedef uint32_t type __attribute__((ext_vector_type(4)));
};
template <class T>
__device__ __forceinline__ T gld(const T *p) {
    typedef __attribute__((address_space(1))) const typename gmem_word<T>::type g_t;
    return __builtin_bit_cast(T, *(g_t *)(p));   // generic -> global address space
}
template <class T, class V>
__device__ __forceinline__ void gst(T *p, V v) {
    typedef __attribute__((address_space(1))) typename gmem_word<T>::type g_t;
    *(g_t *)(p) = __builtin_bit_cast(typename gmem_word<T>::type, T(v));
}

// Workgroup barrier ordering LDS only (the fold's waves share nothing else
// inside its diagonal loop): outstanding global loads are not drained, so a
// prefetch issued before the barrier completes in the shadow of the next
// iteration instead of stalling the barrier.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Workgroup OR of v through the LDS word *w, which must hold 0 and have been
// written before a barrier every thread has passed since.  Replaces
// __syncthreads_or, whose library implementation adds 256 B of static LDS:
// with none, the dynamic LDS starts at address 0 and every carve address is a
// literal the compiler rematerialises instead of keeping it in an SGPR.
__device__ __forceinline__ bool block_or(int *w, bool v) {
    if (__ballot(v) != 0 && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(w, 1);
    __syncthreads();
    return *w != 0;
}

// The walker a fold workgroup takes at launch position wb (order: a step's
// launch order, mc_step.hip order_kernel; null: blockIdx order), or -1 when
// mask (1 = fold) leaves it nothing to fold.
__device__ __forceinline__ int walker_at(const int *order, const int *mask, int wb) {
    const int w = order ? order[wb] : wb;
    if (mask && mask[w] != 1) return -1;
    return w;
}

// A fold workgroup's per-walker words -- its mask, slot index, slot validity and
// the proposal's changed range -- loaded in one round trip after the walker's index
// (the chain order -> mask -> slot -> change waited on three); valid is false and
// c0 < 0 without incremental state.  K: KArgs (dev_types.hpp)
struct WalkerRef {
    int w, cur, c0, c1;
    bool on, valid;
};
template <class K>
__device__ __forceinline__ WalkerRef walker_ref(const K &ka, const int *mask, int wb) {
    WalkerRef r;
    r.w = ka.order ? gld(ka.order + wb) : wb;
    const int w = r.w;
    const int mk = mask ? gld(mask + w) : 1;
    r.cur = ka.tab ? int(gld(ka.cur_slot + w)) : 0;
    r.valid = ka.tab ? gld(ka.tab_valid + w) != 0 : false;
    r.c0 = ka.chg ? gld(ka.chg + 2 * w) : -1;
    r.c1 = ka.chg ? gld(ka.chg + 2 * w + 1) : -1;
    r.on = mk == 1;
    return r;
}

typedef short s16x2 __attribute__((ext_vector_type(2)));
constexpr int MFE16_FLOOR = -12000;
// Exactness of the packed 16-bit MFE encoding (fold_rows.hip MinPlus16): a half
// >= 0x4000 is "impossible".  A true finite value can only reach that band as
// a sum of at most two stored values plus loop constants (each < 40.96
// kcal/mol, i.e. < 0x1000), so while every stored finite value is below
// MFE16_CEIL = 0x1800 (61.44 kcal/mol) no finite value is ever mistaken for an
// impossible one; and an impossible operand plus one stored value >= FLOOR
// stays >= 0x7FFF - 12000 > 0x4000, so no impossible value passes for finite.
// A fold with a stored half outside [FLOOR, CEIL) -- other than the impossible
// band [0x4000, 0x7FFF] -- is re-folded by the FP32 kernel (round 6: the
// ceiling; before, a forced fold above 163.84 kcal/mol read as impossible).
constexpr int MFE16_CEIL = 0x1800;
__device__ __forceinline__ bool mfe16_inexact(s16x2 q) {
    auto out = [](int h) { return h < MFE16_FLOOR || (h >= MFE16_CEIL && h < 0x4000); };
    return out(q.x) || out(q.y);
}

// Index of the special hairpin whose key is `key` in spk[0, MAX_SPECIAL_HP) (LDS,
// 16-byte aligned, padded with 0xFFFFFFFF, which hp_key never returns), or -1; the
// last match, as a scan would find.  Every key comes in wave-uniform 16-byte loads
// issued before any compare: the compare -> value-load chain per key it replaces
// serialised ~16 LDS round trips per 8 keys, ~10k cycles per cell-pass item on the
// special-hairpin diagonals (stamps, profiles/r06s_mfe_pair_stamps_setup.txt)
__device__ __forceinline__ int special_hp(const uint32_t *spk, uint32_t key) {
    static_assert(MAX_SPECIAL_HP % 16 == 0, "whole 16-key chunks");
    int hit = -1;
#pragma unroll
    for (int q0 = 0; q0 < MAX_SPECIAL_HP; q0 += 16) {
        uint4 k[4];
#pragma unroll
        for (int t = 0; t < 4; t++) k[t] = reinterpret_cast<const uint4 *>(spk + q0)[t];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            hit = k[t].x == key ? q0 + 4 * t : hit;
            hit = k[t].y == key ? q0 + 4 * t + 1 : hit;
            hit = k[t].z == key ? q0 + 4 * t + 2 : hit;
            hit = k[t].w == key ? q0 + 4 * t + 3 : hit;
        }
    }
    return hit;
}

// The band of a refold after positions m_lo .. m_hi changed: rows clo .. chi of
// span dd hold the cells of qbm / qm1 that contain a changed position (or the
// neighbour whose dangle they read), rows qlo .. qhi of span s the cells of qm
// that do.  A fold from scratch: every row
struct Band {
    bool incr;
    int N, m_lo, m_hi;
    __device__ __forceinline__ int clo(int dd) const { return incr ? max(1, m_lo - 1 - dd) : 1; }
    __device__ __forceinline__ int chi(int dd) const { return incr ? min(N - dd, m_hi + 1) : N - dd; }
    __device__ __forceinline__ int qlo(int s) const { return incr ? max(1, m_lo - 2 - s) : 1; }
    __device__ __forceinline__ int qhi(int s) const { return incr ? min(N - s, m_hi + 2) : N - s; }
};

// ---------------------------------------------------------------- motif sites by wave
// The sequence scan, one lane per start o: mat[o] = the motif's bases stand at o
template <int NT, class LT>
__device__ __forceinline__ void motif_scan(const LT &L, const uint8_t *mcode, int mL, int N, int tid) {
    for (int o = tid + 1; o + mL - 1 <= N; o += NT) L.mat[o] = motif_seq_match(L.S, mcode, mL, o) ? 1 : 0;
}
// The constraints, after a barrier: one of the NW waves per matching start o,
// lanes = motif positions with partner table mpt (fold_setup_core.hpp
// motif_site's second half, spread over the lanes)
template <int NW, class LT>
__device__ __forceinline__ void motif_constraints(const LT &L, const int8_t *mpt, int mL, int N, int wid, int lane) {
    for (int o = 1 + wid; o + mL - 1 <= N; o += NW) {
        if (!uni(L.mat[o])) continue;
        bool ok = true;
        for (int k = lane; k < mL; k += WAVE) {
            const int pk = mpt[k];
            if (pk < 0) ok = ok && L.up[o + k] >= 1;
            else if (pk > k) ok = ok && allowed(L, o + k, o + pk);
        }
        const bool all = __ballot(!ok) == 0;
        if (lane == 0) L.mat[o] = all ? 1 : 0;
    }
}

// ---------------------------------------------------------------- the structure kernels' setup
// mfe_trace.hip and pf_sample.hip, NT threads: the sequence in its context, the
// variant's constraint arrays, the special hairpins (values through
// special_value(listed, table value)), the motif tables, the wrap and the motif
// sites into L (TraceLds, PfSeqLds: the same field names); ends with a barrier
template <int NT, class LT, class SV>
__device__ void seq_setup(LT &L, const KArgs &ka, const DevVariant &V, const uint8_t *raw, int tid, SV special_value) {
    const DevScaled *X = ka.X;
    const int N = V.N, np = N + 2;
    const uint8_t *cons = ka.cons + V.cons_off;
    const SeqSrc src = seq_src(ka, V, raw);
    for (int k = tid; k < np; k += NT) {
        L.S[k] = src.code(k, N);
        L.up[k] = cons[k];
        L.ptn[k] = cons[2 * np + k];
        L.enc[k] = cons[3 * np + k];
        L.flg[k] = cons[4 * np + k];
        L.mat[k] = 0;
    }
    for (int k = tid; k < MAX_SPECIAL_HP; k += NT) {
        const bool on = k < X->n_special;
        L.spk[k] = on ? X->sp_key[k] : 0xFFFFFFFFu;   // hp_key never sets the top bits
        L.spv[k] = special_value(on, X->sp_val[k]);
    }
    for (int k = tid; k < MAX_MOTIF; k += NT) {
        L.mcode[k] = X->motif_code[k];
        L.mpt[k] = X->motif_pt[k];
    }
    __syncthreads();
    if (tid == 0) wrap_ends(L, N);   // (no motif site reads the two ends)
    const int mL = X->motif_len;
    if (V.motif != 0 && mL > 0)
        for (int o = tid + 1; o + mL - 1 <= N; o += NT) L.mat[o] = motif_site(L, L.mcode, L.mpt, mL, o) ? 1 : 0;
    __syncthreads();
}

// ---------------------------------------------------------------- quad sum
typedef float f2 __attribute__((ext_vector_type(2)));
// v + (v of the lane DPP control CTRL selects; 0 where it selects none)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ f2 dpp_add(f2 v) {
    const float x = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v.x), CTRL, 0xf, 0xf, false));
    const float y = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v.y), CTRL, 0xf, 0xf, false));
    return v + f2{x, y};
}
template <class V>
__device__ __forceinline__ V quad_sum(V v) {   // sum over the 4 lanes of a quad, in every lane
    v = dpp_add<0xb1>(v);      // quad_perm [1,0,3,2]
    return dpp_add<0x4e>(v);   // quad_perm [2,3,0,1]
}

}  // namespace
}  // namespace adx
