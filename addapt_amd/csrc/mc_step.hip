// The fused Monte Carlo step (MonteCarlo::apply, sampling.cc:55-99): the
// walkers' MT19937 streams, the median of the auto thermostat, the Metropolis
// decision and the next proposal (step_tail_kernel), the launch order of a
// step's folds (order_kernel) and the from-scratch rescore.  The folds and
// scores of a step's window are launched through dispatch.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "combine.hpp"
#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"

namespace adx {

namespace {

// ---------------------------------------------------------------- mt19937
__device__ void mt_twist_wave(uint32_t *mt, int lane) {
    // three dependency-free phases (see DESIGN.md "RNG")
    for (int i = lane; i < 227; i += WAVE) {
        const uint32_t y = (mt[i] & 0x80000000u) | (mt[i + 1] & 0x7fffffffu);
        const uint32_t v = mt[i + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        mt[i] = v;
    }
    for (int i = 227 + lane; i < 454; i += WAVE) {
        const uint32_t y = (mt[i] & 0x80000000u) | (mt[i + 1] & 0x7fffffffu);
        const uint32_t v = mt[i - 227] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        mt[i] = v;
    }
    for (int i = 454 + lane; i < 624; i += WAVE) {
        const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
        const uint32_t v = mt[i - 227] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        mt[i] = v;
    }
}

// Orders a wave's LDS accesses around it (the LDS executes one wave's
// instructions in order; this keeps the compiler from moving them across):
// the MC step's waves each own their LDS and never wait for one another.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A walker's MT19937 stream (MT_WORDS words in HBM: state + index) as a step
// reads it: only the words [lo, hi) it will draw are staged in LDS (a step
// draws a few), the whole state only when it twists (then written back).
struct MtView {
    uint32_t *mt;          // LDS, words [lo, hi) valid
    const uint32_t *g;     // HBM state
    int idx, lo, hi;
    bool twisted;
};

__device__ uint32_t mt_next(MtView &g, int lane) {
    if (g.idx >= 624) {
        if (g.lo != 0 || g.hi != 624) {
            for (int k = lane; k < 624; k += WAVE) g.mt[k] = g.g[k];
            wave_sync();
            g.lo = 0;
            g.hi = 624;
        }
        mt_twist_wave(g.mt, lane);
        g.idx = 0;
        g.twisted = true;
    }
    uint32_t y = (g.idx < g.hi) ? g.mt[g.idx] : g.g[g.idx];   // past the window: a rejection draw
    g.idx++;
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// libstdc++-11 uniform_int_distribution (Lemire) for [0, R-1]
__device__ uint32_t mt_uniform(MtView &g, uint32_t R, int lane) {
    uint64_t product = uint64_t(mt_next(g, lane)) * R;
    uint32_t low = uint32_t(product);
    if (low < R) {
        const uint32_t threshold = (0u - R) % R;
        while (low < threshold) {
            product = uint64_t(mt_next(g, lane)) * R;
            low = uint32_t(product);
        }
    }
    return uint32_t(product >> 32);
}

__device__ double mt_canonical(MtView &g, int lane) {
    const double r = 4294967296.0;
    double sum = double(mt_next(g, lane));
    sum += double(mt_next(g, lane)) * r;
    double ret = sum / (r * r);
    if (ret >= 1.0) ret = 0.99999999999999989;  // nextafter(1, 0)
    return ret;
}

// ---------------------------------------------------------------- median
// std::nth_element(a, a + k, a + n) over doubles with operator<, following
// libstdc++ 11's introselect (<bits/stl_algo.h> __introselect,
// __unguarded_partition_pivot, __move_median_to_first, __insertion_sort;
// <bits/stl_heap.h> __heap_select / __adjust_heap / __push_heap) compare for
// compare and swap for swap.  AutoScalingThermostat::adjust calls it on its
// training set (sampling.cc:389-393); keeping the same order of operations
// puts the same element at k even among +0.0 / -0.0 ties and NaNs.  Run by one
// lane on the walker's training buffer (<= period doubles, once per period).
__device__ __forceinline__ void nth_swap(double *a, int i, int j) {
    const double t = a[i];
    a[i] = a[j];
    a[j] = t;
}

__device__ void nth_adjust_heap(double *a, int hole, int len, double v) {
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (a[child] < a[child - 1]) child--;
        a[hole] = a[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        a[hole] = a[child - 1];
        hole = child - 1;
    }
    int parent = (hole - 1) / 2;
    while (hole > top && a[parent] < v) {
        a[hole] = a[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    a[hole] = v;
}

__device__ void nth_element_libstdcxx(double *a, int k, int n) {
    if (n == 0 || k == n) return;
    int first = 0, last = n;
    int depth = 2 * (31 - __clz(n));
    while (last - first > 3) {
        if (depth == 0) {
            // __heap_select(first, k + 1, last) then iter_swap(first, k)
            double *h = a + first;
            const int mid = k + 1 - first, len = last - first;
            if (mid >= 2)
                for (int p = (mid - 2) / 2;; p--) {
                    nth_adjust_heap(h, p, mid, h[p]);
                    if (p == 0) break;
                }
            for (int i = mid; i < len; i++)
                if (h[i] < h[0]) {
                    const double v = h[i];
                    h[i] = h[0];
                    nth_adjust_heap(h, 0, mid, v);
                }
            nth_swap(a, first, k);
            return;
        }
        --depth;
        // __unguarded_partition_pivot: median of (first+1, mid, last-1) to first
        const int m = first + (last - first) / 2, x = first + 1, z = last - 1;
        int pick;
        if (a[x] < a[m]) pick = (a[m] < a[z]) ? m : (a[x] < a[z]) ? z : x;
        else pick = (a[x] < a[z]) ? x : (a[m] < a[z]) ? z : m;
        nth_swap(a, first, pick);
        int lo = first + 1, hi = last;
        for (;;) {
            while (a[lo] < a[first]) lo++;
            hi--;
            while (a[first] < a[hi]) hi--;
            if (!(lo < hi)) break;
            nth_swap(a, lo, hi);
            lo++;
        }
        if (lo <= k) first = lo;
        else last = lo;
    }
    // __insertion_sort(first, last)
    for (int i = first + 1; i < last; i++) {
        const double v = a[i];
        if (v < a[first]) {
            for (int j = i; j > first; j--) a[j] = a[j - 1];
            a[first] = v;
        } else {
            int hole = i;
            while (v < a[hole - 1]) {
                a[hole] = a[hole - 1];
                hole--;
            }
            a[hole] = v;
        }
    }
}

// ---------------------------------------------------------------- MC step
// One MonteCarlo::apply iteration (sampling.cc:55-99) on one stream: the fold
// launches of the walkers whose sequence changed (launch_window) between two
// runs of step_tail_kernel, one wave per walker: the Metropolis decision of
// the step before (accept_walker) and the next proposal (propose_walker:
// thermostat, RNG streams, mutation move, unchanged check) with its fold's
// weight class (fold_class, for order_kernel).  The MC state stays out of the
// fold kernels' register allocation.

// What a tail reads that nothing in it writes, loaded in one batch at its top
// (the decision's and the proposal's chains then wait on LDS and on the
// move tables only)
struct TailIn {
    int err = 0, changed = 0, ovf = 0, tabv = 0;
    double ps = 0.0, cs = 0.0, temp = 1.0, u = 0.0;
    int ia = 624, ic = 624;   // MT stream indices
    int ntrain = 0;
    double auto_T = 0.0, last_diff = 0.0;
};

struct Accepted {
    bool ran = false;       // a decision was taken (no move error)
    bool changed = false;   // the proposal was scored: last_diff = diff
    bool took = false;      // accepted: the proposal is the current sequence
    double diff = 0.0;
    int tab_valid = -1;     // >= 0: the walker's new tab_valid
};

// Metropolis (sampling.cc:76-89).  cur_slot / tab_valid (null without stored
// tables): an accepted proposal's tables become current, and complete (every
// kernel writes the whole slot), so a walker whose current tables were invalid
// (imported configuration, MFE fold outside the 16-bit range) refolds
// incrementally again -- unless this very fold left the 16-bit range (ovf,
// MFE: its slot is not exact).  Every lane takes the (uniform) decision, lane 0
// writes the walker's state; the accepted sequence is copied by the tail.
// kc (comb set): the step's fold launches left the proposal's score as
// per-variant energies (KArgs::defer_comb): combined here (combine_wave) and
// stored, but for an MFE fold the FP32 fallback redid (ovf; it stored the score).
__device__ Accepted accept_walker(const StepArgs &st, const KArgs &kc, bool comb, double *tv, int w, int lane, int s,
                                  int nt_tot, const TailIn &in) {
    Accepted a;
    if (in.err) return a;
    a.ran = true;
    const bool changed = in.changed == 1;
    int outcome = 2;  // ACCEPT_UNCHANGED
    double prop = in.ps;
    if (changed && comb && !in.ovf) {
        prop = combine_wave(kc, w, lane, tv ? tv + size_t(w) * nt_tot : nullptr);
        if (lane == 0) st.prop_score[w] = prop;
    }
    double diff = 0.0;
    if (changed) {
        diff = prop - in.cs;
        const double crit = exp(diff / in.temp);
        outcome = (crit < in.u) ? 0 : (diff > 0) ? 3 : 1;
    }
    a.changed = changed;
    a.diff = diff;
    const bool acc = outcome == 1 || outcome == 3;
    a.took = acc;
    if (acc && st.cur_slot) a.tab_valid = in.ovf ? 0 : 1;
    if (lane == 0) {
        if (changed) st.last_diff[w] = diff;
        if (acc) {
            st.cur_score[w] = prop;
            if (st.cur_slot) {
                st.cur_slot[w] ^= 1;   // the proposal's tables become current
                st.tab_valid[w] = uint8_t(a.tab_valid);
            }
        }
        st.counters[size_t(w) * 4 + outcome] += 1;
        if (st.tr_pos) {
            const size_t r = size_t(s) * st.W + w;
            st.tr_outcome[r] = outcome;
            if (st.tr_prop) st.tr_prop[r] = changed ? prop : __builtin_nan("");
            st.tr_cur[r] = acc ? prop : in.cs;
            if (st.tr_u) st.tr_u[r] = changed ? in.u : __builtin_nan("");
            if (!changed && st.tr_terms)
                for (int k = 0; k < nt_tot; k++) st.tr_terms[r * nt_tot + k] = __builtin_nan("");
        }
    }
    return a;
}

struct Proposed {
    bool scored = false;    // the fold launch scores this walker
    int plo = -1, phi = -1;
};

// The proposal of step `step` (trace row s).  seq: the walker's current
// sequence, staged in LDS by the tail (the proposal of the step before when
// acc took it); acc's score difference is the auto thermostat's training
// value.  a, c: the streams, their next words staged by the tail (MtView).
__device__ Proposed propose_walker(const StepArgs &st, long long step, int s, int w, int lane, const Accepted &acc,
                                   const TailIn &in, const uint8_t *seq, MtView &a, MtView &c) {
    Proposed out;
    if (in.err) {
        if (lane == 0) st.changed[w] = 0;
        return out;
    }
    uint8_t *prop = st.prop_seq + size_t(w) * st.Nraw;
    uint32_t *gA = st.mtA + size_t(w) * MT_WORDS;
    uint32_t *gC = st.mtC + size_t(w) * MT_WORDS;
    // ---- thermostat (sampling.cc:59; 309-401)
    double T;
    if (st.thermo_kind == 0) {
        T = st.t_fixed;
    } else if (st.thermo_kind == 1) {
        const int Nc = st.cycle_len;
        T = ((st.t_lo - st.t_hi) / Nc) * double(int(step % Nc)) + st.t_hi;
    } else {
        double *tr = st.train + size_t(w) * st.period;
        const int n = in.ntrain + 1;
        T = in.auto_T;
        double Tn = T;
        if (lane == 0) {
            tr[n - 1] = acc.changed ? acc.diff : in.last_diff;
            if (n >= st.period) {
                // median = std::nth_element at n/2, clamp = std::max(t, 0.0)
                // (sampling.cc:389-396): the libstdc++ selection, so -0.0 / NaN
                // land exactly where the reference's do
                const int k = n / 2;
                nth_element_libstdcxx(tr, k, n);
                const double t = tr[k] / st.ln_target_rate;
                Tn = (t < 0.0) ? 0.0 : t;
                st.auto_T[w] = Tn;
                st.ntrain[w] = 0;
            } else {
                st.ntrain[w] = n;
            }
        }
        T = __shfl(Tn, 0, WAVE);
    }
    // ---- move: stream A (and C if the step will be scored)
    const int pick = int(mt_uniform(a, uint32_t(st.M), lane));
    const int bcode = int(mt_uniform(a, 4u, lane)) + 1;  // "ACGU"[r]
    const int e = st.clo_err[pick];
    const int k0 = st.clo_off[pick], k1 = st.clo_off[pick + 1];
    bool changed = false;
    int plo = 1 << 30, phi = -1;   // hull of the positions whose base changes (incremental folds)
    if (e == 0) {
        for (int k = k0 + lane; k < k1; k += WAVE) {
            const int pos = st.clo_pos[k];
            const int nb = st.clo_par[k] ? 5 - bcode : bcode;
            if (seq[pos] != nb) {
                changed = true;
                plo = min(plo, pos);
                phi = max(phi, pos);
            }
        }
        changed = __ballot(changed) != 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            plo = min(plo, __shfl_xor(plo, o, WAVE));
            phi = max(phi, __shfl_xor(phi, o, WAVE));
        }
    }
    // The end cells read a wrapped dangle: cells (i, N) the base S[N + 1] = S[1],
    // cells (1, j) the base S[0] = S[N].  No fold uses their qm1 values, so the band
    // of a refold (fold_common.hpp Band) leaves them out; the outside pass on the
    // stored tables reads them and divides by the proposal's mismatch factor, and so
    // do the exterior sums of the kernels that recompute every cell's code but restore
    // qbm outside the band (mfe_cells.hip, fold_rows.hip: the restored value carries
    // the old code's mismatch).  A proposal that changes an end base folds from scratch
    if (changed && (plo == 0 || phi == st.Nraw - 1)) plo = phi = -1;
    double u = 0.0;
    if (e == 0 && changed) u = mt_canonical(c, lane);
    if (a.twisted)
        for (int k = lane; k < 624; k += WAVE) gA[k] = a.mt[k];
    if (c.twisted)
        for (int k = lane; k < 624; k += WAVE) gC[k] = c.mt[k];
    if (changed) {
        // the proposal: the staged sequence with the move's positions replaced
        for (int k = lane; k < st.Nraw; k += WAVE) {
            uint8_t b = seq[k];
            for (int q = k0; q < k1; q++)
                if (st.clo_pos[q] == k) b = uint8_t(st.clo_par[q] ? 5 - bcode : bcode);
            prop[k] = b;
        }
    }
    if (lane == 0) {
        gA[624] = uint32_t(a.idx);
        gC[624] = uint32_t(c.idx);
        st.pick[w] = pick;
        st.bcode[w] = bcode;
        st.temp[w] = T;
        st.u[w] = u;
        st.changed[w] = (e != 0) ? 0 : (changed ? 1 : 0);
        if (st.chg) {
            st.chg[2 * w] = changed ? plo : -1;
            st.chg[2 * w + 1] = changed ? phi : -1;
        }
        if (e != 0) st.err[w] = e;
        if (st.tr_pos) {
            const size_t r = size_t(s) * st.W + w;
            st.tr_pos[r] = st.mut[pick];
            st.tr_base[r] = int8_t(bcode);
            if (st.tr_temp) st.tr_temp[r] = T;
        }
    }
    out.scored = e == 0 && changed;
    out.plo = changed ? plo : -1;
    out.phi = changed ? phi : -1;
    return out;
}

// The weight class of a proposal's fold for the launch order (order_kernel):
// 0 = heaviest .. 63 by the band of cells containing a changed position, about
// (m_hi + 2) (N - m_lo + 1), a fold from scratch (no valid stored tables)
// counting as the whole triangle; 64 = not scored.
__device__ __forceinline__ int fold_class(const StepArgs &st, const Proposed &p, int tabv) {
    if (!p.scored) return 64;
    const long long full = (long long)st.Nraw * st.Nraw;
    long long key = full;
    if (tabv && st.chg && p.plo >= 0) key = (long long)(p.phi + 2) * (st.Nraw - p.plo + 1);
    return 63 - int(min(full, max(0LL, key)) * 63 / (full > 0 ? full : 1));
}

// One wave per walker: the decision of step s_acc (< 0: none, the first
// proposal of a launch; comb, tv: accept_walker) and the proposal of global
// step `step` (< 0: none, the last step of a launch; trace row s_prop).
// Across a launch_steps call the two halves of a step meet only through HBM
// written by the launches between.  The walker's scalars, its current and
// proposed sequences and its MT streams' next words are loaded in one batch
// first; the sequence the proposal starts from is staged in LDS.
constexpr int TAIL_NMAX = 256;   // sequences staged whole
static_assert(NMAX < TAIL_NMAX, "the C ABI limits sequences to NMAX: the step tail stages them whole");
constexpr int TAIL_WPB = 4;      // walkers (waves) per workgroup
__global__ void __launch_bounds__(TAIL_WPB * 64) step_tail_kernel(StepArgs st, KArgs kc, int comb, double *tv,
                                                                  int s_acc, long long step, int s_prop, int nt_tot) {
    __shared__ uint32_t mts[TAIL_WPB][2 * MT_WORDS];
    __shared__ uint8_t seqs[TAIL_WPB][TAIL_NMAX];
    const int wv = int(threadIdx.x) >> 6;
    const int w = int(blockIdx.x) * TAIL_WPB + wv;
    const int lane = int(threadIdx.x) & (WAVE - 1);
    if (w >= st.W) return;   // no workgroup barrier below: each wave owns its walker and LDS
    uint32_t *mt = mts[wv];
    uint8_t *seq = seqs[wv];
    const int Nr = st.Nraw;
    uint32_t *gA = st.mtA + size_t(w) * MT_WORDS;
    uint32_t *gC = st.mtC + size_t(w) * MT_WORDS;
    const uint8_t *curg = st.cur_seq + size_t(w) * Nr, *propg = st.prop_seq + size_t(w) * Nr;
    TailIn in;
    in.err = st.err[w];
    in.changed = st.changed[w];
    in.ps = st.prop_score[w];
    in.cs = st.cur_score[w];
    in.temp = st.temp[w];
    in.u = st.u[w];
    in.ovf = st.ovf ? st.ovf[w] : 0;
    in.tabv = st.tab_valid ? st.tab_valid[w] : 0;
    in.ia = int(gA[624]);
    in.ic = int(gC[624]);
    if (st.thermo_kind == 2) {
        in.ntrain = st.ntrain[w];
        in.auto_T = st.auto_T[w];
        in.last_diff = st.last_diff[w];
    }
    constexpr int SP = TAIL_NMAX / WAVE;   // bytes a lane holds, packed (position q * 64 + lane in byte q)
    uint32_t cb = 0, pb = 0;
#pragma unroll
    for (int q = 0; q < SP; q++) {
        const int k = q * WAVE + lane;
        cb |= uint32_t(k < Nr ? curg[k] : 0) << (8 * q);
        pb |= uint32_t((k < Nr && s_acc >= 0) ? propg[k] : 0) << (8 * q);
    }
    // the streams' next 8 words (a step draws 2 + 2 but for a rejection: past
    // the window MtView reads HBM, at a twist it stages the whole state)
    if (step >= 0) {
        if (lane < 8) {
            if (in.ia + lane < 624) mt[in.ia + lane] = gA[in.ia + lane];
        } else if (lane < 16) {
            if (in.ic + lane - 8 < 624) mt[MT_WORDS + in.ic + lane - 8] = gC[in.ic + lane - 8];
        }
    }
    Accepted acc;
    if (s_acc >= 0) {
        acc = accept_walker(st, kc, comb != 0, tv, w, lane, s_acc, nt_tot, in);
        if (acc.took) {   // the proposal becomes the current sequence
            uint8_t *c = st.cur_seq + size_t(w) * Nr;
#pragma unroll
            for (int q = 0; q < SP; q++) {
                const int k = q * WAVE + lane;
                if (k < Nr) c[k] = uint8_t(pb >> (8 * q));
            }
        }
    }
    if (step < 0) return;
#pragma unroll
    for (int q = 0; q < SP; q++) {
        const int k = q * WAVE + lane;
        if (k < Nr) seq[k] = uint8_t((acc.took ? pb : cb) >> (8 * q));
    }
    wave_sync();
    MtView a{mt, gA, in.ia, in.ia, min(in.ia + 8, 624), false};
    MtView c{mt + MT_WORDS, gC, in.ic, in.ic, min(in.ic + 8, 624), false};
    const Proposed p = propose_walker(st, step, s_prop, w, lane, acc, in, seq, a, c);
    if (lane == 0) {
        if (st.ovf) st.ovf[w] = 0;   // set again by this proposal's fold if it leaves the 16-bit range
        if (st.cls) st.cls[w] = uint8_t(fold_class(st, p, acc.tab_valid >= 0 ? acc.tab_valid : in.tabv));
    }
}

}  // namespace

// Launch order of an MC step's folds: the walkers whose proposal is scored,
// heaviest refold first, then the unscored ones (their blocks exit at once) --
// a counting sort of the weight classes the proposals computed (fold_class;
// a rescore's are all 0).  The folds' durations vary by several times and the
// GPU starts workgroups in launch order, so heavy folds no longer trail the
// launch.  One workgroup, LDS counters, the class bases by one wave's scan;
// the order within a class does not matter (each walker's fold is independent
// of where it runs).
// pairq (KArgs::pairq, may be null): the scored walkers' count bounds mfe_pair_kernel's
// work queue, whose counter starts at zero -- this kernel runs before the folds
// in the same stream.
__global__ void __launch_bounds__(1024) order_kernel(int W, const uint8_t *cls, int *order, int *pairq) {
    __shared__ int hist[65];
    const int tid = threadIdx.x;
    if (tid < 65) hist[tid] = 0;
    __syncthreads();
#pragma unroll 4
    for (int w = tid; w < W; w += 1024) atomicAdd(&hist[cls[w]], 1);
    __syncthreads();
    if (tid < WAVE) {   // exclusive scan of classes 0..63; the unscored (64) after them
        const int h = hist[tid];
        int incl = h;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int t = __shfl_up(incl, o, WAVE);
            if (tid >= o) incl += t;
        }
        hist[tid] = incl - h;
        if (tid == WAVE - 1) {
            hist[64] = incl;
            if (pairq) {
                pairq[0] = 0;
                pairq[1] = incl;
            }
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int w = tid; w < W; w += 1024) order[atomicAdd(&hist[cls[w]], 1)] = w;
}

// The score window of one MC step for the walkers flagged in `changed`: the
// proposals' folds (prop_seq; incremental against the stored tables where
// tab_valid allows), the outside pass when terms read base-pair probabilities,
// the scores (prop_score) and term values (tv, optional).  evs (optional, 4):
// window start, outside pass start, outside pass end, window end.
static hipError_t launch_window(const KArgs &ka, const StepArgs &st, const int *changed, double *tv,
                                hipStream_t stream, hipEvent_t *evs) {
    if (evs) (void)hipEventRecord(evs[0], stream);
    if (ka.order) hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, stream, st.W, ka.ocls, ka.order,
                                     ka.pairq);
    hipError_t e;
    if (ka.n_pairs > 0 && ka.mode == 0 && ka.tab && ka.gstep) {
        // inside folds first (they write the proposal's tables), then the outside
        // pass on those tables, then the scores with the pair probabilities
        KArgs ki = ka;
        ki.pair_p = nullptr;
        e = launch_score_m(ki, st.prop_seq, st.W, st.prop_score, nullptr, ka.gstep, changed, stream);
        if (e != hipSuccess) return e;
        if (evs) (void)hipEventRecord(evs[1], stream);
        e = launch_outside_m(ka, st.prop_seq, st.W, changed, stream);
        if (e != hipSuccess) return e;
        if (evs) (void)hipEventRecord(evs[2], stream);
        if (!ka.defer_comb) e = launch_combine(ka, st.W, changed, st.prop_score, tv, stream);
    } else {
        // events 1 / 2 bracket the outside pass (here before the folds; none: empty)
        if (evs) (void)hipEventRecord(evs[1], stream);
        if (ka.n_pairs > 0) {   // base-pair probabilities the score terms read (outside pass)
            e = launch_bppm(ka, st.prop_seq, st.W, changed, nullptr, 0, const_cast<double *>(ka.pair_p),
                            ka.bppm_scratch, stream);
            if (e != hipSuccess) return e;
        }
        if (evs) (void)hipEventRecord(evs[2], stream);
        e = launch_score_m(ka, st.prop_seq, st.W, st.prop_score, tv, nullptr, changed, stream);
    }
    if (evs) (void)hipEventRecord(evs[3], stream);
    return e;
}

// evs (optional): 4 * nsteps events per step: window start, outside pass
// start, outside pass end, window end (score written); the inside share of a
// window is the window minus its outside pass (api_ctx.cpp).  Launches:
// step_tail_kernel (the first proposals), then per step the score window and
// step_tail_kernel (its decisions and the next step's proposals).
hipError_t launch_steps(const KArgs &ka, const StepArgs &st0, hipStream_t stream, hipEvent_t *evs) {
    const int nt_tot = ka.n_terms * ka.n_ctx_eff;
    if (st0.nsteps <= 0) return hipSuccess;   // (the first tail would draw a proposal)
    StepArgs st = st0;
    st.cur_slot = ka.tab ? ka.cur_slot : nullptr;
    st.tab_valid = ka.tab ? ka.tab_valid : nullptr;
    st.ovf = ka.mode == 1 ? ka.ovf : nullptr;
    st.cls = ka.order ? const_cast<uint8_t *>(ka.ocls) : nullptr;   // ordering off: ADX_NO_ORDER / no stored tables
    const dim3 tg((st.W + TAIL_WPB - 1) / TAIL_WPB), tb(TAIL_WPB * 64);
    hipLaunchKernelGGL(step_tail_kernel, tg, tb, 0, stream, st, ka, 0, (double *)nullptr, -1, st.step0, 0, nt_tot);
    KArgs kas = ka;
    kas.defer_comb = 1;   // the tails combine the scores the windows leave as energies
    const int comb = window_defers(kas) ? 1 : 0;
    for (int s = 0; s < st.nsteps; s++) {
        double *tv = st.tr_terms ? st.tr_terms + size_t(s) * st.W * nt_tot : nullptr;
        hipError_t e = launch_window(kas, st, st.changed, tv, stream, evs ? evs + 4 * s : nullptr);
        if (e != hipSuccess) return e;
        const bool more = s + 1 < st.nsteps;
        hipLaunchKernelGGL(step_tail_kernel, tg, tb, 0, stream, st, kas, comb, tv, s, more ? st.step0 + s + 1 : -1LL,
                           s + 1, nt_tot);
    }
    return hipGetLastError();
}

__global__ void rescore_begin_kernel(int W, int *changed, uint8_t *tab_valid, uint8_t *cls, int *ovf) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    changed[w] = 1;
    if (tab_valid) tab_valid[w] = 0;
    if (cls) cls[w] = 0;   // folds from scratch: one weight class
    if (ovf) ovf[w] = 0;
}

__global__ void rescore_end_kernel(int W, uint8_t *cur_slot, uint8_t *tab_valid, const int *ovf) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    // the fresh tables of the (unchanged) current sequence are in the other slot;
    // an MFE fold that left the 16-bit range (re-folded in FP32) wrote none
    cur_slot[w] = uint8_t(1 - cur_slot[w]);
    tab_valid[w] = (ovf && ovf[w]) ? 0 : 1;
}

// Every walker's current configuration folded and scored FROM SCRATCH with the
// MC step's own kernels (launch_window: the same inside, outside and combine
// launches, tables written to the walker's other slot and then adopted): the
// walkers' first scores (adx_walkers_init) and adx_walkers_rescore, so stored
// scores, incremental refolds and a fresh fold agree bit for bit.  Scores land
// in st.prop_score (tv: term values, optional); no move, no Metropolis.
hipError_t launch_rescore(const KArgs &ka, const StepArgs &st, double *tv, hipStream_t stream) {
    hipError_t e = hipMemcpyAsync(st.prop_seq, st.cur_seq, size_t(st.W) * st.Nraw, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return e;
    const dim3 g((st.W + 255) / 256), b(256);
    hipLaunchKernelGGL(rescore_begin_kernel, g, b, 0, stream, st.W, st.changed, ka.tab ? ka.tab_valid : nullptr,
                       ka.order ? const_cast<uint8_t *>(ka.ocls) : nullptr, ka.mode == 1 ? ka.ovf : nullptr);
    e = launch_window(ka, st, st.changed, tv, stream, nullptr);
    if (e != hipSuccess) return e;
    if (ka.tab)
        hipLaunchKernelGGL(rescore_end_kernel, g, b, 0, stream, st.W, ka.cur_slot, ka.tab_valid,
                           ka.mode == 1 ? ka.ovf : nullptr);
    return hipGetLastError();
}

}  // namespace adx
