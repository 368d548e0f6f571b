// gfx950 Zuker suboptimal structures: mfe_subopt_kernel fills the MFE inside
// tables of one (sequence, variant) per workgroup exactly as mfe_trace_kernel
// does, runs the MFE OUTSIDE pass over them, and lists the structures within
// delta of the minimum by Zuker's rule.  An off-step utility (the C ABI's
// adx_*subopt_structures*), in plain 32-bit dcal like mfe_trace.hip.
//
//   phase 0    inside fill, f5, f3, the outside fill on descending diagonals (one
//   (fill)     barrier per diagonal) and th(i,j), the energy of the best structure
//              through each pair: seven triangles plus f5 / f3 in the workgroup's
//              HBM scratch slice.  Writes the MFE, the number of pairs within
//              delta and, on request, th as an L x L matrix in kcal/mol.
//   phase 1    repeatedly the first unmarked pair by (th, i, j) within delta (a
//   (select)   block-wide min of one 64-bit key per lane, not a sort), the
//              traceback of its structure through inside and outside items, and
//              the marking of every pair of that structure (its th becomes
//              "impossible": the matrix was written in phase 0).
// The two phases are two launches of the one kernel, so each has a device time.
// The per-lane work is in mfe_outside_core.hpp; this file is the barriers around it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"

#define TR_FN __device__
#include "mfe_outside_core.hpp"

namespace adx {
namespace {

constexpr int SO_NT = 256;       // threads per workgroup
constexpr int SO_TRIANGLES = 7;  // c, fm, fm1, co, fm1o, fmo, th

struct SuboptLds {
    TraceLds t;
    int f3[TR_NP];
    unsigned long long best;
    int count;
};
static_assert(sizeof(SuboptLds) <= 48 * 1024 && sizeof(SuboptLds) <= size_t(LDS_LIMIT), "static LDS of mfe_subopt_kernel");

__device__ __forceinline__ int unpaired_from(const TraceLds &L, const int *f, int k, int prev) {
    return (k >= 1 && k < TR_NP && L.up[k] >= 1 && f[prev] < TR_INF) ? f[prev] : TR_INF;
}

// one lane: pop the next item into L.cur (kind -1: the stack is empty) and reset the reduction
__device__ __forceinline__ void next_item(TraceLds &L) {
    if (L.top == 0) {
        L.cur[0] = -1;
    } else {
        const int *s = L.stk + 3 * --L.top;
        L.cur[0] = s[0];
        L.cur[1] = s[1];
        L.cur[2] = s[2];
    }
    L.win = TR_NONE;
}

__device__ __forceinline__ float kcal(int dcal) { return static_cast<float>(static_cast<double>(dcal) / 100.0); }

__global__ void __launch_bounds__(SO_NT)
mfe_subopt_kernel(KArgs ka, int variant, const uint8_t *__restrict__ seqs, int w0, int *scratch, int phase,
                  int delta_dcal, int max_structs, SuboptOut out) {
    __shared__ SuboptLds SL;
    TraceLds &L = SL.t;
    const int tid = threadIdx.x;
    const int w = w0 + blockIdx.x;
    const DevVariant V = ka.variants[variant];
    const int N = V.N, np = N + 2;
    const size_t cells = size_t(ka.cells);
    int *slice = scratch + size_t(blockIdx.x) * (SO_TRIANGLES * cells + 2 * TR_NP);
    int *sf5 = slice + SO_TRIANGLES * cells, *sf3 = sf5 + TR_NP;
    const DevScaled *X = ka.X;
    const Trace M{ka.T, X, L, slice, slice + cells, slice + 2 * cells, N,
                  ei(X->mlclosing), ei(X->mlbase_sig), ei(X->motif_extra), X->motif_len, V.motif != 0};
    const Outside O{M, slice + 3 * cells, slice + 4 * cells, slice + 5 * cells, slice + 6 * cells, SL.f3};

    for (int k = tid; k < np; k += SO_NT) L.out[k] = '.';
    seq_setup<SO_NT>(L, ka, V, seqs + size_t(w) * ka.Nraw, tid,
                     [](bool on, float v) { return on ? ei(v) : TR_INF; });

    if (phase == 0) {
        if (tid == 0) {
            L.f5[0] = 0;
            SL.f3[N + 1] = 0;
            SL.count = 0;
            L.red = unpaired_from(L, L.f5, 1, 0);
        }
        __syncthreads();
        // ---- inside fill, as mfe_trace_kernel: one anti-diagonal per barrier, then f5
        for (int d = 4; d <= N - 1; d++) {
            for (int r = tid; r < N - d; r += SO_NT) M.fill_cell(r + 1, r + 1 + d);
            __syncthreads();
        }
        for (int j = 1; j <= N; j++) {   // L.red holds the "j unpaired" form
            const int v = M.f5_pairs(j, tid, SO_NT);
            if (v < TR_INF) atomicMin(&L.red, v);
            __syncthreads();
            if (tid == 0) {
                L.f5[j] = L.red;
                L.red = j < N ? unpaired_from(L, L.f5, j + 1, j) : unpaired_from(L, SL.f3, N, N + 1);
            }
            __syncthreads();
        }
        for (int i = N; i >= 1; i--) {   // f3, right to left: L.red holds the "i unpaired" form
            const int v = O.f3_pairs(i, tid, SO_NT);
            if (v < TR_INF) atomicMin(&L.red, v);
            __syncthreads();
            if (tid == 0) {
                SL.f3[i] = L.red;
                L.red = unpaired_from(L, SL.f3, i - 1, i);
            }
            __syncthreads();
        }
        // ---- outside fill on descending diagonals, then th
        for (int d = N - 1; d >= 4; d--) {
            for (int r = tid; r < N - d; r += SO_NT) O.outside_cell(r + 1, r + 1 + d);
            __syncthreads();
        }
        for (int d = 4; d <= N - 1; d++)
            for (int r = tid; r < N - d; r += SO_NT) O.through_cell(r + 1, r + 1 + d);
        for (int k = tid; k <= N + 1; k += SO_NT) {
            sf5[k] = k <= N ? L.f5[k] : 0;
            sf3[k] = k >= 1 ? SL.f3[k] : 0;
        }
        if (out.pair_energy)
            for (int k = tid; k < N * N; k += SO_NT) out.pair_energy[size_t(w) * N * N + k] = INFINITY;
        __syncthreads();
        const int total = L.f5[N];
        const bool feasible = total < int(0.5f * MFE_BIG);   // as the score kernels read their f5[N]
        const int n = feasible ? O.count_within(total + delta_dcal, tid, SO_NT) : 0;
        if (n) atomicAdd(&SL.count, n);
        if (out.pair_energy)
            for (int d = 4; d <= N - 1; d++)
                for (int r = tid; r < N - d; r += SO_NT) {
                    const int v = O.th[off(d, N) + r];
                    if (v >= TR_INF) continue;
                    float *pe = out.pair_energy + size_t(w) * N * N;
                    pe[size_t(r) * N + r + d] = pe[size_t(r + d) * N + r] = kcal(v);
                }
        __syncthreads();
        if (tid == 0) {
            out.n_within[w] = SL.count;
            out.mfe[w] = feasible ? kcal(total) : INFINITY;
        }
        return;
    }

    // ---- phase 1: the tables are the slice's; f5 and f3 come back to LDS
    for (int k = tid; k <= N + 1; k += SO_NT) {
        L.f5[k] = sf5[k];
        SL.f3[k] = sf3[k];
    }
    for (int k = tid; k < max_structs; k += SO_NT) {
        out.energies[size_t(w) * max_structs + k] = INFINITY;
        out.seeds[(size_t(w) * max_structs + k) * 2] = out.seeds[(size_t(w) * max_structs + k) * 2 + 1] = 0;
    }
    for (size_t k = tid; k < size_t(max_structs) * N; k += SO_NT) out.structures[size_t(w) * max_structs * N + k] = '.';
    if (tid == 0) {
        L.top = 0;
        SL.best = SO_NOKEY;
    }
    __syncthreads();
    const int total = L.f5[N];
    const bool feasible = total < int(0.5f * MFE_BIG);
    const int limit = total + delta_dcal;
    int found = 0;
    while (feasible && found < max_structs) {
        const unsigned long long key = O.lane_best(limit, tid, SO_NT);
        if (key != SO_NOKEY) atomicMin(&SL.best, key);
        __syncthreads();
        const unsigned long long best = SL.best;
        if (best == SO_NOKEY) break;   // block-uniform
        const int si = Outside::key_i(best), sj = Outside::key_j(best);
        const int e = O.th[M.idx(si, sj)];
        for (int k = tid; k < np; k += SO_NT) L.out[k] = '.';
        __syncthreads();
        // lane 0 owns the stack; its work sits BETWEEN the two barriers of an item and
        // the loop's exit test is wave-uniform (mfe_trace.hip)
        if (tid == 0) {
            SL.best = SO_NOKEY;
            O.seed_begin(si, sj);
            next_item(L);
        }
        __syncthreads();
        for (;;) {
            const int kind = uni(L.cur[0]), i = uni(L.cur[1]), j = uni(L.cur[2]);
            if (kind < 0) break;
            const int cand = O.candidate(kind, i, j, tid, SO_NT);
            if (cand != TR_NONE) atomicMin(&L.win, cand);
            __syncthreads();
            if (tid == 0) {
                O.resolve(kind, i, j, L.win);
                next_item(L);
            }
            __syncthreads();
        }
        const size_t slot = size_t(w) * max_structs + found;
        for (int k = tid; k < N; k += SO_NT) out.structures[slot * N + k] = L.out[k];
        if (tid == 0) {
            O.mark_structure();
            out.energies[slot] = kcal(e);
            out.seeds[2 * slot] = si;
            out.seeds[2 * slot + 1] = sj;
        }
        found++;
        __syncthreads();
    }
    if (tid == 0) out.n_found[w] = found;
}

}  // namespace

size_t mfe_subopt_slice_ints(const KArgs &ka) { return SO_TRIANGLES * size_t(ka.cells) + 2 * TR_NP; }

int mfe_subopt_chunk(const KArgs &ka, int W) {
    constexpr size_t cap = size_t(256) << 20;   // scratch bound (bytes)
    const size_t fit = cap / (mfe_subopt_slice_ints(ka) * sizeof(int));
    return int(std::max<size_t>(1, std::min<size_t>(size_t(std::max(W, 1)), fit)));
}

hipError_t launch_mfe_subopt(const KArgs &ka, int variant, const uint8_t *seqs, int w0, int n, int *scratch, int phase,
                             int delta_dcal, int max_structs, const SuboptOut &out, hipStream_t stream) {
    if (ka.mode != 1 || variant < 0 || variant >= ka.n_variants || n < 1 || phase < 0 || phase > 1 || delta_dcal < 0 ||
        max_structs < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mfe_subopt_kernel, dim3(n), dim3(SO_NT), 0, stream, ka, variant, seqs, w0, scratch, phase,
                       delta_dcal, max_structs, out);
    return hipGetLastError();
}

}  // namespace adx
