// gfx950 minimum-free-energy fold WITH the structure: mfe_trace_kernel fills
// the Zuker tables of one (sequence, variant) per workgroup and traces the
// optimal structure back on the device.  An off-step utility (the C ABI's
// adx_*mfe_structure*), not the Monte Carlo score: same recursion and energy
// tables as the score's MFE kernels (oracle/fold.c orc_mfe_energy), written
// for clarity, with no 16-bit range and no fallback.
//
//   fill       plain 32-bit integers (dcal/mol; the FP32 MinPlus tables DevTables /
//              DevScaled hold integers).  c, fm, fm1 are triangular and live in an
//              HBM scratch slice of the workgroup (diagonal-major, fold_common.hpp
//              off()); f5 in LDS.  Lanes are the cells of one anti-diagonal, one
//              barrier per diagonal; a lane walks its cell's interior loops,
//              multiloop splits and fm splits serially.
//   traceback  a stack of (kind, i, j) items in LDS as oracle/fold.c orc_mfe keeps
//              it.  An item's candidates are spread over the lanes; every
//              candidate has an index that grows in the oracle's search order, and
//              the smallest matching index (LDS atomicMin) wins, so the structure
//              does not depend on the lane count or on timing.
//
// The per-lane work is in mfe_trace_core.hpp; this file is the barriers around it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"

#define TR_FN __device__
#include "mfe_trace_core.hpp"

namespace adx {
namespace {

constexpr int TR_NT = 256;   // threads per workgroup
static_assert(sizeof(TraceLds) <= 48 * 1024 && sizeof(TraceLds) <= size_t(LDS_LIMIT), "static LDS of mfe_trace_kernel");

// f5(j)'s "j unpaired" form (one lane; f5[j - 1] is final)
__device__ __forceinline__ int f5_unpaired(const TraceLds &L, int j) {
    return (j < TR_NP && L.up[j] >= 1 && L.f5[j - 1] < TR_INF) ? L.f5[j - 1] : TR_INF;
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

__global__ void __launch_bounds__(TR_NT)
mfe_trace_kernel(KArgs ka, int variant, const uint8_t *__restrict__ seqs, int w0, int *scratch,
                 char *structures, float *energies) {
    __shared__ TraceLds L;
    const int tid = threadIdx.x;
    const int w = w0 + blockIdx.x;
    const DevVariant V = ka.variants[variant];
    const int N = V.N, np = N + 2;
    int *slice = scratch + size_t(blockIdx.x) * 3 * size_t(ka.cells);
    const DevScaled *X = ka.X;
    const Trace M{ka.T, X, L, slice, slice + ka.cells, slice + 2 * size_t(ka.cells), N,
                  ei(X->mlclosing), ei(X->mlbase_sig), ei(X->motif_extra), X->motif_len, V.motif != 0};

    // ---- sequence (context-padded), constraint arrays, special hairpins, motif
    // sites (fold_common.hpp seq_setup), then the trace's own start values
    for (int k = tid; k < np; k += TR_NT) L.out[k] = '.';
    seq_setup<TR_NT>(L, ka, V, seqs + size_t(w) * ka.Nraw, tid,
                     [](bool on, float v) { return on ? ei(v) : TR_INF; });
    if (tid == 0) {
        L.f5[0] = 0;
        L.top = 0;
        L.red = f5_unpaired(L, 1);
    }
    __syncthreads();

    // ---- fill: one anti-diagonal per barrier, then f5 left to right
    for (int d = 4; d <= N - 1; d++) {
        for (int r = tid; r < N - d; r += TR_NT) M.fill_cell(r + 1, r + 1 + d);
        __syncthreads();
    }
    for (int j = 1; j <= N; j++) {   // L.red holds the "j unpaired" form
        const int v = M.f5_pairs(j, tid, TR_NT);
        if (v < TR_INF) atomicMin(&L.red, v);
        __syncthreads();
        if (tid == 0) {
            L.f5[j] = L.red;
            L.red = f5_unpaired(L, j + 1);
        }
        __syncthreads();
    }
    const int total = L.f5[N];
    const bool feasible = total < int(0.5f * MFE_BIG);   // as the score kernels read their f5[N]

    // ---- traceback: lane 0 owns the stack.  Its work sits BETWEEN the two barriers
    // of an item and the loop's exit test is wave-uniform: with single-lane blocks
    // on both sides of the back edge the compiler merged them and split the loop
    // in two, leaving the other lanes to run ahead through the barrier.
    if (tid == 0) {
        if (feasible) M.push(TI_F5, 0, N);
        next_item(L);
    }
    __syncthreads();
    for (;;) {
        const int kind = uni(L.cur[0]), i = uni(L.cur[1]), j = uni(L.cur[2]);
        if (kind < 0) break;
        const int cand = M.candidate(kind, i, j, tid, TR_NT);
        if (cand != TR_NONE) atomicMin(&L.win, cand);
        __syncthreads();
        if (tid == 0) {
            M.resolve(kind, i, j, L.win);
            next_item(L);
        }
        __syncthreads();
    }
    for (int k = tid; k < N; k += TR_NT) structures[size_t(w) * N + k] = L.out[k];
    if (tid == 0 && energies)
        energies[w] = feasible ? static_cast<float>(static_cast<double>(total) / 100.0) : INFINITY;
}

}  // namespace

size_t mfe_trace_slice_ints(const KArgs &ka) { return 3 * size_t(ka.cells); }

int mfe_trace_chunk(const KArgs &ka, int W) {
    constexpr size_t cap = size_t(256) << 20;   // scratch bound (bytes)
    const size_t fit = cap / (mfe_trace_slice_ints(ka) * sizeof(int));
    return int(std::max<size_t>(1, std::min<size_t>(size_t(std::max(W, 1)), fit)));
}

hipError_t launch_mfe_trace(const KArgs &ka, int variant, const uint8_t *seqs, int W, int *scratch, int chunk,
                            char *structures, float *energies, hipStream_t stream) {
    if (ka.mode != 1 || variant < 0 || variant >= ka.n_variants || chunk < 1) return hipErrorInvalidValue;
    for (int w0 = 0; w0 < W; w0 += chunk) {
        const int n = std::min(chunk, W - w0);
        hipLaunchKernelGGL(mfe_trace_kernel, dim3(n), dim3(TR_NT), 0, stream, ka, variant, seqs, w0, scratch,
                           structures, energies);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace adx
