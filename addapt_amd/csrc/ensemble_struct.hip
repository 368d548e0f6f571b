// gfx950 centroid and maximum-expected-accuracy (MEA) structures from pair
// probabilities (RNAfold -p --MEA): an off-step utility (the C ABI's
// adx_*ensemble_structures*), not the Monte Carlo score.  ensemble_struct_kernel
// reads the matrices launch_bppm left on the device, one workgroup of 256
// threads per sequence, and returns two strings and three doubles for each.
// The definitions are stated in ensemble_struct_core.hpp, which holds the
// per-lane work; this file is the barriers around it.
//
//   columns    thread c reads column c of the symmetric matrix top to bottom
//              (row c in ascending j, coalesced across the threads): pu[c], row
//              c of w = 2 gamma P and of the "P > 1/2" bitmap.
//   centroid   one lane takes the bitmap's pairs in ascending (i, j) through the
//              conflict filter; then thread c sums column c's share of the
//              distance and of the diversity, and one lane each adds the L
//              shares in ascending order.  No floating-point atomics: the
//              results do not depend on timing.
//   fill       lanes are the cells of one anti-diagonal, one barrier per
//              diagonal; a lane walks its cell's k serially (the two end
//              candidates peeled, so the loop's loads wait for no branch).  M and w are
//              triangular, diagonal-major, in the workgroup's HBM scratch slice
//              (261 KB each at NMAX: they do not fit LDS); pu, the interval
//              stack and the output strings are in LDS.
//   traceback  lane 0 owns the interval stack; an interval's candidates are
//              spread over the lanes and the smallest matching index (LDS
//              atomicMin) wins, as in mfe_trace_kernel.  At most 2 L pops.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"

#define ES_FN __device__
#include "ensemble_struct_core.hpp"

namespace adx {
namespace {

static_assert(ES_LMAX == NMAX, "the core header's length bound is the engine's");
static_assert(sizeof(EnsLds) <= 48 * 1024 && sizeof(EnsLds) <= size_t(LDS_LIMIT), "static LDS of ensemble_struct_kernel");

__global__ void __launch_bounds__(ES_NT)
ensemble_struct_kernel(const double *__restrict__ probs, int L, double g2, double *scratch, size_t slice,
                       char *centroid, char *mea, double *stats) {
    __shared__ EnsLds S;
    const int tid = threadIdx.x;
    const size_t w = blockIdx.x;
    double *tab = scratch + w * slice;
    const Ens E{S, probs + w * size_t(L) * L, tab, tab + es_cells(L), L};

    if (tid == 0) {
        S.top = 0;
        S.pops = 0;
        S.bad = 0;
    }
    __syncthreads();
    if (tid < L) E.column(tid, g2);
    __syncthreads();
    if (tid == 0) E.centroid_scan();
    __syncthreads();
    if (tid < L) E.column_stats(tid);
    // the stats' shares are read after the fill's first barrier

    // ---- fill: one anti-diagonal per barrier
    for (int d = 0; d < L; d++) {
        if (tid < L - d) E.fill_cell(tid, tid + d);
        __syncthreads();
    }
    const bool bad = S.bad != 0;
    if ((tid == 0 || tid == WAVE) && stats) {   // one lane of two waves: the columns' shares, ascending
        const double s = es_sum(S.part[tid / WAVE], L);
        stats[3 * w + 1 + tid / WAVE] = bad ? NAN : (tid == 0 ? s : 2.0 * s);
    }

    // ---- traceback: lane 0's work sits between the two barriers of an interval
    // and the loop's exit test is wave-uniform (see mfe_trace_kernel)
    if (tid == 0) {
        E.push(0, L - 1);
        E.next_item();
    }
    __syncthreads();
    for (;;) {
        const int i = uni(S.cur[0]), j = uni(S.cur[1]);
        if (i < 0) break;
        const int cand = E.candidate(i, j, tid, ES_NT);
        if (cand != ES_NONE) atomicMin(&S.win, cand);
        __syncthreads();
        if (tid == 0) {
            E.resolve(i, j, S.win);
            E.next_item();
        }
        __syncthreads();
    }
    if (tid < L) {
        if (mea) mea[w * L + tid] = S.out[tid];
        if (centroid) {
            const int p = S.pt[tid];
            centroid[w * L + tid] = p < 0 ? '.' : (p > tid ? '(' : ')');
        }
    }
    if (tid == 0 && stats) stats[3 * w] = bad ? NAN : E.m(0, L - 1);
}

}  // namespace

size_t ensemble_struct_slice_doubles(int L) { return 2 * es_cells(std::max(L, 1)); }

int ensemble_struct_chunk(int L, int W) {
    constexpr size_t cap = size_t(256) << 20;   // probability matrices + scratch slices of one launch (bytes)
    const size_t len = size_t(std::max(L, 1));
    const size_t each = (len * len + ensemble_struct_slice_doubles(L)) * sizeof(double);
    return int(std::max<size_t>(1, std::min<size_t>(size_t(std::max(W, 1)), cap / each)));
}

hipError_t launch_ensemble_struct(const double *probs, int L, int n, double gamma, double *scratch, char *centroid,
                                  char *mea, double *stats, hipStream_t stream) {
    if (!probs || !scratch || L < 1 || L > NMAX || n < 1 || !(gamma > 0.0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ensemble_struct_kernel, dim3(n), dim3(ES_NT), 0, stream, probs, L, 2.0 * gamma, scratch,
                       ensemble_struct_slice_doubles(L), centroid, mea, stats);
    return hipGetLastError();
}

}  // namespace adx
