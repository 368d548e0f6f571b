// gfx950 unpaired-region probabilities (RNAplfold -u / RNAup's accessibility):
// P_u(i,j), the probability that i..j is all unpaired in one fold variant's
// ensemble, for every window up to a length and for given regions.  An off-step
// utility (the C ABI's adx_*unpaired_probs*): no walker or fold state is touched.
//
//   pf_access_kernel   one workgroup per (sequence, variant), after pf_fill_kernel
//                      (pf_sample.hip) on the same, longer scratch slice: the FP64
//                      OUTSIDE pass over the fill's qb, qm, qm1 and q5.
//     a5               the exterior adjoint, a suffix recursion (one barrier per
//                      position: the waves' partial sums alternate between two rows)
//     ab, am, am1      on descending diagonals, lanes = the cells of a diagonal,
//                      one barrier per diagonal; every sum is a gather
//     R                lanes = the runs (a, b): the mass of each maximal unpaired
//                      run, then the two prefix passes (lanes = rows, then columns)
//     windows          lanes = the windows of the profile, the regions, the pairs
// Every sum runs in a fixed order and nothing is accumulated atomically: equal
// inputs give equal bytes, whatever the launch chunking.  The tables stay in the
// HBM slice (L2 resident); the per-lane work is in pf_access_core.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"

#define TR_FN __device__
#include "pf_access_core.hpp"

namespace adx {
namespace {

constexpr int PA_NT = 256;              // threads per workgroup
constexpr int PA_WAVES = PA_NT / WAVE;

struct AccessLds {
    PfSeqLds q;
    double q5[PS_NP], a5[PS_NP];
    double pw5[PS_NP], pwm[PS_NP];
    double part[2][PA_WAVES];
};
static_assert(sizeof(AccessLds) <= 48 * 1024, "static LDS of pf_access_kernel");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__global__ void __launch_bounds__(PA_NT)
pf_access_kernel(KArgs ka, int variant, const uint8_t *__restrict__ seqs, int w0, double *scratch, size_t slice,
                 size_t fill_doubles, AccessOut out) {
    __shared__ AccessLds L;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int w = w0 + blockIdx.x;
    const DevVariant V = ka.variants[variant];
    const int N = V.N;
    const size_t cells = size_t(ka.cells);
    double *tab = scratch + size_t(blockIdx.x) * slice;
    double *adj = tab + fill_doubles;
    const DevScaled *X = ka.X;
    seq_setup<PA_NT>(L.q, ka, V, seqs + size_t(w) * ka.Nraw, tid, [](bool on, float v) { return on ? v : 0.f; });
    const PfModel M{ka.T, X, L.q, tab, tab + cells, tab + 2 * cells, L.q5, N, X->motif_len, V.motif != 0};
    const Access A{M, adj, adj + cells, adj + 2 * cells, L.a5, adj + 3 * cells, L.pw5, L.pwm};

    const double *q5 = tab + 3 * cells;
    for (int k = tid; k <= N; k += PA_NT) {
        L.q5[k] = q5[k];
        double a = 1.0, b = 1.0;   // the products the fill forms, one factor per base
        for (int t = 0; t < k; t++) {
            a *= double(X->sig[1]);
            b *= double(X->mlbase_sig);
        }
        L.pw5[k] = a;
        L.pwm[k] = b;
    }
    L.a5[N] = 1.0;   // every thread, the same value
    __syncthreads();
    const double Z = L.q5[N];

    if (N >= 5 && Z > 0.0 && Z < INFINITY) {
        // ---- a5 right to left (one barrier per m, as pf_fill_kernel's q5)
        for (int m = N - 1; m >= 0; m--) {
            const double v = wave_sum(A.a5_pairs(m, tid, PA_NT));
            if (lane == 0) L.part[m & 1][wid] = v;
            __syncthreads();
            double s = A.a5_unpaired(m);
#pragma unroll
            for (int k = 0; k < PA_WAVES; k++) s += L.part[m & 1][k];
            L.a5[m] = s;   // every thread, the same value
        }
        __syncthreads();
        // ---- the adjoint triangles on descending diagonals
        for (int d = N - 1; d >= 4; d--) {
            for (int r = tid; r < N - d; r += PA_NT) A.adjoint_cell(r + 1, r + 1 + d);
            __syncthreads();
        }
        // ---- the run masses and their dominance sums
        for (int t = tid; t < N * N; t += PA_NT) {
            const int a = t / N + 1, b = t % N + 1;
            A.R[t] = a <= b ? A.run_mass(a, b) : 0.0;
        }
        __syncthreads();
        for (int a = tid + 1; a <= N; a += PA_NT) A.sum_row(a);
        __syncthreads();
        for (int b = tid + 1; b <= N; b += PA_NT) A.sum_column(b);
        __syncthreads();
    }

    // ---- the windows
    if (out.profile) {
        double *dst = out.profile + size_t(blockIdx.x) * out.max_len * N;
        for (int t = tid; t < out.max_len * N; t += PA_NT) {
            const int i = t % N + 1, j = i + t / N;
            dst[t] = j <= N ? A.unpaired_prob(i, j, Z) : 0.0;
        }
    }
    if (out.region_probs)
        for (int r = tid; r < out.n_regions; r += PA_NT) {
            const int i = out.regions[2 * r] + 1, j = i + out.regions[2 * r + 1] - 1;
            out.region_probs[size_t(blockIdx.x) * out.n_regions + r] = A.unpaired_prob(i, j, Z);
        }
    if (out.pair_probs) {
        double *dst = out.pair_probs + size_t(blockIdx.x) * N * N;
        for (int t = tid; t < N * N; t += PA_NT) {
            const int x = t / N + 1, y = t % N + 1;
            const bool none = x == y || N < 5;   // and NaN where the constraint admits nothing, as the windows
            dst[t] = !(Z > 0.0 && Z < INFINITY) ? double(NAN) : none ? 0.0 : A.pair_prob(min(x, y), max(x, y), Z);
        }
    }
}

}  // namespace

size_t pf_access_slice_doubles(const KArgs &ka) {
    return pf_sample_slice_doubles(ka) + 3 * size_t(ka.cells) + size_t(ka.Nmax) * size_t(ka.Nmax);
}

int pf_access_chunk(const KArgs &ka, int W, size_t out_doubles) {
    constexpr size_t cap = size_t(256) << 20;   // tables + device-side output of one launch (bytes)
    const size_t fit = cap / ((pf_access_slice_doubles(ka) + out_doubles) * sizeof(double));
    return int(std::max<size_t>(1, std::min<size_t>(size_t(std::max(W, 1)), fit)));
}

hipError_t launch_pf_access(const KArgs &ka, int variant, const uint8_t *seqs, int w0, int n, double *scratch,
                            const AccessOut &out, hipStream_t stream) {
    if (ka.mode != 0 || variant < 0 || variant >= ka.n_variants || n < 1 || out.max_len < 0 || out.n_regions < 0 ||
        (out.profile && out.max_len < 1) || (out.region_probs && (out.n_regions < 1 || !out.regions)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pf_access_kernel, dim3(n), dim3(PA_NT), 0, stream, ka, variant, seqs, w0, scratch,
                       pf_access_slice_doubles(ka), pf_sample_slice_doubles(ka), out);
    return hipGetLastError();
}

}  // namespace adx
