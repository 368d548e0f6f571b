// gfx950 structures drawn from the Boltzmann ensemble (vrna_pbacktrack): an
// off-step utility (the C ABI's adx_*sample_structures*), not the Monte Carlo
// score.  Two kernels, so that many workgroups can sample from one sequence's
// tables:
//
//   pf_fill_kernel    one workgroup per (sequence, variant): the inside
//                     recursion of oracle/fold.c with the context's FP32 factors
//                     (DevTables / DevScaled, sigma scale included), multiplied,
//                     summed and stored in FP64 -- no range to leave, so no
//                     fallback.  qb, qm, qm1 (triangular, diagonal-major,
//                     fold_common.hpp off()) and q5 go to the sequence's HBM
//                     scratch slice.  Lanes are the cells of one anti-diagonal,
//                     one barrier per diagonal.
//   pf_sample_kernel  grid (block of samples, sequence), one wave per sample.
//                     The wave keeps a stack of packed (kind, i, j) items in
//                     LDS; an item's candidates are spread over the 64 lanes in
//                     rounds, their weights prefix-summed across lanes and
//                     rounds, and the first candidate whose cumulative weight
//                     exceeds u * total wins (pf_sample_core.hpp pick).  No
//                     workgroup barrier inside the loop: it is wave-synchronous,
//                     every lane holds the same stack pointer and writes the
//                     same values.  Every loop has a static bound; a sample that
//                     reaches one is written as dots and raises *flag.
//
// The per-lane work is in pf_sample_cells.hpp, the RNG and the selection rule
// in pf_sample_core.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"

#define TR_FN __device__
#define PS_FN __device__
#include "pf_sample_cells.hpp"
#include "pf_sample_core.hpp"

namespace adx {
namespace {

constexpr int PS_NT = 256;                  // threads per workgroup, both kernels
constexpr int PS_WAVES = PS_NT / WAVE;      // samples per sampling workgroup
constexpr int PS_STACK = NMAX + 8;          // live items cover disjoint spans of >= 1 base
constexpr int PS_MAXPOPS = 8 * NMAX + 16;   // a sample pops < 4 N items (one per base, pair, branch)

struct FillLds {
    PfSeqLds q;
    double q5[PS_NP];
    double part[2][PS_WAVES];
};
struct SampleLds {
    PfSeqLds q;
    uint32_t stk[PS_WAVES][PS_STACK];
    char out[PS_WAVES][PS_NP + 6];
};
static_assert(sizeof(FillLds) <= 48 * 1024 && sizeof(SampleLds) <= 48 * 1024, "static LDS of the pf_sample kernels");

// The sequence (context-padded), the variant's constraint arrays, the special
// hairpins and the motif sites into LDS, exactly as mfe_trace_kernel gets them
// (fold_common.hpp seq_setup); ends with a barrier.
__device__ void load_sequence(PfSeqLds &L, const KArgs &ka, const DevVariant &V, const uint8_t *raw, int tid) {
    seq_setup<PS_NT>(L, ka, V, raw, tid, [](bool on, float v) { return on ? v : 0.f; });
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__global__ void __launch_bounds__(PS_NT)
pf_fill_kernel(KArgs ka, int variant, const uint8_t *__restrict__ seqs, int w0, double *scratch, size_t slice,
               float *energies) {
    __shared__ FillLds L;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int w = w0 + blockIdx.x;
    const DevVariant V = ka.variants[variant];
    const int N = V.N;
    double *tab = scratch + size_t(blockIdx.x) * slice;
    const DevScaled *X = ka.X;
    load_sequence(L.q, ka, V, seqs + size_t(w) * ka.Nraw, tid);
    const PfModel M{ka.T, X, L.q, tab, tab + ka.cells, tab + 2 * size_t(ka.cells), L.q5, N, X->motif_len, V.motif != 0};

    // ---- one anti-diagonal per barrier, then q5 left to right (one barrier per j:
    // the waves' partial sums alternate between two rows of L.part)
    for (int d = 4; d <= N - 1; d++) {
        for (int r = tid; r < N - d; r += PS_NT) M.fill_cell(r + 1, r + 1 + d);
        __syncthreads();
    }
    L.q5[0] = 1.0;   // every thread, the same value
    double prev = 1.0;
    for (int j = 1; j <= N; j++) {
        const double v = wave_sum(M.q5_pairs(j, tid, PS_NT));
        if (lane == 0) L.part[j & 1][wid] = v;
        __syncthreads();
        double s = L.q.up[j] >= 1 ? prev * double(X->sig[1]) : 0.0;
#pragma unroll
        for (int k = 0; k < PS_WAVES; k++) s += L.part[j & 1][k];
        L.q5[j] = s;   // every thread, the same value
        prev = s;
    }
    __syncthreads();
    double *q5 = tab + 3 * size_t(ka.cells);
    for (int k = tid; k <= N; k += PS_NT) q5[k] = L.q5[k];
    if (tid == 0 && energies) {
        float e;
        if (!(prev > 0.0)) e = prev == 0.0 ? INFINITY : float(prev);   // empty ensemble; a non-finite total as computed
        else if (N < 5) e = 0.f;                                        // nothing can pair: the open chain alone
        else e = float(-X->kT * (log(prev) - N * X->log_sigma));
        energies[w] = e;
    }
}

// Which of the n candidates of item (kind, i, j) wins under the draw u, by
// pf_sample_core.hpp pick's rule; -1: no candidate has weight.  All 64 lanes
// call it with the same arguments and get the same answer.
__device__ int wave_pick(const PfModel &M, int kind, int i, int j, int n, float u, int lane) {
    double total = 0.0;
    for (int r = 0; r < PS_MAXCAND; r += WAVE) {
        if (r >= n) break;
        const double wt = M.weight(kind, i, j, r + lane);
        total += wt > 0.0 ? wt : 0.0;
    }
    total = wave_sum(total);
    const double thr = double(u) * total;
    double carry = 0.0;
    int last = -1;
    for (int r = 0; r < PS_MAXCAND; r += WAVE) {
        if (r >= n) break;
        double wt = M.weight(kind, i, j, r + lane);
        wt = wt > 0.0 ? wt : 0.0;
        double inc = wt;   // inclusive prefix sum over the lanes
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const double o = __shfl_up(inc, d, WAVE);
            if (lane >= d) inc += o;
        }
        const unsigned long long nz = __ballot(wt > 0.0);
        const unsigned long long hit = __ballot(wt > 0.0 && carry + inc > thr);
        if (hit != 0) return r + __builtin_ctzll(hit);
        if (nz != 0) last = r + 63 - __builtin_clzll(nz);
        carry += __shfl(inc, WAVE - 1, WAVE);
    }
    return last;
}

__device__ __forceinline__ uint32_t pack_item(int kind, int i, int j) { return uint32_t(kind) << 18 | uint32_t(i) << 9 | uint32_t(j); }

__global__ void __launch_bounds__(PS_NT)
pf_sample_kernel(KArgs ka, int variant, const uint8_t *__restrict__ seqs, int w0, double *scratch, size_t slice,
                 int k0, int nk, unsigned long long seed, char *structures, int *flag) {
    __shared__ SampleLds L;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int w = w0 + blockIdx.y;
    const DevVariant V = ka.variants[variant];
    const int N = V.N;
    double *tab = scratch + size_t(blockIdx.y) * slice;
    const DevScaled *X = ka.X;
    load_sequence(L.q, ka, V, seqs + size_t(w) * ka.Nraw, tid);   // the kernel's only barriers
    const PfModel M{ka.T, X, L.q, tab, tab + ka.cells, tab + 2 * size_t(ka.cells), tab + 3 * size_t(ka.cells), N,
                    X->motif_len, V.motif != 0};
    const int ks = blockIdx.x * PS_WAVES + wid;   // the wave's sample within this launch
    if (ks >= nk) return;
    const int k = k0 + ks;
    uint32_t *stk = L.stk[wid];
    char *out = L.out[wid];
    for (int p = lane; p < N; p += WAVE) out[p] = '.';
    // From here on every lane of the wave runs the same uniform control flow and
    // writes the same values to the same LDS addresses, so each lane reads back
    // what it wrote itself.
    const double Z = M.q5[N];
    int top = 0;
    bool bad = false;
    if (Z > 0.0 && Z < INFINITY && N >= 1) stk[top++] = pack_item(PI_Q5, 0, N);
    int pops = 0;
    for (; pops < PS_MAXPOPS; pops++) {
        if (top == 0) break;
        const uint32_t it = stk[--top];
        const int kind = int(it >> 18), i = int(it >> 9) & 511, j = int(it) & 511;
        const float u = ps_uniform(ps_draw(seed, uint32_t(w), uint32_t(k), uint32_t(pops)));
        const int c = wave_pick(M, kind, i, j, M.n_cand(kind, i, j), u, lane);
        if (c < 0 || top + 2 > PS_STACK) {   // inconsistent tables: never with a finite positive total
            bad = true;
            break;
        }
        if (kind == PI_Q5) {
            if (c == 0) {
                if (j - 1 >= 1) stk[top++] = pack_item(PI_Q5, 0, j - 1);
            } else {
                if (c - 1 >= 1) stk[top++] = pack_item(PI_Q5, 0, c - 1);
                stk[top++] = pack_item(PI_QB, c, j);
            }
        } else if (kind == PI_QB) {
            out[i - 1] = '(';
            out[j - 1] = ')';
            const int ns = M.n_shapes(i, j);
            if (c == PC_MOTIF) {   // the motif's own fold over i..j
                for (int m = 0; m < MAX_MOTIF; m++) {
                    if (m >= M.mL) break;
                    const int pm = L.q.mpt[m];
                    out[i - 1 + m] = pm < 0 ? '.' : (pm > m ? '(' : ')');
                }
            } else if (c >= PC_INT + ns) {
                const int s = i + 6 + (c - PC_INT - ns);
                stk[top++] = pack_item(PI_QM, i + 1, s - 1);
                stk[top++] = pack_item(PI_QM1, s, j - 1);
            } else if (c >= PC_INT) {
                int n1, n2;
                M.shape(c - PC_INT, n1, n2);
                stk[top++] = pack_item(PI_QB, i + 1 + n1, j - 1 - n2);
            }
        } else if (kind == PI_QM) {
            const int s = i + (c >> 1);
            if (c & 1) stk[top++] = pack_item(PI_QM, i, s - 1);
            stk[top++] = pack_item(PI_QM1, s, j);
        } else {
            stk[top++] = c == 0 ? pack_item(PI_QB, i, j) : pack_item(PI_QM1, i, j - 1);
        }
    }
    if (top != 0) bad = true;   // the pop bound was reached
    char *dst = structures + (size_t(blockIdx.y) * nk + ks) * N;
    for (int p = lane; p < N; p += WAVE) dst[p] = bad ? '.' : out[p];
    if (bad && lane == 0) atomicOr(flag, 1);
}

}  // namespace

size_t pf_sample_slice_doubles(const KArgs &ka) { return 3 * size_t(ka.cells) + size_t(ka.Nmax) + 2; }

SamplePlan pf_sample_plan(const KArgs &ka, int L, int W, int n_samples) {
    constexpr size_t cap = size_t(256) << 20;   // tables + device-side output of one launch (bytes)
    const size_t slice = pf_sample_slice_doubles(ka) * sizeof(double);
    const size_t len = size_t(std::max(L, 1));
    SamplePlan p;
    p.samples = int(std::min<size_t>(size_t(std::max(n_samples, 1)), std::max<size_t>(1, (cap - slice) / len)));
    const size_t most = std::min<size_t>(size_t(std::max(W, 1)), 65535);   // grid.y of pf_sample_kernel
    p.seqs = int(std::max<size_t>(1, std::min<size_t>(most, cap / (slice + size_t(p.samples) * len))));
    return p;
}

hipError_t launch_pf_fill(const KArgs &ka, int variant, const uint8_t *seqs, int w0, int n, double *scratch,
                          float *energies, hipStream_t stream, size_t slice_doubles) {
    if (ka.mode != 0 || variant < 0 || variant >= ka.n_variants || n < 1) return hipErrorInvalidValue;
    if (slice_doubles != 0 && slice_doubles < pf_sample_slice_doubles(ka)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pf_fill_kernel, dim3(n), dim3(PS_NT), 0, stream, ka, variant, seqs, w0, scratch,
                       slice_doubles ? slice_doubles : pf_sample_slice_doubles(ka), energies);
    return hipGetLastError();
}

hipError_t launch_pf_sample(const KArgs &ka, int variant, const uint8_t *seqs, int w0, int n, double *scratch,
                            int k0, int nk, uint64_t seed, char *structures, int *flag,
                            hipStream_t stream) {
    if (ka.mode != 0 || variant < 0 || variant >= ka.n_variants || n < 1 || n > 65535 || nk < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pf_sample_kernel, dim3((nk + PS_WAVES - 1) / PS_WAVES, n), dim3(PS_NT), 0, stream, ka, variant,
                       seqs, w0, scratch, pf_sample_slice_doubles(ka), k0, nk,
                       static_cast<unsigned long long>(seed), structures, flag);
    return hipGetLastError();
}

}  // namespace adx
