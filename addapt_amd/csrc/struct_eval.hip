// gfx950 energies and ensemble probabilities of GIVEN structures (RNAeval on
// the device): an off-step utility (the C ABI's adx_*eval_structures*), not the
// Monte Carlo score.  struct_eval_kernel prices (sequence, structure) items in
// the PF or the MFE convention of struct_eval_core.hpp, honouring the variant's
// context padding, constraint and ligand motif, and reports a status byte.
//
//   mapping    grid (blocks of SE_WAVES structures, sequence); one wave per item.
//              The workgroup's items fold the same sequence, so the sequence in
//              its context, the constraint arrays and the motif tables are
//              staged once per workgroup (fold_common.hpp seq_setup).
//   partners   lanes stride over positions; each scans to its bracket's match.
//   loops      each opening position walks and prices the loop it closes; the
//              last lane walks the exterior loop.
//   sites      per formed motif site the wave sums the loops the site encloses
//              and lane 0 applies the convention's adjustment.
//   totals     integer dcal by an integer wave sum (exact), the non-integer
//              terms (PF loops above 30) in FP64, the status by OR.
//
// The waves of a workgroup run the same phases, so the phases are separated by
// workgroup barriers; a wave without an item runs them empty.  The per-lane
// work is in struct_eval_core.hpp; this file is the barriers and sums around it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"

#define SE_FN __device__
#include "struct_eval_core.hpp"

namespace adx {
namespace {

constexpr int SE_NT = 256;              // threads per workgroup
constexpr int SE_WAVES = SE_NT / WAVE;  // items per workgroup

struct EvalLds {
    EvalSeqLds q;
    uint8_t br[SE_WAVES][SE_NP];        // bracket codes, 1-based
    uint8_t pt[SE_WAVES][SE_NP];        // partners, 1-based, 0 = unpaired
    double le[SE_WAVES][SE_NP];         // the loop each opening position closes, dcal
};
static_assert(sizeof(EvalLds) <= 48 * 1024, "static LDS of struct_eval_kernel");

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}
__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v |= __shfl_xor(v, d, WAVE);
    return v;
}

// Items: sequence b = blockIdx.y of n (raw codes at seqs + (w0 + b) * Nraw),
// structure k of n_per at structures + b * seq_stride + k * L; outputs at
// out0 + b * n_per + k.  fill: pf_fill_kernel's slices of these n sequences
// (q5[N] at slice b), or null when no probability is asked for.
__global__ void __launch_bounds__(SE_NT)
struct_eval_kernel(KArgs ka, const DevTables *TE, const EvalTab *E, int variant, const uint8_t *__restrict__ seqs,
                   int w0, int n_per, const char *__restrict__ structures, size_t seq_stride, const double *fill,
                   size_t slice, size_t out0, double *energies, double *probs, uint8_t *status) {
    __shared__ EvalLds L;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int b = blockIdx.y;
    const DevVariant V = ka.variants[variant];
    const int N = V.N;
    seq_setup<SE_NT>(L.q, ka, V, seqs + size_t(w0 + b) * ka.Nraw, tid, [](bool, float) { return 0; });
    for (int k = tid; k < MAX_SPECIAL_HP; k += SE_NT) L.q.spv[k] = E->sp_e[k];

    const int item = blockIdx.x * SE_WAVES + wid;
    const bool on = item < n_per;   // wave-uniform
    uint8_t *br = L.br[wid], *pt = L.pt[wid];
    double *le = L.le[wid];
    const StructEval<EvalSeqLds> M{TE, E, L.q, pt, N};
    EvalAcc acc;

    // ---- the structure where it lies
    if (on) {
        const char *st = structures + size_t(b) * seq_stride + size_t(item) * N;
        for (int k = lane + 1; k <= N; k += WAVE) {
            const uint8_t c = bracket_code(st[k - 1]);
            br[k] = c;
            if (c == SB_BAD) acc.status |= SE_MALFORMED;
        }
    }
    __syncthreads();
    // ---- partners
    if (on) {
        for (int k = lane + 1; k <= N; k += WAVE) {
            const int p = partner_of(br, N, k);
            if (p < 0) acc.status |= SE_MALFORMED;
            pt[k] = uint8_t(p > 0 ? p : 0);
        }
    }
    const bool unparsed = wave_or(acc.status) != 0;   // so far only the string itself was judged
    __syncthreads();
    // ---- every opening position's loop, every position's admission, the exterior loop
    if (on) {
        for (int k = lane + 1; k <= N; k += WAVE) {
            if (!M.admits(k)) acc.status |= SE_EXCLUDED;
            if (pt[k] > k) {
                EvalAcc one;
                M.loop_of(k, one);
                le[k] = double(one.e) + one.d;
                acc.e += one.e;
                acc.d += one.d;
                acc.status |= one.status;
            }
        }
        if (lane == WAVE - 1) M.exterior(acc);
    }
    __syncthreads();
    // ---- formed motif sites (disjoint: each holds the motif's own fold)
    double adj = 0.0;
    const int mL = ka.X->motif_len;
    if (on && V.motif != 0 && mL > 0) {
        for (int o = 1; o + mL - 1 <= N; o++) {
            if (!uni(L.q.mat[o])) continue;
            bool same = true;
            double enc = 0.0;
            for (int m = lane; m < mL; m += WAVE) {
                same = same && M.site_position(o, m);
                if (pt[o + m] > o + m) enc += le[o + m];
            }
            if (__ballot(!same) != 0) continue;
            enc = wave_sum_d(enc);
            if (lane == 0) {
                if (E->mfe) acc.e += M.site_adjust_mfe(int(enc));
                else adj += M.site_adjust_pf(enc);
            }
        }
    }
    // ---- totals
    const int e = wave_sum_i(acc.e);
    const double d = wave_sum_d(acc.d);
    const int stat = item_status(unparsed, wave_or(acc.status));
    if (on && lane == 0) {
        const size_t o = out0 + size_t(b) * n_per + item;
        const double en = item_energy(e, d, adj, stat);
        energies[o] = en;
        if (status) status[o] = uint8_t(stat);
        if (probs) {
            // pf_fill_kernel's total on the context's scale: ln Z = ln q5[N] - N ln sigma
            const double z = fill[size_t(b) * slice + 3 * size_t(ka.cells) + N];
            const double lnZ = z > 0.0 ? log(z) - N * ka.X->log_sigma : -INFINITY;
            probs[o] = item_prob(en, stat, lnZ, E->kT);
        }
    }
}

}  // namespace

hipError_t launch_struct_eval(const KArgs &ka, const DevTables *TE, const EvalTab *E, int variant,
                              const uint8_t *seqs, int w0, int n, int n_per, const char *structures,
                              size_t seq_stride, const double *fill, size_t out0, double *energies, double *probs,
                              uint8_t *status, hipStream_t stream) {
    if (variant < 0 || variant >= ka.n_variants || n < 1 || n > 65535 || n_per < 1 || !TE || !E || !energies ||
        (probs && (!fill || ka.mode != 0)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(struct_eval_kernel, dim3((n_per + SE_WAVES - 1) / SE_WAVES, n), dim3(SE_NT), 0, stream, ka, TE,
                       E, variant, seqs, w0, n_per, structures, seq_stride, fill, pf_sample_slice_doubles(ka), out0,
                       energies, probs, status);
    return hipGetLastError();
}

}  // namespace adx
