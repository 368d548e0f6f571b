// Which kernel folds a workload: the one place that chooses among the fold
// kernels (fold_rows.hip, mfe_cells.hip, mfe_pair.hip, pf_cells.hip,
// pf_ring.hip) and the outside kernels (outside_cells.hip, outside_ring.hip,
// bppm_kernel), reads the kernel-choice environment variables, and names the
// choice for the bench (adx_last_kernel_names).  The other files only launch
// their own kernels.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "combine.hpp"
#include "dev_types.hpp"
#include "launch.hpp"

namespace adx {

// Scores from the per-variant energies a fold kernel left in KArgs::gstep
// (combine_score, one thread per walker): after pf_cells_kernel, and after the
// outside pass once it has written the pair probabilities (pair_p null: the
// pair terms read 0.5, as combine_score).
__global__ void combine_kernel(KArgs ka, int W, const int *mask, double *scores, double *terms) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W || (mask && mask[w] != 1)) return;
    const float *g = ka.gstep + size_t(w) * ka.n_variants;
    const double *pp = ka.pair_p ? ka.pair_p + size_t(w) * ka.n_pairs : nullptr;
    const int nt = ka.n_terms * ka.n_ctx_eff;
    double *tv = terms ? terms + size_t(w) * nt : nullptr;
    ContextSum score{ka.n_terms};
    for (int idx = 0; idx < nt; idx++) {
        double wt;
        const double val = term_value(ka, g, pp, idx, wt);
        if (tv) tv[idx] = val;
        score.add(wt * val);
    }
    scores[w] = score.sum();
}

hipError_t launch_combine(const KArgs &ka, int W, const int *mask, double *scores, double *terms,
                          hipStream_t stream) {
    hipLaunchKernelGGL(combine_kernel, dim3((W + 255) / 256), dim3(256), 0, stream, ka, W, mask, scores, terms);
    return hipGetLastError();
}

// The kernel-choice environment variables are read at every launch, so a test
// can switch them between contexts (the paths they select are the tests'
// references).
static bool env_is(const char *name, const char *value) {
    const char *e = std::getenv(name);
    return e && std::strcmp(e, value) == 0;
}
// ADX_MFE_KERNEL: cells (default) = mfe_cells_kernel / mfe_pair_kernel (lanes =
// cells, two folds per cell, two walkers per CU); rows = score_kernel<MinPlus16>
// (lanes = terms) -- also the kernel for energy models or lengths the cells
// kernel does not cover (mfe_cells_lds() == 0)
static bool mfe_rows_forced() { return env_is("ADX_MFE_KERNEL", "rows"); }
static bool pf_rows_forced() { return env_is("ADX_PF_KERNEL", "rows"); }
// Two diagonals per barrier (mfe_pair.hip) for folded lengths up to 100 unless
// ADX_MFE_PAIR=0
static bool mfe_pair_active(const KArgs &k16) {
    const char *e = std::getenv("ADX_MFE_PAIR");
    return !(e && e[0] == '0') && mfe_pair_covers(k16);
}
// ADX_PAIR_GRID=n: mfe_pair_kernel's workgroup count (default 0: as many as are
// resident at once).  The folds do not depend on it; a test sets 1 so that one
// workgroup takes every item of the queue in turn
static int mfe_pair_grid() {
    const char *e = std::getenv("ADX_PAIR_GRID");
    const int n = e ? std::atoi(e) : 0;
    return n > 0 ? n : 0;
}

static KArgs packed16(const KArgs &ka) {   // the packed 16-bit MFE kernels' energy tables
    KArgs k16 = ka;
    k16.T = ka.T16;
    k16.X = ka.X16;
    return k16;
}

// PF folds longer than pf_cells covers take the ring kernel (pf_ring.hip).
// One choice per context (api_problem.hpp upload_all): it fixes the layout of the
// walkers' stored tables, which every later kernel of the context must read
// the same way.
bool pf_ring_layout(const KArgs &ka) {
    return ka.mode == 0 && !pf_rows_forced() && pf_ring_lds(ka) > 0 && (ka.n_pairs <= 0 || outside_ring_lds(ka) > 0);
}

// The fold kernel launch_score_m runs for a workload (one choice, used by the
// dispatch and by the names the bench reports)
enum class InsideK { MfeCells, MfeRows16, MinPlusP2, MinPlus512, PfCells, PfRing, SumProdP2, SumProd768, SumProd512 };
static InsideK inside_choice(const KArgs &ka, bool has_g) {
    // ka.mode: 0 = partition functions (vrna_pf), 1 = minimum free energies
    if (ka.mode == 1 && ka.X16 && ka.ovf)
        return (!mfe_rows_forced() && mfe_cells_lds(packed16(ka)) > 0) ? InsideK::MfeCells : InsideK::MfeRows16;
    if (ka.mode == 1) return rows_lockstep(ka) == 2 ? InsideK::MinPlusP2 : InsideK::MinPlus512;
    if (ka.pf_ring) return InsideK::PfRing;   // the context's slot layout (pf_ring_layout)
    if (has_g && !pf_rows_forced() && rows_lockstep(ka) == 2 && ka.n_groups2 > 0 && pf_cells_lds(ka) > 0)
        return InsideK::PfCells;
    if (rows_lockstep(ka) == 2) return InsideK::SumProdP2;
    // one workgroup per CU (N = 150: the P = 1 tables take most of the LDS): 12
    // waves instead of 8, 168 VGPRs a lane (16 waves at 128 spill: 29.9 vs 28.2 ms)
    if (rows_one_per_cu(ka)) return InsideK::SumProd768;
    return InsideK::SumProd512;
}

const char *inside_kernel_name(const KArgs &ka) {
    switch (inside_choice(ka, ka.gstep != nullptr)) {
        case InsideK::MfeCells:
            return mfe_pair_active(packed16(ka))
                       ? "mfe_pair_kernel + score_kernel<MinPlus> (FP32 fallback launch); scores combined in step_tail_kernel"
                       : "mfe_cells_kernel + score_kernel<MinPlus> (FP32 fallback launch); scores combined in step_tail_kernel";
        case InsideK::MfeRows16: return rows_kernel_name(RowsK::MinPlus16);
        case InsideK::MinPlusP2: return rows_kernel_name(RowsK::MinPlusP2);
        case InsideK::MinPlus512: return rows_kernel_name(RowsK::MinPlus512);
        case InsideK::PfCells: return "pf_cells_kernel (scores combined in step_tail_kernel)";
        case InsideK::PfRing: return "pf_ring_kernel (scores combined in step_tail_kernel)";
        case InsideK::SumProdP2: return rows_kernel_name(RowsK::SumProdP2);
        case InsideK::SumProd768: return rows_kernel_name(RowsK::SumProd768);
        default: return rows_kernel_name(RowsK::SumProd512);
    }
}

hipError_t launch_score_m(const KArgs &ka, const uint8_t *seqs, int W, double *scores, double *terms,
                          float *dG, const int *mask, hipStream_t stream) {
    float *g = dG ? dG : ka.gstep;
    const InsideK k = inside_choice(ka, g != nullptr);
    // the kernels that write per-variant energies to g: then the scores (the same
    // arithmetic as combine_score), unless the step's tail combines them
    auto combine = [&]() {
        if (ka.defer_comb && mask) return hipSuccess;
        KArgs kc = ka;
        kc.gstep = g;
        return launch_combine(kc, W, mask, scores, terms, stream);
    };
    if (k == InsideK::MfeCells || k == InsideK::MfeRows16) {
        // packed 16-bit folds (two variants per value, two workgroups per CU), then
        // the FP32 MinPlus kernel for the walkers whose values left the exact range
        const KArgs k16 = packed16(ka);
        hipError_t e;
        if (k == InsideK::MfeCells) {
            // one workgroup per (walker, fold group): energies to dG (or the gstep scratch)
            if (!g) return hipErrorInvalidValue;
            if (ka.ovf && !ka.order) {   // the fold groups of a walker only ever set its flag (an MC step's
                                         // proposal or a rescore's first launch cleared them)
                e = hipMemsetAsync(ka.ovf, 0, sizeof(int) * size_t(W), stream);
                if (e != hipSuccess) return e;
            }
            e = mfe_pair_active(k16) ? launch_mfe_pair(k16, seqs, W, g, mask, stream, mfe_pair_grid())
                                     : launch_mfe_cells(k16, seqs, W, g, mask, stream);
            if (e == hipSuccess) e = combine();
        } else {
            e = launch_score_rows(RowsK::MinPlus16, k16, seqs, W, scores, terms, dG, mask, stream);
        }
        if (e != hipSuccess) return e;
        KArgs kf = ka;            // the FP32 fallback folds from scratch, keeps no state
        kf.tab = nullptr;
        // overflows are rare: one block per CU scans the flags (ovf) instead of W
        // blocks that mostly exit at once
        constexpr int FB_GRID = 64;
        return launch_score_rows(rows_lockstep(ka) == 2 ? RowsK::MinPlusP2 : RowsK::MinPlus512, kf, seqs, W, scores,
                                 terms, dG, ka.ovf, stream, FB_GRID);
    }
    switch (k) {
        case InsideK::MinPlusP2: return launch_score_rows(RowsK::MinPlusP2, ka, seqs, W, scores, terms, dG, mask, stream);
        case InsideK::MinPlus512: return launch_score_rows(RowsK::MinPlus512, ka, seqs, W, scores, terms, dG, mask, stream);
        case InsideK::PfCells: {
            // lanes = cells (pf_cells.hip): energies to dG (or the gstep scratch), then the scores
            hipError_t e = launch_pf_cells(ka, seqs, W, mask, g, stream);
            return e != hipSuccess ? e : combine();
        }
        case InsideK::PfRing: {
            // one workgroup per variant, qb ring (pf_ring.hip), then the scores
            if (!g) return hipErrorInvalidValue;
            hipError_t e = launch_pf_ring(ka, seqs, W, mask, g, ka.tab ? nullptr : ka.ring_scratch, stream);
            return e != hipSuccess ? e : combine();
        }
        case InsideK::SumProdP2: return launch_score_rows(RowsK::SumProdP2, ka, seqs, W, scores, terms, dG, mask, stream);
        case InsideK::SumProd768: return launch_score_rows(RowsK::SumProd768, ka, seqs, W, scores, terms, dG, mask, stream);
        default: return launch_score_rows(RowsK::SumProd512, ka, seqs, W, scores, terms, dG, mask, stream);
    }
}

hipError_t launch_score(const KArgs &ka, const uint8_t *seqs, int W, double *scores, double *terms, float *dG,
                        hipStream_t stream) {
    return launch_score_m(ka, seqs, W, scores, terms, dG, nullptr, stream);
}

// The outside pass of an MC step with pair terms (mc_step.hip launch_window),
// on the tables the inside folds stored: the ring's kernel for the ring's slot
// layout, the lanes = cells kernel where it covers the workload, else
// bppm_kernel (ADX_OUTSIDE_KERNEL=bppm forces the latter)
static bool outside_is_cells(const KArgs &ka) {
    if (ka.pf_ring) return false;   // the ring's slot layout: outside_ring_kernel
    return !env_is("ADX_OUTSIDE_KERNEL", "bppm") && outside_cells_lds(ka) > 0;
}
hipError_t launch_outside_m(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, hipStream_t stream) {
    double *pair_p = const_cast<double *>(ka.pair_p);
    if (ka.pf_ring) return launch_outside_ring(ka, seqs, W, mask, pair_p, stream);
    if (outside_is_cells(ka)) return launch_outside_cells(ka, seqs, W, mask, pair_p, rows_lockstep(ka), stream);
    return launch_bppm_rows(ka, seqs, W, mask, nullptr, 0, pair_p, ka.bppm_scratch, stream, true);
}
const char *outside_kernel_name(const KArgs &ka) {
    if (ka.n_pairs <= 0) return "";
    if (!(ka.mode == 0 && ka.tab && ka.gstep)) {   // launch_window's fallback branch: bppm from scratch
        bool gout = false;
        bppm_lds_bytes(ka, &gout);
        return gout ? "bppm_kernel<1024, GOUT> (inside refold + outside)" : "bppm_kernel<512> (inside refold + outside)";
    }
    if (ka.pf_ring) return "outside_ring_kernel";
    if (outside_is_cells(ka)) return "outside_cells_kernel";
    bool gout = false;
    bppm_lds_bytes(ka, &gout);
    return gout ? "bppm_kernel<1024, GOUT>" : "bppm_kernel<512>";
}

// scratch: bppm_scratch_bytes(ka, W) bytes of device memory (null when 0)
hipError_t launch_bppm(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, double *full, int ld,
                       double *pair_p, char *scratch, hipStream_t stream) {
    return launch_bppm_rows(ka, seqs, W, mask, full, ld, pair_p, scratch, stream, false);
}

// Whether launch_window leaves a step's scores as energies in gstep (KArgs::
// defer_comb set): the fold kernels that write per-variant energies and the
// outside pass of the pair terms
bool window_defers(const KArgs &ka) {
    if (!ka.defer_comb) return false;
    if (ka.n_pairs > 0 && ka.mode == 0 && ka.tab && ka.gstep) return true;
    const InsideK k = inside_choice(ka, ka.gstep != nullptr);
    return k == InsideK::MfeCells || k == InsideK::PfCells || k == InsideK::PfRing;
}

}  // namespace adx
