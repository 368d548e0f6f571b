// The score combination shared by the MC step tail (mc_step.hip) and
// combine_kernel (dispatch.hip): one term's value, and a walker's score by one wave.
#pragma once

#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "fold_common.hpp"

namespace adx {
namespace {

// combine_score's arithmetic (scoring.cc:53-71): term idx (= context * n_terms
// + term) of the walker whose per-variant energies are g and pair
// probabilities pp (null: the pair terms read 0.5)
__device__ __forceinline__ double term_value(const KArgs &ka, const float *g, const double *pp, int idx,
                                             double &weight) {
    const DevTermMap m = ka.tmap[idx];
    double p = (m.kind == 1) ? (pp ? pp[m.pidx] : 0.5)
                             : exp((static_cast<double>(g[m.vfree]) - static_cast<double>(g[m.vcons])) / ka.X->kT);
    if (!m.favorable) p = 1.0 - p;
    weight = m.weight;
    return log(p);
}

// A score as the reference sums it: each context's terms in term order
// (evaluate_terms, scoring.cc:154), the contexts' sums in context order
// (scoring.cc:124-130).  One flat sum over contexts x terms differs from it in the
// last bit, which decides between ACCEPT_IMPROVED and ACCEPT_WORSENED when a
// move leaves an MFE score where it was (energies are whole dcal: different terms,
// the same total).  add() takes the weighted terms in idx order.
struct ContextSum {
    int n_terms, k = 0;
    double total = 0.0, part = 0.0;
    __device__ __forceinline__ void add(double x) {
        if (k == n_terms) {
            total += part;
            part = 0.0;
            k = 0;
        }
        part += x;
        k++;
    }
    __device__ __forceinline__ double sum() const { return total + part; }
};

// The score of walker w from KArgs::gstep, one wave: the terms' values on
// lanes, summed by ContextSum (the same sum as combine_kernel's loop); tv
// (the walker's term values, optional).  Result uniform.
__device__ double combine_wave(const KArgs &ka, int w, int lane, double *tv) {
    const float *g = ka.gstep + size_t(w) * ka.n_variants;
    const double *pp = ka.pair_p ? ka.pair_p + size_t(w) * ka.n_pairs : nullptr;
    const int nt = ka.n_terms * ka.n_ctx_eff;
    ContextSum score{ka.n_terms};
    for (int b0 = 0; b0 < nt; b0 += WAVE) {
        const int idx = b0 + lane;
        double val = 0.0, wt = 0.0;
        if (idx < nt) {
            val = term_value(ka, g, pp, idx, wt);
            if (tv) tv[idx] = val;
        }
        const int n = min(WAVE, nt - b0);
        for (int k = 0; k < n; k++) score.add(__shfl(wt, k, WAVE) * __shfl(val, k, WAVE));
    }
    return score.sum();
}

}  // namespace
}  // namespace adx
