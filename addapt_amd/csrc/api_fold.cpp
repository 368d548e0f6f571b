// C ABI of the MI355X engine (include/addapt_gpu.h), the fold layer: one
// sequence with an optional motif and constraint, folded as a one-variant Problem.
#include <cctype>
#include <cmath>
#include <cstring>
#include <memory>

#include "api_problem.hpp"

using namespace adx;

// ================================================================== fold layer
struct adx_fold {
    const adx_params *params = nullptr;
    std::string seq;
    int with_bppm = 0;
    int device = 0;
    std::string constraint;  // accumulated (last one wins, like a fresh DB constraint)
    Motif motif;
    std::vector<double> bpp; // cached N*N probabilities (scoring.cc:41-44 computes them once)
};

extern "C" adx_status adx_fold_create(const adx_params *p, const char *seq, int with_bppm, int device,
                                      adx_fold **out) {
    if (!p || !seq || !out) return fail(ADX_EINVAL, "adx_fold_create: null argument");
    const int N = static_cast<int>(std::strlen(seq));
    if (N < 1 || N > NMAX) return fail(ADX_EINVAL, "sequence length %d outside [1, %d]", N, NMAX);
    auto f = std::make_unique<adx_fold>();
    f->params = p;
    f->seq = seq;
    for (auto &c : f->seq) c = static_cast<char>(std::toupper(static_cast<unsigned char>(c)));
    f->with_bppm = with_bppm;
    f->device = device;
    *out = f.release();
    return ADX_OK;
}

extern "C" adx_status adx_fold_add_motif(adx_fold *f, const char *mseq, const char *mfold, double e) {
    if (!f || !mseq || !mfold) return fail(ADX_EINVAL, "adx_fold_add_motif: null argument");
    f->motif.seq = mseq;
    for (auto &c : f->motif.seq) c = static_cast<char>(std::toupper(static_cast<unsigned char>(c)));
    f->motif.fold = mfold;
    f->motif.energy_kcal = e;
    f->motif.present = true;
    f->bpp.clear();
    return ADX_OK;
}

extern "C" adx_status adx_fold_add_constraint(adx_fold *f, const char *db) {
    if (!f || !db) return fail(ADX_EINVAL, "adx_fold_add_constraint: null argument");
    if (std::strlen(db) != f->seq.size())
        return fail(ADX_ECONSTRAINT, "constraint length %zu != sequence length %zu", std::strlen(db), f->seq.size());
    std::vector<uint8_t> tmp;
    SetupError err;
    if (build_constraint(db, static_cast<int>(f->seq.size()), tmp, err)) return fail(err);
    f->constraint = db;
    f->bpp.clear();
    return ADX_OK;
}

// The one-variant problem the compound f currently describes, uploaded.
static adx_status fold_problem(adx_fold *f, int mode, Problem &pb) {
    pb.mode = mode;
    pb.P = &f->params->P;
    adx_status s = pb.open(f->device);
    if (s) return s;
    const int N = static_cast<int>(f->seq.size());
    pb.Nraw = pb.Nmax = N;
    pb.motif = f->motif;
    SetupError err;
    if (pb.motif.present && prepare_motif(*pb.P, pb.motif, pb.motif_eint, pb.motif_pt, err)) return fail(err);
    // variant 0: the ensemble this fold compound currently describes
    if (build_constraint(f->constraint, N, pb.cons, err)) return fail(err);
    pb.variants.push_back(DevVariant{N, 0, -1, 0, pb.motif.present ? 1 : 0, 0});
    pb.ctx_seq.assign(1, 0);
    pb.ctx_off.assign(4, 0);
    pb.tmap.assign(1, DevTermMap{0, 0, 1, 0.0});
    pb.n_terms = 0;
    return pb.upload_all();
}

// One fold of the compound f in mode 0 (partition function, on a calibrated
// scale) or 1 (MFE): pb is left uploaded and dseq holds the sequence, for an
// outside pass to follow.
static adx_status fold_one(adx_fold *f, int mode, Problem &pb, DevBuf<uint8_t> &dseq, float *energy) {
    adx_status s = fold_problem(f, mode, pb);
    if (s) return s;
    const int N = static_cast<int>(f->seq.size());
    DevBuf<double> dsc;
    DevBuf<float> ddg;
    s = upload_codes(f->seq.data(), f->seq.size(), dseq, pb.stream);
    if (s) return s;
    HIP_TRY(dsc.alloc(1));
    HIP_TRY(ddg.alloc(1));
    float g = NAN;
    if (mode == 1) {   // integer min-plus: no scale to calibrate
        s = pb.score(dseq.p, 1, dsc.p, nullptr, ddg.p);
        if (s) return s;
        HIP_TRY(hipMemcpyAsync(&g, ddg.p, sizeof(float), hipMemcpyDeviceToHost, pb.stream));
        HIP_TRY(hipStreamSynchronize(pb.stream));
        *energy = g;
        return ADX_OK;
    }
    for (int attempt = 0; attempt < 6; attempt++) {
        s = pb.score(dseq.p, 1, dsc.p, nullptr, ddg.p);
        if (s) return s;
        HIP_TRY(hipMemcpyAsync(&g, ddg.p, sizeof(float), hipMemcpyDeviceToHost, pb.stream));
        HIP_TRY(hipStreamSynchronize(pb.stream));
        if (std::isfinite(g) || (std::isinf(g) && g > 0)) {
            // +inf = empty (constrained) ensemble; recalibrate once for accuracy
            if (attempt == 0 && std::isfinite(g) && N > 0) {
                pb.g0 = std::min(-0.05, static_cast<double>(g) / N);
                s = pb.upload_scaled();
                if (s) return s;
                continue;
            }
            // +inf on the assumed scale is also what a constrained ensemble of positive energy gives
            // once its weight times sigma^N falls below FP32 (about 64 kcal/mol above N * g0): fold
            // once more on the mildest scale, which a finite first fold would have chosen for it
            if (attempt == 0 && !std::isfinite(g) && pb.g0 < -0.05) {
                pb.g0 = -0.05;
                s = pb.upload_scaled();
                if (s) return s;
                continue;
            }
            break;
        }
        pb.g0 *= 2.0;
        s = pb.upload_scaled();
        if (s) return s;
    }
    *energy = g;
    return ADX_OK;
}

// The outside pass of a fold_one(mode 0) problem whose energy is finite: the
// N x N pair probabilities into dfull, which stays on the device (queued on
// pb.stream, not awaited).
static adx_status fold_outside(Problem &pb, const DevBuf<uint8_t> &dseq, int N, DevBuf<double> &dfull) {
    pb.bvars.assign(1, 0);   // the buffers stay with pb: the launch is still queued when this returns
    KArgs ka;
    adx_status s = pb.free_outside_args(pb.bvars[0], 1, pb.dBvars, pb.dScratch, ka);
    if (s) return s;
    HIP_TRY(dfull.alloc(size_t(N) * N));
    HIP_TRY(hipMemsetAsync(dfull.p, 0, sizeof(double) * N * N, pb.stream));
    HIP_TRY(launch_bppm(ka, dseq.p, 1, nullptr, dfull.p, N, nullptr, ka.bppm_scratch, pb.stream));
    return ADX_OK;
}

// The compound's energy in mode 0 or 1 and, in mode 0, optionally its pair probabilities.
static adx_status fold_energy(adx_fold *f, int mode, float *energy, std::vector<double> *bpp = nullptr) {
    Problem pb;
    DevBuf<uint8_t> dseq;
    adx_status s = fold_one(f, mode, pb, dseq, energy);
    if (s || mode == 1 || !bpp) return s;
    const int N = static_cast<int>(f->seq.size());
    bpp->assign(size_t(N) * N, 0.0);
    if (!std::isfinite(*energy)) return ADX_OK;   // empty ensemble: every probability is 0
    DevBuf<double> dfull;
    s = fold_outside(pb, dseq, N, dfull);   // on the calibrated scale
    if (s) return s;
    HIP_TRY(hipMemcpyAsync(bpp->data(), dfull.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    return ADX_OK;
}

extern "C" adx_status adx_fold_pf(adx_fold *f, float *energy) {
    if (!f || !energy) return fail(ADX_EINVAL, "adx_fold_pf: null argument");
    return fold_energy(f, 0, energy);
}

extern "C" adx_status adx_fold_mfe(adx_fold *f, float *energy) {
    if (!f || !energy) return fail(ADX_EINVAL, "adx_fold_mfe: null argument");
    return fold_energy(f, 1, energy);
}

extern "C" adx_status adx_fold_mfe_structure(adx_fold *f, char *structure, float *energy) {
    if (!f || !structure || !energy) return fail(ADX_EINVAL, "adx_fold_mfe_structure: null argument");
    Problem pb;
    adx_status s = fold_problem(f, 1, pb);
    if (s) return s;
    const size_t N = f->seq.size();
    DevBuf<uint8_t> dseq;
    DevBuf<char> dst;
    DevBuf<float> de;
    s = upload_codes(f->seq.data(), N, dseq, pb.stream);
    if (s) return s;
    HIP_TRY(dst.alloc(N));
    HIP_TRY(de.alloc(1));
    s = pb.trace(dseq.p, 1, 0, dst.p, de.p);
    if (s) return s;
    HIP_TRY(hipMemcpyAsync(structure, dst.p, N, hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipMemcpyAsync(energy, de.p, sizeof(float), hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    structure[N] = 0;
    return ADX_OK;
}

extern "C" adx_status adx_fold_subopt_structures(adx_fold *f, double delta_kcal, int max_structs, int *n_found,
                                                 int *n_pairs_within, float *mfe_kcal, char *structures,
                                                 float *energies, int *seeds, float *pair_energy) {
    if (!f || !n_found || !mfe_kcal || !structures || !energies)
        return fail(ADX_EINVAL, "adx_fold_subopt_structures: null argument");
    if (!subopt_args_ok(delta_kcal, max_structs))
        return fail(ADX_EINVAL, "adx_fold_subopt_structures: delta %g < 0 or max_structs %d < 1", delta_kcal, max_structs);
    Problem pb;
    adx_status s = fold_problem(f, 1, pb);
    if (s) return s;
    const size_t N = f->seq.size();
    DevBuf<uint8_t> dseq;
    s = upload_codes(f->seq.data(), N, dseq, pb.stream);
    if (s) return s;
    std::vector<char> rows(size_t(max_structs) * N);
    s = pb.subopt(dseq.p, 1, 0, delta_kcal, max_structs,
                  SuboptOut{n_found, n_pairs_within, mfe_kcal, rows.data(), energies, seeds, pair_energy});
    if (s) return s;
    for (int k = 0; k < max_structs; k++) {   // NUL-terminated rows
        std::memcpy(structures + size_t(k) * (N + 1), rows.data() + size_t(k) * N, N);
        structures[size_t(k) * (N + 1) + N] = 0;
    }
    return ADX_OK;
}

extern "C" adx_status adx_fold_sample_structures(adx_fold *f, int n_samples, uint64_t seed, char *structures,
                                                 float *energy) {
    if (!f || !structures) return fail(ADX_EINVAL, "adx_fold_sample_structures: null argument");
    if (n_samples < 1) return fail(ADX_EINVAL, "adx_fold_sample_structures: n_samples %d < 1", n_samples);
    Problem pb;
    // the default scale serves: pf_fill_kernel sums in FP64, which the factors of
    // no sequence of <= NMAX bases leave, so there is no calibration loop here
    adx_status s = fold_problem(f, 0, pb);
    if (s) return s;
    DevBuf<uint8_t> dseq;
    s = upload_codes(f->seq.data(), f->seq.size(), dseq, pb.stream);
    if (s) return s;
    return pb.sample("adx_fold_sample_structures", dseq.p, 1, 0, n_samples, seed, structures, energy);
}

extern "C" adx_status adx_fold_eval_structures(adx_fold *f, int convention, int n, const char *structures,
                                               double *energies, double *probs, uint8_t *status) {
    if (!f || !structures || !energies) return fail(ADX_EINVAL, "adx_fold_eval_structures: null argument");
    if (convention != ADX_FOLD_PF && convention != ADX_FOLD_MFE)
        return fail(ADX_EINVAL, "adx_fold_eval_structures: convention %d is neither ADX_FOLD_PF nor ADX_FOLD_MFE",
                    convention);
    if (n < 1) return fail(ADX_EINVAL, "adx_fold_eval_structures: n %d < 1", n);
    if (probs && convention != ADX_FOLD_PF)
        return fail(ADX_EINVAL, "adx_fold_eval_structures: probabilities exist in the ADX_FOLD_PF convention only");
    Problem pb;
    // the default scale serves the probabilities: pf_fill_kernel sums in FP64
    adx_status s = fold_problem(f, convention, pb);
    if (s) return s;
    DevBuf<uint8_t> dseq;
    s = upload_codes(f->seq.data(), f->seq.size(), dseq, pb.stream);
    if (s) return s;
    return pb.eval_structures(dseq.p, 1, 0, n, structures, true, energies, probs, status);
}

extern "C" adx_status adx_fold_unpaired_probs(adx_fold *f, int max_len, double *probs, double *pair_probs,
                                              float *energy_kcal) {
    if (!f || !probs) return fail(ADX_EINVAL, "adx_fold_unpaired_probs: null argument");
    const int N = static_cast<int>(f->seq.size());
    if (!unpaired_args_ok(N, max_len, true, 0, nullptr))
        return fail(ADX_EINVAL, "adx_fold_unpaired_probs: max_len %d outside [1, %d]", max_len, N);
    Problem pb;
    // the default scale serves: pf_fill_kernel and pf_access_kernel sum in FP64
    adx_status s = fold_problem(f, 0, pb);
    if (s) return s;
    DevBuf<uint8_t> dseq;
    s = upload_codes(f->seq.data(), f->seq.size(), dseq, pb.stream);
    if (s) return s;
    return pb.unpaired(dseq.p, 1, 0, max_len, 0, nullptr, probs, nullptr, pair_probs, energy_kcal);
}

extern "C" adx_status adx_fold_bpp(adx_fold *f, int i, int j, double *prob) {
    if (!f || !prob) return fail(ADX_EINVAL, "adx_fold_bpp: null argument");
    const int N = static_cast<int>(f->seq.size());
    if (i < 1 || j < 1 || i > N || j > N) return fail(ADX_EINVAL, "adx_fold_bpp: (%d, %d) outside [1, %d]", i, j, N);
    if (f->bpp.empty()) {
        float g = 0.f;
        adx_status s = fold_energy(f, 0, &g, &f->bpp);
        if (s) {
            f->bpp.clear();
            return s;
        }
    }
    *prob = (i != j) ? f->bpp[size_t(i - 1) * N + (j - 1)] : 0.0;
    return ADX_OK;
}

// The centroid, MEA structure and stats of the compound's ensemble from its N x N
// probabilities in dfull, on pb's device; dfull null: the empty ensemble.  The
// probabilities become those adx_fold_bpp serves, as a by-product.
static adx_status ensemble_summary(adx_fold *f, const DeviceStream &pb, const DevBuf<double> *dfull, double gamma,
                                   char *centroid, char *mea, adx_ensemble_stats *stats) {
    const size_t N = f->seq.size();
    if (centroid) centroid[N] = 0;
    if (mea) mea[N] = 0;
    std::vector<double> bpp(N * N, 0.0);
    if (!dfull) {   // every probability is 0 and there is nothing to summarise
        f->bpp.swap(bpp);
        if (centroid) std::memset(centroid, '.', N);
        if (mea) std::memset(mea, '.', N);
        if (stats) stats->mea = stats->centroid_dist = stats->diversity = NAN;
        return ADX_OK;
    }
    DevBuf<double> dtab, dst;
    DevBuf<char> dcen, dmea;
    HIP_TRY(dtab.alloc(ensemble_struct_slice_doubles(int(N))));
    HIP_TRY(dcen.alloc(N));
    HIP_TRY(dmea.alloc(N));
    HIP_TRY(dst.alloc(3));
    HIP_TRY(launch_ensemble_struct(dfull->p, int(N), 1, gamma, dtab.p, dcen.p, dmea.p, dst.p, pb.stream));
    if (centroid) HIP_TRY(hipMemcpyAsync(centroid, dcen.p, N, hipMemcpyDeviceToHost, pb.stream));
    if (mea) HIP_TRY(hipMemcpyAsync(mea, dmea.p, N, hipMemcpyDeviceToHost, pb.stream));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, dst.p, sizeof(*stats), hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipMemcpyAsync(bpp.data(), dfull->p, sizeof(double) * N * N, hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    f->bpp.swap(bpp);
    return ADX_OK;
}

extern "C" adx_status adx_fold_ensemble_structures(adx_fold *f, double gamma, char *centroid, char *mea,
                                                   adx_ensemble_stats *stats) {
    if (!f) return fail(ADX_EINVAL, "adx_fold_ensemble_structures: null argument");
    if (!ensemble_args_ok(gamma, centroid, mea, stats))
        return fail(ADX_EINVAL, "adx_fold_ensemble_structures: gamma %g not finite and > 0, or nothing to return", gamma);
    const size_t N = f->seq.size();
    if (N < 5) {
        // no pair closes a hairpin of 3 in fewer than 5 bases: the ensemble is the open
        // chain (every probability 0), or nothing when the constraint demands a pair.
        // The fold kernels are not run, and no Problem is set up.
        DeviceStream pb;
        DevBuf<double> dfull;
        adx_status s = pb.open(f->device);
        if (s) return s;
        if (f->constraint.find_first_of("()|<>") != std::string::npos)
            return ensemble_summary(f, pb, nullptr, gamma, centroid, mea, stats);
        HIP_TRY(dfull.alloc(N * N));
        HIP_TRY(hipMemsetAsync(dfull.p, 0, sizeof(double) * N * N, pb.stream));
        return ensemble_summary(f, pb, &dfull, gamma, centroid, mea, stats);
    }
    Problem pb;
    DevBuf<uint8_t> dseq;
    DevBuf<double> dfull;
    float g = NAN;
    adx_status s = fold_one(f, 0, pb, dseq, &g);
    if (s) return s;
    if (!std::isfinite(g)) return ensemble_summary(f, pb, nullptr, gamma, centroid, mea, stats);
    s = fold_outside(pb, dseq, int(N), dfull);
    if (s) return s;
    return ensemble_summary(f, pb, &dfull, gamma, centroid, mea, stats);
}

extern "C" void adx_fold_free(adx_fold *f) { delete f; }
