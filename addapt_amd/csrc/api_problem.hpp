// What the fold layer (api_fold.cpp) and the Monte Carlo layer (api_ctx.cpp) share
#pragma once

#include <cmath>
#include <cstdlib>
#include <memory>

#include "api_common.hpp"
#include "launch.hpp"
#include "loop_codetab_core.hpp"

namespace adx {

// One folding problem: energy tables, scaled constants, variants,
// constraint blobs and score-term map on one device.
struct Problem : DeviceStream {
    const EnergyParams *P = nullptr;
    int Nraw = 0, Nmax = 0;
    Motif motif;
    double motif_eint = 0.0;
    std::vector<int> motif_pt;
    double g0 = -0.30;  // assumed free energy per nucleotide for the pf scale
    std::vector<DevVariant> variants;
    std::vector<int> vmac;       // per variant: macrostate index, -1 = unconstrained
    std::vector<int> groups2;    // variant pairs folded in lockstep (fold_rows.hip pf_group)
    std::vector<uint8_t> cons;
    std::vector<uint8_t> ctx_seq;
    std::vector<int> ctx_off;
    std::vector<DevTermMap> tmap;
    int n_terms = 0, n_ctx_eff = 1;
    int mode = 0;                // 0 = partition functions, 1 = MFE (ADX_FOLD_*)
    DevBuf<DevTables> dT;
    DevBuf<DevScaled> dX;
    DevBuf<DevVariant> dV;
    DevBuf<uint8_t> dCons, dCtxSeq;
    DevBuf<int> dCtxOff;
    DevBuf<DevTermMap> dTmap;
    DevBuf<int> dGroups2;
    // base-pair probability terms: outside variants, requested pairs, per-walker results
    std::vector<int> bvars;
    std::vector<int> pairs;      // [n][3]: bvars index, i, j (1-based folded coordinates)
    DevBuf<int> dBvars, dPairs, dBvarSlot;
    DevBuf<double> dPairP;
    DevBuf<char> dScratch;       // outside tables in HBM when they do not fit LDS
    bool pf_ring = false;        // PF folds by pf_ring_kernel (fixes the slot layout, dispatch.hip pf_ring_layout)
    DevBuf<float> dRingScr;      // its qb scratch for stateless launches
    // MFE: packed 16-bit copies of the energy tables (fold_rows.hip MinPlus16)
    DevBuf<DevTables> dT16;
    DevBuf<DevScaled> dX16;
    DevBuf<uint16_t> dLoop16;    // T16's 1x1 .. 2x2 energies by code pair (loop_codetab_core.hpp)
    DevBuf<int> dOvf;
    bool mfe16 = false;
    bool mfe_cells_ok = false;   // Ninio saturated from |n1-n2| = 5 on, MLbase >= 0 (mfe_cells.hip)
    // incremental-fold state of the MC walkers (fold_rows.hip Inc)
    DevBuf<float> dTab;
    DevBuf<float> dGstep;        // [W][n_variants] energies of the step's folds (pf_cells_kernel,
                                 //   and the pair-term score that waits for the outside pass)
    DevBuf<uint8_t> dCur, dValid;
    DevBuf<int> dChg;
    DevBuf<int> dOrder;          // launch order of a rescore's folds (KArgs::order, order_kernel)
    DevBuf<uint8_t> dCls;        // the folds' weight classes (KArgs::ocls, the proposals' or a rescore's)
    DevBuf<int> dPairQ;          // mfe_pair_kernel's work queue (KArgs::pairq)
    DevBuf<int> dTrace;          // c / fm / fm1 scratch of mfe_trace_kernel, one launch chunk
    DevBuf<int> dSubopt;         // the seven triangles, f5 and f3 of mfe_subopt_kernel, one launch chunk
    float subopt_fill_ms = 0.f, subopt_select_ms = 0.f;   // the last subopt() call, from HIP events
    DevBuf<double> dSample;      // qb / qm / qm1 / q5 scratch of pf_fill_kernel, one launch chunk
    float sample_fill_ms = 0.f, sample_draw_ms = 0.f;   // the last sample() call, from HIP events
    float ens_bppm_ms = 0.f, ens_struct_ms = 0.f;       // the last ensemble() call, from HIP events
    DevBuf<DevTables> dTE;       // struct_eval_kernel: energy-valued tables of a PF problem (an MFE problem's dT serves)
    DevBuf<EvalTab> dEval;       // and the convention's loop-length table (setup_core.hpp build_eval_tab)
    float eval_fill_ms = 0.f, eval_ms = 0.f;            // the last eval_structures() call, from HIP events
    DevBuf<double> dAccess;      // pf_fill_kernel's tables, the adjoints and the run table of pf_access_kernel, one launch chunk
    float access_fill_ms = 0.f, access_outside_ms = 0.f;   // the last unpaired() call, from HIP events
    size_t tab_slot = 0;
    bool state_on = false;   // set for MC launches only (not for adx_score_batch)
    std::unique_ptr<DevTables> hT;
    std::unique_ptr<DevScaled> hX;

    double sigma() const { return std::exp(g0 / kT_kcal()); }

    KArgs kargs() const {
        KArgs ka{};
        ka.T = dT.p;
        ka.X = dX.p;
        ka.variants = dV.p;
        ka.cons = dCons.p;
        ka.ctx_seq = dCtxSeq.p;
        ka.ctx_off = dCtxOff.p;
        ka.tmap = dTmap.p;
        ka.n_variants = static_cast<int>(variants.size());
        ka.n_terms = n_terms;
        ka.n_ctx_eff = n_ctx_eff;
        ka.Nraw = Nraw;
        ka.Nmax = Nmax;
        ka.cells = Nmax >= 5 ? (Nmax - 4) * (Nmax - 3) / 2 : 1;
        ka.groups2 = dGroups2.p;
        ka.n_groups2 = static_cast<int>(groups2.size() / 2);
        ka.opt = 0;
        ka.mode = mode;
        ka.bvars = dBvars.p;
        ka.n_bvars = static_cast<int>(bvars.size());
        ka.bvar_slot = dBvarSlot.p;
        ka.pairs = dPairs.p;
        ka.n_pairs = static_cast<int>(pairs.size() / 3);
        ka.pair_p = dPairP.p;
        ka.bppm_scratch = dScratch.p;
        ka.T16 = mfe16 ? dT16.p : nullptr;
        ka.X16 = mfe16 ? dX16.p : nullptr;
        ka.ovf = mfe16 ? dOvf.p : nullptr;
        ka.loop16 = mfe16 ? dLoop16.p : nullptr;
        ka.mfe_cells_ok = mfe16 && mfe_cells_ok ? 1 : 0;
        const bool st = state_on && dTab.p && !std::getenv("ADX_NO_INCR");
        ka.tab = st ? dTab.p : nullptr;
        ka.tab_slot = tab_slot;
        ka.cur_slot = st ? dCur.p : nullptr;
        ka.tab_valid = st ? dValid.p : nullptr;
        ka.chg = st ? dChg.p : nullptr;
        ka.order = st && !std::getenv("ADX_NO_ORDER") ? dOrder.p : nullptr;
        ka.ocls = dCls.p;
        ka.pairq = dPairQ.p;
        ka.gstep = dGstep.p;
        ka.pf_ring = pf_ring ? 1 : 0;
        ka.ring_scratch = dRingScr.p;
        return ka;
    }

    // every context must fit the rows kernel (the fallback of every other fold kernel)
    adx_status check_lds() {
        const size_t need = lds_bytes(kargs());
        if (need > size_t(LDS_LIMIT))
            return fail(ADX_EUNSUPPORTED, "sequence length %d needs %zu B of LDS (> %zu)", Nmax, need,
                        size_t(LDS_LIMIT));
        return ADX_OK;
    }

    adx_status upload_scaled() {
        build_scaled(*P, sigma(), motif, motif_eint, motif_pt, *hX, mode == 1);
        HIP_TRY(dX.upload(hX.get(), 1, stream));
        return ADX_OK;
    }

    // MFE: the packed 16-bit copies of the tables (setup_core.hpp pack_mfe16), when every value fits
    adx_status upload_mfe16() {
        mfe16 = false;
        if (mode != 1 || std::getenv("ADX_NO_MFE16")) return ADX_OK;
        auto T16 = std::make_unique<DevTables>(*hT);
        auto X16 = std::make_unique<DevScaled>(*hX);
        if (!pack_mfe16(*T16, *X16)) return ADX_OK;   // FP32 MinPlus only
        // the 1x1 .. 2x2 energies by code pair (mfe_pair.hip bcell_tables)
        std::vector<uint16_t> loop16(LCT_ALLOC);
        static_assert(sizeof(float) == sizeof(uint32_t), "packed words in the tables' floats");
        if (!loop_codetab_build(reinterpret_cast<const uint32_t *>(&T16->int11[0][0][0][0]),
                                reinterpret_cast<const uint32_t *>(&T16->int21[0][0][0][0][0]),
                                reinterpret_cast<const uint32_t *>(&T16->int22[0][0][0][0][0][0]), loop16.data()))
            return ADX_OK;   // FP32 MinPlus only
        HIP_TRY(dLoop16.upload(loop16.data(), loop16.size(), stream));
        HIP_TRY(dT16.upload(T16.get(), 1, stream));
        HIP_TRY(dX16.upload(X16.get(), 1, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        mfe16 = true;
        mfe_cells_ok = mfe_cells_model_ok(*P);
        return ADX_OK;
    }
    // per walker two slots of every group's tables: sized for the largest kernel
    // configuration (P = 2 value arrays, one group per variant)
    adx_status alloc_state(int W) {
        tab_slot = size_t(variants.size()) * inc_group_floats(kargs().cells, Nmax, 2);
        // the MFE16 slots' per-cell codes follow the groups' tables (dev_types.hpp)
        const int ng = int((variants.size() + 1) / 2) + int(variants.size());
        tab_slot = std::max(tab_slot, inc_cc_offset(kargs().cells, Nmax, ng, ng));
        tab_slot = std::max(tab_slot, inc_cc_offset_pf(kargs().cells, Nmax, ng, ng));
        tab_slot = (tab_slot + 3) / 4 * 4;   // 16-byte aligned slots (the codes are read as uint4)
        HIP_TRY(dTab.alloc(size_t(W) * 2 * tab_slot));
        HIP_TRY(dCur.alloc(W));
        HIP_TRY(dValid.alloc(W));
        HIP_TRY(dChg.alloc(size_t(W) * 2));
        HIP_TRY(dOrder.alloc(W));
        HIP_TRY(dCls.alloc(W));
        HIP_TRY(hipMemsetAsync(dCls.p, 64, W, stream));   // "not scored" until a proposal or rescore sets it
        if (adx_status sg = ensure_gstep(W)) return sg;
        HIP_TRY(hipMemsetAsync(dCur.p, 1, W, stream));     // the initial fold writes slot 0
        HIP_TRY(hipMemsetAsync(dValid.p, 0, W, stream));
        HIP_TRY(hipMemsetAsync(dChg.p, 0xff, sizeof(int) * 2 * W, stream));
        return ADX_OK;
    }
    adx_status ensure_ovf(int W) {
        if (mfe16 && dOvf.n < size_t(W)) {
            HIP_TRY(dOvf.alloc(W));
            HIP_TRY(hipMemsetAsync(dOvf.p, 0, sizeof(int) * W, stream));
        }
        return ADX_OK;
    }

    adx_status upload_all() {
        hT = std::make_unique<DevTables>();
        hX = std::make_unique<DevScaled>();
        build_tables(*P, *hT, mode == 1);
        HIP_TRY(dT.upload(hT.get(), 1, stream));
        adx_status s = upload_scaled();
        if (s) return s;
        HIP_TRY(dV.upload(variants.data(), variants.size(), stream));
        HIP_TRY(dCons.upload(cons.data(), cons.size(), stream));
        HIP_TRY(dCtxSeq.upload(ctx_seq.data(), ctx_seq.size(), stream));
        HIP_TRY(dCtxOff.upload(ctx_off.data(), ctx_off.size(), stream));
        HIP_TRY(dTmap.upload(tmap.data(), tmap.size(), stream));
        if (vmac.size() != variants.size()) vmac.assign(variants.size(), -1);
        groups2 = pair_groups2(variants, vmac);
        HIP_TRY(dGroups2.upload(groups2.data(), groups2.size(), stream));
        HIP_TRY(dBvars.upload(bvars.data(), bvars.size(), stream));
        std::vector<int> bslot;
        SetupError err;
        if (outside_slots(groups2, bvars, bslot, err)) return fail(err);
        HIP_TRY(dBvarSlot.upload(bslot.data(), bslot.size(), stream));
        HIP_TRY(dPairs.upload(pairs.data(), pairs.size(), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        // the slot layout of the walkers' stored tables: one choice per context
        pf_ring = false;
        pf_ring = pf_ring_layout(kargs());
        s = upload_mfe16();
        if (s) return s;
        if (!pairs.empty() && bppm_lds_bytes(kargs(), nullptr) == 0)
            return fail(ADX_EUNSUPPORTED, "base-pair probabilities of length %d do not fit one CU's LDS yet", Nmax);
        return check_lds();
    }

    // A free fold's outside pass: variant v alone, no stored tables reused, no pair terms,
    // scratch for W sequences per launch (dbv, dscr: the caller's; v outlives the queued copy)
    adx_status free_outside_args(const int &v, int W, DevBuf<int> &dbv, DevBuf<char> &dscr, KArgs &ka) {
        HIP_TRY(dbv.upload(&v, 1, stream));
        ka = kargs();
        ka.bvars = dbv.p;
        ka.n_bvars = 1;
        ka.bvar_slot = nullptr;
        ka.n_pairs = 0;
        ka.pairs = nullptr;
        ka.pair_p = nullptr;
        if (bppm_lds_bytes(ka, nullptr) == 0)
            return fail(ADX_EUNSUPPORTED, "base-pair probabilities of length %d do not fit one CU's LDS yet", Nmax);
        const size_t scr = bppm_scratch_bytes(ka, W);
        if (scr) HIP_TRY(dscr.alloc(scr));
        ka.bppm_scratch = dscr.p;
        return ADX_OK;
    }

    // per-walker pair-probability buffer (grow-only)
    adx_status ensure_pairs(int W) {
        const size_t need = size_t(W) * (pairs.size() / 3);
        if (need > 0 && dPairP.n < need) HIP_TRY(dPairP.alloc(need));
        return ensure_scratch(kargs(), W);
    }
    adx_status ensure_scratch(const KArgs &ka, int W) {
        const size_t need = bppm_scratch_bytes(ka, W);
        if (need > 0 && dScratch.n < need) HIP_TRY(dScratch.alloc(need));
        return ADX_OK;
    }

    adx_status ensure_gstep(int W) {
        const size_t need = size_t(W) * variants.size();
        if (dGstep.n < need) HIP_TRY(dGstep.alloc(need));
        return ADX_OK;
    }

    // MFE structures of W sequences (device codes) for one variant: W * variants[v].N
    // chars and W energies to device buffers (mfe_trace.hip); touches no fold state
    adx_status trace(const uint8_t *dseqs, int W, int v, char *dstruct, float *denergy) {
        const KArgs ka = kargs();
        const int chunk = mfe_trace_chunk(ka, W);
        const size_t need = size_t(chunk) * mfe_trace_slice_ints(ka);
        if (dTrace.n < need) HIP_TRY(dTrace.alloc(need));
        HIP_TRY(launch_mfe_trace(ka, v, dseqs, W, dTrace.p, chunk, dstruct, denergy, stream));
        return ADX_OK;
    }

    // Zuker suboptimal structures of W sequences (device codes) for one variant, to the
    // HOST buffers of h (launch.hpp SuboptOut's layout; n_within, seeds and pair_energy
    // optional).  mfe_subopt.hip: per launch chunk the fill phase, then the selection
    // phase on the same scratch slices; touches no fold state.
    // ADX_SUBOPT_CHUNK=<n> (tests) bounds the sequences per launch; the results do not depend on it.
    adx_status subopt(const uint8_t *dseqs, int W, int v, double delta_kcal, int max_structs, const SuboptOut &h) {
        const KArgs ka = kargs();
        const size_t L = size_t(variants[v].N), K = size_t(max_structs);
        const int delta_dcal = int(std::lround(100.0 * std::min(delta_kcal, 1.0e6)));   // 1e8 dcal: every pair
        int chunk = mfe_subopt_chunk(ka, W);
        if (const char *env = std::getenv("ADX_SUBOPT_CHUNK"))
            if (std::atoi(env) > 0) chunk = std::min(chunk, std::atoi(env));
        const size_t need = size_t(chunk) * mfe_subopt_slice_ints(ka);
        if (dSubopt.n < need) HIP_TRY(dSubopt.alloc(need));
        DevBuf<int> dnf, dnw, dsd;
        DevBuf<float> dmfe, de, dpe;
        DevBuf<char> dst;
        HIP_TRY(dnf.alloc(W));
        HIP_TRY(dnw.alloc(W));
        HIP_TRY(dmfe.alloc(W));
        HIP_TRY(dst.alloc(size_t(W) * K * L));
        HIP_TRY(de.alloc(size_t(W) * K));
        HIP_TRY(dsd.alloc(size_t(W) * K * 2));
        if (h.pair_energy) HIP_TRY(dpe.alloc(size_t(W) * L * L));
        const SuboptOut d{dnf.p, dnw.p, dmfe.p, dst.p, de.p, dsd.p, h.pair_energy ? dpe.p : nullptr};
        Events ev;
        if (adx_status se = ev.create(3)) return se;
        subopt_fill_ms = subopt_select_ms = 0.f;
        for (int w0 = 0; w0 < W; w0 += chunk) {
            const int n = std::min(chunk, W - w0);
            HIP_TRY(hipEventRecord(ev[0], stream));
            HIP_TRY(launch_mfe_subopt(ka, v, dseqs, w0, n, dSubopt.p, 0, delta_dcal, max_structs, d, stream));
            HIP_TRY(hipEventRecord(ev[1], stream));
            HIP_TRY(launch_mfe_subopt(ka, v, dseqs, w0, n, dSubopt.p, 1, delta_dcal, max_structs, d, stream));
            HIP_TRY(hipEventRecord(ev[2], stream));
            HIP_TRY(hipStreamSynchronize(stream));   // the events are recorded again by the next chunk
            float a = 0.f, b = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
            subopt_fill_ms += a;
            subopt_select_ms += b;
        }
        HIP_TRY(hipMemcpyAsync(h.n_found, dnf.p, sizeof(int) * W, hipMemcpyDeviceToHost, stream));
        if (h.n_within) HIP_TRY(hipMemcpyAsync(h.n_within, dnw.p, sizeof(int) * W, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(h.mfe, dmfe.p, sizeof(float) * W, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(h.structures, dst.p, size_t(W) * K * L, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(h.energies, de.p, sizeof(float) * W * K, hipMemcpyDeviceToHost, stream));
        if (h.seeds) HIP_TRY(hipMemcpyAsync(h.seeds, dsd.p, sizeof(int) * W * K * 2, hipMemcpyDeviceToHost, stream));
        if (h.pair_energy)
            HIP_TRY(hipMemcpyAsync(h.pair_energy, dpe.p, sizeof(float) * W * L * L, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ADX_OK;
    }

    // n_samples structures drawn from the ensemble of each of W sequences (device
    // codes) for one variant, to HOST buffers: structures[W][n_samples][variants[v].N]
    // chars, energies[W] (optional).  pf_sample.hip; touches no fold state.
    // chunk > 0 overrides the sequences per launch (the results do not depend on it).
    adx_status sample(const char *who, const uint8_t *dseqs, int W, int v, int n_samples, uint64_t seed,
                      char *structures, float *energies, int chunk = 0) {
        const KArgs ka = kargs();
        const size_t L = size_t(variants[v].N);
        SamplePlan plan = pf_sample_plan(ka, int(L), W, n_samples);
        if (chunk > 0) plan.seqs = std::min(plan.seqs, chunk);
        const size_t slice = pf_sample_slice_doubles(ka);
        if (dSample.n < size_t(plan.seqs) * slice) HIP_TRY(dSample.alloc(size_t(plan.seqs) * slice));
        DevBuf<char> dout;
        DevBuf<float> de;
        DevBuf<int> dflag;
        HIP_TRY(dout.alloc(size_t(plan.seqs) * plan.samples * L));
        HIP_TRY(de.alloc(W));
        HIP_TRY(dflag.alloc(1));
        HIP_TRY(hipMemsetAsync(dflag.p, 0, sizeof(int), stream));
        Events ev;
        if (adx_status se = ev.create(3)) return se;
        sample_fill_ms = sample_draw_ms = 0.f;
        for (int w0 = 0; w0 < W; w0 += plan.seqs) {
            const int n = std::min(plan.seqs, W - w0);
            HIP_TRY(hipEventRecord(ev[0], stream));
            HIP_TRY(launch_pf_fill(ka, v, dseqs, w0, n, dSample.p, de.p, stream));
            HIP_TRY(hipEventRecord(ev[1], stream));
            float fill = 0.f;
            for (int k0 = 0; k0 < n_samples; k0 += plan.samples) {
                const int nk = std::min(plan.samples, n_samples - k0);
                if (k0 > 0) HIP_TRY(hipEventRecord(ev[1], stream));
                HIP_TRY(launch_pf_sample(ka, v, dseqs, w0, n, dSample.p, k0, nk, seed, dout.p, dflag.p, stream));
                HIP_TRY(hipEventRecord(ev[2], stream));
                if (nk == n_samples) {   // the chunk's rows are contiguous on both sides
                    HIP_TRY(hipMemcpyAsync(structures + size_t(w0) * n_samples * L, dout.p, size_t(n) * nk * L,
                                           hipMemcpyDeviceToHost, stream));
                } else {
                    for (int r = 0; r < n; r++)
                        HIP_TRY(hipMemcpyAsync(structures + (size_t(w0 + r) * n_samples + k0) * L,
                                               dout.p + size_t(r) * nk * L, size_t(nk) * L, hipMemcpyDeviceToHost,
                                               stream));
                }
                HIP_TRY(hipStreamSynchronize(stream));   // dout is reused by the next launch
                float ms = 0.f;
                if (k0 == 0) HIP_TRY(hipEventElapsedTime(&fill, ev[0], ev[1]));
                HIP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
                sample_draw_ms += ms;
            }
            sample_fill_ms += fill;
        }
        int flag = 0;
        HIP_TRY(hipMemcpyAsync(&flag, dflag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        if (energies) HIP_TRY(hipMemcpyAsync(energies, de.p, sizeof(float) * W, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (flag)
            return fail(ADX_EHIP, "%s: a sample reached the sampler's loop bound (inconsistent tables); its "
                        "structure is all '.'", who);
        return ADX_OK;
    }

    // Centroid and MEA structures of W sequences (device codes) for the unconstrained
    // variant v, to HOST buffers: centroid, mea = W * variants[v].N chars, stats[W]
    // (each optional), probs = the W matrices (optional).  Per launch chunk the
    // outside pass writes the matrices to a device buffer and ensemble_struct_kernel
    // reads them there.  Every buffer is the call's own: no fold state is touched.
    // chunk > 0 overrides the sequences per launch (the results do not depend on it).
    adx_status ensemble(const uint8_t *dseqs, int W, int v, double gamma, char *centroid, char *mea,
                        adx_ensemble_stats *stats, double *probs, int chunk = 0) {
        static_assert(sizeof(adx_ensemble_stats) == 3 * sizeof(double), "the kernel writes three doubles per sequence");
        const size_t L = size_t(variants[v].N);
        int per = ensemble_struct_chunk(int(L), W);
        if (chunk > 0) per = std::min(per, chunk);
        const size_t slice = ensemble_struct_slice_doubles(int(L));
        DevBuf<int> dbv;
        DevBuf<char> dscr, dcen, dmea;
        DevBuf<double> dfull, dtab, dst;
        KArgs ka;
        if (adx_status so = free_outside_args(v, per, dbv, dscr, ka)) return so;
        HIP_TRY(dfull.alloc(size_t(per) * L * L));
        HIP_TRY(dtab.alloc(size_t(per) * slice));
        HIP_TRY(dcen.alloc(size_t(per) * L));
        HIP_TRY(dmea.alloc(size_t(per) * L));
        HIP_TRY(dst.alloc(size_t(per) * 3));
        Events ev;
        if (adx_status se = ev.create(3)) return se;
        ens_bppm_ms = ens_struct_ms = 0.f;
        for (int w0 = 0; w0 < W; w0 += per) {
            const int n = std::min(per, W - w0);
            HIP_TRY(hipMemsetAsync(dfull.p, 0, sizeof(double) * n * L * L, stream));   // the outside pass writes pairs only
            HIP_TRY(hipEventRecord(ev[0], stream));
            HIP_TRY(launch_bppm(ka, dseqs + size_t(w0) * Nraw, n, nullptr, dfull.p, int(L), nullptr, ka.bppm_scratch,
                                stream));
            HIP_TRY(hipEventRecord(ev[1], stream));
            HIP_TRY(launch_ensemble_struct(dfull.p, int(L), n, gamma, dtab.p, dcen.p, dmea.p, dst.p, stream));
            HIP_TRY(hipEventRecord(ev[2], stream));
            if (centroid)
                HIP_TRY(hipMemcpyAsync(centroid + size_t(w0) * L, dcen.p, size_t(n) * L, hipMemcpyDeviceToHost, stream));
            if (mea) HIP_TRY(hipMemcpyAsync(mea + size_t(w0) * L, dmea.p, size_t(n) * L, hipMemcpyDeviceToHost, stream));
            if (stats)
                HIP_TRY(hipMemcpyAsync(stats + w0, dst.p, sizeof(adx_ensemble_stats) * n, hipMemcpyDeviceToHost, stream));
            if (probs)
                HIP_TRY(hipMemcpyAsync(probs + size_t(w0) * L * L, dfull.p, sizeof(double) * n * L * L,
                                       hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));   // the buffers are reused by the next chunk
            float a = 0.f, b = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
            ens_bppm_ms += a;
            ens_struct_ms += b;
        }
        return ADX_OK;
    }

    // struct_eval_kernel's tables in this problem's convention (PF or MFE), uploaded once
    adx_status ensure_eval() {
        if (dEval.p) return ADX_OK;
        auto E = std::make_unique<EvalTab>();
        build_eval_tab(*P, motif, motif_eint, *E, mode == 1);
        if (mode != 1) {
            auto TE = std::make_unique<DevTables>();
            build_tables(*P, *TE, true);
            HIP_TRY(dTE.upload(TE.get(), 1, stream));
        }
        HIP_TRY(dEval.upload(E.get(), 1, stream));
        HIP_TRY(hipStreamSynchronize(stream));   // E and TE are locals
        return ADX_OK;
    }

    // Energies, probabilities and status bytes of n_per given structures for each of W
    // sequences (device codes) under variant v, to HOST buffers of W * n_per,
    // sequence-major (probs and status optional; probs on PF problems only).
    // structures (host): W * n_per * L chars, or n_per * L shared by every sequence.
    // struct_eval.hip; probs adds pf_fill_kernel's FP64 fill per sequence.  Every
    // buffer is the call's own but the fill scratch: no fold state is touched.
    // ADX_EVAL_CHUNK=<n> (tests) bounds the sequences per launch; the results do not depend on it.
    adx_status eval_structures(const uint8_t *dseqs, int W, int v, int n_per, const char *structures, bool shared,
                               double *energies, double *probs, uint8_t *status) {
        if (adx_status se = ensure_eval()) return se;
        const KArgs ka = kargs();
        const size_t L = size_t(variants[v].N);
        const size_t items = size_t(W) * n_per;
        int per = std::min(W, 65535);   // grid.y of struct_eval_kernel
        if (probs) per = std::min(per, pf_sample_plan(ka, int(L), W, 1).seqs);
        if (const char *env = std::getenv("ADX_EVAL_CHUNK"))
            if (std::atoi(env) > 0) per = std::min(per, std::atoi(env));
        const size_t slice = pf_sample_slice_doubles(ka);
        if (probs && dSample.n < size_t(per) * slice) HIP_TRY(dSample.alloc(size_t(per) * slice));
        DevBuf<char> dst;
        DevBuf<double> de, dp;
        DevBuf<uint8_t> ds;
        HIP_TRY(dst.upload(structures, (shared ? size_t(n_per) : items) * L, stream));
        HIP_TRY(de.alloc(items));
        if (probs) HIP_TRY(dp.alloc(items));
        if (status) HIP_TRY(ds.alloc(items));
        Events ev;
        if (adx_status se = ev.create(3)) return se;
        eval_fill_ms = eval_ms = 0.f;
        const size_t stride = shared ? 0 : size_t(n_per) * L;
        for (int w0 = 0; w0 < W; w0 += per) {
            const int n = std::min(per, W - w0);
            HIP_TRY(hipEventRecord(ev[0], stream));
            if (probs) HIP_TRY(launch_pf_fill(ka, v, dseqs, w0, n, dSample.p, nullptr, stream));
            HIP_TRY(hipEventRecord(ev[1], stream));
            HIP_TRY(launch_struct_eval(ka, mode == 1 ? dT.p : dTE.p, dEval.p, v, dseqs, w0, n, n_per,
                                       dst.p + size_t(w0) * stride, stride, probs ? dSample.p : nullptr,
                                       size_t(w0) * n_per, de.p, probs ? dp.p : nullptr, status ? ds.p : nullptr,
                                       stream));
            HIP_TRY(hipEventRecord(ev[2], stream));
            HIP_TRY(hipStreamSynchronize(stream));   // the fill scratch is reused by the next chunk
            float a = 0.f, b = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
            if (probs) eval_fill_ms += a;
            eval_ms += b;
        }
        HIP_TRY(hipMemcpyAsync(energies, de.p, sizeof(double) * items, hipMemcpyDeviceToHost, stream));
        if (probs) HIP_TRY(hipMemcpyAsync(probs, dp.p, sizeof(double) * items, hipMemcpyDeviceToHost, stream));
        if (status) HIP_TRY(hipMemcpyAsync(status, ds.p, items, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ADX_OK;
    }

    // Unpaired-region probabilities of W sequences (device codes) under variant v, to HOST
    // buffers (each optional): profile[W][max_len][L], region_probs[W][n_regions] for the
    // n_regions (first, length) pairs of `regions` (host), pair_probs[W][L][L], energies[W].
    // pf_sample.hip's FP64 fill on the longer slices of pf_access.hip, then its outside
    // pass; only what was asked for crosses to the host.  Every buffer is the call's own:
    // no fold state is touched.  ADX_ACCESS_CHUNK=<n> (tests) bounds the sequences per
    // launch; the results do not depend on it.
    adx_status unpaired(const uint8_t *dseqs, int W, int v, int max_len, int n_regions, const int *regions,
                        double *profile, double *region_probs, double *pair_probs, float *energies) {
        const KArgs ka = kargs();
        const size_t L = size_t(variants[v].N);
        const size_t n_prof = profile ? size_t(max_len) * L : 0, n_reg = region_probs ? size_t(n_regions) : 0;
        const size_t n_pair = pair_probs ? L * L : 0;
        int per = pf_access_chunk(ka, W, n_prof + n_reg + n_pair);
        if (const char *env = std::getenv("ADX_ACCESS_CHUNK"))
            if (std::atoi(env) > 0) per = std::min(per, std::atoi(env));
        const size_t slice = pf_access_slice_doubles(ka);
        if (dAccess.n < size_t(per) * slice) HIP_TRY(dAccess.alloc(size_t(per) * slice));
        DevBuf<double> dprof, dreg, dpair;
        DevBuf<int> dregions;
        DevBuf<float> de;
        if (n_prof) HIP_TRY(dprof.alloc(size_t(per) * n_prof));
        if (n_reg) {
            HIP_TRY(dreg.alloc(size_t(per) * n_reg));
            HIP_TRY(dregions.upload(regions, 2 * n_reg, stream));
        }
        if (n_pair) HIP_TRY(dpair.alloc(size_t(per) * n_pair));
        HIP_TRY(de.alloc(W));
        const AccessOut d{profile ? max_len : 0, int(n_reg), dregions.p, dprof.p, dreg.p, dpair.p};
        Events ev;
        if (adx_status se = ev.create(3)) return se;
        access_fill_ms = access_outside_ms = 0.f;
        for (int w0 = 0; w0 < W; w0 += per) {
            const int n = std::min(per, W - w0);
            HIP_TRY(hipEventRecord(ev[0], stream));
            HIP_TRY(launch_pf_fill(ka, v, dseqs, w0, n, dAccess.p, de.p, stream, slice));
            HIP_TRY(hipEventRecord(ev[1], stream));
            HIP_TRY(launch_pf_access(ka, v, dseqs, w0, n, dAccess.p, d, stream));
            HIP_TRY(hipEventRecord(ev[2], stream));
            if (n_prof)
                HIP_TRY(hipMemcpyAsync(profile + size_t(w0) * n_prof, dprof.p, sizeof(double) * n * n_prof,
                                       hipMemcpyDeviceToHost, stream));
            if (n_reg)
                HIP_TRY(hipMemcpyAsync(region_probs + size_t(w0) * n_reg, dreg.p, sizeof(double) * n * n_reg,
                                       hipMemcpyDeviceToHost, stream));
            if (n_pair)
                HIP_TRY(hipMemcpyAsync(pair_probs + size_t(w0) * n_pair, dpair.p, sizeof(double) * n * n_pair,
                                       hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));   // the buffers are reused by the next chunk
            float a = 0.f, b = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
            access_fill_ms += a;
            access_outside_ms += b;
        }
        if (energies) HIP_TRY(hipMemcpyAsync(energies, de.p, sizeof(float) * W, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ADX_OK;
    }

    // the per-walker buffers a fold of W walkers writes (grow-only)
    adx_status prepare(int W) {
        adx_status so = ensure_ovf(W);
        if (so) return so;
        if (mfe16 && !dPairQ.p) {
            HIP_TRY(dPairQ.alloc(2));
            HIP_TRY(hipMemsetAsync(dPairQ.p, 0, sizeof(int) * 2, stream));
        }
        so = ensure_gstep(W);
        if (so) return so;
        if (pf_ring) {   // qb scratch of the stateless ring folds
            const size_t need = pf_ring_scratch_floats(kargs(), W);
            if (dRingScr.n < need) HIP_TRY(dRingScr.alloc(need));
        }
        return pairs.empty() ? ADX_OK : ensure_pairs(W);
    }

    // Score W sequences (device pointer of W*Nraw codes); outputs are device pointers.
    adx_status score(const uint8_t *dseqs, int W, double *dscores, double *dterms, float *ddG) {
        adx_status so = prepare(W);
        if (so) return so;
        if (!pairs.empty())
            HIP_TRY(launch_bppm(kargs(), dseqs, W, nullptr, nullptr, 0, dPairP.p, dScratch.p, stream));
        HIP_TRY(launch_score(kargs(), dseqs, W, dscores, dterms, ddG, stream));
        return ADX_OK;
    }
};

// pick a pf scale from the ensemble energy of a reference sequence
inline adx_status calibrate(Problem &pb, const std::vector<uint8_t> &codes) {
    DevBuf<uint8_t> dseq;
    DevBuf<double> dsc;
    DevBuf<float> ddg;
    HIP_TRY(dseq.upload(codes.data(), codes.size(), pb.stream));
    HIP_TRY(dsc.alloc(1));
    HIP_TRY(ddg.alloc(pb.variants.size()));
    std::vector<float> g(pb.variants.size());
    for (int attempt = 0; attempt < 6; attempt++) {
        adx_status s = pb.upload_scaled();
        if (s) return s;
        s = pb.score(dseq.p, 1, dsc.p, nullptr, ddg.p);
        if (s) return s;
        HIP_TRY(hipMemcpyAsync(g.data(), ddg.p, g.size() * sizeof(float), hipMemcpyDeviceToHost, pb.stream));
        HIP_TRY(hipStreamSynchronize(pb.stream));
        // variant 0 is always the unconstrained apo ensemble of the first context
        const double G = g[0];
        const int N = pb.variants[0].N;
        if (std::isfinite(G) && N > 0) {
            const double g_new = std::min(-0.05, G / N);
            if (std::fabs(g_new - pb.g0) < 1e-9) return ADX_OK;
            pb.g0 = g_new;
            return pb.upload_scaled();
        }
        pb.g0 *= 2.0;  // overflow: scale harder and retry
    }
    return fail(ADX_EINVAL, "could not find a partition-function scale for this sequence");
}

inline bool subopt_args_ok(double delta_kcal, int max_structs) { return delta_kcal >= 0.0 && max_structs >= 1; }   // NaN: no

// max_len in [1, L] with a profile, 0 allowed without; every region inside [0, L), length >= 1
inline bool unpaired_args_ok(int L, int max_len, bool with_profile, int n_regions, const int *regions) {
    if (max_len < (with_profile ? 1 : 0) || max_len > L || n_regions < 0 || (n_regions > 0 && !regions)) return false;
    for (int r = 0; r < n_regions; r++) {
        const int first = regions[2 * r], len = regions[2 * r + 1];
        if (first < 0 || len < 1 || first >= L || len > L - first) return false;
    }
    return true;
}

inline bool ensemble_args_ok(double gamma, const char *centroid, const char *mea, const adx_ensemble_stats *stats) {
    return std::isfinite(gamma) && gamma > 0.0 && (centroid || mea || stats);
}

}  // namespace adx
