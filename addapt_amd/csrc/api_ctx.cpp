// C ABI of the MI355X engine (include/addapt_gpu.h), the Monte Carlo layer:
// contexts, walkers, steps, and the batch / walkers forms of the structure utilities.
#include <cctype>
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <tuple>

#include "api_ctx.hpp"

using namespace adx;

// ================================================================== MC layer
extern "C" adx_status adx_ctx_create(const adx_run_desc *d, adx_ctx **out) {
    if (!d || !out || !d->params || !d->sequence) return fail(ADX_EINVAL, "adx_ctx_create: null argument");
    auto c = std::make_unique<adx_ctx>();
    Problem &pb = c->pb;
    pb.P = &d->params->P;
    c->templ = d->sequence;
    const int N = static_cast<int>(c->templ.size());
    if (N < 1) return fail(ADX_EINVAL, "empty sequence");
    for (int m = 0; m < d->n_macrostates; m++) {
        std::string s = d->macrostates[m];
        if (static_cast<int>(s.size()) != N)
            return fail(ADX_EINVAL, "constraint length doesn't match sequence length");
        c->macrostates.push_back(s);
    }
    if (d->n_terms < 0 || d->n_terms > MAX_TERMS) return fail(ADX_EINVAL, "n_terms out of range");
    for (int t = 0; t < d->n_terms; t++) {
        const adx_term &T = d->terms[t];
        if (T.kind == ADX_TERM_PAIR) {
            if (T.pair_i < 0 || T.pair_j >= N || T.pair_j - T.pair_i < 1)
                return fail(ADX_EINVAL, "term %d: pair (%d, %d) outside [0, %d)", t, T.pair_i, T.pair_j, N);
        } else if (T.kind != ADX_TERM_MACROSTATE) {
            return fail(ADX_EINVAL, "term %d: bad kind %d", t, T.kind);
        } else if (T.macrostate < 0 || T.macrostate >= d->n_macrostates) {
            return fail(ADX_EINVAL, "term %d names macrostate %d (have %d)", t, T.macrostate, d->n_macrostates);
        }
        if (T.condition != ADX_APO && T.condition != ADX_HOLO) return fail(ADX_EINVAL, "bad condition");
        c->terms.push_back(T);
    }
    if (d->fold_mode != ADX_FOLD_PF && d->fold_mode != ADX_FOLD_MFE) return fail(ADX_EINVAL, "bad fold_mode");
    pb.mode = d->fold_mode;
    c->thermo = d->thermostat;
    if (c->thermo.kind == ADX_THERMO_ANNEAL && c->thermo.cycle_len <= 0)
        return fail(ADX_EINVAL, "annealing cycle length must be positive");
    if (c->thermo.kind == ADX_THERMO_AUTO && c->thermo.period <= 0)
        return fail(ADX_EINVAL, "auto thermostat training period must be positive");
    if (c->thermo.kind < 0 || c->thermo.kind > 2) return fail(ADX_EINVAL, "bad thermostat kind");

    adx_status s = pb.open(d->device);
    if (s) return s;
    pb.Nraw = N;
    // motif
    if (d->aptamer_seq && d->aptamer_fold) {
        pb.motif.seq = d->aptamer_seq;
        for (auto &ch : pb.motif.seq) ch = static_cast<char>(std::toupper(static_cast<unsigned char>(ch)));
        pb.motif.fold = d->aptamer_fold;
        pb.motif.energy_kcal = d->aptamer_energy_kcal;
        pb.motif.mode = d->motif_mode;
        pb.motif.present = true;
        SetupError err;
        if (prepare_motif(*pb.P, pb.motif, pb.motif_eint, pb.motif_pt, err)) return fail(err);
    }
    // contexts (ScoreFunction::evaluate scoring.cc:123-132, map order)
    c->n_contexts = d->n_contexts;
    pb.n_ctx_eff = std::max(1, d->n_contexts);
    pb.n_terms = static_cast<int>(c->terms.size());
    pb.ctx_seq.clear();
    pb.ctx_off.clear();
    std::vector<int> ctxN;
    for (int k = 0; k < pb.n_ctx_eff; k++) {
        std::string b, a;
        if (d->n_contexts > 0) {
            b = d->contexts[k].before ? d->contexts[k].before : "";
            a = d->contexts[k].after ? d->contexts[k].after : "";
        }
        pb.ctx_off.push_back(static_cast<int>(pb.ctx_seq.size()));
        pb.ctx_off.push_back(static_cast<int>(b.size()));
        for (char ch : b) pb.ctx_seq.push_back(static_cast<uint8_t>(base_code(ch)));
        pb.ctx_off.push_back(static_cast<int>(pb.ctx_seq.size()));
        pb.ctx_off.push_back(static_cast<int>(a.size()));
        for (char ch : a) pb.ctx_seq.push_back(static_cast<uint8_t>(base_code(ch)));
        ctxN.push_back(static_cast<int>(b.size() + a.size()) + N);
    }
    if (pb.ctx_seq.empty()) pb.ctx_seq.push_back(0);
    pb.Nmax = *std::max_element(ctxN.begin(), ctxN.end());
    if (pb.Nmax > NMAX) return fail(ADX_EUNSUPPORTED, "folded length %d exceeds %d", pb.Nmax, NMAX);
    // variants: per context, (condition, macrostate | free); holo == apo without an aptamer
    std::map<std::tuple<int, int, int>, int> vindex;
    auto variant = [&](int ctx, int cond, int mac) -> int {
        if (!pb.motif.present) cond = ADX_APO;
        auto key = std::make_tuple(ctx, cond, mac);
        auto it = vindex.find(key);
        if (it != vindex.end()) return it->second;
        const int Nc = ctxN[ctx];
        std::string cst;
        if (mac >= 0) {
            const int lb = pb.ctx_off[4 * ctx + 1];
            cst = std::string(lb, '.') + c->macrostates[mac] + std::string(Nc - lb - N, '.');
        }
        std::vector<uint8_t> blob;
        SetupError err;
        if (build_constraint(cst, Nc, blob, err)) {
            fail(err);   // the text of the ADX_ECONSTRAINT the callers return
            return -1;
        }
        DevVariant v{Nc, pb.ctx_off[4 * ctx + 1], d->n_contexts > 0 ? ctx : -1,
                     static_cast<int>(pb.cons.size()), cond == ADX_HOLO ? 1 : 0, 0};
        pb.cons.insert(pb.cons.end(), blob.begin(), blob.end());
        const int id = static_cast<int>(pb.variants.size());
        pb.variants.push_back(v);
        pb.vmac.push_back(mac);
        vindex[key] = id;
        return id;
    };
    variant(0, ADX_APO, -1);  // variant 0 = apo ensemble (calibration anchor)
    for (int k = 0; k < pb.n_ctx_eff; k++) {
        for (auto &T : c->terms) {
            const int vf = variant(k, T.condition, -1);
            if (T.kind == ADX_TERM_PAIR) {   // RnaFold::base_pair_prob of the unconstrained fold
                if (vf < 0) return ADX_ECONSTRAINT;
                int bv = -1;
                for (size_t b = 0; b < pb.bvars.size(); b++)
                    if (pb.bvars[b] == vf) bv = static_cast<int>(b);
                if (bv < 0) {
                    bv = static_cast<int>(pb.bvars.size());
                    pb.bvars.push_back(vf);
                }
                const int lb = pb.variants[vf].before_len;
                const int pidx = static_cast<int>(pb.pairs.size() / 3);
                pb.pairs.insert(pb.pairs.end(), {bv, T.pair_i + lb + 1, T.pair_j + lb + 1});
                DevTermMap m{vf, vf, T.favorable, T.weight};
                m.kind = 1;
                m.pidx = pidx;
                pb.tmap.push_back(m);
                continue;
            }
            const int vc = variant(k, T.condition, T.macrostate);
            if (vf < 0 || vc < 0) return ADX_ECONSTRAINT;
            pb.tmap.push_back(DevTermMap{vf, vc, T.favorable, T.weight});
        }
    }
    if (pb.tmap.empty()) pb.tmap.push_back(DevTermMap{0, 0, 1, 0.0});
    if (static_cast<int>(pb.variants.size()) > MAX_VARIANTS) return fail(ADX_EUNSUPPORTED, "too many fold variants");
    // moves: freely mutable positions and their closures
    for (int i = 0; i < N; i++) {
        bool free_ = std::isupper(static_cast<unsigned char>(c->templ[i])) != 0;
        for (auto &m : c->macrostates)
            if (m[i] == ')') free_ = false;
        if (free_) c->mut.push_back(i);
    }
    c->clo_off.push_back(0);
    for (int pos : c->mut) {
        std::vector<std::pair<int, int>> cl;
        const int rc = closure(c->templ, c->macrostates, pos, cl);
        c->clo_err.push_back(rc);
        if (rc == 0)
            for (auto &pp : cl) {
                c->clo_pos.push_back(pp.first);
                c->clo_par.push_back(static_cast<uint8_t>(pp.second));
            }
        c->clo_off.push_back(static_cast<int>(c->clo_pos.size()));
    }
    if (c->clo_pos.empty()) { c->clo_pos.push_back(0); c->clo_par.push_back(0); }
    s = pb.upload_all();
    if (s) return s;
    if (pb.mode == ADX_FOLD_PF) {   // the MFE tables carry no scale
        s = calibrate(pb, encode(c->templ));
        if (s) return s;
    }
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    HIP_TRY(c->d_mut.upload(c->mut.data(), c->mut.size(), pb.stream));
    HIP_TRY(c->d_clo_off.upload(c->clo_off.data(), c->clo_off.size(), pb.stream));
    HIP_TRY(c->d_clo_pos.upload(c->clo_pos.data(), c->clo_pos.size(), pb.stream));
    HIP_TRY(c->d_clo_par.upload(c->clo_par.data(), c->clo_par.size(), pb.stream));
    HIP_TRY(c->d_clo_err.upload(c->clo_err.data(), c->clo_err.size(), pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    *out = c.release();
    return ADX_OK;
}

extern "C" void adx_ctx_destroy(adx_ctx *c) { delete c; }

extern "C" adx_status adx_ctx_info(const adx_ctx *c, adx_info *info) {
    if (!c || !info) return fail(ADX_EINVAL, "adx_ctx_info: null argument");
    info->length = c->pb.Nraw;
    info->n_variants = static_cast<int>(c->pb.variants.size());
    info->n_terms = c->pb.n_terms;
    info->n_mutable = static_cast<int>(c->mut.size());
    info->max_walkers = 1 << 24;
    info->scale_per_nt = c->pb.sigma();
    return ADX_OK;
}

extern "C" adx_status adx_variant_desc(const adx_ctx *c, int v, int *ctx, int *cond, int *mac) {
    if (!c || v < 0 || v >= static_cast<int>(c->pb.variants.size())) return fail(ADX_EINVAL, "bad variant");
    const DevVariant &V = c->pb.variants[v];
    if (ctx) *ctx = V.ctx;
    if (cond) *cond = V.motif ? ADX_HOLO : ADX_APO;
    if (mac) {
        *mac = -1;
        for (size_t t = 0; t < c->pb.tmap.size(); t++)
            if (c->pb.tmap[t].vcons == v && c->pb.n_terms > 0)
                *mac = c->terms[t % c->pb.n_terms].macrostate;
    }
    return ADX_OK;
}

static void mt_seed_host(uint32_t seed, uint32_t *mt) {
    mt[0] = seed;
    for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + static_cast<uint32_t>(i);
    mt[624] = 624;
}

// Every walker's current configuration folded from scratch by the MC step's
// kernels (mc_step.hip launch_rescore): fresh scores to prop_score, term
// values to dtv (device, optional), fresh tables adopted.
static adx_status rescore_walkers(adx_ctx *c, double *dtv) {
    Problem &pb = c->pb;
    const int W = c->W;
    adx_status s = pb.prepare(W);
    if (s) return s;
    StepArgs st{};
    st.cur_seq = c->cur_seq.p;
    st.prop_seq = c->prop_seq.p;
    st.prop_score = c->prop_score.p;
    st.changed = c->changed.p;
    st.Nraw = pb.Nraw;
    st.W = W;
    pb.state_on = true;
    const KArgs ka = pb.kargs();
    pb.state_on = false;
    HIP_TRY(launch_rescore(ka, st, dtv, pb.stream));
    return ADX_OK;
}

extern "C" adx_status adx_walkers_init(adx_ctx *c, int W, const char *seqs, const uint32_t *seeds) {
    if (!c || W <= 0 || !seeds) return fail(ADX_EINVAL, "adx_walkers_init: bad argument");
    Problem &pb = c->pb;
    const int N = pb.Nraw;
    if (c->mut.empty()) return fail(ADX_EMOVE, "no freely mutable positions (vector index out of range)");
    std::vector<uint8_t> codes(size_t(W) * N);
    for (int w = 0; w < W; w++)
        for (int k = 0; k < N; k++) {
            const char ch = seqs ? seqs[size_t(w) * N + k] : c->templ[k];
            codes[size_t(w) * N + k] = static_cast<uint8_t>(base_code(ch));
        }
    std::vector<uint32_t> mt(size_t(W) * MT_WORDS);
    for (int w = 0; w < W; w++) mt_seed_host(seeds[w], &mt[size_t(w) * MT_WORDS]);
    c->W = W;
    c->step = 0;
    if (c->rec.on) c->rec.broken = true;   // new sequences outside the log
    HIP_TRY(c->cur_seq.upload(codes.data(), codes.size(), pb.stream));
    HIP_TRY(c->mtA.upload(mt.data(), mt.size(), pb.stream));
    HIP_TRY(c->mtC.upload(mt.data(), mt.size(), pb.stream));
    HIP_TRY(c->cur_score.alloc(W));
    HIP_TRY(c->last_diff.alloc(W));
    HIP_TRY(c->auto_T.alloc(W));
    HIP_TRY(c->counters.alloc(size_t(W) * 4));
    HIP_TRY(c->ntrain.alloc(W));
    HIP_TRY(c->err.alloc(W));
    HIP_TRY(c->prop_seq.alloc(size_t(W) * N));
    HIP_TRY(c->prop_score.alloc(W));
    HIP_TRY(c->temp.alloc(W));
    HIP_TRY(c->u.alloc(W));
    HIP_TRY(c->changed.alloc(W));
    HIP_TRY(c->pick.alloc(W));
    HIP_TRY(c->bcode.alloc(W));
    const int period = std::max(1, c->thermo.period);
    HIP_TRY(c->train.alloc(c->thermo.kind == ADX_THERMO_AUTO ? size_t(W) * period : 1));
    HIP_TRY(hipMemsetAsync(c->last_diff.p, 0, sizeof(double) * W, pb.stream));
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(int64_t) * W * 4, pb.stream));
    HIP_TRY(hipMemsetAsync(c->ntrain.p, 0, sizeof(int) * W, pb.stream));
    HIP_TRY(hipMemsetAsync(c->err.p, 0, sizeof(int) * W, pb.stream));
    std::vector<double> t0(W, c->thermo.t_init);
    HIP_TRY(hipMemcpyAsync(c->auto_T.p, t0.data(), sizeof(double) * W, hipMemcpyHostToDevice, pb.stream));
    // initial score (sampling.cc:40) with the MC step's own kernels; it also
    // stores the walkers' first tables
    adx_status s = pb.alloc_state(W);
    if (s) return s;
    s = rescore_walkers(c, nullptr);
    if (s) return s;
    HIP_TRY(hipMemcpyAsync(c->cur_score.p, c->prop_score.p, sizeof(double) * W, hipMemcpyDeviceToDevice, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    return ADX_OK;
}

extern "C" adx_status adx_walkers_rescore(adx_ctx *c, double *scores, double *term_values) {
    if (!c || !scores) return fail(ADX_EINVAL, "adx_walkers_rescore: null argument");
    if (c->W <= 0) return fail(ADX_ESTATE, "adx_walkers_rescore before adx_walkers_init");
    Problem &pb = c->pb;
    const int W = c->W, ntt = pb.n_terms * pb.n_ctx_eff;
    DevBuf<double> dtv;
    if (term_values && ntt > 0) HIP_TRY(dtv.alloc(size_t(W) * ntt));
    adx_status s = rescore_walkers(c, dtv.p);
    if (s) return s;
    HIP_TRY(hipMemcpyAsync(scores, c->prop_score.p, sizeof(double) * W, hipMemcpyDeviceToHost, pb.stream));
    if (dtv.p)
        HIP_TRY(hipMemcpyAsync(term_values, dtv.p, sizeof(double) * W * ntt, hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    return ADX_OK;
}

extern "C" adx_status adx_run_steps(adx_ctx *c, int steps, adx_trace *trace) {
    if (!c) return fail(ADX_EINVAL, "adx_run_steps: null context");
    if (c->W <= 0) return fail(ADX_ESTATE, "adx_run_steps before adx_walkers_init");
    if (steps <= 0) return ADX_OK;
    Problem &pb = c->pb;
    auto &rec = c->rec;
    const bool recording = rec.live();
    if (recording && steps > rec.max_steps - rec.rows)
        return fail(ADX_ESTATE, "adx_run_steps: %d steps on top of the %d recorded exceed the record's max_steps %d",
                    steps, rec.rows, rec.max_steps);
    StepArgs st{};
    st.cur_seq = c->cur_seq.p;
    st.cur_score = c->cur_score.p;
    st.mtA = c->mtA.p;
    st.mtC = c->mtC.p;
    st.counters = c->counters.p;
    st.last_diff = c->last_diff.p;
    st.auto_T = c->auto_T.p;
    st.train = c->train.p;
    st.ntrain = c->ntrain.p;
    st.err = c->err.p;
    st.prop_seq = c->prop_seq.p;
    st.prop_score = c->prop_score.p;
    st.changed = c->changed.p;
    st.chg = c->pb.dChg.p;
    st.pick = c->pick.p;
    st.bcode = c->bcode.p;
    st.temp = c->temp.p;
    st.u = c->u.p;
    st.Nraw = pb.Nraw;
    st.mut = c->d_mut.p;
    st.clo_off = c->d_clo_off.p;
    st.clo_pos = c->d_clo_pos.p;
    st.clo_par = c->d_clo_par.p;
    st.clo_err = c->d_clo_err.p;
    st.M = static_cast<int>(c->mut.size());
    st.thermo_kind = c->thermo.kind;
    st.t_fixed = c->thermo.t_fixed;
    st.t_hi = c->thermo.t_hi;
    st.t_lo = c->thermo.t_lo;
    st.cycle_len = std::max(1, c->thermo.cycle_len);
    st.ln_target_rate = std::log(c->thermo.target_rate);
    st.period = std::max(1, c->thermo.period);
    st.step0 = c->step;
    st.nsteps = steps;
    st.W = c->W;
    const int W = c->W;
    const int ntt = pb.n_terms * pb.n_ctx_eff;
    DevBuf<int32_t> tpos, tout;
    DevBuf<int8_t> tbase;
    DevBuf<double> ttemp, tprop, tcur, tu, tterms;
    const size_t R = size_t(steps) * W;
    if (recording) {   // the record's next rows; a trace reads these four back from them
        const size_t r0 = size_t(rec.rows) * W;
        st.tr_pos = rec.pos.p + r0;
        st.tr_outcome = rec.out.p + r0;
        st.tr_base = rec.base.p + r0;
        st.tr_cur = rec.cur.p + r0;
    } else if (trace) {
        HIP_TRY(tpos.alloc(R));
        HIP_TRY(tout.alloc(R));
        HIP_TRY(tbase.alloc(R));
        HIP_TRY(tcur.alloc(R));
        st.tr_pos = tpos.p;
        st.tr_outcome = tout.p;
        st.tr_base = tbase.p;
        st.tr_cur = tcur.p;
    }
    if (trace) {
        HIP_TRY(ttemp.alloc(R));
        HIP_TRY(tprop.alloc(R));
        HIP_TRY(tu.alloc(R));
        HIP_TRY(tterms.alloc(R * std::max(1, ntt)));
        st.tr_temp = ttemp.p;
        st.tr_prop = tprop.p;
        st.tr_u = tu.p;
        st.tr_terms = ntt > 0 ? tterms.p : nullptr;
    }
    // rows of a failed launch stay unwritten: the record counts as broken until the steps are in
    if (recording) rec.broken = true;
    // events around every score window (the dominant kernels) for its average duration
    Events evs;
    if (adx_status se = evs.create(4 * size_t(steps))) return se;
    HIP_TRY(hipEventRecord(c->ev0, pb.stream));
    pb.state_on = true;   // incremental folds against the walkers' stored tables
    const KArgs ka_steps = pb.kargs();
    pb.state_on = false;
    c->inside_kernel = inside_kernel_name(ka_steps);
    c->outside_kernel = outside_kernel_name(ka_steps);
    HIP_TRY(launch_steps(ka_steps, st, pb.stream, evs.v.data()));
    HIP_TRY(hipEventRecord(c->ev1, pb.stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last_ms = ms;
    double sk = 0.0, si = 0.0, so = 0.0;
    for (int k = 0; k < steps; k++) {
        float e = 0.f, b = 0.f;
        HIP_TRY(hipEventElapsedTime(&e, evs[4 * k], evs[4 * k + 3]));
        HIP_TRY(hipEventElapsedTime(&b, evs[4 * k + 1], evs[4 * k + 2]));
        sk += e;
        si += e - b;   // the window minus its outside pass (mc_step.hip launch_steps)
        so += b;
    }
    c->score_ms_total = sk;
    c->inside_ms_total = si;
    c->outside_ms_total = so;
    c->score_launches = steps;
    c->step += steps;
    std::vector<int> errs(W);
    HIP_TRY(hipMemcpy(errs.data(), c->err.p, sizeof(int) * W, hipMemcpyDeviceToHost));
    if (trace) {
        std::vector<int8_t> b(R);
        if (trace->position) HIP_TRY(hipMemcpy(trace->position, st.tr_pos, R * 4, hipMemcpyDeviceToHost));
        if (trace->outcome) HIP_TRY(hipMemcpy(trace->outcome, st.tr_outcome, R * 4, hipMemcpyDeviceToHost));
        if (trace->base) {
            HIP_TRY(hipMemcpy(b.data(), st.tr_base, R, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < R; k++) trace->base[k] = b[k] >= 1 && b[k] <= 4 ? "ACGU"[b[k] - 1] : 'N';
        }
        if (trace->temperature) HIP_TRY(hipMemcpy(trace->temperature, ttemp.p, R * 8, hipMemcpyDeviceToHost));
        if (trace->proposed_score) HIP_TRY(hipMemcpy(trace->proposed_score, tprop.p, R * 8, hipMemcpyDeviceToHost));
        if (trace->current_score) HIP_TRY(hipMemcpy(trace->current_score, st.tr_cur, R * 8, hipMemcpyDeviceToHost));
        if (trace->random_threshold) HIP_TRY(hipMemcpy(trace->random_threshold, tu.p, R * 8, hipMemcpyDeviceToHost));
        if (trace->term_values && ntt > 0)
            HIP_TRY(hipMemcpy(trace->term_values, tterms.p, R * ntt * 8, hipMemcpyDeviceToHost));
    }
    for (int w = 0; w < W; w++)
        if (errs[w]) return fail(ADX_EMOVE, "walker %d: %s", w, move_error_text(errs[w]));
    if (recording) {
        rec.rows += steps;
        rec.broken = false;
    }
    return ADX_OK;
}

extern "C" adx_status adx_last_kernel_ms(const adx_ctx *c, double *ms) {
    if (!c || !ms) return fail(ADX_EINVAL, "adx_last_kernel_ms: null argument");
    *ms = c->last_ms;
    return ADX_OK;
}

extern "C" adx_status adx_last_score_kernel_ms(const adx_ctx *c, double *avg_ms, int *launches) {
    if (!c || !avg_ms) return fail(ADX_EINVAL, "adx_last_score_kernel_ms: null argument");
    *avg_ms = c->score_launches ? c->score_ms_total / c->score_launches : 0.0;
    if (launches) *launches = c->score_launches;
    return ADX_OK;
}

extern "C" adx_status adx_last_kernel_split_ms(const adx_ctx *c, double *inside_ms, double *outside_ms) {
    if (!c || !inside_ms || !outside_ms) return fail(ADX_EINVAL, "adx_last_kernel_split_ms: null argument");
    const int n = c->score_launches;
    *inside_ms = n ? c->inside_ms_total / n : 0.0;
    *outside_ms = n ? c->outside_ms_total / n : 0.0;
    return ADX_OK;
}

extern "C" adx_status adx_last_kernel_names(const adx_ctx *c, char *inside, int inside_len, char *outside,
                                            int outside_len) {
    if (!c || !inside || !outside || inside_len <= 0 || outside_len <= 0)
        return fail(ADX_EINVAL, "adx_last_kernel_names: bad argument");
    std::snprintf(inside, size_t(inside_len), "%s", c->inside_kernel.c_str());
    std::snprintf(outside, size_t(outside_len), "%s", c->outside_kernel.c_str());
    return ADX_OK;
}

extern "C" adx_status adx_walkers_download(adx_ctx *c, char *seqs, double *scores, int64_t *counters) {
    if (!c) return fail(ADX_EINVAL, "adx_walkers_download: null context");
    if (c->W <= 0) return fail(ADX_ESTATE, "no walkers");
    const int W = c->W, N = c->pb.Nraw;
    HIP_TRY(hipStreamSynchronize(c->pb.stream));
    if (seqs) {
        std::vector<uint8_t> codes(size_t(W) * N);
        HIP_TRY(hipMemcpy(codes.data(), c->cur_seq.p, codes.size(), hipMemcpyDeviceToHost));
        for (int w = 0; w < W; w++)
            for (int k = 0; k < N; k++) {
                const uint8_t b = codes[size_t(w) * N + k];
                char ch = b >= 1 && b <= 4 ? "ACGU"[b - 1] : 'N';
                if (std::islower(static_cast<unsigned char>(c->templ[k])))
                    ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
                seqs[size_t(w) * N + k] = ch;
            }
    }
    if (scores) HIP_TRY(hipMemcpy(scores, c->cur_score.p, sizeof(double) * W, hipMemcpyDeviceToHost));
    if (counters) HIP_TRY(hipMemcpy(counters, c->counters.p, sizeof(int64_t) * W * 4, hipMemcpyDeviceToHost));
    return ADX_OK;
}

extern "C" adx_status adx_walkers_export(adx_ctx *c, void *dev_seqs, void *dev_scores) {
    if (!c) return fail(ADX_EINVAL, "adx_walkers_export: null context");
    if (c->W <= 0) return fail(ADX_ESTATE, "no walkers");
    const size_t W = size_t(c->W), N = size_t(c->pb.Nraw);
    if (dev_seqs) HIP_TRY(hipMemcpyAsync(dev_seqs, c->cur_seq.p, W * N, hipMemcpyDeviceToDevice, c->pb.stream));
    if (dev_scores)
        HIP_TRY(hipMemcpyAsync(dev_scores, c->cur_score.p, W * sizeof(double), hipMemcpyDeviceToDevice, c->pb.stream));
    HIP_TRY(hipStreamSynchronize(c->pb.stream));
    return ADX_OK;
}

// `a` waits (on the device) for the work queued on `b` so far
static hipError_t stream_after(hipStream_t a, hipStream_t b) {
    hipEvent_t ev;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    e = hipEventRecord(ev, b);
    if (e == hipSuccess) e = hipStreamWaitEvent(a, ev, 0);
    (void)hipEventDestroy(ev);
    return e;
}

extern "C" adx_status adx_walkers_export_on(adx_ctx *c, void *dev_seqs, void *dev_scores, void *stream) {
    if (!c) return fail(ADX_EINVAL, "adx_walkers_export_on: null context");
    if (c->W <= 0) return fail(ADX_ESTATE, "no walkers");
    const size_t W = size_t(c->W), N = size_t(c->pb.Nraw);
    const hipStream_t other = hipStream_t(stream);   // NULL: the null stream, a valid handle
    // the caller's earlier reads of the buffers finish before the copies overwrite them
    HIP_TRY(stream_after(c->pb.stream, other));
    if (dev_seqs) HIP_TRY(hipMemcpyAsync(dev_seqs, c->cur_seq.p, W * N, hipMemcpyDeviceToDevice, c->pb.stream));
    if (dev_scores)
        HIP_TRY(hipMemcpyAsync(dev_scores, c->cur_score.p, W * sizeof(double), hipMemcpyDeviceToDevice, c->pb.stream));
    // and the caller's later work on `stream` sees them
    HIP_TRY(stream_after(other, c->pb.stream));
    return ADX_OK;
}

// The copies and resets of an import, queued on the engine stream (both import
// entry points: they differ only in how they order against the caller)
static hipError_t import_queue(adx_ctx *c, const void *dev_seqs, const void *dev_scores) {
    const size_t W = size_t(c->W), N = size_t(c->pb.Nraw);
    hipError_t e = hipSuccess;
    if (c->rec.on) c->rec.broken = true;   // the configurations change outside the log
    if (dev_seqs) e = hipMemcpyAsync(c->cur_seq.p, dev_seqs, W * N, hipMemcpyDeviceToDevice, c->pb.stream);
    if (e == hipSuccess && dev_scores)
        e = hipMemcpyAsync(c->cur_score.p, dev_scores, W * sizeof(double), hipMemcpyDeviceToDevice, c->pb.stream);
    if (e == hipSuccess && dev_seqs && c->pb.dValid.p)   // new configurations: their next fold starts from scratch
        e = hipMemsetAsync(c->pb.dValid.p, 0, W, c->pb.stream);
    return e;
}

extern "C" adx_status adx_walkers_import_after(adx_ctx *c, const void *dev_seqs, const void *dev_scores,
                                               void *producer_stream) {
    if (!c) return fail(ADX_EINVAL, "adx_walkers_import_after: null context");
    if (c->W <= 0) return fail(ADX_ESTATE, "no walkers");
    // NULL is the null stream (torch's default stream), not "no producer": the
    // engine stream is non-blocking and would not otherwise wait for it
    const hipStream_t other = hipStream_t(producer_stream);
    HIP_TRY(stream_after(c->pb.stream, other));
    HIP_TRY(import_queue(c, dev_seqs, dev_scores));
    // the producer's later writes to the buffers wait for the copies
    HIP_TRY(stream_after(other, c->pb.stream));
    return ADX_OK;
}

extern "C" adx_status adx_walkers_import(adx_ctx *c, const void *dev_seqs, const void *dev_scores) {
    if (!c) return fail(ADX_EINVAL, "adx_walkers_import: null context");
    if (c->W <= 0) return fail(ADX_ESTATE, "no walkers");
    HIP_TRY(import_queue(c, dev_seqs, dev_scores));
    HIP_TRY(hipStreamSynchronize(c->pb.stream));
    return ADX_OK;
}

extern "C" adx_status adx_set_temperature(adx_ctx *c, double t) {
    if (!c) return fail(ADX_EINVAL, "adx_set_temperature: null context");
    if (c->thermo.kind != ADX_THERMO_FIXED) return fail(ADX_EINVAL, "adx_set_temperature: not a fixed thermostat");
    c->thermo.t_fixed = t;
    return ADX_OK;
}

// the variant that folds (context, condition) without a constraint, or -1
static int free_fold_variant(const adx_ctx *c, int condition, int context) {
    const Problem &pb = c->pb;
    const int want_ctx = c->n_contexts > 0 ? context : -1;
    int v = -1;
    for (size_t k = 0; k < pb.variants.size(); k++)
        if (pb.variants[k].ctx == want_ctx && pb.vmac[k] == -1 && pb.variants[k].motif == (condition == ADX_HOLO ? 1 : 0))
            v = static_cast<int>(k);
    return v;
}

extern "C" adx_status adx_bppm_batch(adx_ctx *c, int W, const char *seqs, int condition, int context,
                                      double *probs) {
    if (!c || W <= 0 || !seqs || !probs) return fail(ADX_EINVAL, "adx_bppm_batch: bad argument");
    Problem &pb = c->pb;
    if (pb.mode != ADX_FOLD_PF) return fail(ADX_EUNSUPPORTED, "adx_bppm_batch: partition-function contexts only");
    const int v = free_fold_variant(c, condition, context);
    if (v < 0) return fail(ADX_EINVAL, "adx_bppm_batch: the objective has no (context %d, condition %d) fold", context, condition);
    const int L = pb.variants[v].N;
    DevBuf<uint8_t> dseq;
    DevBuf<int> dbv;
    DevBuf<double> dfull;
    DevBuf<char> dscr;
    KArgs ka;
    adx_status s = upload_codes(seqs, size_t(W) * pb.Nraw, dseq, pb.stream);
    if (!s) s = pb.free_outside_args(v, W, dbv, dscr, ka);
    if (s) return s;
    HIP_TRY(dfull.alloc(size_t(W) * L * L));
    HIP_TRY(hipMemsetAsync(dfull.p, 0, sizeof(double) * W * L * L, pb.stream));
    HIP_TRY(launch_bppm(ka, dseq.p, W, nullptr, dfull.p, L, nullptr, ka.bppm_scratch, pb.stream));
    HIP_TRY(hipMemcpyAsync(probs, dfull.p, sizeof(double) * W * L * L, hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    return ADX_OK;
}

// MFE structures of W device sequences for variant v, copied to the host
static adx_status mfe_structures(adx_ctx *c, const char *who, const uint8_t *dseqs, int W, int v, char *structures,
                                 float *energies) {
    Problem &pb = c->pb;
    if (pb.mode != ADX_FOLD_MFE)
        return fail(ADX_EUNSUPPORTED, "%s: ADX_FOLD_MFE contexts only (a partition-function context holds no "
                    "energies; use adx_fold_mfe_structure)", who);
    if (v < 0 || v >= static_cast<int>(pb.variants.size()))
        return fail(ADX_EINVAL, "%s: variant %d outside [0, %zu)", who, v, pb.variants.size());
    const size_t L = size_t(pb.variants[v].N);
    DevBuf<char> dst;
    DevBuf<float> de;
    HIP_TRY(dst.alloc(size_t(W) * L));
    HIP_TRY(de.alloc(W));
    adx_status s = pb.trace(dseqs, W, v, dst.p, de.p);
    if (s) return s;
    HIP_TRY(hipMemcpyAsync(structures, dst.p, size_t(W) * L, hipMemcpyDeviceToHost, pb.stream));
    if (energies) HIP_TRY(hipMemcpyAsync(energies, de.p, sizeof(float) * W, hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    return ADX_OK;
}

extern "C" adx_status adx_mfe_structure_batch(adx_ctx *c, int W, const char *seqs, int variant, char *structures,
                                              float *energies) {
    if (!c || W <= 0 || !seqs || !structures) return fail(ADX_EINVAL, "adx_mfe_structure_batch: bad argument");
    Problem &pb = c->pb;
    DevBuf<uint8_t> dseq;
    if (adx_status su = upload_codes(seqs, size_t(W) * pb.Nraw, dseq, pb.stream)) return su;
    return mfe_structures(c, "adx_mfe_structure_batch", dseq.p, W, variant, structures, energies);
}

extern "C" adx_status adx_walkers_mfe_structures(adx_ctx *c, int variant, char *structures, float *energies) {
    if (!c || !structures) return fail(ADX_EINVAL, "adx_walkers_mfe_structures: null argument");
    if (c->pb.mode == ADX_FOLD_MFE && c->W <= 0)
        return fail(ADX_ESTATE, "adx_walkers_mfe_structures before adx_walkers_init");
    return mfe_structures(c, "adx_walkers_mfe_structures", c->cur_seq.p, c->W, variant, structures, energies);
}

// Zuker suboptimal structures of W device sequences for variant v, copied to the host
static adx_status subopt_structures(adx_ctx *c, const char *who, const uint8_t *dseqs, int W, int v, double delta_kcal,
                                    int max_structs, const SuboptOut &h) {
    Problem &pb = c->pb;
    if (pb.mode != ADX_FOLD_MFE)
        return fail(ADX_EUNSUPPORTED, "%s: ADX_FOLD_MFE contexts only (a partition-function context holds no "
                    "energies; use adx_fold_subopt_structures)", who);
    if (v < 0 || v >= static_cast<int>(pb.variants.size()))
        return fail(ADX_EINVAL, "%s: variant %d outside [0, %zu)", who, v, pb.variants.size());
    if (!subopt_args_ok(delta_kcal, max_structs))
        return fail(ADX_EINVAL, "%s: delta %g < 0 or max_structs %d < 1", who, delta_kcal, max_structs);
    const size_t L = size_t(pb.variants[v].N);
    if (size_t(W) > SIZE_MAX / L / std::max(L, size_t(max_structs)) / sizeof(float))
        return fail(ADX_EINVAL, "%s: %d x %d structures of %zu chars overflow", who, W, max_structs, L);
    return pb.subopt(dseqs, W, v, delta_kcal, max_structs, h);
}

extern "C" adx_status adx_subopt_structures_batch(adx_ctx *c, int W, const char *seqs, int variant, double delta_kcal,
                                                  int max_structs, int *n_found, int *n_pairs_within, float *mfe_kcal,
                                                  char *structures, float *energies, int *seeds, float *pair_energy) {
    if (!c || W <= 0 || !seqs || !n_found || !mfe_kcal || !structures || !energies)
        return fail(ADX_EINVAL, "adx_subopt_structures_batch: bad argument");
    Problem &pb = c->pb;
    DevBuf<uint8_t> dseq;
    if (adx_status su = upload_codes(seqs, size_t(W) * pb.Nraw, dseq, pb.stream)) return su;
    return subopt_structures(c, "adx_subopt_structures_batch", dseq.p, W, variant, delta_kcal, max_structs,
                             SuboptOut{n_found, n_pairs_within, mfe_kcal, structures, energies, seeds, pair_energy});
}

extern "C" adx_status adx_walkers_subopt_structures(adx_ctx *c, int variant, double delta_kcal, int max_structs,
                                                    int *n_found, int *n_pairs_within, float *mfe_kcal,
                                                    char *structures, float *energies, int *seeds, float *pair_energy) {
    if (!c || !n_found || !mfe_kcal || !structures || !energies)
        return fail(ADX_EINVAL, "adx_walkers_subopt_structures: null argument");
    if (c->pb.mode == ADX_FOLD_MFE && c->W <= 0)
        return fail(ADX_ESTATE, "adx_walkers_subopt_structures before adx_walkers_init");
    return subopt_structures(c, "adx_walkers_subopt_structures", c->cur_seq.p, c->W, variant, delta_kcal, max_structs,
                             SuboptOut{n_found, n_pairs_within, mfe_kcal, structures, energies, seeds, pair_energy});
}

extern "C" adx_status adx_last_subopt_ms(const adx_ctx *c, double *fill_ms, double *select_ms) {
    if (!c || !fill_ms || !select_ms) return fail(ADX_EINVAL, "adx_last_subopt_ms: null argument");
    *fill_ms = c->pb.subopt_fill_ms;
    *select_ms = c->pb.subopt_select_ms;
    return ADX_OK;
}

// n_samples structures per device sequence for variant v, drawn from its ensemble
static adx_status sample_structures(adx_ctx *c, const char *who, const uint8_t *dseqs, int W, int v, int n_samples,
                                    uint64_t seed, char *structures, float *energies) {
    Problem &pb = c->pb;
    if (pb.mode != ADX_FOLD_PF)
        return fail(ADX_EUNSUPPORTED, "%s: ADX_FOLD_PF contexts only (an MFE context holds no Boltzmann "
                    "factors; use adx_fold_sample_structures)", who);
    if (v < 0 || v >= static_cast<int>(pb.variants.size()))
        return fail(ADX_EINVAL, "%s: variant %d outside [0, %zu)", who, v, pb.variants.size());
    if (n_samples < 1) return fail(ADX_EINVAL, "%s: n_samples %d < 1", who, n_samples);
    const size_t L = size_t(pb.variants[v].N);
    if (size_t(W) > SIZE_MAX / L / size_t(n_samples))
        return fail(ADX_EINVAL, "%s: %d x %d structures of %zu chars overflow", who, W, n_samples, L);
    return pb.sample(who, dseqs, W, v, n_samples, seed, structures, energies);
}

extern "C" adx_status adx_sample_structures_batch(adx_ctx *c, int W, const char *seqs, int variant, int n_samples,
                                                  uint64_t seed, char *structures, float *energies) {
    if (!c || W <= 0 || !seqs || !structures) return fail(ADX_EINVAL, "adx_sample_structures_batch: bad argument");
    Problem &pb = c->pb;
    DevBuf<uint8_t> dseq;
    if (adx_status su = upload_codes(seqs, size_t(W) * pb.Nraw, dseq, pb.stream)) return su;
    return sample_structures(c, "adx_sample_structures_batch", dseq.p, W, variant, n_samples, seed, structures,
                             energies);
}

extern "C" adx_status adx_walkers_sample_structures(adx_ctx *c, int variant, int n_samples, uint64_t seed,
                                                    char *structures, float *energies) {
    if (!c || !structures) return fail(ADX_EINVAL, "adx_walkers_sample_structures: null argument");
    if (c->pb.mode == ADX_FOLD_PF && c->W <= 0)
        return fail(ADX_ESTATE, "adx_walkers_sample_structures before adx_walkers_init");
    return sample_structures(c, "adx_walkers_sample_structures", c->cur_seq.p, c->W, variant, n_samples, seed,
                             structures, energies);
}

extern "C" adx_status adx_last_sample_ms(const adx_ctx *c, double *fill_ms, double *sample_ms) {
    if (!c || !fill_ms || !sample_ms) return fail(ADX_EINVAL, "adx_last_sample_ms: null argument");
    *fill_ms = c->pb.sample_fill_ms;
    *sample_ms = c->pb.sample_draw_ms;
    return ADX_OK;
}

// energies, probabilities and status bytes of n_per structures per device sequence for variant v
static adx_status eval_structures(adx_ctx *c, const char *who, const uint8_t *dseqs, int W, int v, int n_per,
                                  const char *structures, bool shared, double *energies, double *probs,
                                  uint8_t *status) {
    Problem &pb = c->pb;
    if (v < 0 || v >= static_cast<int>(pb.variants.size()))
        return fail(ADX_EINVAL, "%s: variant %d outside [0, %zu)", who, v, pb.variants.size());
    if (n_per < 1) return fail(ADX_EINVAL, "%s: %d structures per sequence < 1", who, n_per);
    if (probs && pb.mode != ADX_FOLD_PF)
        return fail(ADX_EUNSUPPORTED, "%s: probabilities on ADX_FOLD_PF contexts only (an MFE context holds no "
                    "Boltzmann factors; use adx_fold_eval_structures)", who);
    const size_t L = size_t(pb.variants[v].N);
    if (size_t(W) > SIZE_MAX / L / size_t(n_per) / sizeof(double))
        return fail(ADX_EINVAL, "%s: %d x %d structures of %zu chars overflow", who, W, n_per, L);
    return pb.eval_structures(dseqs, W, v, n_per, structures, shared, energies, probs, status);
}

extern "C" adx_status adx_eval_structures_batch(adx_ctx *c, int W, const char *seqs, int variant, int n_per_seq,
                                                const char *structures, double *energies, double *probs,
                                                uint8_t *status) {
    if (!c || W <= 0 || !seqs || !structures || !energies)
        return fail(ADX_EINVAL, "adx_eval_structures_batch: bad argument");
    Problem &pb = c->pb;
    DevBuf<uint8_t> dseq;
    if (adx_status su = upload_codes(seqs, size_t(W) * pb.Nraw, dseq, pb.stream)) return su;
    return eval_structures(c, "adx_eval_structures_batch", dseq.p, W, variant, n_per_seq, structures, false, energies,
                           probs, status);
}

extern "C" adx_status adx_walkers_eval_structures(adx_ctx *c, int variant, int n_structs, const char *structures,
                                                  double *energies, double *probs, uint8_t *status) {
    if (!c || !structures || !energies) return fail(ADX_EINVAL, "adx_walkers_eval_structures: null argument");
    if (c->W <= 0) return fail(ADX_ESTATE, "adx_walkers_eval_structures before adx_walkers_init");
    return eval_structures(c, "adx_walkers_eval_structures", c->cur_seq.p, c->W, variant, n_structs, structures, true,
                           energies, probs, status);
}

extern "C" adx_status adx_last_eval_ms(const adx_ctx *c, double *fill_ms, double *eval_ms) {
    if (!c || !fill_ms || !eval_ms) return fail(ADX_EINVAL, "adx_last_eval_ms: null argument");
    *fill_ms = c->pb.eval_fill_ms;
    *eval_ms = c->pb.eval_ms;
    return ADX_OK;
}

// unpaired-region probabilities of W device sequences for variant v
static adx_status unpaired_probs(adx_ctx *c, const char *who, const uint8_t *dseqs, int W, int v, int max_len,
                                 int n_regions, const int *regions, double *profile, double *region_probs,
                                 float *energies) {
    Problem &pb = c->pb;
    if (pb.mode != ADX_FOLD_PF)
        return fail(ADX_EUNSUPPORTED, "%s: ADX_FOLD_PF contexts only (an MFE context holds no Boltzmann "
                    "factors; use adx_fold_unpaired_probs)", who);
    if (v < 0 || v >= static_cast<int>(pb.variants.size()))
        return fail(ADX_EINVAL, "%s: variant %d outside [0, %zu)", who, v, pb.variants.size());
    if (!profile && !region_probs) return fail(ADX_EINVAL, "%s: neither a profile nor region probabilities asked for", who);
    const int L = pb.variants[v].N;
    if (!region_probs) n_regions = 0;
    if (region_probs && n_regions < 1) return fail(ADX_EINVAL, "%s: region_probs without regions", who);
    if (!unpaired_args_ok(L, max_len, profile != nullptr, n_regions, regions))
        return fail(ADX_EINVAL, "%s: max_len %d outside [%d, %d], or a region outside [0, %d) or of length < 1", who,
                    max_len, profile ? 1 : 0, L, L);
    if (size_t(W) > SIZE_MAX / sizeof(double) / size_t(L) / size_t(std::max(max_len, 1)))
        return fail(ADX_EINVAL, "%s: %d profiles of %d x %d overflow", who, W, max_len, L);
    return pb.unpaired(dseqs, W, v, max_len, n_regions, regions, profile, region_probs, nullptr, energies);
}

extern "C" adx_status adx_unpaired_probs_batch(adx_ctx *c, int W, const char *seqs, int variant, int max_len,
                                               int n_regions, const int *regions, double *profile,
                                               double *region_probs, float *energies) {
    if (!c || W <= 0 || !seqs) return fail(ADX_EINVAL, "adx_unpaired_probs_batch: bad argument");
    Problem &pb = c->pb;
    DevBuf<uint8_t> dseq;
    if (adx_status su = upload_codes(seqs, size_t(W) * pb.Nraw, dseq, pb.stream)) return su;
    return unpaired_probs(c, "adx_unpaired_probs_batch", dseq.p, W, variant, max_len, n_regions, regions, profile,
                          region_probs, energies);
}

extern "C" adx_status adx_walkers_unpaired_probs(adx_ctx *c, int variant, int max_len, int n_regions,
                                                 const int *regions, double *profile, double *region_probs,
                                                 float *energies) {
    if (!c) return fail(ADX_EINVAL, "adx_walkers_unpaired_probs: null argument");
    if (c->pb.mode == ADX_FOLD_PF && c->W <= 0)
        return fail(ADX_ESTATE, "adx_walkers_unpaired_probs before adx_walkers_init");
    return unpaired_probs(c, "adx_walkers_unpaired_probs", c->cur_seq.p, c->W, variant, max_len, n_regions, regions,
                          profile, region_probs, energies);
}

extern "C" adx_status adx_last_unpaired_ms(const adx_ctx *c, double *fill_ms, double *outside_ms) {
    if (!c || !fill_ms || !outside_ms) return fail(ADX_EINVAL, "adx_last_unpaired_ms: null argument");
    *fill_ms = c->pb.access_fill_ms;
    *outside_ms = c->pb.access_outside_ms;
    return ADX_OK;
}

// centroid and MEA structures of W device sequences for the (context, condition) unconstrained fold
static adx_status ensemble_structures(adx_ctx *c, const char *who, const uint8_t *dseqs, int W, int condition,
                                      int context, double gamma, char *centroid, char *mea,
                                      adx_ensemble_stats *stats, double *probs) {
    Problem &pb = c->pb;
    if (!ensemble_args_ok(gamma, centroid, mea, stats))
        return fail(ADX_EINVAL, "%s: gamma %g not finite and > 0, or nothing to return", who, gamma);
    if (pb.mode != ADX_FOLD_PF) return fail(ADX_EUNSUPPORTED, "%s: partition-function contexts only", who);
    const int v = free_fold_variant(c, condition, context);
    if (v < 0) return fail(ADX_EINVAL, "%s: the objective has no (context %d, condition %d) fold", who, context, condition);
    return pb.ensemble(dseqs, W, v, gamma, centroid, mea, stats, probs);
}

extern "C" adx_status adx_ensemble_structures_batch(adx_ctx *c, int W, const char *seqs, int condition, int context,
                                                    double gamma, char *centroid, char *mea,
                                                    adx_ensemble_stats *stats, double *probs) {
    if (!c || W <= 0 || !seqs) return fail(ADX_EINVAL, "adx_ensemble_structures_batch: bad argument");
    Problem &pb = c->pb;
    DevBuf<uint8_t> dseq;
    if (adx_status su = upload_codes(seqs, size_t(W) * pb.Nraw, dseq, pb.stream)) return su;
    return ensemble_structures(c, "adx_ensemble_structures_batch", dseq.p, W, condition, context, gamma, centroid, mea,
                               stats, probs);
}

extern "C" adx_status adx_walkers_ensemble_structures(adx_ctx *c, int condition, int context, double gamma,
                                                      char *centroid, char *mea, adx_ensemble_stats *stats,
                                                      double *probs) {
    if (!c) return fail(ADX_EINVAL, "adx_walkers_ensemble_structures: null context");
    if (c->pb.mode == ADX_FOLD_PF && c->W <= 0)
        return fail(ADX_ESTATE, "adx_walkers_ensemble_structures before adx_walkers_init");
    return ensemble_structures(c, "adx_walkers_ensemble_structures", c->cur_seq.p, c->W, condition, context, gamma,
                               centroid, mea, stats, probs);
}

extern "C" adx_status adx_last_ensemble_ms(const adx_ctx *c, double *bppm_ms, double *struct_ms) {
    if (!c || !bppm_ms || !struct_ms) return fail(ADX_EINVAL, "adx_last_ensemble_ms: null argument");
    *bppm_ms = c->pb.ens_bppm_ms;
    *struct_ms = c->pb.ens_struct_ms;
    return ADX_OK;
}

extern "C" adx_status adx_score_batch(adx_ctx *c, int W, const char *seqs, double *scores,
                                      double *term_values, float *dG) {
    if (!c || W <= 0 || !seqs || !scores) return fail(ADX_EINVAL, "adx_score_batch: bad argument");
    Problem &pb = c->pb;
    const int V = static_cast<int>(pb.variants.size());
    const int ntt = pb.n_terms * pb.n_ctx_eff;
    DevBuf<uint8_t> dseq;
    DevBuf<double> dsc, dterms;
    DevBuf<float> ddg;
    adx_status s = upload_codes(seqs, size_t(W) * pb.Nraw, dseq, pb.stream);
    if (s) return s;
    HIP_TRY(dsc.alloc(W));
    HIP_TRY(dterms.alloc(size_t(W) * std::max(1, ntt)));
    HIP_TRY(ddg.alloc(size_t(W) * V));
    HIP_TRY(hipEventRecord(c->ev0, pb.stream));
    s = pb.score(dseq.p, W, dsc.p, ntt > 0 ? dterms.p : nullptr, ddg.p);
    if (s) return s;
    HIP_TRY(hipEventRecord(c->ev1, pb.stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last_ms = ms;
    HIP_TRY(hipMemcpy(scores, dsc.p, sizeof(double) * W, hipMemcpyDeviceToHost));
    if (term_values && ntt > 0)
        HIP_TRY(hipMemcpy(term_values, dterms.p, sizeof(double) * W * ntt, hipMemcpyDeviceToHost));
    if (dG) HIP_TRY(hipMemcpy(dG, ddg.p, sizeof(float) * W * V, hipMemcpyDeviceToHost));
    return ADX_OK;
}
