// Monte Carlo sampling (reference src/sampling.cc semantics): the
// single-walker reference loop, and the batched path over the fused GPU
// engine (adx_ctx_* / adx_run_steps) for built-in setups.
#include "addapt/sampling.hh"

#include <algorithm>
#include <cctype>
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <functional>
#include <iostream>
#include <limits>
#include <unistd.h>

#include "gpu.hh"

namespace addapt {

static string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
static string fmt(const char *f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// ---------------------------------------------------------------- moves
bool can_be_mutated(DeviceConstPtr device, int i) { return std::isupper(static_cast<unsigned char>(device->seq()[i])) != 0; }

bool can_be_freely_mutated(DeviceConstPtr device, int i) {
    if (!can_be_mutated(device, i)) return false;
    for (auto &m : device->macrostates())
        if (m.second[i] == ')') return false;   // mutated as a unit with its '(' partner
    return true;
}

static void mutate_rec(DevicePtr device, int pos, char base, std::vector<bool> &done) {
    device->mutate(pos, base);
    done[pos] = true;
    for (auto &m : device->macrostates()) {
        const string &ms = m.second;
        int step;
        char open, close;
        if (ms[pos] == '(') { open = '('; close = ')'; step = 1; }
        else if (ms[pos] == ')') { open = ')'; close = '('; step = -1; }
        else continue;
        int level = 1, partner = pos;
        while (level != 0) {
            partner += step;
            if (partner < 0 || partner >= static_cast<int>(ms.size()))
                throw fmt("mismatched base-pair in '%s' macrostate: '%s'", m.first.c_str(), ms.c_str());
            level += ms[partner] == open;
            level -= ms[partner] == close;
        }
        if (!can_be_mutated(device, partner))
            throw fmt("position '%d' can be mutated, but it's base-paired to position '%d' which can't be.", pos, partner);
        const char comp = COMPLEMENTARY_NUCS.at(base);
        if (!done[partner]) mutate_rec(device, partner, comp, done);
        else if (device->seq()[partner] != comp) throw string("no way to satisfy all base pairing constraints.");
    }
}

void mutate_recursively(DevicePtr device, int i, char base) {
    std::vector<bool> done(device->len(), false);
    mutate_rec(device, i, base, done);
}

void UnbiasedMutationMove::apply(DevicePtr device, std::mt19937 &rng) const {
    std::vector<int> free_pos;
    for (int i = 0; i < device->len(); i++)
        if (can_be_freely_mutated(device, i)) free_pos.push_back(i);
    if (free_pos.empty()) throw string("no freely mutable positions");
    const int pick = free_pos[std::uniform_int_distribution<>(0, int(free_pos.size()) - 1)(rng)];
    const char base = "ACGU"[std::uniform_int_distribution<>(0, 3)(rng)];
    mutate_recursively(device, pick, base);
}

// ---------------------------------------------------------------- thermostats
double AnnealingThermostat::adjust(MonteCarloStep const &step) {
    return ((lo_ - hi_) / n_) * (step.i % n_) + hi_;
}

double AutoScalingThermostat::adjust(MonteCarloStep const &step) {
    train_.push_back(step.score_diff);
    if (train_.size() >= period_) {
        const size_t n = train_.size() / 2;
        std::nth_element(train_.begin(), train_.begin() + n, train_.end());
        t_ = std::max(train_[n] / std::log(rate_), 0.0);
        train_.clear();
    }
    return t_;
}

// ---------------------------------------------------------------- reporters
void ProgressReporter::update(MonteCarloStep const &step) {
    if (!isatty(fileno(stdout))) return;
    std::cout << "\033[2K\r[" << step.i + 1 << "/" << step.num_steps << "]";
    if (step.i + 1 == step.num_steps) std::cout << std::endl;
    else std::cout << std::flush;
}

void TsvTrajectoryReporter::start(MonteCarloStep const &step) {
    tsv_.open(path_);
    if (!tsv_.is_open()) throw fmt("couldn't open '%s' for writing", path_.c_str());
    tsv_ << "#\tinitial_seq\t" << step.current_device->seq() << "\n";
    tsv_ << "step\tnum_steps\tcurrent_score\tproposed_score\t";
    for (auto &row : step.score_table) tsv_ << "term_weight[" << row.name << "]\tterm_value[" << row.name << "]\t";
    tsv_ << "score_diff\ttemperature\tmetropolis_criterion\trandom_threshold\tmove\toutcome\tcurrent_seq\tproposed_seq\t"
         << std::endl;
}

void TsvTrajectoryReporter::update(MonteCarloStep const &step) {
    if (step.i % interval_ != 0) return;
    tsv_ << step.i << "\t" << step.num_steps << "\t" << step.current_score << "\t" << step.proposed_score << "\t";
    for (auto &row : step.score_table) tsv_ << row.weight << "\t" << row.term << "\t";
    tsv_ << step.score_diff << "\t" << step.temperature << "\t" << step.metropolis_criterion << "\t"
         << step.random_threshold << "\t" << step.move->name() << "\t" << step.outcome << "\t"
         << step.current_device->seq() << "\t" << step.proposed_device->seq() << "\t" << std::endl;
}

void TsvTrajectoryReporter::finish(MonteCarloStep const &) { tsv_.close(); }

// ---------------------------------------------------------------- reference loop
MonteCarlo::MonteCarlo()
    : steps_(0), thermostat_(std::make_shared<FixedThermostat>(1)), scorefxn_(std::make_shared<ScoreFunction>()) {}

// sampling.cc:22-107.  The move draws from `rng` itself; the move picker and
// the Metropolis uniform draw from copies of its state at entry (std::bind
// copies the engine), exactly as the reference.
DevicePtr MonteCarlo::apply(DevicePtr device, std::mt19937 &rng) const {
    if (moves_.empty()) return device;
    MonteCarloStep step;
    step.num_steps = steps_;
    step.i = -1;
    step.current_device = device;
    auto random = std::bind(std::uniform_real_distribution<>(), rng);
    auto randmove = std::bind(std::uniform_int_distribution<>(0, int(moves_.size()) - 1), rng);
    step.current_score = scorefxn_->evaluate(step.current_device, step.score_table);
    step.proposed_score = step.current_score;
    for (auto o : {OutcomeEnum::REJECT, OutcomeEnum::ACCEPT_WORSENED, OutcomeEnum::ACCEPT_UNCHANGED,
                   OutcomeEnum::ACCEPT_IMPROVED})
        step.outcome_counters[o] = 0;
    for (auto &r : reporters_) r->start(step);
    for (step.i = 0; step.i < step.num_steps; step.i++) {
        step.temperature = thermostat_->adjust(step);
        step.proposed_device = step.current_device->copy();
        step.move = moves_[randmove()];
        step.move->apply(step.proposed_device, rng);
        if (step.current_device->seq() == step.proposed_device->seq()) {
            step.outcome = OutcomeEnum::ACCEPT_UNCHANGED;
        } else {
            step.proposed_score = scorefxn_->evaluate(step.proposed_device, step.score_table);
            step.score_diff = step.proposed_score - step.current_score;
            step.metropolis_criterion = std::exp(step.score_diff / step.temperature);
            step.random_threshold = random();
            if (step.metropolis_criterion < step.random_threshold) {
                step.outcome = OutcomeEnum::REJECT;
            } else {
                step.outcome = step.score_diff > 0 ? OutcomeEnum::ACCEPT_IMPROVED : OutcomeEnum::ACCEPT_WORSENED;
                step.current_device = step.proposed_device;
                step.current_score = step.proposed_score;
            }
        }
        step.outcome_counters[step.outcome] += 1;
        for (auto &r : reporters_) r->update(step);
    }
    for (auto &r : reporters_) r->finish(step);
    return step.current_device;
}

// ---------------------------------------------------------------- GPU engine path
bool MonteCarlo::gpu_expressible() const {
    if (moves_.size() != 1 || !std::dynamic_pointer_cast<UnbiasedMutationMove>(moves_[0])) return false;
    if (!std::dynamic_pointer_cast<FixedThermostat>(thermostat_) &&
        !std::dynamic_pointer_cast<AnnealingThermostat>(thermostat_) &&
        !std::dynamic_pointer_cast<AutoScalingThermostat>(thermostat_))
        return false;
    if (scorefxn_->terms().empty()) return false;
    for (auto &t : scorefxn_->terms())
        if (!std::dynamic_pointer_cast<MacrostateProbTerm>(t)) return false;
    return true;
}

namespace {
struct EngineSetup {
    std::vector<string> names, macro;
    std::vector<const char *> macro_c;
    std::vector<adx_term> terms;
    std::vector<string> ctx_b, ctx_a;
    std::vector<adx_context_desc> ctx;
    string seq, apt_seq, apt_fold;
    adx_run_desc d{};
};

void build_setup(const MonteCarlo &mc, DeviceConstPtr device, int g, EngineSetup &e) {
    if (device->context() && (!device->context()->before().empty() || !device->context()->after().empty()))
        throw string("the engine folds devices without a context (contexts belong to the score function)");
    e.seq = device->raw_seq();
    e.names = device->macrostate_names();
    for (auto &n : e.names) e.macro.push_back(device->macrostate(n));
    for (auto &m : e.macro) e.macro_c.push_back(m.c_str());
    for (auto &t : mc.scorefxn()->terms()) {
        auto m = std::dynamic_pointer_cast<MacrostateProbTerm>(t);
        auto it = std::find(e.names.begin(), e.names.end(), m->macrostate());
        if (it == e.names.end()) throw string("no macrostate named '" + m->macrostate() + "'");
        e.terms.push_back(adx_term{m->condition() == ConditionEnum::APO ? ADX_APO : ADX_HOLO,
                                   int(it - e.names.begin()), m->favorable() == FavorableEnum::YES ? 1 : 0,
                                   m->weight()});
    }
    for (auto &kv : mc.scorefxn()->contexts()) {
        e.ctx_b.push_back(kv.second->before());
        e.ctx_a.push_back(kv.second->after());
    }
    for (size_t k = 0; k < e.ctx_b.size(); k++) e.ctx.push_back(adx_context_desc{e.ctx_b[k].c_str(), e.ctx_a[k].c_str()});
    adx_run_desc &d = e.d;
    d.params = gpu::params();
    d.sequence = e.seq.c_str();
    d.n_macrostates = int(e.macro_c.size());
    d.macrostates = e.macro_c.data();
    d.n_terms = int(e.terms.size());
    d.terms = e.terms.data();
    if (auto a = mc.scorefxn()->aptamer()) {
        e.apt_seq = a->seq();
        e.apt_fold = a->fold();
        d.aptamer_seq = e.apt_seq.c_str();
        d.aptamer_fold = e.apt_fold.c_str();
        d.aptamer_energy_kcal = kT() * std::log(a->affinity() / 1e6);
    }
    d.motif_mode = ADX_MOTIF_AUTO;   // ADD in partition functions, REPLACE in MFE folds (every reference pin)
    d.n_contexts = int(e.ctx.size());
    d.contexts = e.ctx.empty() ? nullptr : e.ctx.data();
    auto th = mc.thermostat();
    if (auto f = std::dynamic_pointer_cast<FixedThermostat>(th)) {
        d.thermostat.kind = ADX_THERMO_FIXED;
        d.thermostat.t_fixed = f->temperature();
    } else if (auto a = std::dynamic_pointer_cast<AnnealingThermostat>(th)) {
        d.thermostat.kind = ADX_THERMO_ANNEAL;
        d.thermostat.cycle_len = a->cycle_len();
        d.thermostat.t_hi = a->max_temperature();
        d.thermostat.t_lo = a->min_temperature();
    } else if (auto s = std::dynamic_pointer_cast<AutoScalingThermostat>(th)) {
        d.thermostat.kind = ADX_THERMO_AUTO;
        d.thermostat.target_rate = s->target_acceptance_rate();
        d.thermostat.period = int(s->training_period());
        d.thermostat.t_init = s->initial_temperature();
    }
    d.device = g;
}
}  // namespace

BatchResult MonteCarlo::apply_batch(DevicePtr device, const std::vector<uint32_t> &seeds, int g, int pick_window) const {
    BatchOptions opt;
    opt.pick_window = pick_window;
    return apply_batch(device, seeds, g, opt);
}

BatchResult MonteCarlo::apply_batch(DevicePtr device, const std::vector<uint32_t> &seeds, int g,
                                    const BatchOptions &opt) const {
    if (!gpu_expressible()) throw string("apply_batch: the score function / moves / thermostat are not GPU-expressible");
    if (opt.pick_window < 0) throw string("apply_batch: negative pick window");
    if (opt.autocorr_lag < 0 || opt.autocorr_discard < 0) throw string("apply_batch: negative autocorrelation lag or discard");
    if (opt.auto_window && opt.autocorr_lag <= 0)
        throw string("apply_batch: an automatic pick window needs the autocorrelation (autocorr_lag > 0)");
    if (opt.autocorr_lag > 0 && steps_ > 0 && opt.autocorr_discard >= steps_)   // before the run, not after it
        throw string("apply_batch: autocorrelation discard " + std::to_string(opt.autocorr_discard) +
                     " leaves none of the " + std::to_string(steps_) + " steps");
    if (opt.design_radius >= 0 && opt.pick_window <= 0 && !opt.auto_window)
        throw string("apply_batch: designs are selected from the picks and need a pick window (pick_window > 0 or auto_window)");
    if (opt.design_radius >= 0 && opt.max_designs < 1) throw string("apply_batch: max_designs must be at least 1");
    EngineSetup e;
    build_setup(*this, device, g, e);
    // the folded length of a context's variants (no contexts: the device's own)
    auto folded_length = [&](int c) { return e.seq.size() + (c >= 0 ? e.ctx_b[size_t(c)].size() + e.ctx_a[size_t(c)].size() : 0); };
    for (auto &t : opt.eval_structures) {   // before the run, not after it
        bool fits = e.ctx.empty() && t.size() == folded_length(-1);
        for (size_t c = 0; c < e.ctx.size(); c++) fits = fits || t.size() == folded_length(int(c));
        if (!fits) throw string("apply_batch: target structure '" + t + "' has the folded length of no context");
    }
    if (opt.access_len != 0 && opt.access_regions.empty()) throw string("apply_batch: access_len goes with access_regions");
    for (auto &r : opt.access_regions) {   // inside every fold they are asked of
        size_t shortest = folded_length(-1);
        for (size_t c = 0; c < e.ctx.size(); c++) shortest = c == 0 ? folded_length(0) : std::min(shortest, folded_length(int(c)));
        if (r.first < 0 || r.second < 1 || size_t(r.first) + size_t(r.second) > shortest)
            throw string("apply_batch: access region (" + std::to_string(r.first) + ", " + std::to_string(r.second) +
                         ") leaves the folded sequence of a context");
        if (opt.access_len < 0 || size_t(opt.access_len) > shortest)
            throw string("apply_batch: access_len " + std::to_string(opt.access_len) + " outside the folded sequence");
    }
    adx_ctx *raw = nullptr;
    gpu::check(adx_ctx_create(&e.d, &raw));
    gpu::CtxPtr ctx(raw);
    const int W = int(seeds.size());
    gpu::check(adx_walkers_init(ctx.get(), W, nullptr, seeds.data()));
    const bool correlating = opt.autocorr_lag > 0 && steps_ > 0;
    const bool picking = (opt.pick_window > 0 || opt.auto_window) && steps_ > 0;
    if (picking || correlating) gpu::check(adx_record_begin(ctx.get(), steps_));
    if (steps_ > 0) gpu::check(adx_run_steps(ctx.get(), steps_, nullptr));
    const size_t N = e.seq.size();
    std::vector<char> seqs(N * W);
    std::vector<double> scores(W);
    std::vector<int64_t> cnt(4 * size_t(W));
    gpu::check(adx_walkers_download(ctx.get(), seqs.data(), scores.data(), cnt.data()));
    BatchResult out;
    out.resize(W);
    if (correlating) {
        Autocorr &ac = out.autocorr;
        ac.discard = opt.autocorr_discard;
        ac.kept_steps = steps_ - ac.discard;
        ac.max_lag = int(std::min<int64_t>(opt.autocorr_lag, ac.kept_steps - 1));
        const size_t L = size_t(ac.max_lag) + 1;
        std::vector<int64_t> pm(N * L), bc(4 * N), oc(4 * size_t(W));
        std::vector<unsigned char> flag(N);
        int nch = 0;
        gpu::check(adx_record_autocorr(ctx.get(), ac.max_lag, ac.discard, pm.data(), nullptr, bc.data(), oc.data(),
                                       flag.data(), &nch));
        std::vector<int64_t> pooled(L, 0);
        double base = 0.0;
        for (size_t p = 0; p < N; p++) {
            if (!flag[p]) continue;
            ac.positions.push_back(int(p));
            double sq = 0.0;
            for (int c4 = 0; c4 < 4; c4++) {
                const double f = double(bc[4 * p + c4]) / double(int64_t(W) * ac.kept_steps);
                sq += f * f;
            }
            base += sq;
            for (size_t k = 0; k < L; k++) {
                pooled[k] += pm[p * L + k];
                ac.curves.push_back(double(pm[p * L + k]) / (double(W) * double(ac.kept_steps - int64_t(k))));
            }
        }
        ac.pooled.assign(L, 1.0);
        if (nch > 0) {
            ac.baseline = base / double(nch);
            for (size_t k = 0; k < L; k++)
                ac.pooled[k] = double(pooled[k]) / (double(int64_t(W) * nch) * double(ac.kept_steps - int64_t(k)));
            gpu::check(adx_autocorr_time(pooled.data(), ac.max_lag, int64_t(W) * nch, ac.kept_steps, ac.baseline, &ac.tau));
        }
        for (int c4 = 0; c4 < 4; c4++) {
            int64_t n = 0;
            for (int w = 0; w < W; w++) n += oc[size_t(w) * 4 + c4];
            ac.outcome_share[c4] = double(n) / double(int64_t(W) * ac.kept_steps);
        }
    }
    int pick_window = opt.pick_window;
    if (picking && opt.auto_window) {
        pick_window = out.autocorr.tau;
        if (pick_window < 1) {
            pick_window = 500;
            std::cerr << "Warning: the correlation time is " << out.autocorr.tau
                      << (out.autocorr.tau < 0 ? " (the autocorrelation has not decayed within " : " (nothing changed within ")
                      << out.autocorr.max_lag << " lags); picking with a window of 500 steps instead" << std::endl;
        }
    }
    if (picking) {
        const size_t cap = size_t((steps_ - 1) / pick_window + 1);
        std::vector<int> n(W);
        std::vector<int64_t> psteps(cap * W);
        std::vector<double> pscores(cap * W);
        std::vector<char> pseqs(cap * W * N);
        out.base_counts.assign(4 * N, 0);
        gpu::check(adx_record_picks(ctx.get(), pick_window, int(cap), n.data(), psteps.data(), pscores.data(),
                                    pseqs.data(), out.base_counts.data()));
        for (int w = 0; w < W; w++)
            for (int k = 0; k < n[w]; k++) {   // n[w] = -1 (a non-finite score): no picks
                const size_t o = size_t(w) * cap + k;
                out[w].picks.push_back(Pick{w, psteps[o], pscores[o], string(&pseqs[o * N], N)});
            }
    }
    if (picking && opt.design_radius >= 0) {
        const size_t K = size_t(opt.max_designs);
        int nd = 0;
        std::vector<int32_t> dw(K), dsz(K), dnw(K);
        std::vector<int64_t> dsteps(K);
        std::vector<double> dscores(K);
        std::vector<char> dseqs(K * N);
        out.pair_hist.assign(N + 1, 0);
        gpu::check(adx_record_designs(ctx.get(), pick_window, opt.design_radius, opt.max_designs, &nd, dw.data(),
                                      dsteps.data(), dscores.data(), dseqs.data(), dsz.data(), dnw.data(), &out.n_picks,
                                      out.pair_hist.data()));
        for (int d = 0; d < nd; d++)
            out.designs.push_back(Design{dw[d], dsteps[d], dscores[d], string(&dseqs[size_t(d) * N], N), dsz[d], dnw[d]});
    }
    if (picking || correlating) gpu::check(adx_record_end(ctx.get()));
    if (!opt.eval_structures.empty()) {
        adx_info info;
        gpu::check(adx_ctx_info(ctx.get(), &info));
        const size_t T = opt.eval_structures.size();
        std::vector<std::vector<TargetEval>> per(size_t(W) * T);   // rows of (walker, target), folds in variant order
        for (int v = 0; v < info.n_variants; v++) {
            int c = -1, cond = 0, mac = -1;
            gpu::check(adx_variant_desc(ctx.get(), v, &c, &cond, &mac));
            if (mac >= 0) continue;   // the unconstrained folds only
            std::vector<int> idx;
            string all;
            for (size_t t = 0; t < T; t++)
                if (opt.eval_structures[t].size() == folded_length(c)) {
                    idx.push_back(int(t));
                    all += opt.eval_structures[t];
                }
            if (idx.empty()) continue;
            const size_t n = idx.size();
            std::vector<double> en(size_t(W) * n), pr(size_t(W) * n);
            std::vector<uint8_t> st(size_t(W) * n);
            gpu::check(adx_walkers_eval_structures(ctx.get(), v, int(n), all.c_str(), en.data(), pr.data(), st.data()));
            for (int w = 0; w < W; w++)
                for (size_t k = 0; k < n; k++) {
                    const size_t o = size_t(w) * n + k;
                    per[size_t(w) * T + size_t(idx[k])].push_back(TargetEval{w, idx[k], c, cond, en[o], pr[o], int(st[o])});
                }
        }
        gpu::check(adx_last_eval_ms(ctx.get(), &out.eval_fill_ms, &out.eval_ms));
        for (auto &rows : per) out.evals.insert(out.evals.end(), rows.begin(), rows.end());
    }
    if (!opt.access_regions.empty()) {
        adx_info info;
        gpu::check(adx_ctx_info(ctx.get(), &info));
        const size_t R = opt.access_regions.size(), U = size_t(opt.access_len);
        std::vector<int> reg;
        for (auto &r : opt.access_regions) {
            reg.push_back(r.first);
            reg.push_back(r.second);
        }
        std::vector<std::vector<RegionAccess>> per;   // per walker, folds in variant order
        per.resize(size_t(W));
        for (int v = 0; v < info.n_variants; v++) {
            int c = -1, cond = 0, mac = -1;
            gpu::check(adx_variant_desc(ctx.get(), v, &c, &cond, &mac));
            if (mac >= 0) continue;   // the unconstrained folds only
            const size_t L = folded_length(c);
            std::vector<double> rp(size_t(W) * R), prof(size_t(W) * U * L);
            gpu::check(adx_walkers_unpaired_probs(ctx.get(), v, int(U), int(R), reg.data(), U ? prof.data() : nullptr,
                                                  rp.data(), nullptr));
            for (int w = 0; w < W; w++) {
                for (size_t k = 0; k < R; k++)
                    per[size_t(w)].push_back(RegionAccess{w, c, cond, reg[2 * k], reg[2 * k + 1], rp[size_t(w) * R + k]});
                for (size_t u = 1; u <= U; u++)
                    for (size_t i = 0; i + u <= L; i++)
                        per[size_t(w)].push_back(RegionAccess{w, c, cond, int(i), int(u), prof[(size_t(w) * U + u - 1) * L + i]});
            }
        }
        gpu::check(adx_last_unpaired_ms(ctx.get(), &out.access_fill_ms, &out.access_outside_ms));
        for (auto &rows : per) out.access.insert(out.access.end(), rows.begin(), rows.end());
    }
    for (int w = 0; w < W; w++) {
        out[w].device = device->copy();
        for (size_t k = 0; k < N; k++) out[w].device->mutate(int(k), seqs[size_t(w) * N + k]);
        out[w].score = scores[w];
        const OutcomeEnum o[4] = {OutcomeEnum::REJECT, OutcomeEnum::ACCEPT_WORSENED, OutcomeEnum::ACCEPT_UNCHANGED,
                                  OutcomeEnum::ACCEPT_IMPROVED};
        for (int k = 0; k < 4; k++) out[w].outcome_counters[o[k]] = cnt[size_t(w) * 4 + k];
    }
    return out;
}

// One walker on the engine, replayed through the reporters: the engine's
// per-step trace (position, base, outcome, T, proposed / current score,
// uniform draw, term values) rebuilds the reference's MonteCarloStep,
// including the values the reference leaves stale on ACCEPT_UNCHANGED steps.
DevicePtr MonteCarlo::apply(DevicePtr device, uint32_t seed) const {
    if (!gpu_expressible()) {
        std::mt19937 rng(seed);
        return apply(device, rng);
    }
    EngineSetup e;
    build_setup(*this, device, gpu_, e);
    adx_ctx *raw = nullptr;
    gpu::check(adx_ctx_create(&e.d, &raw));
    gpu::CtxPtr ctx(raw);
    gpu::check(adx_walkers_init(ctx.get(), 1, nullptr, &seed));
    MonteCarloStep step;
    step.num_steps = steps_;
    step.current_device = device;
    // initial score and table
    const int nctx = std::max<int>(1, int(e.ctx.size()));
    const int nt = int(e.terms.size()) * nctx;
    std::vector<double> tv(nt);
    double s0 = 0;
    gpu::check(adx_score_batch(ctx.get(), 1, e.seq.c_str(), &s0, tv.data(), nullptr));
    std::vector<string> names;
    std::vector<double> weights;
    if (e.ctx.empty()) {
        for (auto &t : scorefxn_->terms()) { names.push_back(t->name()); weights.push_back(t->weight()); }
    } else {
        for (auto &kv : scorefxn_->contexts())
            for (auto &t : scorefxn_->terms()) { names.push_back(kv.first + ": " + t->name()); weights.push_back(t->weight()); }
    }
    auto table = [&](const double *v) {
        EvaluatedScoreFunction t;
        for (int k = 0; k < nt; k++) t.push_back(EvaluatedScoreTerm{names[k], weights[k], v[k]});
        return t;
    };
    step.current_score = step.proposed_score = s0;
    step.score_table = table(tv.data());
    for (auto o : {OutcomeEnum::REJECT, OutcomeEnum::ACCEPT_WORSENED, OutcomeEnum::ACCEPT_UNCHANGED,
                   OutcomeEnum::ACCEPT_IMPROVED})
        step.outcome_counters[o] = 0;
    for (auto &r : reporters_) r->start(step);
    const int chunk = 4096;
    std::vector<int32_t> pos(chunk), outc(chunk);
    std::vector<char> base(chunk);
    std::vector<double> temp(chunk), prop(chunk), cur(chunk), thr(chunk), terms(size_t(chunk) * nt);
    const OutcomeEnum omap[4] = {OutcomeEnum::REJECT, OutcomeEnum::ACCEPT_WORSENED, OutcomeEnum::ACCEPT_UNCHANGED,
                                 OutcomeEnum::ACCEPT_IMPROVED};
    step.move = moves_[0];
    for (int s0i = 0; s0i < steps_; s0i += chunk) {
        const int n = std::min(chunk, steps_ - s0i);
        adx_trace tr{pos.data(), base.data(), outc.data(), temp.data(), prop.data(), cur.data(), thr.data(),
                     nt > 0 ? terms.data() : nullptr};
        gpu::check(adx_run_steps(ctx.get(), n, &tr));
        for (int k = 0; k < n; k++) {
            step.i = s0i + k;
            step.temperature = temp[k];
            step.proposed_device = step.current_device->copy();
            mutate_recursively(step.proposed_device, pos[k], base[k]);
            step.outcome = omap[outc[k]];
            if (step.outcome != OutcomeEnum::ACCEPT_UNCHANGED) {
                step.proposed_score = prop[k];
                step.score_diff = step.proposed_score - step.current_score;
                step.metropolis_criterion = std::exp(step.score_diff / step.temperature);
                step.random_threshold = thr[k];
                step.score_table = table(&terms[size_t(k) * nt]);
                if (step.outcome != OutcomeEnum::REJECT) {
                    step.current_device = step.proposed_device;
                    step.current_score = cur[k];
                }
            }
            step.outcome_counters[step.outcome] += 1;
            for (auto &r : reporters_) r->update(step);
        }
    }
    for (auto &r : reporters_) r->finish(step);
    return step.current_device;
}

}  // namespace addapt

namespace std {
ostream &operator<<(ostream &out, const addapt::OutcomeEnum &o) {
    switch (o) {
        case addapt::OutcomeEnum::REJECT: out << "REJECT"; break;
        case addapt::OutcomeEnum::ACCEPT_WORSENED: out << "ACCEPT_WORSENED"; break;
        case addapt::OutcomeEnum::ACCEPT_UNCHANGED: out << "ACCEPT_UNCHANGED"; break;
        case addapt::OutcomeEnum::ACCEPT_IMPROVED: out << "ACCEPT_IMPROVED"; break;
    }
    return out;
}
}  // namespace std
