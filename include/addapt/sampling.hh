// addapt-amd C++ host API: Monte Carlo sampling (reference include/sampling.hh).
//
// MonteCarlo::apply(device, rng) is the reference's single-walker loop
// (sampling.cc:22-107) with folds on the GPU (GpuRnaFold).  When the score
// function, move set and thermostat are the built-in ones (everything the
// config files can express), MonteCarlo::apply(device, seed) and
// MonteCarlo::apply_batch run the fused GPU engine instead (adx_ctx_* /
// adx_run_steps): the same trajectory per walker, thousands of walkers at once.
#pragma once

#include <cstdint>
#include <fstream>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "addapt/model.hh"
#include "addapt/scoring.hh"

namespace addapt {

class MonteCarlo;
using MonteCarloPtr = std::shared_ptr<MonteCarlo>;
class Move;
using MovePtr = std::shared_ptr<Move>;
using MoveList = std::vector<MovePtr>;
class Thermostat;
using ThermostatPtr = std::shared_ptr<Thermostat>;
class Reporter;
using ReporterPtr = std::shared_ptr<Reporter>;
using ReporterList = std::vector<ReporterPtr>;

enum class OutcomeEnum { REJECT, ACCEPT_WORSENED, ACCEPT_UNCHANGED, ACCEPT_IMPROVED };

struct MonteCarloStep {
    int i = -1, num_steps = 0;
    DevicePtr current_device, proposed_device;
    MovePtr move;
    EvaluatedScoreFunction score_table;
    double current_score = 0, proposed_score = 0, score_diff = 0;
    double temperature = 0, metropolis_criterion = 0, random_threshold = 0;
    OutcomeEnum outcome = OutcomeEnum::ACCEPT_UNCHANGED;
    std::map<OutcomeEnum, int> outcome_counters;
};

const std::map<char, char> COMPLEMENTARY_NUCS = {{'A', 'U'}, {'G', 'C'}, {'C', 'G'}, {'U', 'A'}};

bool can_be_mutated(DeviceConstPtr device, int i);
bool can_be_freely_mutated(DeviceConstPtr device, int i);
/// set position i to base and every macrostate partner to its complement,
/// recursively (sampling.cc:195-282); throws std::string on conflicts
void mutate_recursively(DevicePtr device, int i, char base);

class Move {
public:
    virtual ~Move() = default;
    virtual string name() const = 0;
    virtual void apply(DevicePtr device, std::mt19937 &rng) const = 0;
};

/// pick a freely mutable position uniformly, then a base from "ACGU"
class UnbiasedMutationMove : public Move {
public:
    string name() const override { return "UnbiasedMutation"; }
    void apply(DevicePtr device, std::mt19937 &rng) const override;
};

class Thermostat {
public:
    virtual ~Thermostat() = default;
    virtual double adjust(MonteCarloStep const &step) = 0;
};

class FixedThermostat : public Thermostat {
public:
    explicit FixedThermostat(double t) : t_(t) {}
    double adjust(MonteCarloStep const &) override { return t_; }
    double temperature() const { return t_; }
    void temperature(double t) { t_ = t; }

private:
    double t_;
};

/// T(i) = ((lo - hi) / N) * (i mod N) + hi  (sampling.cc:332-338)
class AnnealingThermostat : public Thermostat {
public:
    AnnealingThermostat(int cycle_len, double hi, double lo) : n_(cycle_len), hi_(hi), lo_(lo) {}
    double adjust(MonteCarloStep const &step) override;
    int cycle_len() const { return n_; }
    double max_temperature() const { return hi_; }
    double min_temperature() const { return lo_; }

private:
    int n_;
    double hi_, lo_;
};

/// every `period` scored steps T = max(median(score_diff) / ln(rate), 0)
/// (sampling.cc:381-401)
class AutoScalingThermostat : public Thermostat {
public:
    AutoScalingThermostat(double rate = 0.5, unsigned period = 100, double t0 = 1.0)
        : t_(t0), rate_(rate), period_(period) {}
    double adjust(MonteCarloStep const &step) override;
    double target_acceptance_rate() const { return rate_; }
    unsigned training_period() const { return period_; }
    double initial_temperature() const { return t0_; }

private:
    double t_, rate_;
    unsigned period_;
    double t0_ = t_;
    std::vector<double> train_;
};

class Reporter {
public:
    virtual ~Reporter() = default;
    virtual void start(MonteCarloStep const &) {}
    virtual void update(MonteCarloStep const &) {}
    virtual void finish(MonteCarloStep const &) {}
};

class ProgressReporter : public Reporter {
public:
    void update(MonteCarloStep const &step) override;
};

/// The reference's trajectory format (sampling.cc:427-494), one row per
/// `interval` steps.
class TsvTrajectoryReporter : public Reporter {
public:
    TsvTrajectoryReporter(string path, int interval) : path_(path), interval_(interval) {}
    void start(MonteCarloStep const &step) override;
    void update(MonteCarloStep const &step) override;
    void finish(MonteCarloStep const &step) override;

private:
    string path_;
    int interval_;
    std::ofstream tsv_;
};

/// one peak of a walker's trajectory (what the reference's pick_seqs script
/// takes from a trajectory file): the 0-based step, the current score after
/// it and the sequence then
struct Pick {
    int walker;
    int64_t step;
    double score;
    std::string seq;
};

/// one walker's result of a batched run
struct WalkerResult {
    DevicePtr device;
    double score;
    std::map<OutcomeEnum, long long> outcome_counters;
    std::vector<Pick> picks;   ///< ascending steps; empty without a pick window
};

/// the per-position autocorrelation of the walkers' sequence trajectories (what
/// the reference's auto_corr script plots from a trajectory file), over the
/// steps kept after `discard`: at lag k the share of steps i whose base equals
/// that of step i + k
struct Autocorr {
    int max_lag = -1;                  ///< -1: not computed
    int discard = 0;
    int64_t kept_steps = 0;
    std::vector<int> positions;        ///< the changeable positions (0-based): freely mutable ones and their partners
    std::vector<double> curves;        ///< curves[i * (max_lag + 1) + k]: position positions[i], all walkers
    std::vector<double> pooled;        ///< [max_lag + 1] over all walkers and changeable positions
    double baseline = 1.0;             ///< the chance that two independent draws at a changeable position match
    int tau = 0;                       ///< the correlation time of `pooled` in steps (adx_autocorr_time); -1: not decayed
    double outcome_share[4] = {0, 0, 0, 0};   ///< reject, accept worsened / unchanged / improved over the kept steps
};

/// one distinct design among all walkers' picks (adx_record_designs): its
/// leader, the best pick no earlier leader is within the radius of, and what
/// it covers
struct Design {
    int walker;          ///< the leader's walker,
    int64_t step;        ///< 0-based step,
    double score;        ///< score
    std::string seq;     ///< and sequence
    int picks;           ///< the picks within the radius of the leader that no earlier design took
    int walkers;         ///< the distinct walkers among them: how often the design was found independently
};

/// one target structure priced on one walker's final sequence (adx_walkers_eval_structures)
/// for one unconstrained (context, condition) fold of the score function
struct TargetEval {
    int walker;
    int target;          ///< index into BatchOptions::eval_structures
    int context;         ///< the score function's context (-1: none)
    int condition;       ///< 0 apo, 1 holo
    double energy;       ///< kcal/mol (NaN malformed, +inf hairpin below 3)
    double prob;         ///< its share of that fold's ensemble; 0 for a non-member
    int status;          ///< 0: a member, else ADX_EVAL_* bits (addapt_gpu.h)
};

/// the probability that a window of one walker's final sequence is all unpaired
/// (adx_walkers_unpaired_probs) in one unconstrained (context, condition) fold
struct RegionAccess {
    int walker;
    int context;         ///< the score function's context (-1: none)
    int condition;       ///< 0 apo, 1 holo
    int first, length;   ///< the window, first 0-based, in the fold's (context-padded) coordinates
    double prob;         ///< NaN: the fold's ensemble is empty
};

/// the walkers' results; with a pick window also how often A, C, G, U stand at
/// each position over all walkers' picks (base_counts[4 * position + base])
struct BatchResult : std::vector<WalkerResult> {
    std::vector<int64_t> base_counts;
    Autocorr autocorr;                 ///< filled with BatchOptions::autocorr_lag > 0
    std::vector<Design> designs;       ///< filled with BatchOptions::design_radius >= 0: best leader first
    std::vector<int64_t> pair_hist;    ///< then [d], d = 0..N: the pairs of picks d mutations apart
    int64_t n_picks = 0;               ///< and the number of picks the designs were selected from
    double eval_fill_ms = 0.0, eval_ms = 0.0;   ///< device time of the last eval call (adx_last_eval_ms): FP64 fill, kernel
    std::vector<TargetEval> evals;     ///< filled with BatchOptions::eval_structures: walker-major, then target, then fold
    double access_fill_ms = 0.0, access_outside_ms = 0.0;   ///< device time of the last access call (adx_last_unpaired_ms)
    std::vector<RegionAccess> access;  ///< filled with BatchOptions::access_regions: walker-major, then fold, then the
                                       ///< regions and, with access_len > 0, every window of up to that length
};

/// what a batched run does besides stepping
struct BatchOptions {
    int pick_window = 0;        ///< > 0: pick each trajectory's peaks at least this many steps apart
    bool auto_window = false;   ///< pick with the correlation time as window (needs autocorr_lag > 0);
                                ///< if it is below 1 (not decayed, or nothing changed) with 500, warning on stderr
    int autocorr_lag = 0;       ///< > 0: the autocorrelation up to this lag (clipped to the kept steps - 1)
    int autocorr_discard = 0;   ///< steps dropped from the start (equilibration); must be below the number of steps
    int design_radius = -1;     ///< >= 0: the distinct designs among the picks, leaders more than this many
                                ///< mutations apart (needs a pick window, fixed or automatic)
    int max_designs = 100;      ///< at most this many designs
    std::vector<std::string> eval_structures;   ///< target dot-brackets priced on every walker's final sequence, in each
                                                ///< unconstrained (context, condition) fold of their (context-padded) length
    std::vector<std::pair<int, int>> access_regions;   ///< (first, length), first 0-based, in folded coordinates: the probability
                                                       ///< that each is all unpaired on every walker's final sequence, in each
                                                       ///< unconstrained (context, condition) fold
    int access_len = 0;         ///< > 0: with access_regions also every window of up to this many bases
};

class MonteCarlo {
public:
    MonteCarlo();
    /// the reference loop; every score evaluation folds on the GPU
    DevicePtr apply(DevicePtr device, std::mt19937 &rng) const;
    /// mt19937(seed): the fused GPU engine when the setup is built-in, else
    /// the reference loop
    DevicePtr apply(DevicePtr device, uint32_t seed) const;
    /// W independent walkers (seeds[w]) on one GPU; reporters are not called.
    /// pick_window > 0: each walker's trajectory is recorded on the GPU and its
    /// peaks (threshold: the trajectory's 75th percentile; at least pick_window
    /// steps apart) come back as WalkerResult::picks
    BatchResult apply_batch(DevicePtr device, const std::vector<uint32_t> &seeds, int gpu = 0,
                            int pick_window = 0) const;
    /// the same with options: picks, the sequence autocorrelation of the recorded
    /// trajectories (BatchResult::autocorr), and picks whose window is its correlation time
    BatchResult apply_batch(DevicePtr device, const std::vector<uint32_t> &seeds, int gpu,
                            const BatchOptions &options) const;
    /// true if the fused GPU engine can run this setup
    bool gpu_expressible() const;

    int num_steps() const { return steps_; }
    void num_steps(int n) { steps_ = n; }
    ThermostatPtr thermostat() const { return thermostat_; }
    void thermostat(ThermostatPtr t) { thermostat_ = t; }
    ScoreFunctionPtr scorefxn() const { return scorefxn_; }
    void scorefxn(ScoreFunctionPtr s) { scorefxn_ = s; }
    MoveList moves() const { return moves_; }
    void add_move(MovePtr m) { moves_.push_back(m); }
    void operator+=(MovePtr m) { add_move(m); }
    ReporterList reporters() const { return reporters_; }
    void add_reporter(ReporterPtr r) { reporters_.push_back(r); }
    void operator+=(ReporterPtr r) { add_reporter(r); }
    void gpu(int g) { gpu_ = g; }

private:
    int steps_;
    ThermostatPtr thermostat_;
    ScoreFunctionPtr scorefxn_;
    MoveList moves_;
    ReporterList reporters_;
    int gpu_ = 0;
};

}  // namespace addapt

namespace std {
ostream &operator<<(ostream &, const addapt::OutcomeEnum &);
}
