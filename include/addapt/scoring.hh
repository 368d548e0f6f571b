// addapt-amd C++ host API: folding and scoring (reference include/scoring.hh).
//
//   RnaFold            abstract fold (scoring.hh:42-55)
//   GpuRnaFold         ViennaRnaFold's role (scoring.cc:17-103), folds on the
//                      MI355X through the per-fold C ABI (adx_fold_*)
//   ScoreTerm / MacrostateProbTerm / ScoreFunction   (scoring.hh:94-192)
#pragma once

#include <map>
#include <memory>
#include <string>
#include <cstdint>
#include <utility>
#include <vector>

#include "addapt/model.hh"

struct adx_fold;   // include/addapt_gpu.h (C ABI fold compound)

namespace addapt {

class ScoreFunction;
using ScoreFunctionPtr = std::shared_ptr<ScoreFunction>;
class ScoreTerm;
using ScoreTermPtr = std::shared_ptr<ScoreTerm>;
using ScoreTermList = std::vector<ScoreTermPtr>;

struct EvaluatedScoreTerm {
    string name;
    double weight, term;
};
using EvaluatedScoreFunction = std::vector<EvaluatedScoreTerm>;

enum class ConditionEnum { APO, HOLO };
enum class FavorableEnum { NO, YES };

class RnaFold {
public:
    virtual ~RnaFold() = default;
    virtual double base_pair_prob(int i, int j) const = 0;
    virtual double macrostate_prob(string constraint) const = 0;
};

/// Energy parameters shared by every GPU fold (ViennaRNA 2.0 file layout).
void set_parameter_file(const string &path);
/// kT at 37 C in kcal/mol (scoring.cc:69-70).
double kT();

/// What RNAfold -p --MEA prints after the MFE line (GpuRnaFold::ensemble_structures).
struct EnsembleStructures {
    string centroid;        ///< the pairs with probability above 1/2
    string mea;             ///< the maximum-expected-accuracy structure
    double mea_value;       ///< its expected accuracy
    double centroid_dist;   ///< the centroid's mean base-pair distance to the ensemble
    double diversity;       ///< the ensemble's mean base-pair distance (vrna_mean_bp_distance)
};

/// What a sequence pays for one given structure (GpuRnaFold::eval_structures).
struct StructureEval {
    double energy;   ///< kcal/mol; NaN when malformed, +inf for a hairpin below 3 or a structure the constraint excludes
    double prob;     ///< exp(-(energy - G) / kT) in the ensemble, 0 for a non-member; NaN in the MFE convention
    int status;      ///< 0: a member of the ensemble, else ADX_EVAL_* bits (addapt_gpu.h)
};

/// Unpaired-region probabilities of one sequence (GpuRnaFold::unpaired_probs).
struct UnpairedProbs {
    int max_len;                 ///< the longest window
    std::vector<double> probs;   ///< [max_len][L]: row u-1, column i the window of u bases from 0-based i on; 0 past L-u
    double energy;               ///< the ensemble energy, kcal/mol; +inf (and every window NaN) when the constraint admits nothing
    /// the probability that the `length` bases from 0-based `first` on are all unpaired
    double at(int first, int length) const { return probs[size_t(length - 1) * (probs.size() / size_t(max_len)) + size_t(first)]; }
};

/// Zuker suboptimal structures of one sequence (GpuRnaFold::subopt_structures).
struct SuboptStructures {
    double mfe;                              ///< kcal/mol; +inf when the constraint admits nothing
    int n_pairs_within;                      ///< pairs whose best structure lies within delta of the MFE
    std::vector<string> structures;          ///< the listed structures, energies non-decreasing
    std::vector<double> energies;            ///< kcal/mol
    std::vector<std::pair<int, int>> seeds;  ///< the pair each was chosen through, 1-based
};

class GpuRnaFold : public RnaFold {
public:
    explicit GpuRnaFold(DeviceConstPtr device, AptamerConstPtr aptamer = nullptr, int gpu = 0);
    double base_pair_prob(int i, int j) const override;
    double macrostate_prob(string constraint) const override;
    /// One minimum-free-energy structure (dot-bracket) and its energy in
    /// kcal/mol, under an optional hard constraint; the aptamer motif counts as
    /// in macrostate_prob.  All '.' and +inf when the constraint admits nothing.
    std::pair<string, double> mfe_structure(string constraint = "") const;
    /// RNAsubopt --zuker: the structures within delta kcal/mol of the MFE, at most one
    /// per base pair and max_structs in all, under an optional hard constraint; the
    /// aptamer motif counts as in macrostate_prob.  An MFE outside pass on the GPU.
    SuboptStructures subopt_structures(double delta = 3.0, int max_structs = 32, string constraint = "") const;
    /// n structures drawn from the Boltzmann ensemble (vrna_pbacktrack) under an
    /// optional hard constraint, and the ensemble energy in kcal/mol; the aptamer
    /// motif counts as in macrostate_prob.  Sample k under `seed` does not depend on n.
    std::pair<std::vector<string>, double> sample_structures(int n, uint64_t seed, string constraint = "") const;
    /// RNAplfold -u's accessibility: the probability that a window is all unpaired, for
    /// every window of up to max_len bases, under an optional hard constraint; the
    /// aptamer motif counts as in macrostate_prob.  An FP64 outside pass on the GPU.
    UnpairedProbs unpaired_probs(int max_len, string constraint = "") const;
    /// The centroid and the MEA structure (weight gamma, RNAfold's default 1) of the
    /// ensemble under an optional hard constraint, with the three statistics; the
    /// aptamer motif counts as in macrostate_prob.  Both all '.' and the statistics
    /// NaN when the constraint admits nothing.
    EnsembleStructures ensemble_structures(double gamma = 1.0, string constraint = "") const;
    /// RNAeval on the GPU: the energy, ensemble probability and status of each given
    /// dot-bracket on this sequence, under an optional hard constraint; the aptamer
    /// motif counts as in macrostate_prob.  mfe: the MFE folds' integer arithmetic
    /// (no probabilities) instead of -kT ln of the partition function's weight.
    std::vector<StructureEval> eval_structures(const std::vector<string> &structures, string constraint = "",
                                               bool mfe = false) const;

private:
    string seq_;
    AptamerConstPtr aptamer_;
    int gpu_;
    // the bppm fold compound, built and folded on first use (scoring.cc:41-44)
    mutable std::shared_ptr<::adx_fold> bppm_fold_;
};
using ViennaRnaFold = GpuRnaFold;   // the reference's name for this role

class ScoreTerm {
public:
    explicit ScoreTerm(string name = "", double weight = 1.0) : name_(name), weight_(weight) {}
    virtual ~ScoreTerm() = default;
    virtual double evaluate(DeviceConstPtr device, RnaFold const &apo, RnaFold const &holo) const = 0;
    string name() const { return name_; }
    void name(string n) { name_ = n; }
    double weight() const { return weight_; }
    void weight(double w) { weight_ = w; }

private:
    string name_;
    double weight_;
};

/// ln P(macrostate) (or ln(1-P) if not favorable) in the apo or holo fold
/// (scoring.cc:233-259); name "apo: x" / "holo: not x".
class MacrostateProbTerm : public ScoreTerm {
public:
    MacrostateProbTerm(string macrostate, ConditionEnum cond, FavorableEnum fav = FavorableEnum::YES);
    double evaluate(DeviceConstPtr device, RnaFold const &apo, RnaFold const &holo) const override;
    string macrostate() const { return macrostate_; }
    ConditionEnum condition() const { return condition_; }
    FavorableEnum favorable() const { return favorable_; }

private:
    string macrostate_;
    ConditionEnum condition_;
    FavorableEnum favorable_;
};

/// Factory for the folds a score function evaluates with (GpuRnaFold by
/// default; tests substitute their own, as the reference tests do with
/// DummyRnaFold).
using FoldFactory = std::shared_ptr<RnaFold> (*)(DeviceConstPtr, AptamerConstPtr);

class ScoreFunction {
public:
    ScoreFunction();
    double evaluate(DeviceConstPtr device) const;
    virtual double evaluate(DeviceConstPtr device, EvaluatedScoreFunction &table) const;
    void add_term(ScoreTermPtr t) { terms_.push_back(t); }
    void operator+=(ScoreTermPtr t) { add_term(t); }
    const ScoreTermList &terms() const { return terms_; }
    AptamerConstPtr aptamer() const { return aptamer_; }
    void aptamer(AptamerConstPtr a) { aptamer_ = a; }
    ContextConstPtr context(string name) const;
    void add_context(string name, ContextConstPtr c) { contexts_[name] = c; }
    const std::map<string, ContextConstPtr> &contexts() const { return contexts_; }
    void fold_factory(FoldFactory f) { factory_ = f; }
    virtual ~ScoreFunction() = default;

protected:
    double evaluate_terms(DeviceConstPtr device, EvaluatedScoreFunction &table, string prefix = "") const;

private:
    ScoreTermList terms_;
    AptamerConstPtr aptamer_;
    std::map<string, ContextConstPtr> contexts_;
    FoldFactory factory_;
};

}  // namespace addapt

namespace std {
ostream &operator<<(ostream &, const addapt::ConditionEnum &);
ostream &operator<<(ostream &, const addapt::FavorableEnum &);
}  // namespace std
