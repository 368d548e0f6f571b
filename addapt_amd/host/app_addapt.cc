// addapt: Monte Carlo sgRNA design from config files (the reference's
// apps/addapt.cc command line, run on the MI355X engine).
//
//   addapt <config>... [-n <num>] [-T <schedule>] [-r <seed>] [-o <path>]
//                      [-i <steps>] [--walkers <W>] [--gpu <id>] [--params <file>]
//                      [--reference-loop] [--picks <path>] [--pick-window <steps>|auto]
//                      [--autocorr <path>] [--autocorr-lag <steps>] [--autocorr-discard <steps>]
//                      [--eval <path> --eval-structure <db>[,<db>...]]
//                      [--access <path> --access-region <first>-<last>[,...] [--access-len <u>]]
//                      [--designs <path>] [--design-radius <mutations>] [--max-designs <num>]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "addapt/config.hh"
#include "addapt/model.hh"
#include "addapt/sampling.hh"
#include "addapt/scoring.hh"

using namespace addapt;

static const char USAGE[] =
    "Run a Monte Carlo design simulation of an sgRNA with an aptamer (addapt).\n"
    "\n"
    "Usage:\n"
    "  addapt <config>... [options]\n"
    "\n"
    "Options:\n"
    "  -n <num>, --num-moves <num>            [default: 100]\n"
    "    The number of moves to attempt in the design simulation.\n"
    "  -T <schedule>, --temperature <schedule>\n"
    "    Metropolis temperature: fixed (\"5\"), annealing (\"1 to 0 in 500 steps\")\n"
    "    or auto-scaling (\"auto 50%\").  Default: the config's 'thermostat' or 1.\n"
    "  -r <seed>, --random-seed <seed>        [default: 0]\n"
    "    Seed of the random number generator (std::mt19937).\n"
    "  -o <path>, --output <path>             [default: traj.tsv]\n"
    "    Trajectory (TSV) of the simulation.\n"
    "  -i <steps>, --output-interval <steps>  [default: 1]\n"
    "    How often a snapshot is recorded.\n"
    "  --walkers <W>                          [default: 1]\n"
    "    Run W independent walkers (seeds r .. r+W-1) on the GPU at once and write\n"
    "    their final sequences and scores to the output instead of a trajectory.\n"
    "  --picks <path>\n"
    "    With --walkers: record every walker's trajectory on the GPU and write the\n"
    "    peaks of each (scores at or above the trajectory's 75th percentile, best\n"
    "    first, at least the pick window apart) with the sequences there.\n"
    "  --pick-window <steps>|auto             [default: 500]\n"
    "    The least distance between two picks of one trajectory.  auto: the\n"
    "    correlation time of the sequence autocorrelation (see --autocorr; computed\n"
    "    with its defaults if --autocorr is absent), or 500 with a warning if the\n"
    "    autocorrelation has not decayed.\n"
    "  --autocorr <path>\n"
    "    With --walkers: record every walker's trajectory on the GPU and write the\n"
    "    per-position autocorrelation of the sequences: '#' lines with the\n"
    "    correlation time, the baseline and the shares of the four outcomes, then\n"
    "    one row per lag: the lag, the autocorrelation pooled over all walkers and\n"
    "    changeable positions, and one column per changeable position (0-based).\n"
    "  --autocorr-lag <steps>                 [default: 500]\n"
    "    The largest lag (clipped to the kept steps - 1).\n"
    "  --autocorr-discard <steps>             [default: 100]\n"
    "    Steps dropped from the start of every trajectory (equilibration).\n"
    "  --designs <path>\n"
    "    With --walkers: record every walker's trajectory on the GPU, pick as --picks\n"
    "    does (with the run's pick window) and write the distinct designs among all\n"
    "    walkers' picks: best score first, a pick leads a new design if no earlier\n"
    "    leader is within the design radius of it, and else counts towards the first\n"
    "    leader that is.  '#' lines with the numbers of picks and designs, the radius\n"
    "    and the pick pairs per distance (d:count), then one row per design: its\n"
    "    leader, the picks it covers and the distinct walkers among them.\n"
    "  --design-radius <mutations>            [default: 3]\n"
    "    Leaders are more than this many mutations apart (0: exact duplicates only).\n"
    "  --max-designs <num>                    [default: 100]\n"
    "  --eval <path>\n"
    "    With --walkers and --eval-structure: price the target structures on every\n"
    "    walker's final sequence on the GPU and write one row per walker, target and\n"
    "    unconstrained (context, condition) fold of the target's length: the energy\n"
    "    (kcal/mol), the structure's probability in that fold's ensemble and a status\n"
    "    (0: in the ensemble; 1 malformed, 2 hairpin below 3, 4 excluded, 8 interior\n"
    "    loop above 30, or-ed).  A '#' line gives the device time of the last call.\n"
    "  --eval-structure <db>[,<db>...]\n"
    "    The target structures, dot-bracket, of the (context-padded) folded length.\n"
    "  --access <path>\n"
    "    With --walkers and --access-region: the probability that each region is all\n"
    "    unpaired (RNAplfold -u's accessibility) on every walker's final sequence, on\n"
    "    the GPU: one row per walker, unconstrained (context, condition) fold and\n"
    "    region.  A '#' line gives the device time of the last call.\n"
    "  --access-region <first>-<last>[,<first>-<last>...]\n"
    "    The regions, 1-based and inclusive, in the (context-padded) folded coordinates.\n"
    "  --access-len <u>\n"
    "    Also one row for every window of up to u bases: the accessibility profile.\n"
    "  --gpu <id>                             [default: 0]\n"
    "  --params <file>  Energy parameters (ViennaRNA 2.0 format).\n"
    "  --reference-loop  Run the reference's single-walker loop (one GPU fold call\n"
    "    per partition function) instead of the fused engine.\n"
    "  --version\n"
    "  -h, --help\n";

// The picks of a batched run: the summary the reference's pick_seqs prints
// (number of picks, best, worst, mean and sample standard deviation of their
// scores) as '#' lines, then one row per pick.
static void write_picks(const std::string &path, const BatchResult &res, const std::vector<uint32_t> &seeds) {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) throw std::string("couldn't open '" + path + "' for writing");
    size_t n = 0;
    double best = 0, worst = 0, sum = 0;
    for (auto &r : res)
        for (auto &p : r.picks) {
            best = n ? std::max(best, p.score) : p.score;
            worst = n ? std::min(worst, p.score) : p.score;
            sum += p.score;
            n++;
        }
    if (n == 0) {
        std::fprintf(f, "# No picks made\n");
    } else {
        const double mean = sum / double(n);
        double ss = 0;
        for (auto &r : res)
            for (auto &p : r.picks) ss += (p.score - mean) * (p.score - mean);
        const double sd = n > 1 ? std::sqrt(ss / double(n - 1)) : std::nan("");
        std::fprintf(f, "# Num Picks: %zu\n# Best Score: %.4f\n# Worst Score: %.4f\n# Average Score: %.4f \xc2\xb1 %.4f\n",
                     n, best, worst, mean, sd);
    }
    std::fprintf(f, "walker\tseed\tstep\tscore\tseq\n");
    for (auto &r : res)
        for (auto &p : r.picks)
            std::fprintf(f, "%d\t%u\t%lld\t%.17g\t%s\n", p.walker, seeds[size_t(p.walker)], (long long)p.step, p.score,
                         p.seq.c_str());
    std::fclose(f);
}

// The sequence autocorrelation of a batched run (what the reference's auto_corr
// plots and mc_stats prints): '#' lines, then one row per lag.
static void write_autocorr(const std::string &path, const Autocorr &ac) {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) throw std::string("couldn't open '" + path + "' for writing");
    std::fprintf(f, "# tau: %d\n# baseline: %.6f\n# kept steps: %lld (discarded %d)\n", ac.tau, ac.baseline,
                 (long long)ac.kept_steps, ac.discard);
    static const char *names[4] = {"reject", "accept_worsened", "accept_unchanged", "accept_improved"};
    for (int k = 0; k < 4; k++) std::fprintf(f, "# %s: %.2f%%\n", names[k], 100.0 * ac.outcome_share[k]);
    std::fprintf(f, "lag\tpooled");
    for (int p : ac.positions) std::fprintf(f, "\t%d", p);
    std::fprintf(f, "\n");
    const size_t L = size_t(ac.max_lag) + 1;
    for (size_t k = 0; k < L; k++) {
        std::fprintf(f, "%zu\t%.6f", k, ac.pooled[k]);
        for (size_t i = 0; i < ac.positions.size(); i++) std::fprintf(f, "\t%.6f", ac.curves[i * L + k]);
        std::fprintf(f, "\n");
    }
    std::fclose(f);
}

// The distinct designs of a batched run: '#' lines, then one row per design.
static void write_designs(const std::string &path, const BatchResult &res, int radius,
                          const std::vector<uint32_t> &seeds) {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) throw std::string("couldn't open '" + path + "' for writing");
    std::fprintf(f, "# Num Picks: %lld\n# Num Designs: %zu\n# Radius: %d\n# Pair Distances:", (long long)res.n_picks,
                 res.designs.size(), radius);
    for (size_t d = 0; d < res.pair_hist.size(); d++)
        if (res.pair_hist[d]) std::fprintf(f, " %zu:%lld", d, (long long)res.pair_hist[d]);
    std::fprintf(f, "\ndesign\twalker\tseed\tstep\tscore\tpicks\twalkers\tseq\n");
    for (size_t d = 0; d < res.designs.size(); d++) {
        const Design &x = res.designs[d];
        std::fprintf(f, "%zu\t%d\t%u\t%lld\t%.17g\t%d\t%d\t%s\n", d, x.walker, seeds[size_t(x.walker)],
                     (long long)x.step, x.score, x.picks, x.walkers, x.seq.c_str());
    }
    std::fclose(f);
}

// The target structures of a batched run priced on the final walkers.
static void write_evals(const std::string &path, const BatchResult &res, const std::vector<std::string> &targets,
                        const std::vector<uint32_t> &seeds) {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) throw std::string("couldn't open '" + path + "' for writing");
    std::fprintf(f, "# Num Targets: %zu\n# Last Eval ms: fill %.3f kernel %.3f\n", targets.size(), res.eval_fill_ms,
                 res.eval_ms);
    std::fprintf(f, "walker\tseed\ttarget\tcontext\tcondition\tenergy\tprobability\tstatus\tstructure\n");
    for (auto &x : res.evals)
        std::fprintf(f, "%d\t%u\t%d\t%d\t%s\t%.17g\t%.17g\t%d\t%s\n", x.walker, seeds[size_t(x.walker)], x.target,
                     x.context, x.condition ? "holo" : "apo", x.energy, x.prob, x.status,
                     targets[size_t(x.target)].c_str());
    std::fclose(f);
}

// The accessibility of the regions (and windows) on the final walkers of a batched run.
static void write_access(const std::string &path, const BatchResult &res, size_t n_regions, int access_len,
                         const std::vector<uint32_t> &seeds) {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) throw std::string("couldn't open '" + path + "' for writing");
    std::fprintf(f, "# Num Regions: %zu\n# Profile Length: %d\n# Last Access ms: fill %.3f outside %.3f\n", n_regions,
                 access_len, res.access_fill_ms, res.access_outside_ms);
    std::fprintf(f, "walker\tseed\tcontext\tcondition\tfirst\tlast\tunpaired_probability\n");
    for (auto &x : res.access)
        std::fprintf(f, "%d\t%u\t%d\t%s\t%d\t%d\t%.17g\n", x.walker, seeds[size_t(x.walker)], x.context,
                     x.condition ? "holo" : "apo", x.first + 1, x.first + x.length, x.prob);
    std::fclose(f);
}

int main(int argc, char **argv) {
    std::vector<std::string> configs;
    std::string temp, out = "traj.tsv", params, picks, autocorr, designs, evals, access;
    std::vector<std::string> targets;
    std::vector<std::pair<int, int>> regions;   // (first 0-based, length)
    int access_len = 0;
    int num = 100, interval = 1, walkers = 1, gpu = 0, pick_window = 500, autocorr_lag = 500, autocorr_discard = 100;
    int design_radius = 3, max_designs = 100;
    bool auto_window = false;
    unsigned long seed = 0;
    bool ref_loop = false;
    try {
        for (int k = 1; k < argc; k++) {
            const std::string a = argv[k];
            auto val = [&](const char *name) -> std::string {
                if (k + 1 >= argc) throw std::string("option ") + name + " needs a value";
                return argv[++k];
            };
            if (a == "-h" || a == "--help") { std::cout << USAGE; return 0; }
            else if (a == "--version") { std::cout << "addapt-amd 0.1\n"; return 0; }
            else if (a == "-n" || a == "--num-moves") num = std::stoi(val("--num-moves"));
            else if (a == "-T" || a == "--temperature") temp = val("--temperature");
            else if (a == "-r" || a == "--random-seed") seed = std::stoul(val("--random-seed"));
            else if (a == "-o" || a == "--output") out = val("--output");
            else if (a == "-i" || a == "--output-interval") interval = std::stoi(val("--output-interval"));
            else if (a == "--walkers") walkers = std::stoi(val("--walkers"));
            else if (a == "--picks") picks = val("--picks");
            else if (a == "--pick-window") {
                const std::string v = val("--pick-window");
                auto_window = v == "auto";
                if (!auto_window) pick_window = std::stoi(v);
            }
            else if (a == "--autocorr") autocorr = val("--autocorr");
            else if (a == "--autocorr-lag") autocorr_lag = std::stoi(val("--autocorr-lag"));
            else if (a == "--autocorr-discard") autocorr_discard = std::stoi(val("--autocorr-discard"));
            else if (a == "--designs") designs = val("--designs");
            else if (a == "--design-radius") design_radius = std::stoi(val("--design-radius"));
            else if (a == "--max-designs") max_designs = std::stoi(val("--max-designs"));
            else if (a == "--access") access = val("--access");
            else if (a == "--access-len") access_len = std::stoi(val("--access-len"));
            else if (a == "--access-region") {
                std::string v = val("--access-region"), t;
                for (char ch : v + ",") {
                    if (ch != ',') { t.push_back(ch); continue; }
                    const size_t dash = t.find('-');
                    if (dash == std::string::npos || dash == 0) throw std::string("--access-region wants <first>-<last>, not '" + t + "'");
                    const int first = std::stoi(t.substr(0, dash)), last = std::stoi(t.substr(dash + 1));
                    if (first < 1 || last < first) throw std::string("--access-region '" + t + "': 1 <= first <= last");
                    regions.push_back({first - 1, last - first + 1});
                    t.clear();
                }
            }
            else if (a == "--eval") evals = val("--eval");
            else if (a == "--eval-structure") {
                std::string v = val("--eval-structure"), t;
                for (char ch : v + ",") {
                    if (ch != ',') { t.push_back(ch); continue; }
                    if (!t.empty()) targets.push_back(t);
                    t.clear();
                }
            }
            else if (a == "--gpu") gpu = std::stoi(val("--gpu"));
            else if (a == "--params") params = val("--params");
            else if (a == "--reference-loop") ref_loop = true;
            else if (!a.empty() && a[0] == '-') throw std::string("unknown option '" + a + "'");
            else configs.push_back(a);
        }
        if (configs.empty()) {
            std::cerr << USAGE;
            return 1;
        }
        if (!picks.empty() && walkers <= 1) throw std::string("--picks needs --walkers <W> with W > 1");
        if (!designs.empty() && walkers <= 1) throw std::string("--designs needs --walkers <W> with W > 1");
        if (!evals.empty() && walkers <= 1) throw std::string("--eval needs --walkers <W> with W > 1");
        if (evals.empty() != targets.empty()) throw std::string("--eval <path> and --eval-structure <db>[,<db>...] go together");
        if (!access.empty() && walkers <= 1) throw std::string("--access needs --walkers <W> with W > 1");
        if (access.empty() != regions.empty()) throw std::string("--access <path> and --access-region <first>-<last>[,...] go together");
        if (access_len != 0 && access.empty()) throw std::string("--access-len goes with --access");
        if (access_len < 0) throw std::string("--access-len must not be negative");
        const bool picking = !picks.empty() || !designs.empty();
        if (picking && !auto_window && pick_window < 1) throw std::string("--pick-window must be at least 1");
        if (!designs.empty() && design_radius < 0) throw std::string("--design-radius must not be negative");
        if (!designs.empty() && max_designs < 1) throw std::string("--max-designs must be at least 1");
        if (!autocorr.empty() && walkers <= 1) throw std::string("--autocorr needs --walkers <W> with W > 1");
        const bool correlating = !autocorr.empty() || (picking && auto_window);
        if (correlating && autocorr_lag < 1) throw std::string("--autocorr-lag must be at least 1");
        if (correlating && autocorr_discard < 0) throw std::string("--autocorr-discard must not be negative");
        if (!params.empty()) set_parameter_file(params);
        DevicePtr device = device_from_yaml(configs);
        ScoreFunctionPtr sf = scorefxn_from_yaml(configs);
        auto mc = std::make_shared<MonteCarlo>();
        *mc += std::make_shared<UnbiasedMutationMove>();
        mc->thermostat(!temp.empty() ? thermostat_from_str(temp) : thermostat_from_yaml(configs));
        mc->num_steps(num);
        mc->scorefxn(sf);
        mc->gpu(gpu);
        if (walkers > 1) {
            std::vector<uint32_t> seeds(walkers);
            for (int w = 0; w < walkers; w++) seeds[w] = uint32_t(seed + w);
            BatchOptions opt;
            opt.pick_window = !picking || auto_window ? 0 : pick_window;
            opt.auto_window = picking && auto_window;
            if (!designs.empty()) {
                opt.design_radius = design_radius;
                opt.max_designs = max_designs;
            }
            opt.autocorr_lag = correlating ? autocorr_lag : 0;
            opt.autocorr_discard = correlating ? autocorr_discard : 0;
            opt.eval_structures = targets;
            opt.access_regions = regions;
            opt.access_len = access_len;
            auto res = mc->apply_batch(device, seeds, gpu, opt);
            FILE *f = std::fopen(out.c_str(), "w");
            if (!f) throw std::string("couldn't open '" + out + "' for writing");
            std::fprintf(f, "walker\tseed\tscore\treject\taccept_worsened\taccept_unchanged\taccept_improved\tseq\n");
            for (int w = 0; w < walkers; w++) {
                auto &c = res[w].outcome_counters;
                std::fprintf(f, "%d\t%u\t%.17g\t%lld\t%lld\t%lld\t%lld\t%s\n", w, seeds[w], res[w].score,
                             c[OutcomeEnum::REJECT], c[OutcomeEnum::ACCEPT_WORSENED],
                             c[OutcomeEnum::ACCEPT_UNCHANGED], c[OutcomeEnum::ACCEPT_IMPROVED],
                             res[w].device->seq().c_str());
            }
            std::fclose(f);
            if (!picks.empty()) write_picks(picks, res, seeds);
            if (!autocorr.empty()) write_autocorr(autocorr, res.autocorr);
            if (!designs.empty()) write_designs(designs, res, design_radius, seeds);
            if (!evals.empty()) write_evals(evals, res, targets, seeds);
            if (!access.empty()) write_access(access, res, regions.size(), access_len, seeds);
            return 0;
        }
        *mc += std::make_shared<ProgressReporter>();
        *mc += std::make_shared<TsvTrajectoryReporter>(out, interval);
        if (ref_loop) {
            std::mt19937 rng(static_cast<uint32_t>(seed));
            mc->apply(device, rng);
        } else {
            mc->apply(device, static_cast<uint32_t>(seed));
        }
        return 0;
    } catch (const std::string &e) {
        std::cerr << "Error: " << e << std::endl;
        return 1;
    } catch (const char *e) {
        std::cerr << "Error: " << e << std::endl;
        return 1;
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
}
