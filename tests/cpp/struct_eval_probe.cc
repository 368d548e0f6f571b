// The C++ host mirror of the eval-structures calls on the GPU, for the device,
// objective and thermostat of a config file.
//   struct_eval_probe batch <config> <steps> <first seed> <walkers> <db>[,<db>...]
//     MonteCarlo::apply_batch with BatchOptions::eval_structures: per walker
//     "F <walker> <seq>", per row "E <walker> <target> <context> <condition> <energy> <prob> <status>"
//   struct_eval_probe fold <config> <constraint|-> <pf|mfe> <db>[,<db>...]
//     GpuRnaFold::eval_structures on the config's device with its aptamer: per
//     structure "S <energy> <prob> <status>"
// An error is printed and the exit code is 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "addapt/config.hh"
#include "addapt/model.hh"
#include "addapt/sampling.hh"
#include "addapt/scoring.hh"

using namespace addapt;

static std::vector<std::string> split(const std::string &v) {
    std::vector<std::string> out;
    std::string t;
    for (char ch : v + ",") {
        if (ch != ',') { t.push_back(ch); continue; }
        if (!t.empty()) out.push_back(t);
        t.clear();
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    try {
        const std::vector<std::string> configs{argv[2]};
        DevicePtr device = device_from_yaml(configs);
        ScoreFunctionPtr sf = scorefxn_from_yaml(configs);
        if (!std::strcmp(argv[1], "fold") && argc == 6) {
            GpuRnaFold fold(device, sf->aptamer());
            const std::string cst = std::strcmp(argv[3], "-") ? argv[3] : "";
            for (const StructureEval &x : fold.eval_structures(split(argv[5]), cst, !std::strcmp(argv[4], "mfe")))
                std::printf("S %.17g %.17g %d\n", x.energy, x.prob, x.status);
            return 0;
        }
        if (std::strcmp(argv[1], "batch") || argc != 7) return 2;
        MonteCarlo mc;
        mc += std::make_shared<UnbiasedMutationMove>();
        mc.thermostat(thermostat_from_yaml(configs));
        mc.num_steps(std::atoi(argv[3]));
        mc.scorefxn(sf);
        const int W = std::atoi(argv[5]);
        std::vector<uint32_t> seeds(static_cast<size_t>(W));
        for (int w = 0; w < W; w++) seeds[size_t(w)] = uint32_t(std::atoi(argv[4]) + w);
        BatchOptions opt;
        opt.eval_structures = split(argv[6]);
        const BatchResult res = mc.apply_batch(device, seeds, 0, opt);
        for (int w = 0; w < W; w++) std::printf("F %d %s\n", w, res[size_t(w)].device->seq().c_str());
        for (const TargetEval &x : res.evals)
            std::printf("E %d %d %d %d %.17g %.17g %d\n", x.walker, x.target, x.context, x.condition, x.energy, x.prob,
                        x.status);
    } catch (std::string &e) {
        std::fprintf(stderr, "Error: %s\n", e.c_str());
        return 1;
    }
    return 0;
}
