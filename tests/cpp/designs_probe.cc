// MonteCarlo::apply_batch with a pick window and a design radius (the C++ host
// mirror over adx_record_designs) on the GPU, for the device, objective and
// thermostat of a config file.  Prints per walker "F <walker> <score> <seq>"
// (final state), per pick "P <walker> <step> <score> <seq>", "N <picks>", per
// design "D <design> <walker> <step> <score> <picks> <walkers> <seq>" and per
// distance "H <distance> <pairs>".  A radius of -2 asks for designs without a
// pick window: the error is printed and the exit code is 1.
// usage: designs_probe <config> <steps> <first seed> <walkers> <window> <radius> <max designs>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "addapt/config.hh"
#include "addapt/model.hh"
#include "addapt/sampling.hh"
#include "addapt/scoring.hh"

using namespace addapt;

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    try {
        const std::vector<std::string> configs{argv[1]};
        DevicePtr device = device_from_yaml(configs);
        MonteCarlo mc;
        mc += std::make_shared<UnbiasedMutationMove>();
        mc.thermostat(thermostat_from_yaml(configs));
        mc.num_steps(std::atoi(argv[2]));
        mc.scorefxn(scorefxn_from_yaml(configs));
        const int W = std::atoi(argv[4]);
        std::vector<uint32_t> seeds(static_cast<size_t>(W));
        for (int w = 0; w < W; w++) seeds[size_t(w)] = uint32_t(std::atoi(argv[3]) + w);
        BatchOptions opt;
        opt.pick_window = std::atoi(argv[5]);
        opt.design_radius = std::atoi(argv[6]);
        opt.max_designs = std::atoi(argv[7]);
        if (opt.design_radius == -2) {
            opt.pick_window = 0;
            opt.design_radius = 1;
        }
        const BatchResult res = mc.apply_batch(device, seeds, 0, opt);
        for (int w = 0; w < W; w++) {
            std::printf("F %d %.17g %s\n", w, res[size_t(w)].score, res[size_t(w)].device->seq().c_str());
            for (const Pick &p : res[size_t(w)].picks)
                std::printf("P %d %lld %.17g %s\n", p.walker, (long long)p.step, p.score, p.seq.c_str());
        }
        std::printf("N %lld\n", (long long)res.n_picks);
        for (size_t d = 0; d < res.designs.size(); d++) {
            const Design &x = res.designs[d];
            std::printf("D %zu %d %lld %.17g %d %d %s\n", d, x.walker, (long long)x.step, x.score, x.picks, x.walkers,
                        x.seq.c_str());
        }
        for (size_t d = 0; d < res.pair_hist.size(); d++) std::printf("H %zu %lld\n", d, (long long)res.pair_hist[d]);
    } catch (std::string &e) {
        std::fprintf(stderr, "Error: %s\n", e.c_str());
        return 1;
    }
    return 0;
}
