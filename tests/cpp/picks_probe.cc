// MonteCarlo::apply_batch with a pick window (the C++ host mirror over
// adx_record_*) on the GPU, for the device, objective and thermostat of a
// config file.  Prints per walker "F <walker> <score> <seq>" (final state),
// per pick "P <walker> <step> <score> <seq>" and per position
// "C <position> <A> <C> <G> <U>" (the picks' base counts).
// usage: picks_probe <config> <steps> <first seed> <walkers> <window>
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
    if (argc != 6) return 2;
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
        const BatchResult res = mc.apply_batch(device, seeds, 0, std::atoi(argv[5]));
        for (int w = 0; w < W; w++) {
            std::printf("F %d %.17g %s\n", w, res[size_t(w)].score, res[size_t(w)].device->seq().c_str());
            for (const Pick &p : res[size_t(w)].picks)
                std::printf("P %d %lld %.17g %s\n", p.walker, (long long)p.step, p.score, p.seq.c_str());
        }
        for (size_t k = 0; k * 4 < res.base_counts.size(); k++)
            std::printf("C %zu %lld %lld %lld %lld\n", k, (long long)res.base_counts[4 * k],
                        (long long)res.base_counts[4 * k + 1], (long long)res.base_counts[4 * k + 2],
                        (long long)res.base_counts[4 * k + 3]);
    } catch (std::string &e) {
        std::fprintf(stderr, "Error: %s\n", e.c_str());
        return 1;
    }
    return 0;
}
