// GpuRnaFold::sample_structures (the C++ host mirror over
// adx_fold_sample_structures) on the GPU: prints the ensemble energy, then one
// sampled structure per line, for the given sequence, optionally in the holo
// fold of the THEO aptamer and under a hard constraint.
// usage: pf_sample_probe <seq> apo|holo <n> <seed> [constraint]
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "addapt/model.hh"
#include "addapt/scoring.hh"

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    try {
        auto dev = std::make_shared<addapt::Device>(argv[1]);
        addapt::AptamerConstPtr apt;
        if (std::string(argv[2]) == "holo")
            apt = std::make_shared<addapt::Aptamer>("GAUACCAGCCGAAAGGCCCUUGGCAGC", "(...((.(((....)))....))...)", 0.32);
        addapt::GpuRnaFold fold(dev, apt);
        const int n = std::atoi(argv[3]);
        const uint64_t seed = std::strtoull(argv[4], nullptr, 10);
        const auto r = argc > 5 ? fold.sample_structures(n, seed, argv[5]) : fold.sample_structures(n, seed);
        std::printf("%.9g\n", r.second);
        for (const auto &s : r.first) std::printf("%s\n", s.c_str());
    } catch (std::string &e) {
        std::fprintf(stderr, "Error: %s\n", e.c_str());
        return 1;
    }
    return 0;
}
