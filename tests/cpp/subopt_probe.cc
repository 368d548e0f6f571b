// GpuRnaFold::subopt_structures (the C++ host mirror over adx_fold_subopt_structures)
// on the GPU: prints "M <mfe> <pairs within delta>" and per listed structure
// "S <i> <j> <energy> <structure>" for the given sequence, optionally in the holo
// fold of the THEO aptamer and under a hard constraint.
// usage: subopt_probe <seq> apo|holo <delta> <max_structs> [constraint]
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
        const auto r = fold.subopt_structures(std::atof(argv[3]), std::atoi(argv[4]), argc > 5 ? argv[5] : "");
        std::printf("M %.9g %d\n", r.mfe, r.n_pairs_within);
        for (size_t k = 0; k < r.structures.size(); k++)
            std::printf("S %d %d %.9g %s\n", r.seeds[k].first, r.seeds[k].second, r.energies[k], r.structures[k].c_str());
    } catch (std::string &e) {
        std::fprintf(stderr, "Error: %s\n", e.c_str());
        return 1;
    }
    return 0;
}
