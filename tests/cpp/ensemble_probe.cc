// GpuRnaFold::ensemble_structures (the C++ host mirror over
// adx_fold_ensemble_structures) on the GPU: prints the centroid, the MEA
// structure and "mea centroid_dist diversity" (17 significant digits: exact)
// for the given sequence, optionally in the holo fold of the THEO aptamer and
// under a hard constraint.
// usage: ensemble_probe <seq> apo|holo <gamma> [constraint]
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "addapt/model.hh"
#include "addapt/scoring.hh"

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    try {
        auto dev = std::make_shared<addapt::Device>(argv[1]);
        addapt::AptamerConstPtr apt;
        if (std::string(argv[2]) == "holo")
            apt = std::make_shared<addapt::Aptamer>("GAUACCAGCCGAAAGGCCCUUGGCAGC", "(...((.(((....)))....))...)", 0.32);
        addapt::GpuRnaFold fold(dev, apt);
        const double gamma = std::atof(argv[3]);
        const auto r = argc > 4 ? fold.ensemble_structures(gamma, argv[4]) : fold.ensemble_structures(gamma);
        std::printf("%s\n%s\n%.17g %.17g %.17g\n", r.centroid.c_str(), r.mea.c_str(), r.mea_value, r.centroid_dist,
                    r.diversity);
    } catch (std::string &e) {
        std::fprintf(stderr, "Error: %s\n", e.c_str());
        return 1;
    }
    return 0;
}
