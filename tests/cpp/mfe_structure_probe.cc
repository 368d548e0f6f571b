// GpuRnaFold::mfe_structure (the C++ host mirror over adx_fold_mfe_structure)
// on the GPU: prints "<structure> <energy>" for the given sequence, optionally
// in the holo fold of the THEO aptamer and under a hard constraint.
// usage: mfe_structure_probe <seq> apo|holo [constraint]
#include <cstdio>
#include <memory>
#include <string>

#include "addapt/model.hh"
#include "addapt/scoring.hh"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    try {
        auto dev = std::make_shared<addapt::Device>(argv[1]);
        addapt::AptamerConstPtr apt;
        if (std::string(argv[2]) == "holo")
            apt = std::make_shared<addapt::Aptamer>("GAUACCAGCCGAAAGGCCCUUGGCAGC", "(...((.(((....)))....))...)", 0.32);
        addapt::GpuRnaFold fold(dev, apt);
        const auto r = argc > 3 ? fold.mfe_structure(argv[3]) : fold.mfe_structure();
        std::printf("%s %.9g\n", r.first.c_str(), r.second);
    } catch (std::string &e) {
        std::fprintf(stderr, "Error: %s\n", e.c_str());
        return 1;
    }
    return 0;
}
