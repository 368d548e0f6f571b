// GpuRnaFold::unpaired_probs (the C++ host mirror over adx_fold_unpaired_probs) on the
// GPU: prints "E <ensemble energy>" and per window length u a line "U u v(0) .. v(L-1)"
// (17 significant digits) for the given sequence, optionally in the holo fold of the
// THEO aptamer and under a hard constraint.
// usage: unpaired_probe <seq> apo|holo <max_len> [constraint]
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
        const auto r = fold.unpaired_probs(std::atoi(argv[3]), argc > 4 ? argv[4] : "");
        const int L = int(std::string(argv[1]).size());
        std::printf("E %.9g\n", r.energy);
        for (int u = 1; u <= r.max_len; u++) {
            std::printf("U %d", u);
            for (int i = 0; i < L; i++) std::printf(" %.17g", i + u <= L ? r.at(i, u) : r.probs[size_t(u - 1) * L + i]);   // the padding as stored
            std::printf("\n");
        }
    } catch (std::string &e) {
        std::fprintf(stderr, "Error: %s\n", e.c_str());
        return 1;
    }
    return 0;
}
