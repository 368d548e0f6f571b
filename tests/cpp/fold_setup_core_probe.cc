// Stand-alone probe of addapt_amd/csrc/fold_setup_core.hpp (tests/test_fold_setup_core.py),
// built with setup_core.hpp and energy.cpp and nothing else of the engine: the
// functions here are the ones the kernels run.
//   probe seq BEF RAW AFT             ("-" = empty) SeqSrc::code(k, N) for k = 0 .. N + 1 on one line,
//                                     then wrap_pos at 0, 1, N, N + 1
//   probe motif PAR SEQ CST MSEQ MFOLD  motif_site at every start 1 .. N - mL + 1 on one line; the
//                                     constraint arrays from build_constraint, the partner table
//                                     from prepare_motif
//   probe shapes PAR pf|mfe G0        "ctab ...", "fgen ...", build_scaled's term lists as "slist n1 n2 kind f"
//                                     and "glist u n1 f", then per shape "u n1 loop_kind shape_factor"
//   probe hairpin                     per line "u type s5 s3 hairpin_dt_index"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "setup_core.hpp"

#include "fold_setup_core.hpp"

using namespace adx;

namespace {

struct HostL {   // what a kernel's LDS carve offers motif_site / allowed
    const uint8_t *S, *up, *ptn, *enc, *flg;
};

std::string arg(const char *s) { return std::strcmp(s, "-") ? s : ""; }

}  // namespace

int main(int argc, char **argv) {
    const std::string cmd = argc >= 2 ? argv[1] : "";
    SetupError err;
    if (cmd == "seq" && argc == 5) {
        const std::vector<uint8_t> bef = encode(arg(argv[2])), raw = encode(arg(argv[3])), aft = encode(arg(argv[4]));
        const SeqSrc src{bef.data(), raw.data(), aft.data(), int(bef.size()), int(raw.size())};
        const int N = int(bef.size() + raw.size() + aft.size());
        for (int k = 0; k <= N + 1; k++) std::printf("%d ", int(src.code(k, N)));
        std::printf("\n%d %d %d %d\n", wrap_pos(0, N), wrap_pos(1, N), wrap_pos(N, N), wrap_pos(N + 1, N));
        return 0;
    }
    if (cmd == "motif" && argc == 7) {
        EnergyParams P;
        std::string perr;
        if (!load_params(argv[2], P, perr)) return std::fprintf(stderr, "%s\n", perr.c_str()), 2;
        const std::string seq = argv[3];
        const int N = int(seq.size());
        std::vector<uint8_t> cons;
        if (build_constraint(arg(argv[4]), N, cons, err)) return std::fprintf(stderr, "%s\n", err.text.c_str()), 2;
        Motif m;
        m.seq = argv[5];
        m.fold = argv[6];
        m.present = true;
        double eint = 0.0;
        std::vector<int> pt;
        if (prepare_motif(P, m, eint, pt, err)) return std::fprintf(stderr, "%s\n", err.text.c_str()), 2;
        const int mL = int(m.seq.size()), np = N + 2;
        const std::vector<uint8_t> mcode = encode(m.seq);
        std::vector<int8_t> mpt(pt.begin(), pt.end());
        std::vector<uint8_t> S(np, 0);
        const std::vector<uint8_t> codes = encode(seq);
        for (int k = 1; k <= N; k++) S[k] = codes[k - 1];
        const HostL L{S.data(), cons.data(), cons.data() + 2 * np, cons.data() + 3 * np, cons.data() + 4 * np};
        for (int o = 1; o + mL - 1 <= N; o++) std::printf("%d ", motif_site(L, mcode.data(), mpt.data(), mL, o) ? 1 : 0);
        std::printf("\n");
        return 0;
    }
    if (cmd == "shapes" && argc == 5) {
        EnergyParams P;
        std::string perr;
        if (!load_params(argv[2], P, perr)) return std::fprintf(stderr, "%s\n", perr.c_str()), 2;
        auto X = std::make_unique<DevScaled>();
        build_scaled(P, std::exp(std::atof(argv[4]) / kT_kcal()), Motif{}, 0.0, {}, *X, !std::strcmp(argv[3], "mfe"));
        std::printf("ctab");
        for (int k = 0; k < CT_SIZE; k++) std::printf(" %.9g", double(X->ctab[k]));
        std::printf("\nfgen");
        for (int k = 0; k < FG_SIZE; k++) std::printf(" %.9g", double(X->fgen[k]));
        std::printf("\n");
        for (int t = 0; t < X->s_cnt[31]; t++)   // the term lists build_scaled placed (addS, g_f)
            std::printf("slist %d %d %d %.9g\n", int(X->s_n1[t]), int(X->s_n2[t]), int(X->s_kind[t]), double(X->s_f[t]));
        for (int t = 0; t < X->g_cnt[31]; t++)
            std::printf("glist %d %d %.9g\n", int(X->g_u[t]), int(X->g_n1[t]), double(X->g_f[t]));
        for (int u = 0; u <= MAXLOOP; u++)
            for (int n1 = 0; n1 <= u; n1++)
                std::printf("%d %d %d %.9g\n", u, n1, loop_kind(n1, u - n1), double(shape_factor(X.get(), u, n1)));
        return 0;
    }
    if (cmd == "hairpin") {
        for (int u = 3; u <= 5; u++)
            for (int type = 1; type <= 6; type++)
                for (int s = 0; s < 2; s++) {
                    const int s5 = s ? 4 : 1, s3 = s ? 2 : 3;
                    std::printf("%d %d %d %d %d\n", u, type, s5, s3, hairpin_dt_index(u, type, s5, s3));
                }
        return 0;
    }
    return 1;
}
