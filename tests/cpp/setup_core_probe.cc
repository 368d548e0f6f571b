// Stand-alone probe of addapt_amd/csrc/setup_core.hpp (tests/test_setup_core.py), built
// with energy.cpp and nothing else of the engine.
//   probe kt                          kT_cal() to 17 digits
//   probe constraint N CST            status, message, then the five arrays of N + 2 bytes, one per line
//   probe closure SEQ POS MAC...      return code, move_error_text, then "pos parity" per line
//   probe tables PAR pf|mfe           DevTables as raw floats
//   probe scaled PAR pf|mfe G0        named arrays of DevScaled (no motif), one per line
//   probe pack16 V...                 per value "1 <packed word in hex>" or "0" (refused)
//   probe groups CTX,MAC,N,MOTIF...   the groups2 list of these variants
//   probe slots G,G,... B,B,...       status, message, then the slot of every outside variant B
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "setup_core.hpp"

using namespace adx;

static std::vector<int> ints(const char *s) {
    std::vector<int> v;
    for (const char *p = s; *p;) {
        char *end;
        v.push_back(int(std::strtol(p, &end, 10)));
        p = *end ? end + 1 : end;
    }
    return v;
}

template <class T>
static void line(const char *name, const T *a, size_t n) {
    std::printf("%s", name);
    for (size_t k = 0; k < n; k++) std::printf(" %.9g", double(a[k]));
    std::printf("\n");
}

int main(int argc, char **argv) {
    const std::string cmd = argc >= 2 ? argv[1] : "";
    SetupError err;
    if (cmd == "kt") {
        std::printf("%.17g\n", kT_cal());
        return 0;
    }
    if (cmd == "constraint" && argc == 4) {
        const int N = std::atoi(argv[2]);
        std::vector<uint8_t> out;
        const adx_status s = build_constraint(argv[3], N, out, err);
        std::printf("%d\n%s\n", int(s), err.text.c_str());
        if (s) return 0;
        if (out.size() != size_t(5 * (N + 2))) return 2;
        for (int a = 0; a < 5; a++) line("", out.data() + a * (N + 2), size_t(N + 2));
        return 0;
    }
    if (cmd == "closure" && argc >= 4) {
        std::vector<std::string> ms(argv + 4, argv + argc);
        std::vector<std::pair<int, int>> out;
        const int rc = closure(argv[2], ms, std::atoi(argv[3]), out);
        std::printf("%d\n%s\n", rc, move_error_text(rc));
        for (auto &p : out) std::printf("%d %d\n", p.first, p.second);
        return 0;
    }
    if ((cmd == "tables" && argc == 4) || (cmd == "scaled" && argc == 5)) {
        EnergyParams P;
        std::string perr;
        if (!load_params(argv[2], P, perr)) return std::fprintf(stderr, "%s\n", perr.c_str()), 2;
        const bool mfe = !std::strcmp(argv[3], "mfe");
        if (cmd == "tables") {
            auto T = std::make_unique<DevTables>();
            build_tables(P, *T, mfe);
            const size_t n = sizeof(DevTables) / sizeof(float);
            return std::fwrite(T.get(), sizeof(float), n, stdout) == n ? 0 : 3;
        }
        auto X = std::make_unique<DevScaled>();
        build_scaled(P, std::exp(std::atof(argv[4]) / kT_kcal()), Motif{}, 0.0, {}, *X, mfe);
        line("ctab", X->ctab, CT_SIZE);
        line("fgen", X->fgen, FG_SIZE);
        line("hp", X->hp, NMAX + 1);
        line("sig", X->sig, NMAX + 4);
        line("mlclosing", &X->mlclosing, 1);
        line("s_cnt", X->s_cnt, 32);
        line("g_cnt", X->g_cnt, 32);
        line("s_n1", X->s_n1, NS_MAX);
        line("s_n2", X->s_n2, NS_MAX);
        line("g_n1", X->g_n1, NG_MAX);
        line("g_u", X->g_u, NG_MAX);
        return 0;
    }
    if (cmd == "pack16") {
        for (int k = 2; k < argc; k++) {
            float v = float(std::atof(argv[k]));
            uint32_t w;
            const bool ok = pack16(&v, 1);
            std::memcpy(&w, &v, 4);
            if (ok) std::printf("1 %08x\n", unsigned(w));
            else std::printf("0\n");
        }
        return 0;
    }
    if (cmd == "groups") {
        std::vector<DevVariant> vs;
        std::vector<int> vmac;
        for (int k = 2; k < argc; k++) {
            const std::vector<int> f = ints(argv[k]);
            if (f.size() != 4) return 2;
            vs.push_back(DevVariant{f[2], 0, f[0], 0, f[3], 0});
            vmac.push_back(f[1]);
        }
        const std::vector<int> g = pair_groups2(vs, vmac);
        line("", g.data(), g.size());
        return 0;
    }
    if (cmd == "slots" && argc == 4) {
        const std::vector<int> bvars = ints(argv[3]);
        std::vector<int> bslot;
        const adx_status s = outside_slots(ints(argv[2]), bvars, bslot, err);
        std::printf("%d\n%s\n", int(s), err.text.c_str());
        if (!s) line("", bslot.data(), bslot.size());
        return 0;
    }
    return 1;
}
