// Stand-alone probe of addapt_amd/csrc/pf_access_core.hpp (tests/test_pf_access_core.py),
// built with setup_core.hpp and energy.cpp and nothing else of the engine: the
// per-lane functions here are the ones pf_fill_kernel and pf_access_kernel run,
// called lane by lane in the kernels' order (inside fill, q5, a5, the adjoints on
// descending diagonals, the run masses, the two prefix passes, the windows) on
// tables built as the API layer builds them for a partition-function problem: in
// FP32 (f32, what the kernels read), or by the same setup code in FP64 (f64), which
// takes the rounding of the factors out of a comparison with an FP64 reference.
//
//   probe PAR LANES SIGMA f32|f64 < cases
//   cases:  n_cases, then per case one line
//             SEQ CST MSEQ MFOLD MENERGY MMODE MAX_LEN     ("-" = none)
//   output: per case "Z <ensemble energy kcal/mol> <max_i |sum_j P(i,j) + P_u(i,i) - 1|>",
//           a line "U u v(1) .. v(N-u+1)" per window length u <= MAX_LEN, a line
//           "P i j v" per pair of nonzero probability, and "E"; 17 significant digits
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "setup_core.hpp"

#include "fold_setup_core.hpp"

namespace adx {
namespace {
// fold_common.hpp special_hp on a host: the last match of a scan
inline int special_hp(const uint32_t *spk, uint32_t key) {
    int hit = -1;
    for (int k = 0; k < MAX_SPECIAL_HP; k++)
        if (spk[k] == key) hit = k;
    return hit;
}
}  // namespace
}  // namespace adx

#define TR_FN
#include "pf_access_core.hpp"

using namespace adx;

namespace {

std::string arg(const std::string &s) { return s == "-" ? "" : s; }

// fold_common.hpp seq_setup, serially (no context: the sequence is the folded one)
template <class F>
void stage(PfSeqLdsT<F> &L, const std::vector<uint8_t> &codes, const std::vector<uint8_t> &cons, const DevScaledT<F> &X,
           bool holo) {
    const int N = int(codes.size()), np = N + 2;
    std::memset(&L, 0, sizeof L);
    for (int k = 0; k < np; k++) {
        L.S[k] = (k >= 1 && k <= N) ? codes[k - 1] : 0;
        L.up[k] = cons[k];
        L.ptn[k] = cons[2 * np + k];
        L.enc[k] = cons[3 * np + k];
        L.flg[k] = cons[4 * np + k];
    }
    for (int k = 0; k < MAX_SPECIAL_HP; k++) {
        const bool on = k < X.n_special;
        L.spk[k] = on ? X.sp_key[k] : 0xFFFFFFFFu;
        L.spv[k] = on ? X.sp_val[k] : F(0);
    }
    for (int k = 0; k < MAX_MOTIF; k++) {
        L.mcode[k] = X.motif_code[k];
        L.mpt[k] = X.motif_pt[k];
    }
    wrap_ends(L, N);
    const int mL = X.motif_len;
    if (holo && mL > 0)
        for (int o = 1; o + mL - 1 <= N; o++) L.mat[o] = motif_site(L, L.mcode, L.mpt, mL, o) ? 1 : 0;
}

template <class F>
void run_case(const DevTablesT<F> &T, const DevScaledT<F> &X, const PfSeqLdsT<F> &L, int N, bool holo, int lanes,
              int max_len) {
    const size_t cells = N >= 5 ? size_t(N - 4) * (N - 3) / 2 : 1;
    std::vector<double> tab(6 * cells, 0.0), q5(N + 2, 0.0), a5(N + 2, 0.0), R(size_t(N) * N, 0.0), pw5(N + 1), pwm(N + 1);
    double *s = tab.data();
    const PfModelT<F> M{&T, &X, L, s, s + cells, s + 2 * cells, q5.data(), N, X.motif_len, holo};
    const AccessT<F> A{M, s + 3 * cells, s + 4 * cells, s + 5 * cells, a5.data(), R.data(), pw5.data(), pwm.data()};
    for (int d = 4; d <= N - 1; d++)
        for (int lane = 0; lane < lanes; lane++)
            for (int r = lane; r < N - d; r += lanes) M.fill_cell(r + 1, r + 1 + d);
    q5[0] = 1.0;
    for (int j = 1; j <= N; j++) {
        double v = L.up[j] >= 1 ? q5[j - 1] * double(X.sig[1]) : 0.0;
        for (int lane = 0; lane < lanes; lane++) v += M.q5_pairs(j, lane, lanes);
        q5[j] = v;
    }
    const double Z = q5[N];
    pw5[0] = pwm[0] = 1.0;
    for (int k = 1; k <= N; k++) {
        pw5[k] = pw5[k - 1] * double(X.sig[1]);
        pwm[k] = pwm[k - 1] * double(X.mlbase_sig);
    }
    a5[N] = 1.0;
    for (int m = N - 1; m >= 0; m--) {
        double v = A.a5_unpaired(m);
        for (int lane = 0; lane < lanes; lane++) v += A.a5_pairs(m, lane, lanes);
        a5[m] = v;
    }
    for (int d = N - 1; d >= 4; d--)
        for (int lane = 0; lane < lanes; lane++)
            for (int r = lane; r < N - d; r += lanes) A.adjoint_cell(r + 1, r + 1 + d);
    for (int lane = 0; lane < lanes; lane++)
        for (int t = lane; t < N * N; t += lanes)
            if (t / N <= t % N) R[t] = A.run_mass(t / N + 1, t % N + 1);
    for (int a = 1; a <= N; a++) A.sum_row(a);
    for (int b = 1; b <= N; b++) A.sum_column(b);

    double energy = 0.0;
    if (!(Z > 0.0)) energy = Z == 0.0 ? INFINITY : Z;
    else if (N >= 5) energy = -X.kT * (std::log(Z) - N * X.log_sigma);
    double dev = 0.0;
    for (int i = 1; i <= N && Z > 0.0; i++) {
        double sum = A.unpaired_prob(i, i, Z);
        for (int j = 1; j <= N; j++)
            if (j != i) sum += A.pair_prob(j < i ? j : i, j < i ? i : j, Z);
        dev = std::fmax(dev, std::fabs(sum - 1.0));
    }
    std::printf("Z %.17g %.17g\n", energy, dev);
    for (int u = 1; u <= max_len && u <= N; u++) {
        std::printf("U %d", u);
        for (int i = 1; i + u - 1 <= N; i++) std::printf(" %.17g", A.unpaired_prob(i, i + u - 1, Z));
        std::printf("\n");
    }
    for (int i = 1; i <= N && Z > 0.0; i++)
        for (int j = i + 1; j <= N; j++) {
            const double p = A.pair_prob(i, j, Z);
            if (p != 0.0) std::printf("P %d %d %.17g\n", i, j, p);
        }
    std::printf("E\n");
}

template <class F>
int run_all(const EnergyParams &P, int lanes, double sigma) {
    auto T = std::make_unique<DevTablesT<F>>();
    build_tables(P, *T, false);
    int n_cases = 0;
    if (!(std::cin >> n_cases)) return 1;
    for (int c = 0; c < n_cases; c++) {
        std::string seq, cst, mseq, mfold;
        double menergy = 0.0;
        int mmode = 0, max_len = 0;
        if (!(std::cin >> seq >> cst >> mseq >> mfold >> menergy >> mmode >> max_len)) return 1;
        const int N = int(seq.size());
        if (N < 1 || N > NMAX) return std::fprintf(stderr, "length %d\n", N), 2;
        SetupError err;
        std::vector<uint8_t> cons;
        if (build_constraint(arg(cst), N, cons, err)) return std::fprintf(stderr, "%s\n", err.text.c_str()), 2;
        Motif m;
        double eint = 0.0;
        std::vector<int> mpt;
        if (mseq != "-") {
            m.seq = mseq;
            m.fold = mfold;
            m.energy_kcal = menergy;
            m.mode = mmode;
            m.present = true;
            if (prepare_motif(P, m, eint, mpt, err)) return std::fprintf(stderr, "%s\n", err.text.c_str()), 2;
        }
        auto X = std::make_unique<DevScaledT<F>>();
        auto L = std::make_unique<PfSeqLdsT<F>>();
        build_scaled(P, sigma, m, eint, mpt, *X, false);
        stage(*L, encode(seq), cons, *X, m.present);
        run_case(*T, *X, *L, N, m.present, lanes, max_len);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) return 1;
    const int lanes = std::atoi(argv[2]);
    const double sigma = std::atof(argv[3]);
    const std::string prec = argv[4];
    if (lanes < 1 || !(sigma > 0.0) || (prec != "f32" && prec != "f64")) return 1;
    EnergyParams P;
    std::string perr;
    if (!load_params(argv[1], P, perr)) return std::fprintf(stderr, "%s\n", perr.c_str()), 2;
    return prec == "f64" ? run_all<double>(P, lanes, sigma) : run_all<float>(P, lanes, sigma);
}
