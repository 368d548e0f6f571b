// Stand-alone probe of addapt_amd/csrc/struct_eval_core.hpp (tests/test_struct_eval_core.py),
// built with setup_core.hpp and energy.cpp and nothing else of the engine: the
// per-lane functions here are the ones struct_eval_kernel runs, called lane by
// lane in the kernel's order (stage, partners, loops + admission + exterior,
// motif sites, totals) on tables built as the API layer builds them.
//
//   probe PAR < cases
//   cases:  n_cases, then per case one line
//             convention(pf|mfe) SEQ CST MSEQ MFOLD MENERGY MMODE N_STRUCTS     ("-" = none)
//           and N_STRUCTS lines of dot-bracket (any characters, the sequence's length)
//   output: per structure "energy status", the energy as %.17g (nan / inf as printf has them)
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

#define SE_FN
#include "struct_eval_core.hpp"

using namespace adx;

namespace {

constexpr int LANES = 64;

std::string arg(const std::string &s) { return s == "-" ? "" : s; }

// fold_common.hpp seq_setup, serially (no context: the sequence is the folded one)
void stage(EvalSeqLds &L, const std::vector<uint8_t> &codes, const std::vector<uint8_t> &cons, const DevScaled &X,
           const EvalTab &E, bool holo) {
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
        L.spk[k] = k < X.n_special ? X.sp_key[k] : 0xFFFFFFFFu;
        L.spv[k] = E.sp_e[k];
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

// struct_eval_kernel's phases for one item, the 64 lanes in turn
void eval_item(const DevTables &T, const EvalTab &E, const EvalSeqLds &L, int N, int mL, bool holo,
               const std::string &st, double &energy, int &status) {
    std::vector<uint8_t> br(SE_NP, 0), pt(SE_NP, 0);
    std::vector<double> le(SE_NP, 0.0);
    std::vector<EvalAcc> acc(LANES);
    const StructEval<EvalSeqLds> M{&T, &E, L, pt.data(), N};
    for (int lane = 0; lane < LANES; lane++)
        for (int k = lane + 1; k <= N; k += LANES) {
            br[k] = bracket_code(st[k - 1]);
            if (br[k] == SB_BAD) acc[lane].status |= SE_MALFORMED;
        }
    for (int lane = 0; lane < LANES; lane++)
        for (int k = lane + 1; k <= N; k += LANES) {
            const int p = partner_of(br.data(), N, k);
            if (p < 0) acc[lane].status |= SE_MALFORMED;
            pt[k] = uint8_t(p > 0 ? p : 0);
        }
    bool unparsed = false;
    for (const EvalAcc &a : acc) unparsed = unparsed || a.status != 0;
    for (int lane = 0; lane < LANES; lane++) {
        EvalAcc &a = acc[lane];
        for (int k = lane + 1; k <= N; k += LANES) {
            if (!M.admits(k)) a.status |= SE_EXCLUDED;
            if (pt[k] > k) {
                EvalAcc one;
                M.loop_of(k, one);
                le[k] = double(one.e) + one.d;
                a.e += one.e;
                a.d += one.d;
                a.status |= one.status;
            }
        }
        if (lane == LANES - 1) M.exterior(a);
    }
    double adj = 0.0;
    if (holo && mL > 0)
        for (int o = 1; o + mL - 1 <= N; o++) {
            if (!L.mat[o]) continue;
            bool same = true;
            double enc = 0.0;
            for (int lane = 0; lane < LANES; lane++)
                for (int m = lane; m < mL; m += LANES) {
                    same = same && M.site_position(o, m);
                    if (pt[o + m] > o + m) enc += le[o + m];
                }
            if (!same) continue;
            if (E.mfe) acc[0].e += M.site_adjust_mfe(int(enc));
            else adj += M.site_adjust_pf(enc);
        }
    int e = 0;
    double d = 0.0;
    status = 0;
    for (const EvalAcc &a : acc) {
        e += a.e;
        d += a.d;
        status |= a.status;
    }
    status = item_status(unparsed, status);
    energy = item_energy(e, d, adj, status);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 1;
    EnergyParams P;
    std::string perr;
    if (!load_params(argv[1], P, perr)) return std::fprintf(stderr, "%s\n", perr.c_str()), 2;
    auto T = std::make_unique<DevTables>();
    build_tables(P, *T, true);
    int n_cases = 0;
    if (!(std::cin >> n_cases)) return 1;
    for (int c = 0; c < n_cases; c++) {
        std::string conv, seq, cst, mseq, mfold;
        double menergy = 0.0;
        int mmode = 0, n_structs = 0;
        if (!(std::cin >> conv >> seq >> cst >> mseq >> mfold >> menergy >> mmode >> n_structs)) return 1;
        const bool mfe = conv == "mfe";
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
        auto X = std::make_unique<DevScaled>();
        auto E = std::make_unique<EvalTab>();
        auto L = std::make_unique<EvalSeqLds>();
        build_scaled(P, 1.0, m, eint, mpt, *X, mfe);
        build_eval_tab(P, m, eint, *E, mfe);
        stage(*L, encode(seq), cons, *X, *E, m.present);
        for (int k = 0; k < n_structs; k++) {
            std::string st;
            if (!(std::cin >> st) || int(st.size()) != N) return std::fprintf(stderr, "structure %d of case %d\n", k, c), 2;
            double energy = 0.0;
            int status = 0;
            eval_item(*T, *E, *L, N, X->motif_len, m.present, st, energy, status);
            std::printf("%.17g %d\n", energy, status);
        }
    }
    return 0;
}
