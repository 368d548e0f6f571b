// Stand-alone probe of addapt_amd/csrc/mfe_outside_core.hpp (tests/test_mfe_outside_core.py),
// built with setup_core.hpp and energy.cpp and nothing else of the engine: the
// per-lane functions here are the ones mfe_subopt_kernel runs, called lane by lane
// in the kernel's order (inside fill, f5, f3, outside fill, th, selection and
// traceback) on tables built as the API layer builds them for an MFE problem.
//
//   probe PAR LANES < cases
//   cases:  n_cases, then per case one line
//             SEQ CST MSEQ MFOLD MENERGY MMODE DELTA_DCAL MAX_STRUCTS     ("-" = none)
//   output: per case "M <f5[N] dcal or inf> <pairs within delta>", a line
//           "T i j dcal" for every pair some structure holds, a line
//           "S i j dcal structure" per listed structure, and "E"
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
#include "mfe_outside_core.hpp"

using namespace adx;

namespace {

std::string arg(const std::string &s) { return s == "-" ? "" : s; }

// fold_common.hpp seq_setup, serially (no context: the sequence is the folded one)
void stage(TraceLds &L, const std::vector<uint8_t> &codes, const std::vector<uint8_t> &cons, const DevScaled &X, bool holo) {
    const int N = int(codes.size()), np = N + 2;
    std::memset(&L, 0, sizeof L);
    for (int k = 0; k < np; k++) {
        L.S[k] = (k >= 1 && k <= N) ? codes[k - 1] : 0;
        L.up[k] = cons[k];
        L.ptn[k] = cons[2 * np + k];
        L.enc[k] = cons[3 * np + k];
        L.flg[k] = cons[4 * np + k];
        L.out[k] = '.';
    }
    for (int k = 0; k < MAX_SPECIAL_HP; k++) {
        const bool on = k < X.n_special;
        L.spk[k] = on ? X.sp_key[k] : 0xFFFFFFFFu;
        L.spv[k] = on ? ei(X.sp_val[k]) : TR_INF;
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

int unpaired_from(const TraceLds &L, const int *f, int k, int prev) {
    return (k >= 1 && L.up[k] >= 1 && f[prev] < TR_INF) ? f[prev] : TR_INF;
}

// the kernel's trace loop: candidates reduced by min over the lanes, lane 0 resolves
void trace(const Outside &O, TraceLds &L, int lanes) {
    while (L.top > 0) {
        const int *s = L.stk + 3 * --L.top;
        const int kind = s[0], i = s[1], j = s[2];
        int win = TR_NONE;
        for (int lane = 0; lane < lanes; lane++) win = tmin(win, O.candidate(kind, i, j, lane, lanes));
        O.resolve(kind, i, j, win);
    }
}

void run_case(const DevTables &T, const DevScaled &X, TraceLds &L, int N, bool holo, int lanes, int delta, int max_structs) {
    const size_t cells = N >= 5 ? size_t(N - 4) * (N - 3) / 2 : 1;
    std::vector<int> tab(7 * cells, TR_INF), f3(TR_NP, TR_INF);
    int *s = tab.data();
    const Trace M{&T, &X, L, s, s + cells, s + 2 * cells, N, ei(X.mlclosing), ei(X.mlbase_sig), ei(X.motif_extra), X.motif_len, holo};
    const Outside O{M, s + 3 * cells, s + 4 * cells, s + 5 * cells, s + 6 * cells, f3.data()};
    for (int d = 4; d <= N - 1; d++)
        for (int lane = 0; lane < lanes; lane++)
            for (int r = lane; r < N - d; r += lanes) M.fill_cell(r + 1, r + 1 + d);
    L.f5[0] = 0;
    for (int j = 1; j <= N; j++) {
        int v = unpaired_from(L, L.f5, j, j - 1);
        for (int lane = 0; lane < lanes; lane++) v = tmin(v, M.f5_pairs(j, lane, lanes));
        L.f5[j] = v;
    }
    f3[N + 1] = 0;
    for (int i = N; i >= 1; i--) {
        int v = unpaired_from(L, f3.data(), i, i + 1);
        for (int lane = 0; lane < lanes; lane++) v = tmin(v, O.f3_pairs(i, lane, lanes));
        f3[i] = v;
    }
    for (int d = N - 1; d >= 4; d--)
        for (int lane = 0; lane < lanes; lane++)
            for (int r = lane; r < N - d; r += lanes) O.outside_cell(r + 1, r + 1 + d);
    for (int d = 4; d <= N - 1; d++)
        for (int lane = 0; lane < lanes; lane++)
            for (int r = lane; r < N - d; r += lanes) O.through_cell(r + 1, r + 1 + d);
    const int total = L.f5[N];
    const bool feasible = total < int(0.5f * MFE_BIG);
    const int limit = total + delta;
    int within = 0;
    for (int lane = 0; lane < lanes && feasible; lane++) within += O.count_within(limit, lane, lanes);
    if (feasible) std::printf("M %d %d\n", total, within);
    else std::printf("M inf 0\n");
    for (int i = 1; i <= N; i++)
        for (int j = i + 4; j <= N; j++)
            if (O.th[M.idx(i, j)] < TR_INF) std::printf("T %d %d %d\n", i, j, O.th[M.idx(i, j)]);
    for (int found = 0; feasible && found < max_structs; found++) {
        unsigned long long best = SO_NOKEY;
        for (int lane = 0; lane < lanes; lane++) {
            const unsigned long long k = O.lane_best(limit, lane, lanes);
            best = k < best ? k : best;
        }
        if (best == SO_NOKEY) break;
        const int si = Outside::key_i(best), sj = Outside::key_j(best), e = O.th[M.idx(si, sj)];
        for (int k = 0; k < N + 2; k++) L.out[k] = '.';
        L.top = 0;
        O.seed_begin(si, sj);
        trace(O, L, lanes);
        O.mark_structure();
        std::printf("S %d %d %d %s\n", si, sj, e, std::string(L.out, L.out + N).c_str());
    }
    std::printf("E\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    const int lanes = std::atoi(argv[2]);
    if (lanes < 1) return 1;
    EnergyParams P;
    std::string perr;
    if (!load_params(argv[1], P, perr)) return std::fprintf(stderr, "%s\n", perr.c_str()), 2;
    auto T = std::make_unique<DevTables>();
    build_tables(P, *T, true);
    int n_cases = 0;
    if (!(std::cin >> n_cases)) return 1;
    for (int c = 0; c < n_cases; c++) {
        std::string seq, cst, mseq, mfold;
        double menergy = 0.0;
        int mmode = 0, delta = 0, max_structs = 0;
        if (!(std::cin >> seq >> cst >> mseq >> mfold >> menergy >> mmode >> delta >> max_structs)) return 1;
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
        auto L = std::make_unique<TraceLds>();
        build_scaled(P, 1.0, m, eint, mpt, *X, true);
        stage(*L, encode(seq), cons, *X, m.present);
        run_case(*T, *X, *L, N, m.present, lanes, delta, max_structs);
    }
    return 0;
}
