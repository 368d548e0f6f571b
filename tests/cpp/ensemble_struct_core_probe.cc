// The centroid / MEA kernel's per-lane code (addapt_amd/csrc/ensemble_struct_core.hpp)
// on the host, lane by lane in the kernel's order.  stdin: "<n_cases>", then per
// case "L gamma" and L*L doubles (row-major; "nan" and "inf" are read as such).
// stdout per case: the centroid, the MEA structure, "mea centroid_dist diversity"
// (17 significant digits: exact), "<n_pops>" and per pop "i j win" (win -1: no
// candidate matched).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "ensemble_struct_core.hpp"

using namespace adx;

int main() {
    int cases = 0;
    if (std::scanf("%d", &cases) != 1) return 2;
    for (int t = 0; t < cases; t++) {
        int L = 0;
        double gamma = 0.0;
        if (std::scanf("%d %lf", &L, &gamma) != 2 || L < 1 || L > ES_LMAX) return 2;
        std::vector<double> P(size_t(L) * L);
        for (auto &x : P)
            if (std::scanf("%lf", &x) != 1) return 2;
        std::vector<double> tab(2 * es_cells(L), 0.0);
        auto S = std::make_unique<EnsLds>();
        const Ens E{*S, P.data(), tab.data(), tab.data() + es_cells(L), L};
        S->top = S->pops = S->bad = 0;
        for (int c = 0; c < L; c++) E.column(c, 2.0 * gamma);
        E.centroid_scan();
        for (int c = 0; c < L; c++) E.column_stats(c);
        for (int d = 0; d < L; d++)
            for (int i = 0; i < L - d; i++) E.fill_cell(i, i + d);
        const bool bad = S->bad != 0;
        const double dist = bad ? NAN : es_sum(S->part[0], L), div = bad ? NAN : 2.0 * es_sum(S->part[1], L);
        std::vector<int> pops;
        E.push(0, L - 1);
        E.next_item();
        while (S->cur[0] >= 0) {
            const int i = S->cur[0], j = S->cur[1];
            for (int lane = 0; lane < ES_NT; lane++) S->win = std::min(S->win, E.candidate(i, j, lane, ES_NT));
            pops.insert(pops.end(), {i, j, S->win == ES_NONE ? -1 : S->win});
            E.resolve(i, j, S->win);
            E.next_item();
        }
        std::string cen(size_t(L), '.');
        for (int k = 0; k < L; k++)
            if (S->pt[k] >= 0) cen[size_t(k)] = S->pt[k] > k ? '(' : ')';
        std::printf("%s\n%.*s\n%.17g %.17g %.17g\n%zu\n", cen.c_str(), L, S->out, bad ? NAN : E.m(0, L - 1), dist, div,
                    pops.size() / 3);
        for (size_t k = 0; k < pops.size(); k += 3) std::printf("%d %d %d\n", pops[k], pops[k + 1], pops[k + 2]);
    }
    return 0;
}
