// The design selection rule (addapt_amd/csrc/design_select_core.hpp) on the
// host, in the kernels' order of operations: pack into bit planes, order by the
// sort key, select in rank order, count the pair distances.
// stdin: "<n_cases> <n_orders> <n_firsts>", then
//   per case   "M N radius K", then M times "<sequence> <score>"
//   per order  "a ia b ib"                  (scores and entry indices)
//   per first  "k d0 .. dk"                 (the designs of a walker's first k + 1 picks)
// stdout: per case five lines: n_designs, the leaders, the sizes, member_of,
// pair_hist[0..N]; per order 1 if (a, ia) stands before (b, ib); per first 1 if
// pick k counts towards its design's walkers.
// Exit 3: a plane's padding bit is set, unpacking does not give the sequence
// back, the packed distance differs from comparing characters, or the sort key
// disagrees with the order comparison.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "design_select_core.hpp"

using namespace adx;

int main() {
    int nc = 0, no = 0, nf = 0;
    if (std::scanf("%d %d %d", &nc, &no, &nf) != 3) return 2;
    for (int c = 0; c < nc; c++) {
        int M = 0, N = 0, radius = 0, K = 0;
        if (std::scanf("%d %d %d %d", &M, &N, &radius, &K) != 4 || M < 1 || N < 1 || N > 255 || K < 1) return 2;
        const int NW = ds_words(N);
        std::vector<std::string> seq(static_cast<size_t>(M));
        std::vector<double> score(seq.size());
        std::vector<uint64_t> lo(seq.size() * NW), hi(seq.size() * NW);
        char buf[300];
        for (int e = 0; e < M; e++) {
            if (std::scanf("%299s %lf", buf, &score[e]) != 2) return 2;
            seq[e] = buf;
            if (int(seq[e].size()) != N) return 2;
            for (int w = 0; w < NW; w++)
                if (!ds_pack_word(seq[e].data(), N, w, &lo[size_t(e) * NW + w], &hi[size_t(e) * NW + w])) return 2;
            if (N % 64) {
                const uint64_t pad = ~0ull << (N % 64);
                if ((lo[size_t(e) * NW + NW - 1] | hi[size_t(e) * NW + NW - 1]) & pad) return 3;
            }
            for (int p = 0; p < N; p++)
                if (ds_unpack(&lo[size_t(e) * NW], &hi[size_t(e) * NW], p) != std::toupper(seq[e][p])) return 3;
        }
        auto dist = [&](int a, int b) {
            int d = 0;
            for (int w = 0; w < NW; w++)
                d += ds_word_dist(lo[size_t(a) * NW + w], hi[size_t(a) * NW + w], lo[size_t(b) * NW + w],
                                  hi[size_t(b) * NW + w]);
            return d;
        };
        // the order: a stable sort by the key, as the device's radix sort is
        std::vector<int> order(seq.size());
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(),
                         [&](int a, int b) { return ds_sort_key(score[a]) < ds_sort_key(score[b]); });
        int F = 0;
        while (F < M && ds_sort_key(score[order[F]]) != DS_KEY_NONE) F++;
        for (int q = 0; q + 1 < F; q++)
            if (!ds_before(score[order[q]], order[q], score[order[q + 1]], order[q + 1])) return 3;
        for (int q = F; q < M; q++)
            if (tp_finite(score[order[q]])) return 3;
        // selection in rank order
        std::vector<int> member(seq.size(), -1), leaders, sizes;
        for (int q = 0; q < F && int(leaders.size()) < K; q++) {
            if (member[order[q]] >= 0) continue;
            const int d = int(leaders.size());
            int n = 0;
            for (int p = q; p < F; p++)
                if (member[order[p]] < 0 && ds_covers(dist(order[q], order[p]), radius)) {
                    member[order[p]] = d;
                    n++;
                }
            leaders.push_back(order[q]);
            sizes.push_back(n);
        }
        std::vector<long long> hist(size_t(N) + 1, 0);
        for (int a = 0; a < F; a++)
            for (int b = a + 1; b < F; b++) {
                const int d = dist(order[a], order[b]);
                int plain = 0;
                for (int p = 0; p < N; p++)
                    plain += std::toupper(seq[order[a]][p]) != std::toupper(seq[order[b]][p]);
                if (d != plain) return 3;
                hist[d]++;
            }
        std::printf("%zu\n", leaders.size());
        for (int x : leaders) std::printf("%d ", x);
        std::printf("\n");
        for (int x : sizes) std::printf("%d ", x);
        std::printf("\n");
        for (int x : member) std::printf("%d ", x);
        std::printf("\n");
        for (long long x : hist) std::printf("%lld ", x);
        std::printf("\n");
    }
    for (int k = 0; k < no; k++) {
        double a, b;
        int ia, ib;
        if (std::scanf("%lf %d %lf %d", &a, &ia, &b, &ib) != 4) return 2;
        std::printf("%d\n", int(ds_before(a, ia, b, ib)));
    }
    for (int k = 0; k < nf; k++) {
        int n;
        if (std::scanf("%d", &n) != 1 || n < 0) return 2;
        std::vector<int32_t> d(size_t(n) + 1);
        for (auto &x : d)
            if (std::scanf("%d", &x) != 1) return 2;
        std::printf("%d\n", int(ds_first_of_walker(d.data(), n)));
    }
    return 0;
}
