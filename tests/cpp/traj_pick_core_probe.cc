// The trajectory picking rule (addapt_amd/csrc/traj_pick_core.hpp) on the host,
// one trajectory at a time, in the kernel's order of operations: keys, the two
// order statistics, the threshold, then argmax-and-block passes over the keys.
// stdin: "<n_cases> <n_replays>", then per case "S window c0 .. c(S-1)", then
// per replay "cur outcome base parity".  stdout: per case "T n s0 .. s(n-1)"
// (T with 17 significant digits: exact; n = -1 for a non-finite score; steps
// ascending), then per replay the resulting base.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "traj_pick_core.hpp"

int main() {
    int nc = 0, nr = 0;
    if (std::scanf("%d %d", &nc, &nr) != 2) return 2;
    for (int c = 0; c < nc; c++) {
        int S = 0, window = 0;
        if (std::scanf("%d %d", &S, &window) != 2 || S < 1 || window < 1) return 2;
        std::vector<double> v(static_cast<size_t>(S));
        for (auto &x : v)
            if (std::scanf("%lf", &x) != 1) return 2;
        bool finite = true;
        std::vector<uint64_t> key(v.size());
        for (int r = 0; r < S; r++) {
            finite = finite && adx::tp_finite(v[r]);
            key[r] = adx::tp_key(v[r]);
            if (finite && (key[r] < adx::TP_KEY_MIN || adx::tp_unkey(key[r]) != v[r])) return 3;
        }
        if (!finite) {
            std::printf("nan -1\n");
            continue;
        }
        std::vector<uint64_t> a(key);
        std::sort(a.begin(), a.end());
        int lo, hi;
        double t;
        adx::tp_ranks(S, &lo, &hi, &t);
        const double T = adx::tp_threshold(adx::tp_unkey(a[lo]), adx::tp_unkey(a[hi]), t);
        int n = 0;
        for (;;) {
            uint64_t bk = adx::TP_BLOCKED;
            int bi = S;
            for (int r = S - 1; r >= 0; r--)   // any order: the tie rule decides
                if (adx::tp_beats(key[r], r, bk, bi)) {
                    bk = key[r];
                    bi = r;
                }
            if (!adx::tp_takes(bk, T)) break;
            int b0, b1;
            adx::tp_block(bi, window, S, &b0, &b1);
            if (b0 < 0 || b1 > S || !(b0 <= bi && bi < b1)) return 4;
            for (int r = b0; r < b1; r++)
                if (key[r] != adx::TP_PICKED) key[r] = adx::TP_BLOCKED;
            key[bi] = adx::TP_PICKED;
            n++;
        }
        std::printf("%.17g %d", T, n);
        for (int r = 0; r < S; r++)
            if (key[r] == adx::TP_PICKED) std::printf(" %d", r);
        std::printf("\n");
    }
    for (int k = 0; k < nr; k++) {
        int cur, outcome, base, parity;
        if (std::scanf("%d %d %d %d", &cur, &outcome, &base, &parity) != 4) return 2;
        std::printf("%d\n", int(adx::tp_replay(uint8_t(cur), outcome, base, parity)));
    }
    return 0;
}
