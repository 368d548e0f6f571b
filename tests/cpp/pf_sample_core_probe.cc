// The sampler's generator and selection rule (addapt_amd/csrc/pf_sample_core.hpp)
// on the host.  stdin: "<n_draws> <n_picks>", then n_draws lines "seed w k t",
// then n_picks lines "u n w0 .. w(n-1)".  stdout: per draw "<word> <u>" (u with 17
// significant digits: exact), then per pick the chosen index.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "pf_sample_core.hpp"

int main() {
    int nd = 0, np = 0;
    if (std::scanf("%d %d", &nd, &np) != 2) return 2;
    for (int d = 0; d < nd; d++) {
        uint64_t seed;
        uint32_t w, k, t;
        if (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32, &seed, &w, &k, &t) != 4) return 2;
        const uint32_t x = adx::ps_draw(seed, w, k, t);
        std::printf("%" PRIu32 " %.17g\n", x, double(adx::ps_uniform(x)));
    }
    for (int p = 0; p < np; p++) {
        double u;
        int n;
        if (std::scanf("%lf %d", &u, &n) != 2 || n < 0) return 2;
        std::vector<double> w(static_cast<size_t>(n));
        for (auto &x : w)
            if (std::scanf("%lf", &x) != 1) return 2;
        std::printf("%d\n", adx::pick(w.data(), n, u));
    }
    return 0;
}
