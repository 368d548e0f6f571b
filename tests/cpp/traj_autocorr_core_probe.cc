// The sequence autocorrelation's per-lane pieces (addapt_amd/csrc/traj_autocorr_core.hpp)
// on the host, in the lag kernel's order of operations: the two bit planes of a
// series, then per lag and word the funnel shift of two neighbouring words, the
// equality of both planes, the tail mask and the popcount.
// stdin: "<n_series> <n_tau>", then per series "S c0 .. c(S-1)" (codes 1..4), then
// per tau case "max_lag n_series kept baseline m0 .. m(max_lag)".
// stdout: per series "m(0) .. m(S-1)", then per tau case the correlation time.
// The word-pair shift and the tail mask are also checked here against bit-by-bit
// forms (exit status 3 or 4 on a difference).
#include <cstdio>
#include <vector>

#include "traj_autocorr_core.hpp"

// word j of a plane of nw words shifted down by k bits: the funnel of words
// j + k / 64 and the next (words from nw on are 0), as the lag kernel reads them
static uint64_t shifted(const std::vector<uint64_t> &p, int j, int k) {
    const size_t q = static_cast<size_t>(j + (k >> 6));
    const uint64_t a = q < p.size() ? p[q] : 0ull, b = q + 1 < p.size() ? p[q + 1] : 0ull;
    return adx::ta_funnel(a, b, k & 63);
}

static bool helpers_ok() {
    const uint64_t words[] = {0ull, ~0ull, 1ull, 1ull << 63, 0x0123456789abcdefull, 0xfedcba9876543210ull,
                              0xaaaaaaaaaaaaaaaaull};
    for (uint64_t a : words)
        for (uint64_t b : words)
            for (int s = 0; s < 64; s++) {
                uint64_t want = 0;
                for (int i = 0; i < 64; i++) {
                    const int src = i + s;
                    const uint64_t bit = src < 64 ? (a >> src) & 1ull : (b >> (src - 64)) & 1ull;
                    want |= bit << i;
                }
                if (adx::ta_funnel(a, b, s) != want) return false;
            }
    for (int n = 0; n <= 260; n++)
        for (int j = 0; j < 6; j++) {
            uint64_t want = 0;
            for (int i = 0; i < 64; i++)
                if (64 * j + i < n) want |= 1ull << i;
            if (adx::ta_tail_mask(n, j) != want) return false;
        }
    if (adx::ta_tail_mask(1 << 30, (1 << 24) - 1) != ~0ull || adx::ta_tail_mask(1 << 30, 1 << 24) != 0ull) return false;
    return adx::ta_words(1) == 1 && adx::ta_words(64) == 1 && adx::ta_words(65) == 2;
}

int main() {
    if (!helpers_ok()) return 3;
    int ns = 0, nt = 0;
    if (std::scanf("%d %d", &ns, &nt) != 2) return 2;
    for (int c = 0; c < ns; c++) {
        int S = 0;
        if (std::scanf("%d", &S) != 1 || S < 1) return 2;
        const int nw = adx::ta_words(S);
        std::vector<uint64_t> lo(static_cast<size_t>(nw), 0), hi(static_cast<size_t>(nw), 0);
        for (int i = 0; i < S; i++) {
            int code = 0;
            if (std::scanf("%d", &code) != 1 || code < 1 || code > 4) return 2;
            lo[static_cast<size_t>(i / 64)] |= uint64_t((code - 1) & 1) << (i % 64);
            hi[static_cast<size_t>(i / 64)] |= uint64_t((code - 1) >> 1) << (i % 64);
        }
        for (int k = 0; k < S; k++) {
            const int n = S - k;
            long long m = 0;
            for (int j = 0; j < adx::ta_words(n); j++) {
                const size_t jj = static_cast<size_t>(j);
                const uint64_t eq = adx::ta_equal(lo[jj], shifted(lo, j, k), hi[jj], shifted(hi, j, k)) &
                                    adx::ta_tail_mask(n, j);
                m += adx::ta_popcount(eq);
            }
            // words past the valid ones hold no comparison
            if (adx::ta_tail_mask(n, adx::ta_words(n)) != 0) return 4;
            std::printf(k ? " %lld" : "%lld", m);
        }
        std::printf("\n");
    }
    for (int c = 0; c < nt; c++) {
        int max_lag = 0;
        long long n_series = 0, kept = 0;
        double baseline = 0;
        if (std::scanf("%d %lld %lld %lf", &max_lag, &n_series, &kept, &baseline) != 4 || max_lag < 0) return 2;
        std::vector<int64_t> m(static_cast<size_t>(max_lag) + 1);
        for (auto &x : m) {
            long long v = 0;
            if (std::scanf("%lld", &v) != 1) return 2;
            x = v;
        }
        std::printf("%d\n", adx::ta_time(m.data(), max_lag, n_series, kept, baseline));
    }
    return 0;
}
