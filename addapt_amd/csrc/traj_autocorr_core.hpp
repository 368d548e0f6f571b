// The per-lane pieces of the sequence autocorrelation of recorded trajectories
// (traj_autocorr.hip), shared by host and device and free of HIP builtins: a
// host program can include this header alone (tests/test_traj_autocorr_core.py
// does).  The includer may define TA_FN (the kernels: __host__ __device__).
//
// The quantity, for one series x[0..S) of base codes 1..4 and a lag k < S:
//   m(k) = #{ i in [0, S - k) : x[i + k] == x[i] }
// The series is kept as two bit planes, the low and the high bit of code - 1,
// bit i of a plane in bit (i mod 64) of its word i / 64; bits from S on are 0.
// x[i + k] == x[i] where both planes agree with themselves shifted down by k
// bits; the shift crosses words (ta_funnel), and the last word of the S - k
// comparisons is masked to its valid bits (ta_tail_mask).
#pragma once

#include <cstdint>

#ifndef TA_FN
#define TA_FN
#endif

namespace adx {
namespace {

// words of a plane of S bits
TA_FN inline int ta_words(int S) { return (S + 63) / 64; }

// bits [s, s + 64) of the 128-bit value (b : a), a the low word; 0 <= s < 64
TA_FN inline uint64_t ta_funnel(uint64_t a, uint64_t b, int s) { return s ? (a >> s) | (b << (64 - s)) : a; }

// the valid bits of word j where only the first n bits of the plane count
TA_FN inline uint64_t ta_tail_mask(int n, int j) {
    const long long left = (long long)n - 64ll * j;
    if (left <= 0) return 0;
    return left >= 64 ? ~0ull : (1ull << left) - 1ull;
}

// bit i set: both planes' bit i equals the shifted planes' bit i
TA_FN inline uint64_t ta_equal(uint64_t lo, uint64_t lo_k, uint64_t hi, uint64_t hi_k) {
    return ~(lo ^ lo_k) & ~(hi ^ hi_k);
}

TA_FN inline int ta_popcount(uint64_t x) { return __builtin_popcountll(x); }

// The correlation time of a pooled curve: a_k = matches[k] / (n_series (kept - k)),
// tau = the least k >= 1 with a_k - baseline <= (1 - baseline) / e; -1 if no lag
// up to max_lag does it (the curve has not decayed), 0 if baseline >= 1 (nothing
// ever changed).
inline int ta_time(const int64_t *matches, int max_lag, int64_t n_series, int64_t kept, double baseline) {
    if (baseline >= 1.0) return 0;
    const double level = (1.0 - baseline) / 2.718281828459045235360287471352662498;
    for (int k = 1; k <= max_lag && k < kept; k++) {
        const double a = double(matches[k]) / (double(n_series) * double(kept - k));
        if (a - baseline <= level) return k;
    }
    return -1;
}

}  // namespace
}  // namespace adx
