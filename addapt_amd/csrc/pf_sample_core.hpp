// The random numbers and the selection rule of pf_sample_kernel (pf_sample.hip),
// shared by host and device and free of HIP builtins: a host program can
// include this header alone (tests/test_pf_sample_core.py does).  The includer
// may define PS_FN (the kernel: __device__).
//
// Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC'11), counter-based: draw t of sample k of
// batch member w under `seed` is word 0 of
//     philox4x32_10(counter = (t, k, w, 0), key = (seed low, seed high)),
// a pure function of (seed, w, k, t) with no state to keep per stream.
#pragma once

#include <cstdint>

#ifndef PS_FN
#define PS_FN
#endif

namespace adx {
namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;   // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;   // key increments (Weyl)

// ten rounds over the counter c[0..3] in place
PS_FN inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = uint64_t(PHILOX_M0) * c[0], p1 = uint64_t(PHILOX_M1) * c[2];
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c[1] ^ k0, n2 = uint32_t(p0 >> 32) ^ c[3] ^ k1;
        c[1] = uint32_t(p1);
        c[3] = uint32_t(p0);
        c[0] = n0;
        c[2] = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
}

// the 32-bit word of draw t of sample k of batch member w
PS_FN inline uint32_t ps_draw(uint64_t seed, uint32_t w, uint32_t k, uint32_t t) {
    uint32_t c[4] = {t, k, w, 0u};
    philox4x32_10(c, uint32_t(seed), uint32_t(seed >> 32));
    return c[0];
}

// the word's top 24 bits as a float in [0, 1): never 1.0
PS_FN inline float ps_uniform(uint32_t x) { return float(x >> 8) * (1.0f / 16777216.0f); }

// The selection rule.  Among n candidates with weights w[0..n) in their fixed
// order: the first whose inclusive partial sum exceeds u * total, total being
// the sum of these weights (not a table entry); when rounding leaves none, the
// last candidate of nonzero weight.  A candidate of zero (or negative) weight
// is never chosen; -1 when there is none to choose.  The wave's scan
// (pf_sample.hip wave_pick) chooses the same, up to FP64 summation order.
PS_FN inline int pick(const double *w, int n, double u) {
    double total = 0.0;
    for (int c = 0; c < n; c++)
        if (w[c] > 0.0) total += w[c];
    const double thr = u * total;
    double cum = 0.0;
    int last = -1;
    for (int c = 0; c < n; c++) {
        if (!(w[c] > 0.0)) continue;
        cum += w[c];
        last = c;
        if (cum > thr) return c;
    }
    return last;
}

}  // namespace
}  // namespace adx
