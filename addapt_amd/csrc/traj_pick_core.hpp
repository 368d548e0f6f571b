// The per-lane pieces of the trajectory picking rule (traj_pick.hip), shared by
// host and device and free of HIP builtins: a host program can include this
// header alone (tests/test_traj_pick_core.py does).  The includer may define
// TP_FN (the kernels: __host__ __device__).
//
// The rule, for one trajectory of S finite scores c[0..S) and a window >= 1:
//   threshold  T = the 75th percentile with linear interpolation between the
//              order statistics a[lo], a[min(lo + 1, S - 1)], lo = floor(0.75 (S - 1))
//   peaks      repeat: among the steps not yet blocked take the largest score
//              (lowest index among equals); stop if none is left or it is not
//              >= T; else record it and block [max(i - window, 0), min(i + window, S))
//   output     the peaks in ascending step order
// Every pass blocks at least its own peak (window >= 1), so there are at most
// ceil(S / window) passes.
#pragma once

#include <cstdint>

#ifndef TP_FN
#define TP_FN
#endif

namespace adx {
namespace {

// Keys below TP_KEY_MIN belong to no finite double: the kernel marks blocked
// steps (TP_BLOCKED) and recorded peaks (TP_PICKED) with them.
constexpr uint64_t TP_BLOCKED = 0, TP_PICKED = 1, TP_KEY_MIN = 2;

TP_FN inline uint64_t tp_bits(double x) {
    union { double d; uint64_t u; } v;
    v.d = x;
    return v.u;
}

TP_FN inline double tp_from_bits(uint64_t u) {
    union { double d; uint64_t u; } v;
    v.u = u;
    return v.d;
}

TP_FN inline bool tp_finite(double x) { return (tp_bits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// The order-preserving key of a finite double: a < b  <=>  key(a) < key(b) and
// a == b  <=>  key(a) == key(b) (-0.0 takes +0.0's key, as operator== has it).
// Finite doubles map to [0x0010000000000000, 0xffefffffffffffff]: >= TP_KEY_MIN.
TP_FN inline uint64_t tp_key(double x) {
    uint64_t b = tp_bits(x);
    if ((b << 1) == 0) b = 0;   // -0.0 -> +0.0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

TP_FN inline double tp_unkey(uint64_t k) { return tp_from_bits((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }

// ranks of the two order statistics the percentile interpolates between, and
// the interpolation weight: h = 0.75 (S - 1), lo = floor(h), t = h - lo
TP_FN inline void tp_ranks(int S, int *lo, int *hi, double *t) {
    const double h = 0.75 * double(S - 1);
    const int l = int(h);   // h >= 0: truncation is the floor
    *lo = l;
    *hi = l + 1 < S ? l + 1 : S - 1;
    *t = h - double(l);
}

// the threshold from the two order statistics x = a[lo] <= y = a[hi]
TP_FN inline double tp_threshold(double x, double y, double t) {
    const double d = y - x;
    return t < 0.5 ? x + d * t : y - d * (1.0 - t);
}

// the steps a peak at i blocks: [lo, hi) (window >= 1, so i itself is in it)
TP_FN inline void tp_block(int i, int window, int S, int *lo, int *hi) {
    *lo = window >= i ? 0 : i - window;
    *hi = window >= S - i ? S : i + window;
}

// the argmax tie rule: candidate (ka, ia) beats (kb, ib)
TP_FN inline bool tp_beats(uint64_t ka, int ia, uint64_t kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// the peak (key, step) is taken: not blocked, and its score >= T
TP_FN inline bool tp_takes(uint64_t key, double T) { return key >= TP_KEY_MIN && tp_unkey(key) >= T; }

// One replay step at one position of a move's closure list: an accepted step
// (outcome 1 worsened, 3 improved) writes the move's base, or its complement
// 5 - base where the position's parity is odd; any other outcome keeps `cur`.
TP_FN inline uint8_t tp_replay(uint8_t cur, int outcome, int base, int parity) {
    if (outcome != 1 && outcome != 3) return cur;
    return uint8_t(parity ? 5 - base : base);
}

}  // namespace
}  // namespace adx
