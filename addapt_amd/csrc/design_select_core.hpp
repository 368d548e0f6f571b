// The per-lane pieces of the design selection rule (design_select.hip), shared
// by host and device and free of HIP builtins: a host program can include this
// header alone (tests/test_design_select_core.py does).  The includer may define
// TP_FN (the kernels: __host__ __device__).
//
// The rule, for M entries (a sequence of N bases and a score each), a radius
// r >= 0 and a cap K >= 1:
//   distance   the Hamming distance, bases compared case-insensitively
//   order      score descending (operator==: -0.0 ties with +0.0), ties by the
//              lower entry index; an entry with a non-finite score takes no part
//   selection  while fewer than K designs exist and an uncovered entry is left:
//              the first uncovered entry in order leads design d = 0, 1, ..., and
//              every uncovered entry within r of it (itself included) is covered
//              by d.  So an entry leads iff no earlier leader is within r of it,
//              and otherwise belongs to the lowest-numbered leader within r.
//   pair_hist  [d] = the unordered pairs of finite-score entries at distance d
// A sequence is held as two bit planes (low and high bit of its base's code
// A, C, G, U = 0..3), 64 positions per word, ds_words(N) words per plane, the
// padding bits of the last word zero in both; the distance is then
// sum over words of popcount((lo_a ^ lo_b) | (hi_a ^ hi_b)).
#pragma once

#include <cstdint>

#include "traj_pick_core.hpp"

namespace adx {
namespace {

constexpr int DS_MAX_WORDS = 4;   // N <= 255

TP_FN inline int ds_words(int N) { return (N + 63) / 64; }

// the code of a base, -1 for a character outside ACGU / acgu
TP_FN inline int ds_code(char ch) {
    switch (ch | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 'u': return 3;
    default: return -1;
    }
}

TP_FN inline char ds_base(int code) { return char((0x55474341u >> (8 * (code & 3))) & 0xffu); }   // "ACGU"

// word `w` of the two planes of seq[0..N); false at a bad character (its bits stay 0)
TP_FN inline bool ds_pack_word(const char *seq, int N, int w, uint64_t *lo, uint64_t *hi) {
    uint64_t l = 0, h = 0;
    bool ok = true;
    for (int b = 0; b < 64 && 64 * w + b < N; b++) {
        const int c = ds_code(seq[64 * w + b]);
        if (c < 0) {
            ok = false;
            continue;
        }
        l |= uint64_t(c & 1) << b;
        h |= uint64_t(c >> 1) << b;
    }
    *lo = l;
    *hi = h;
    return ok;
}

// the base (upper case) at position p of planes lo[], hi[]
TP_FN inline char ds_unpack(const uint64_t *lo, const uint64_t *hi, int p) {
    return ds_base(int((lo[p >> 6] >> (p & 63)) & 1) | int(((hi[p >> 6] >> (p & 63)) & 1) << 1));
}

// the positions of one word at which two sequences differ
TP_FN inline int ds_word_dist(uint64_t lo_a, uint64_t hi_a, uint64_t lo_b, uint64_t hi_b) {
    return __builtin_popcountll((lo_a ^ lo_b) | (hi_a ^ hi_b));
}

// the sort key: ascending in it is the rule's order (score descending); a
// non-finite score sorts behind every finite one (no finite key is all ones)
constexpr uint64_t DS_KEY_NONE = ~0ull;
TP_FN inline uint64_t ds_sort_key(double score) { return tp_finite(score) ? ~tp_key(score) : DS_KEY_NONE; }

// the order: entry (score a, index ia) stands before entry (score b, index ib); both finite
TP_FN inline bool ds_before(double a, int ia, double b, int ib) { return tp_beats(tp_key(a), ia, tp_key(b), ib); }

TP_FN inline bool ds_covers(int dist, int radius) { return dist <= radius; }

// A walker's picks are consecutive entries; design[0..k] are the designs of its
// first k + 1 (-1: none).  Pick k counts towards its design's walkers iff it has
// a design and no earlier pick of the walker has the same.
TP_FN inline bool ds_first_of_walker(const int32_t *design, int k) {
    const int32_t d = design[k];
    if (d < 0) return false;
    for (int j = 0; j < k; j++)
        if (design[j] == d) return false;
    return true;
}

}  // namespace
}  // namespace adx
