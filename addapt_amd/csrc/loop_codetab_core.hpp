// The 1x1, 1x2, 2x1 and 2x2 interior-loop energies of the packed 16-bit MFE
// tables by code pair (mfe_pair.hip bcell_tables; built at upload, api_problem.hpp).
//
// A B cell holds two byte codes: the closing pair's oc = type * 25 + S[i+1] * 5
// + S[j-1] and the inner pair's code c = rtype * 25 + S[q+1] * 5 + S[p-1] (CP::cc,
// the inner pair (p, q) seen from inside the loop).  DevTables::int11, int21 and
// int22 are indexed by the types and the unpaired bases, which the kernel took
// out of the codes with / 5 and % 5 in front of every load.  Each of the four
// energies is a function of (oc, c) alone, so the table here holds
//     E[k][oc][c],  k = LCT_11, LCT_12, LCT_21, LCT_22,
// filled with the kernel's former index formulas for every code pair, the codes
// of non-pairable inner cells (type 0) included: the kernel reads those too and
// must get what it got.  An entry of the packed tables has equal 16-bit halves
// (apo | holo of one energy model); the table stores one half, and the kernel
// puts it back into both.
//
// Plain C++ (no HIP): the host builds the table, tests/test_loop_codetab_core.py
// checks it stand-alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace adx {

constexpr int LCT_CODES = 175;   // codes 0 .. 174: types 0 .. 6, two bases 0 .. 4
constexpr int LCT_11 = 0, LCT_12 = 1, LCT_21 = 2, LCT_22 = 3;
constexpr size_t LCT_SIZE = size_t(4) * LCT_CODES * LCT_CODES;
// entries allocated: a code byte above 174 (none is ever stored) still reads inside the buffer
constexpr size_t LCT_ALLOC = LCT_SIZE + 256;

constexpr int loop_codetab_index(int k, int oc, int c) { return (k * LCT_CODES + oc) * LCT_CODES + c; }

// The word index into int11[8][8][5][5] (k = LCT_11), int21[8][8][5][5][5] (LCT_12,
// LCT_21) or int22[8][8][5][5][5][5] (LCT_22) that the energy of closing code oc and
// inner code c is read at
constexpr int loop_codetab_source(int k, int oc, int c) {
    const int type = oc / 25, si1 = (oc / 5) % 5, sj1 = oc % 5;   // the closing pair: type, S[i+1], S[j-1]
    const int t2 = c / 25, cq = (c / 5) % 5, cp = c % 5;          // the inner pair: rtype, S[q+1], S[p-1]
    return k == LCT_11   ? ((type * 8 + t2) * 5 + si1) * 5 + sj1
           : k == LCT_12 ? (((type * 8 + t2) * 5 + si1) * 5 + cq) * 5 + sj1   // int21[type][t2][si1][sq1][sj1]
           : k == LCT_21 ? (((t2 * 8 + type) * 5 + cq) * 5 + si1) * 5 + cp    // int21[t2][type][sq1][si1][sp1]
                         : ((((type * 8 + t2) * 5 + si1) * 5 + cp) * 5 + cq) * 5 + sj1;   // int22[type][t2][si1][sp1][sq1][sj1]
}

// E (LCT_ALLOC entries) from the packed tables.  False when a word's halves differ
// (the table cannot hold it; upload_mfe16 then leaves the packed kernels off)
inline bool loop_codetab_build(const uint32_t *int11, const uint32_t *int21, const uint32_t *int22, uint16_t *E) {
    for (size_t n = LCT_SIZE; n < LCT_ALLOC; n++) E[n] = 0x7FFFu;
    for (int k = 0; k < 4; k++) {
        const uint32_t *src = k == LCT_11 ? int11 : (k == LCT_22 ? int22 : int21);
        for (int oc = 0; oc < LCT_CODES; oc++)
            for (int c = 0; c < LCT_CODES; c++) {
                const uint32_t w = src[loop_codetab_source(k, oc, c)];
                if ((w & 0xFFFFu) != (w >> 16)) return false;
                E[loop_codetab_index(k, oc, c)] = uint16_t(w & 0xFFFFu);
            }
    }
    return true;
}

}  // namespace adx
