// The per-position autocorrelation of the walkers' sequence trajectories (what the
// reference's auto_corr tool computes from a trajectory file), on the device; only
// integer match counts cross to the host (the quantity: traj_autocorr_core.hpp).
//
//   autocorr_pack_kernel   one wave per walker, as traj_replay_kernel: the sequence
//                          from the record's starting snapshot (positions in lanes:
//                          byte q of a lane's word is position 64 q + lane) through
//                          all recorded rows.  64 log rows are loaded at a time, one
//                          per lane.  For each changeable position a ballot names the
//                          rows whose accepted move writes it; a lane's base after its
//                          row is that of the last such row at or before it, else the
//                          base carried in, and two more ballots give the 64 steps'
//                          word of the low and of the high plane.  The rows before
//                          `discard` are replayed the same way but leave nothing, and
//                          the blocks of 64 start at `discard`, so bit i of a plane is
//                          kept step i.  The same pass counts the four outcomes per
//                          walker and the bases per position over the kept rows (LDS
//                          first, then global atomics, as the replay kernel's counts).
//   autocorr_codes_kernel  the planes of caller-supplied codes (the stateless call);
//                          flags a code outside 1..4.
//   autocorr_lag_kernel    one workgroup per (8 walkers, 8 positions).  A thread owns
//                          one lag of a tile of 256 and walks the words of one
//                          (walker, position) staged in LDS: the plane's words
//                          [j0, j0 + 256) and, for the shifted operand, the words from
//                          j0 + k0 / 64 on.  The lanes of a wave read the same word or
//                          two neighbouring ones (broadcast, no bank conflict) and
//                          differ in the shift, so no lane waits on another and there
//                          is no cross-lane reduction: a thread's 32-bit count of one
//                          (walker, position, lag) goes to its own 64-bit LDS slots,
//                          one per position (summed over the 8 walkers) and one per
//                          walker (summed over the 8 positions), and those leave by
//                          64-bit global atomics, contiguous over the lags.
//
// All stores are plain vector stores and vector atomics; no workgroup waits
// for another.
#include <hip/hip_runtime.h>

#include <cstdint>

#define TA_FN __host__ __device__
#include "launch.hpp"
#include "traj_autocorr_core.hpp"

namespace adx {

namespace {

constexpr int TAW = 64;          // wave
constexpr int PK_WPB = 4;        // pack: walkers (waves) per workgroup
constexpr int LAG_THREADS = 256; // = lags per tile
constexpr int LAG_NW = 8, LAG_NP = 8;   // walkers and positions per workgroup
constexpr int LAG_TJ = 256;      // words of a plane per tile
constexpr int LAG_TB = LAG_TJ + LAG_THREADS / 64 + 1;   // words of the shifted operand's tile

typedef unsigned long long u64;

__global__ void __launch_bounds__(PK_WPB *TAW) autocorr_pack_kernel(AutocorrPackArgs a) {
    __shared__ u64 cnt[256 * 4];
    const int tid = int(threadIdx.x), lane = tid & (TAW - 1), wv = tid / TAW;
    for (int k = tid; k < 256 * 4; k += PK_WPB * TAW) cnt[k] = 0;
    __syncthreads();
    const int wl = int(blockIdx.x) * PK_WPB + wv, w = a.w0 + wl;
    const int N = a.N, S = a.rows, kept = a.rows - a.discard;
    if (wl < a.nw) {   // uniform in the wave
        uint32_t sq = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = q * TAW + lane;
            sq |= uint32_t(k < N ? a.seq0[size_t(w) * N + k] : 0) << (8 * q);
        }
        u64 oc[4] = {0, 0, 0, 0};
        for (int r0 = 0; r0 < S;) {
            const bool keep = r0 >= a.discard;
            const int lim = keep ? min(S, r0 + TAW) : min(a.discard, r0 + TAW);
            const int r = r0 + lane;
            const bool in = r < lim;
            int out = -1, pos = -1, bs = 0;
            if (in) {
                const size_t g = size_t(r) * a.W + w;
                out = a.outcome[g];
                pos = a.pos[g];
                bs = a.base[g];
            }
            int k0 = 0, k1 = 0;   // the closure list of this lane's accepted move
            if ((out == 1 || out == 3) && pos >= 0 && pos < N) {
                const int mi = a.posmap[pos];
                if (mi >= 0) {
                    k0 = a.clo_off[mi];
                    k1 = a.clo_off[mi + 1];
                }
            }
            const u64 valid = __ballot(in);
            const bool moved = __ballot(k1 > k0) != 0;
            if (keep) {
#pragma unroll
                for (int c = 0; c < 4; c++) oc[c] += u64(__popcll(__ballot(out == c)));
            }
            const size_t j = keep ? size_t(r0 - a.discard) / TAW : 0;
            for (int pi = 0; pi < a.P; pi++) {
                const int p = a.chg[pi], pl = p & (TAW - 1), sh = 8 * (p / TAW);
                const int carry = int((uint32_t(__shfl(int(sq), pl, TAW)) >> sh) & 0xffu);
                int v = carry;
                if (moved) {
                    int wr = 0;   // the base this lane's move leaves at p (0: none)
                    for (int k = k0; k < k1; k++)
                        if (a.clo_pos[k] == p) wr = a.clo_par[k] ? 5 - bs : bs;
                    const u64 wm = __ballot(wr != 0);
                    if (wm) {
                        const u64 m = wm & ((2ull << lane) - 1ull);   // writers at or before this row
                        const int src = m ? 63 - __clzll((long long)m) : lane;
                        const int sv = __shfl(wr, src, TAW);
                        if (m) v = sv;
                        const int last = __shfl(v, TAW - 1, TAW);
                        if (lane == pl) sq = (sq & ~(0xffu << sh)) | (uint32_t(last & 0xff) << sh);
                    }
                }
                if (keep) {
                    const int c = v - 1;
                    const u64 lo = __ballot(in && (c & 1)), hi = __ballot(in && (c & 2));
                    if (lane == 0) {
                        u64 *pw = a.planes + (size_t(wl) * a.P + pi) * 2 * a.nwords;
                        pw[j] = lo;
                        pw[a.nwords + j] = hi;
                    }
                    if (lane < 4) {   // A: neither bit, C: low, G: high, U: both
                        const u64 s = lane == 0 ? valid & ~lo & ~hi : lane == 1 ? lo & ~hi : lane == 2 ? ~lo & hi : lo & hi;
                        const int n = __popcll(s);
                        if (n) atomicAdd(&cnt[p * 4 + lane], u64(n));
                    }
                }
            }
            r0 = lim;
        }
        // a position that never changes stands as it started at every kept step
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = q * TAW + lane;
            if (k < N && !a.changeable[k]) {
                const int code = int((sq >> (8 * q)) & 0xffu);
                if (code >= 1 && code <= 4) atomicAdd(&cnt[k * 4 + code - 1], u64(kept));
            }
        }
        if (a.outcome_counts && lane < 4) {
            const u64 n = lane == 0 ? oc[0] : lane == 1 ? oc[1] : lane == 2 ? oc[2] : oc[3];
            a.outcome_counts[size_t(w) * 4 + lane] = n;
        }
    }
    __syncthreads();
    if (a.base_counts)
        for (int k = tid; k < N * 4; k += PK_WPB * TAW)
            if (cnt[k]) atomicAdd(&a.base_counts[k], cnt[k]);
}

// codes[(r * W + w) * P + p]; one wave per trajectory of the chunk [w0, w0 + nw)
__global__ void __launch_bounds__(PK_WPB *TAW) autocorr_codes_kernel(const uint8_t *codes, int W, int S, int P, int w0,
                                                                     int nw, int nwords, u64 *planes, int *bad) {
    const int tid = int(threadIdx.x), lane = tid & (TAW - 1), wv = tid / TAW;
    const int wl = int(blockIdx.x) * PK_WPB + wv, w = w0 + wl;
    if (wl >= nw) return;
    bool wrong = false;
    for (int r0 = 0; r0 < S; r0 += TAW) {
        const int r = r0 + lane;
        const bool in = r < S;
        const uint8_t *row = codes + (size_t(in ? r : 0) * W + w) * P;
        for (int p = 0; p < P; p++) {
            const int c = int(row[p]) - 1;
            if (in && (c < 0 || c > 3)) wrong = true;
            const u64 lo = __ballot(in && (c & 1)), hi = __ballot(in && (c & 2));
            if (lane == 0) {
                u64 *pw = planes + (size_t(wl) * P + p) * 2 * nwords;
                pw[r0 / TAW] = lo;
                pw[nwords + r0 / TAW] = hi;
            }
        }
    }
    if (wrong) *bad = 1;
}

// planes: the chunk's [nw walkers][P positions][2 planes][nwords]; S kept steps;
// lags 0..K.  pos_matches[P * (K + 1)] and walker_matches[W * (K + 1)] are added to.
__global__ void __launch_bounds__(LAG_THREADS) autocorr_lag_kernel(const u64 *planes, int nw, int P, int nwords, int S,
                                                                   int K, int w0, u64 *pos_matches,
                                                                   u64 *walker_matches) {
    __shared__ u64 a_lo[LAG_TJ], a_hi[LAG_TJ], b_lo[LAG_TB], b_hi[LAG_TB];
    __shared__ u64 pacc[LAG_NP][LAG_THREADS], wacc[LAG_NW][LAG_THREADS];
    const int tid = int(threadIdx.x);
    const int wl0 = int(blockIdx.x) * LAG_NW, p0 = int(blockIdx.y) * LAG_NP;
    const int nwl = min(LAG_NW, nw - wl0), np = min(LAG_NP, P - p0);
    for (int k0 = 0; k0 <= K; k0 += LAG_THREADS) {
        const int k = k0 + tid;
        const bool mine = k <= K;
        const int n = mine ? S - k : 0;            // comparisons at this lag (K <= S - 1: n >= 1)
        const int qo = (k >> 6) - (k0 >> 6), s = k & 63;
#pragma unroll
        for (int i = 0; i < LAG_NP; i++) pacc[i][tid] = 0;
#pragma unroll
        for (int i = 0; i < LAG_NW; i++) wacc[i][tid] = 0;
        for (int wi = 0; wi < nwl; wi++)
            for (int pi = 0; pi < np; pi++) {
                const u64 *lo = planes + (size_t(wl0 + wi) * P + p0 + pi) * 2 * nwords, *hi = lo + nwords;
                unsigned c = 0;   // at most S < 2^30
                // the words that hold the least lag's comparisons: uniform bounds
                const int nv0 = ta_words(S - k0);
                for (int j0 = 0; j0 < nv0; j0 += LAG_TJ) {
                    __syncthreads();   // the tile before is read
                    for (int i = tid; i < LAG_TJ; i += LAG_THREADS) {
                        const int g = j0 + i;
                        a_lo[i] = g < nwords ? lo[g] : 0ull;
                        a_hi[i] = g < nwords ? hi[g] : 0ull;
                    }
                    for (int i = tid; i < LAG_TB; i += LAG_THREADS) {
                        const int g = j0 + (k0 >> 6) + i;
                        b_lo[i] = g < nwords ? lo[g] : 0ull;
                        b_hi[i] = g < nwords ? hi[g] : 0ull;
                    }
                    __syncthreads();
                    auto equal = [&](int i) {
                        const u64 lk = ta_funnel(b_lo[i + qo], b_lo[i + qo + 1], s);
                        const u64 hk = ta_funnel(b_hi[i + qo], b_hi[i + qo + 1], s);
                        return ta_equal(a_lo[i], lk, a_hi[i], hk);
                    };
                    // whole words first; only the last word of the n comparisons needs the mask
                    const int jf = min(LAG_TJ, (n >> 6) - j0);
                    for (int i = 0; i < jf; i++) c += unsigned(ta_popcount(equal(i)));
                    const int it = (n >> 6) - j0;
                    if ((n & 63) && it >= 0 && it < LAG_TJ) c += unsigned(ta_popcount(equal(it) & ta_tail_mask(n, n >> 6)));
                }
                pacc[pi][tid] += c;
                wacc[wi][tid] += c;
            }
        if (mine) {
            for (int pi = 0; pi < np; pi++) atomicAdd(&pos_matches[size_t(p0 + pi) * (K + 1) + k], pacc[pi][tid]);
            if (walker_matches)
                for (int wi = 0; wi < nwl; wi++)
                    atomicAdd(&walker_matches[size_t(w0 + wl0 + wi) * (K + 1) + k], wacc[wi][tid]);
        }
    }
}

}  // namespace

int traj_autocorr_chunk(int kept, int P, int n_traj) {
    const size_t budget = size_t(512) << 20;   // bytes of planes per launch
    const size_t per = size_t(P > 0 ? P : 1) * 2 * size_t(ta_words(kept > 0 ? kept : 1)) * sizeof(uint64_t);
    size_t c = budget / per;
    return int(c < 1 ? 1 : (c > size_t(n_traj) ? size_t(n_traj) : c));
}

size_t traj_autocorr_plane_words(int kept, int P, int chunk) {
    return size_t(chunk) * size_t(P) * 2 * size_t(ta_words(kept));
}

hipError_t launch_autocorr_pack(const AutocorrPackArgs &a, hipStream_t stream) {
    if (a.nw <= 0) return hipSuccess;
    hipLaunchKernelGGL(autocorr_pack_kernel, dim3((a.nw + PK_WPB - 1) / PK_WPB), dim3(PK_WPB * TAW), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_autocorr_pack_codes(const uint8_t *codes, int W, int S, int P, int w0, int nw, uint64_t *planes,
                                      int *bad, hipStream_t stream) {
    if (nw <= 0) return hipSuccess;
    hipLaunchKernelGGL(autocorr_codes_kernel, dim3((nw + PK_WPB - 1) / PK_WPB), dim3(PK_WPB * TAW), 0, stream, codes, W,
                       S, P, w0, nw, ta_words(S), reinterpret_cast<u64 *>(planes), bad);
    return hipGetLastError();
}

hipError_t launch_autocorr_lags(const uint64_t *planes, int nw, int P, int kept, int max_lag, int w0,
                                unsigned long long *pos_matches, unsigned long long *walker_matches,
                                hipStream_t stream) {
    if (nw <= 0 || P <= 0) return hipSuccess;
    const dim3 grid((nw + LAG_NW - 1) / LAG_NW, (P + LAG_NP - 1) / LAG_NP);
    hipLaunchKernelGGL(autocorr_lag_kernel, grid, dim3(LAG_THREADS), 0, stream, reinterpret_cast<const u64 *>(planes),
                       nw, P, ta_words(kept), kept, max_lag, w0, pos_matches, walker_matches);
    return hipGetLastError();
}

}  // namespace adx
