// Each walker's best sequences from its recorded trajectory (the rule:
// traj_pick_core.hpp), on the device; only the picks cross to the host.
//
//   traj_keys_kernel    the recorded scores are step-major ([r * W + w]): a
//                       trajectory is a column of stride W doubles.  This
//                       pre-pass transposes 32 x 32 tiles through LDS into
//                       trajectory-major ordered keys (both sides coalesced) and
//                       flags trajectories with a non-finite score.  Chosen over
//                       strided column reads because the pick kernel passes over
//                       a trajectory ten times plus once per peak: one extra read
//                       and write makes every pass unit-stride whatever runs next
//                       to it, and the copy is the pick kernel's to overwrite.
//   traj_pick_kernel    one workgroup per trajectory.  The two order statistics
//                       by an exact 8-bit radix select on the keys (histogram in
//                       LDS, eight passes) and one counting pass; then argmax-
//                       and-block passes that overwrite the blocked keys in the
//                       copy (as the reference overwrites its scores), so no
//                       candidate list is kept and a trajectory that is all ties
//                       costs passes, not memory.  Every pass blocks at least the
//                       peak it took: at most ceil(S / window) passes.  The peaks
//                       are marked in the copy and leave in step order.
//   traj_replay_kernel  one wave per walker: the sequence from the record's
//                       starting snapshot through the move log up to the last
//                       pick, positions in lanes (byte q of a lane's word is
//                       position 64 q + lane).  64 log rows are loaded at a time
//                       and the accepted ones walked by ballot; an accepted step
//                       writes its base, or the complement, on the closure list of
//                       the chosen position (traj_pick_core.hpp tp_replay).  The
//                       sequence at each pick is written out and counted per
//                       position and base, in LDS first, then by global atomics.
//
// All stores are plain vector stores and vector atomics; no workgroup waits
// for another.
#include <hip/hip_runtime.h>

#include <cstdint>

#define TP_FN __host__ __device__
#include "launch.hpp"
#include "traj_pick_core.hpp"

namespace adx {

namespace {

constexpr int TPW = 64;            // wave
constexpr int PICK_THREADS = 256;
constexpr int PICK_WAVES = PICK_THREADS / TPW;
constexpr int TILE = 32;

__global__ void __launch_bounds__(256) traj_keys_kernel(const double *scores, int W, int S, int w0, int nw,
                                                        uint64_t *keys, int *bad) {
    __shared__ uint64_t tile[TILE][TILE + 1];
    const int tx = int(threadIdx.x) & (TILE - 1), ty = int(threadIdx.x) / TILE;   // 32 x 8
    const int r0 = int(blockIdx.x) * TILE, c0 = int(blockIdx.y) * TILE;
#pragma unroll
    for (int k = 0; k < TILE; k += 8) {
        const int r = r0 + ty + k, wl = c0 + tx;
        if (r < S && wl < nw) {
            const double x = scores[size_t(r) * W + w0 + wl];
            if (!tp_finite(x)) bad[wl] = 1;
            tile[ty + k][tx] = tp_key(x);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TILE; k += 8) {
        const int wl = c0 + ty + k, r = r0 + tx;
        if (r < S && wl < nw) keys[size_t(wl) * S + r] = tile[tx][ty + k];
    }
}

// the best (key, step) of the workgroup by the tie rule, in every thread
__device__ void block_best(uint64_t &k, int &i, uint64_t *rk, int *ri) {
#pragma unroll
    for (int o = TPW / 2; o > 0; o >>= 1) {
        const uint64_t ok = __shfl_xor((unsigned long long)k, o, TPW);
        const int oi = __shfl_xor(i, o, TPW);
        if (tp_beats(ok, oi, k, i)) {
            k = ok;
            i = oi;
        }
    }
    const int wv = int(threadIdx.x) / TPW;
    __syncthreads();   // the pass before has read rk / ri
    if ((threadIdx.x & (TPW - 1)) == 0) {
        rk[wv] = k;
        ri[wv] = i;
    }
    __syncthreads();
    k = rk[0];
    i = ri[0];
#pragma unroll
    for (int v = 1; v < PICK_WAVES; v++)
        if (tp_beats(rk[v], ri[v], k, i)) {
            k = rk[v];
            i = ri[v];
        }
}

// keys: the chunk's trajectory-major copy (overwritten); scores / W: the
// step-major original, read for the picks' scores (pick_scores, optional)
__global__ void __launch_bounds__(PICK_THREADS) traj_pick_kernel(uint64_t *keys, const int *bad, int S, int window,
                                                                 int cap, int w0, const double *scores, int W,
                                                                 int *n_picks, int32_t *steps, double *pick_scores) {
    __shared__ unsigned hist[256];
    __shared__ uint64_t rk[PICK_WAVES];
    __shared__ int ri[PICK_WAVES];
    __shared__ int sh_bin, sh_below, sh_cnt;
    __shared__ unsigned long long sh_min;
    __shared__ int wave_cnt[PICK_WAVES];
    const int tid = int(threadIdx.x), lane = tid & (TPW - 1), wv = tid / TPW;
    const int wl = int(blockIdx.x), w = w0 + wl;
    uint64_t *key = keys + size_t(wl) * S;
    if (bad[wl]) {   // uniform: a non-finite score, not picked
        if (tid == 0) n_picks[w] = -1;
        return;
    }
    int lo, hi;
    double t;
    tp_ranks(S, &lo, &hi, &t);
    // ---- a[lo]: radix select, most significant byte first
    uint64_t prefix = 0;
    int rank = lo;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        if (tid == 0) {
            sh_cnt = 0;
            sh_min = ~0ull;
        }
        __syncthreads();
        const uint64_t himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        for (int r = tid; r < S; r += PICK_THREADS) {
            const uint64_t k = key[r];
            if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid < TPW) {   // the bin that holds the rank: four bins per lane, a wave scan
            unsigned c[4], s = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                c[q] = hist[4 * tid + q];
                s += c[q];
            }
            unsigned incl = s;
#pragma unroll
            for (int o = 1; o < TPW; o <<= 1) {
                const unsigned v = __shfl_up(incl, o, TPW);
                if (lane >= o) incl += v;
            }
            unsigned below = incl - s;
            if (below <= unsigned(rank) && unsigned(rank) < incl) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (unsigned(rank) < below + c[q]) {
                        sh_bin = 4 * tid + q;
                        sh_below = int(below);
                        break;
                    }
                    below += c[q];
                }
            }
        }
        __syncthreads();
        prefix |= uint64_t(sh_bin) << shift;
        rank -= sh_below;
    }
    // ---- a[hi]: a[lo] again if enough keys are <= it, else the least key above it
    const uint64_t xkey = prefix;
    {
        int cnt = 0;
        unsigned long long mn = ~0ull;
        for (int r = tid; r < S; r += PICK_THREADS) {
            const uint64_t k = key[r];
            if (k <= xkey) cnt++;
            else if (k < mn) mn = k;
        }
        atomicAdd(&sh_cnt, cnt);
        atomicMin(&sh_min, mn);
    }
    __syncthreads();
    const uint64_t ykey = (hi == lo || sh_cnt >= hi + 1) ? xkey : uint64_t(sh_min);
    const double T = tp_threshold(tp_unkey(xkey), tp_unkey(ykey), t);
    // ---- peaks
    int n = 0;
    for (;;) {
        uint64_t bk = TP_BLOCKED;
        int bi = S;
        for (int r = tid; r < S; r += PICK_THREADS) {
            const uint64_t k = key[r];
            if (tp_beats(k, r, bk, bi)) {
                bk = k;
                bi = r;
            }
        }
        block_best(bk, bi, rk, ri);
        if (!tp_takes(bk, T) || n >= cap) break;   // uniform
        int b0, b1;
        tp_block(bi, window, S, &b0, &b1);
        for (int r = b0 + tid; r < b1; r += PICK_THREADS)
            if (key[r] != TP_PICKED) key[r] = r == bi ? TP_PICKED : TP_BLOCKED;
        n++;
        __syncthreads();   // the next pass reads what this one blocked
    }
    // ---- the marked steps, ascending
    int base = 0;
    for (int r0 = 0; r0 < S; r0 += PICK_THREADS) {
        const int r = r0 + tid;
        const bool picked = r < S && key[r] == TP_PICKED;
        const unsigned long long b = __ballot(picked);
        __syncthreads();
        if (lane == 0) wave_cnt[wv] = __popcll(b);
        __syncthreads();
        int off = base, total = 0;
#pragma unroll
        for (int v = 0; v < PICK_WAVES; v++) {
            if (v < wv) off += wave_cnt[v];
            total += wave_cnt[v];
        }
        const int o = off + __popcll(b & ((1ull << lane) - 1ull));
        if (picked && o < cap) {
            steps[size_t(w) * cap + o] = r;
            if (pick_scores) pick_scores[size_t(w) * cap + o] = scores[size_t(r) * W + w];
        }
        base += total;
    }
    if (tid == 0) n_picks[w] = n;
}

constexpr int RP_WPB = 4;   // walkers (waves) per workgroup

__global__ void __launch_bounds__(RP_WPB * TPW) traj_replay_kernel(ReplayArgs a) {
    __shared__ unsigned cnt[256 * 4];
    const int tid = int(threadIdx.x), lane = tid & (TPW - 1), wv = tid / TPW;
    for (int k = tid; k < 256 * 4; k += RP_WPB * TPW) cnt[k] = 0;
    __syncthreads();
    const int w = int(blockIdx.x) * RP_WPB + wv;
    const int N = a.N;
    int n = 0;
    if (w < a.W) n = min(max(a.n_picks[w], 0), a.cap);
    if (n > 0) {
        const int32_t *steps = a.steps + size_t(w) * a.cap;
        uint32_t sq = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = q * TPW + lane;
            sq |= uint32_t(k < N ? a.seq0[size_t(w) * N + k] : 0) << (8 * q);
        }
        int ip = 0, next = steps[0];
        for (int r0 = 0; ip < n; r0 += TPW) {
            const int r = r0 + lane;
            int out = 0, pos = 0, bs = 0;
            if (r < a.rows) {
                const size_t g = size_t(r) * a.W + w;
                out = a.outcome[g];
                pos = a.pos[g];
                bs = a.base[g];
            }
            unsigned long long acc = __ballot(out == 1 || out == 3);
            // the accepted rows of `m`, in step order
            auto apply = [&](unsigned long long m) {
                while (m) {
                    const int l = __ffsll(m) - 1;
                    m &= m - 1;
                    const int p = __shfl(pos, l, TPW), b = __shfl(bs, l, TPW), o = __shfl(out, l, TPW);
                    if (p < 0 || p >= N) continue;
                    const int mi = a.posmap[p];
                    if (mi < 0) continue;
                    for (int k = a.clo_off[mi]; k < a.clo_off[mi + 1]; k++) {
                        const int cp = a.clo_pos[k];
                        if ((cp & (TPW - 1)) == lane) {
                            const int sh = 8 * (cp / TPW);
                            const uint8_t nb = tp_replay(uint8_t(sq >> sh), o, b, a.clo_par[k]);
                            sq = (sq & ~(0xffu << sh)) | (uint32_t(nb) << sh);
                        }
                    }
                }
            };
            while (ip < n && next < r0 + TPW) {
                const int upto = next - r0;   // 0 .. 63
                const unsigned long long m = acc & (upto >= TPW - 1 ? ~0ull : (2ull << upto) - 1ull);
                apply(m);
                acc &= ~m;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k = q * TPW + lane;
                    if (k < N) {
                        const int code = int((sq >> (8 * q)) & 0xffu);
                        const bool ok = code >= 1 && code <= 4;
                        char ch = ok ? char((0x55474341u >> (8 * (code - 1))) & 0xffu) : 'N';   // "ACGU"
                        if (a.lower[k]) ch = char(ch | 0x20);
                        if (a.seqs) a.seqs[(size_t(w) * a.cap + ip) * N + k] = ch;
                        if (ok) atomicAdd(&cnt[k * 4 + code - 1], 1u);
                    }
                }
                ip++;
                next = ip < n ? steps[ip] : 0;
            }
            apply(acc);
        }
    }
    __syncthreads();
    if (a.counts)
        for (int k = tid; k < N * 4; k += RP_WPB * TPW)
            if (cnt[k]) atomicAdd(&a.counts[k], (unsigned long long)cnt[k]);
}

}  // namespace

int traj_pick_chunk(int S, int n_traj) {
    const size_t budget = size_t(512) << 20;   // bytes of keys per launch
    const size_t per = size_t(S > 0 ? S : 1) * sizeof(uint64_t);
    size_t c = budget / per;
    if (c > (size_t(1) << 20)) c = size_t(1) << 20;   // the keys pre-pass' grid.y
    return int(c < 1 ? 1 : (c > size_t(n_traj) ? size_t(n_traj) : c));
}

size_t traj_pick_key_words(int S, int chunk) { return size_t(S) * size_t(chunk); }

hipError_t launch_traj_pick(const double *scores, int W, int S, int window, int cap, int w0, int nw, uint64_t *keys,
                            int *bad, int *n_picks, int32_t *steps, double *pick_scores, hipStream_t stream) {
    if (nw <= 0 || S <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int) * size_t(nw), stream);
    if (e != hipSuccess) return e;
    const dim3 tg((S + TILE - 1) / TILE, (nw + TILE - 1) / TILE);
    hipLaunchKernelGGL(traj_keys_kernel, tg, dim3(256), 0, stream, scores, W, S, w0, nw, keys, bad);
    hipLaunchKernelGGL(traj_pick_kernel, dim3(nw), dim3(PICK_THREADS), 0, stream, keys, bad, S, window, cap, w0, scores,
                       W, n_picks, steps, pick_scores);
    return hipGetLastError();
}

hipError_t launch_traj_replay(const ReplayArgs &a, hipStream_t stream) {
    if (a.W <= 0) return hipSuccess;
    hipLaunchKernelGGL(traj_replay_kernel, dim3((a.W + RP_WPB - 1) / RP_WPB), dim3(RP_WPB * TPW), 0, stream, a);
    return hipGetLastError();
}

}  // namespace adx
