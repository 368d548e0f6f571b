// Distinct designs from scored sequences by greedy Hamming selection (the rule:
// design_select_core.hpp), on the device; only designs and a histogram leave.
//
//   design_pack_kernel     one wave per sequence, positions in lanes: two ballots
//                          per 64 positions are the words of its two bit planes
//                          ([plane][word][entry], so entries are unit-stride for
//                          every later kernel).  Also the entry's sort key, the
//                          count of finite scores and the bad-character flag.
//                          For a record the wave's slot (walker, pick) is an
//                          entry only if the walker has that many picks; the
//                          entry index comes from a scan of the pick counts.
//   radix_*_kernel         the order: a stable LSD radix sort of (key, entry), 8
//                          bits a pass.  Per pass a histogram per block of 1024
//                          consecutive elements, one exclusive scan over
//                          [digit][block], and a scatter that ranks the elements
//                          of a block stably (same-digit lanes of a wave by
//                          ballots, waves and sub-tiles by running counts).
//   design_resolve_kernel  selection by tiles of 1024 ranked entries.  One
//   design_cover_kernel    workgroup resolves a tile: the lowest uncovered rank
//                          leads the next design and covers the tile's entries
//                          within the radius, until none is uncovered or the cap
//                          is reached.  Then every later rank is compared with
//                          the tile's new leaders, in design order, by a grid of
//                          its own.  Workgroups meet only at kernel boundaries.
//   design_hist_kernel     the distances of all pairs of finite-score entries: a
//                          thread keeps a row's planes in registers, 256 columns
//                          at a time are staged in LDS and read as broadcasts.
//                          Entries are in rank order, where equal sequences (equal
//                          scores) stand side by side: a lane counts a run of
//                          equal distances in a register and adds it to the
//                          workgroup's LDS histogram when the distance changes.
//                          Each workgroup flushes once, with 64-bit atomics.
//   design_walkers_kernel, the record's glue: how many distinct walkers hold each
//   design_gather_kernel   design, and the leaders' walker, step, score, sequence.
//
// All stores are plain vector stores and integer vector atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#define TP_FN __host__ __device__
#include "design_select_core.hpp"
#include "launch.hpp"

namespace adx {

namespace {

constexpr int DSW = 64;              // wave
constexpr int PACK_WAVES = 4;
constexpr int SORT_THREADS = 256;
constexpr int SORT_SUBTILES = 4;
constexpr int SORT_TILE = SORT_THREADS * SORT_SUBTILES;
constexpr int SORT_WAVES = SORT_THREADS / DSW;
constexpr int SCAN_THREADS = 1024;
constexpr int SEL_TILE = 1024;       // ranked entries a workgroup resolves
constexpr int SEL_WAVES = SEL_TILE / DSW;
constexpr int HIST_TILE = 256;
constexpr int HIST_GROUP = 8;        // column tiles per workgroup
constexpr int MAX_PW = 2 * DS_MAX_WORDS;

__global__ void __launch_bounds__(PACK_WAVES *DSW) design_pack_kernel(const char *seqs, const double *scores, int N,
                                                                       int n_slots, const int *n_picks,
                                                                       const int *offset, int cap, int M,
                                                                       uint64_t *planes, uint64_t *keys, int32_t *idx,
                                                                       int32_t *src_of, int *flags) {
    const int lane = int(threadIdx.x) & (DSW - 1);
    const int s = int(blockIdx.x) * PACK_WAVES + int(threadIdx.x) / DSW;   // wave-uniform
    if (s >= n_slots) return;
    int e = s;
    if (n_picks) {
        const int w = s / cap, k = s - w * cap;
        if (k >= n_picks[w]) return;
        e = offset[w] + k;
    }
    if (e >= M) return;
    const int NW = ds_words(N);
    for (int wd = 0; wd < NW; wd++) {
        const int p = wd * DSW + lane;
        const int code = p < N ? ds_code(seqs[size_t(s) * N + p]) : 0;
        const unsigned long long lo = __ballot(code > 0 && (code & 1)), hi = __ballot(code > 0 && (code & 2));
        const bool wrong = __ballot(code < 0) != 0;
        if (lane == 0) {
            planes[size_t(wd) * M + e] = lo;
            planes[size_t(NW + wd) * M + e] = hi;
            if (wrong) flags[DESIGN_BAD] = 1;
        }
    }
    if (lane == 0) {
        const uint64_t key = ds_sort_key(scores[s]);
        keys[e] = key;
        idx[e] = e;
        if (src_of) src_of[e] = s;
        if (key != DS_KEY_NONE) atomicAdd(&flags[DESIGN_FINITE], 1);
    }
}

// out[i] = the sum of max(in[j], 0) over j < i, *total = the sum over all; one workgroup (in may be out)
__global__ void __launch_bounds__(SCAN_THREADS) design_scan_kernel(const int *in, int *out, int n, int *total) {
    __shared__ int wave_sum[SCAN_THREADS / DSW];
    const int tid = int(threadIdx.x), lane = tid & (DSW - 1), wv = tid / DSW;
    const int per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int b = min(tid * per, n), e = min(b + per, n);
    int s = 0;
    for (int i = b; i < e; i++) s += max(in[i], 0);
    int incl = s;
#pragma unroll
    for (int o = 1; o < DSW; o <<= 1) {
        const int v = __shfl_up(incl, o, DSW);
        if (lane >= o) incl += v;
    }
    if (lane == DSW - 1) wave_sum[wv] = incl;
    __syncthreads();
    int run = incl - s, all = 0;
    for (int v = 0; v < SCAN_THREADS / DSW; v++) {
        if (v < wv) run += wave_sum[v];
        all += wave_sum[v];
    }
    for (int i = b; i < e; i++) {
        const int x = max(in[i], 0);
        out[i] = run;
        run += x;
    }
    if (tid == 0 && total) *total = all;
}

// hist[digit * gridDim.x + block]: the block's elements with that digit
__global__ void __launch_bounds__(SORT_THREADS) radix_hist_kernel(const uint64_t *keys, int M, int shift, int *hist) {
    __shared__ int cnt[256];
    const int tid = int(threadIdx.x);
    cnt[tid] = 0;
    __syncthreads();
    const int b0 = int(blockIdx.x) * SORT_TILE;
    for (int k = 0; k < SORT_SUBTILES; k++) {
        const int i = b0 + k * SORT_THREADS + tid;
        if (i < M) atomicAdd(&cnt[int((keys[i] >> shift) & 255)], 1);
    }
    __syncthreads();
    hist[size_t(tid) * gridDim.x + blockIdx.x] = cnt[tid];
}

// base[digit * gridDim.x + block]: where the block's first element with that digit goes
__global__ void __launch_bounds__(SORT_THREADS) radix_scatter_kernel(const uint64_t *keys, const int32_t *idx, int M,
                                                                      int shift, const int *base, uint64_t *keys_out,
                                                                      int32_t *idx_out) {
    __shared__ int run[256];
    __shared__ int cnt[SORT_WAVES][256];
    const int tid = int(threadIdx.x), lane = tid & (DSW - 1), wv = tid / DSW;
    run[tid] = base[size_t(tid) * gridDim.x + blockIdx.x];
    const int b0 = int(blockIdx.x) * SORT_TILE;
    for (int k = 0; k < SORT_SUBTILES; k++) {
#pragma unroll
        for (int v = 0; v < SORT_WAVES; v++) cnt[v][tid] = 0;
        __syncthreads();   // and run[] of the sub-tile before is complete
        const int i = b0 + k * SORT_THREADS + tid;
        const bool on = i < M;
        uint64_t key = 0;
        int32_t id = 0;
        int d = 0;
        if (on) {
            key = keys[i];
            id = idx[i];
            d = int((key >> shift) & 255);
        }
        // the lanes of this wave with the same digit
        unsigned long long same = __ballot(on);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const unsigned long long m = __ballot(on && ((d >> bit) & 1));
            same &= ((d >> bit) & 1) ? m : ~m;
        }
        const int below = __popcll(same & ((1ull << lane) - 1ull));
        if (on && below == 0) cnt[wv][d] = __popcll(same);
        __syncthreads();
        if (on) {
            int o = run[d] + below;
            for (int v = 0; v < wv; v++) o += cnt[v][d];
            keys_out[o] = key;
            idx_out[o] = id;
        }
        __syncthreads();   // run[] read
        int add = 0;
#pragma unroll
        for (int v = 0; v < SORT_WAVES; v++) add += cnt[v][tid];
        run[tid] += add;
    }
}

// the planes in rank order: rp[pw][q] = planes[pw][order[q]]
__global__ void __launch_bounds__(256) design_rank_planes_kernel(const uint64_t *planes, const int32_t *order, int M,
                                                                 int PW, uint64_t *rp) {
    const int q = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (q >= M) return;
    const int e = order[q];
    for (int pw = 0; pw < PW; pw++) rp[size_t(pw) * M + q] = planes[size_t(pw) * M + e];
}

__device__ inline int planes_dist(const uint64_t *a, const uint64_t *b, int NW) {
    int d = 0;
#pragma unroll
    for (int w = 0; w < DS_MAX_WORDS; w++)
        if (w < NW) d += ds_word_dist(a[w], a[DS_MAX_WORDS + w], b[w], b[DS_MAX_WORDS + w]);
    return d;
}

// state: [0] designs so far, [1], [2] the range of designs the last resolved tile added
__global__ void __launch_bounds__(SEL_TILE) design_resolve_kernel(const uint64_t *rp, int M, int NW, int q0,
                                                                   const int *flags, int radius, int K,
                                                                   int32_t *member_rank, int *state,
                                                                   int32_t *leader_rank, uint64_t *lead) {
    __shared__ int wmin[SEL_WAVES];
    __shared__ uint64_t lp[MAX_PW];
    const int tid = int(threadIdx.x), lane = tid & (DSW - 1), wv = tid / DSW;
    const int F = flags[DESIGN_FINITE], q = q0 + tid;
    uint64_t a[MAX_PW] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool open = false;
    if (q < F) {
#pragma unroll
        for (int w = 0; w < DS_MAX_WORDS; w++)
            if (w < NW) {
                a[w] = rp[size_t(w) * M + q];
                a[DS_MAX_WORDS + w] = rp[size_t(NW + w) * M + q];
            }
        open = member_rank[q] < 0;
    }
    const int n0 = state[0];
    int n = n0;
    __syncthreads();   // every thread has read state[0] before thread 0 writes it
    while (n < K) {
        const unsigned long long b = __ballot(open);
        if (lane == 0) wmin[wv] = b ? wv * DSW + __ffsll(b) - 1 : INT_MAX;
        __syncthreads();
        int m = INT_MAX;
#pragma unroll
        for (int v = 0; v < SEL_WAVES; v++) m = min(m, wmin[v]);
        if (m == INT_MAX) break;   // uniform
        if (tid == m) {
#pragma unroll
            for (int w = 0; w < DS_MAX_WORDS; w++)
                if (w < NW) {
                    lp[w] = a[w];
                    lp[DS_MAX_WORDS + w] = a[DS_MAX_WORDS + w];
                    lead[size_t(w) * K + n] = a[w];
                    lead[size_t(NW + w) * K + n] = a[DS_MAX_WORDS + w];
                }
            leader_rank[n] = q;
        }
        __syncthreads();
        if (open && ds_covers(planes_dist(a, lp, NW), radius)) {   // the leader itself: distance 0
            member_rank[q] = n;
            open = false;
        }
        n++;
    }
    if (tid == 0) {
        state[0] = n;
        state[1] = n0;
        state[2] = n;
    }
}

// ranks from q0 on against the designs state[1] .. state[2] - 1, lowest first
__global__ void __launch_bounds__(256) design_cover_kernel(const uint64_t *rp, int M, int NW, int q0, const int *flags,
                                                           int radius, int K, int32_t *member_rank, const int *state,
                                                           const uint64_t *lead) {
    const int d0 = state[1], d1 = state[2];
    const int q = q0 + int(blockIdx.x) * 256 + int(threadIdx.x);
    if (d0 >= d1 || q >= flags[DESIGN_FINITE] || member_rank[q] >= 0) return;
    uint64_t a[MAX_PW] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < DS_MAX_WORDS; w++)
        if (w < NW) {
            a[w] = rp[size_t(w) * M + q];
            a[DS_MAX_WORDS + w] = rp[size_t(NW + w) * M + q];
        }
    for (int d = d0; d < d1; d++) {
        int dist = 0;
#pragma unroll
        for (int w = 0; w < DS_MAX_WORDS; w++)
            if (w < NW)
                dist += ds_word_dist(a[w], a[DS_MAX_WORDS + w], lead[size_t(w) * K + d], lead[size_t(NW + w) * K + d]);
        if (ds_covers(dist, radius)) {
            member_rank[q] = d;
            return;
        }
    }
}

// back to entry order: member_of, the designs' sizes and their leaders' entries
__global__ void __launch_bounds__(256) design_finish_kernel(const int32_t *order, int M, const int *flags,
                                                            const int32_t *member_rank, const int *state,
                                                            const int32_t *leader_rank, int32_t *member_of,
                                                            int32_t *sizes, int32_t *leaders) {
    const int q = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (q >= M) return;
    const int e = order[q];
    const int d = q < flags[DESIGN_FINITE] ? member_rank[q] : -1;
    member_of[e] = d;
    if (d >= 0) atomicAdd(&sizes[d], 1);
    if (q < state[0]) leaders[q] = order[leader_rank[q]];
}

__global__ void __launch_bounds__(HIST_TILE) design_hist_kernel(const uint64_t *rp, int M, int NW, int nbins,
                                                                const int *flags, unsigned long long *pair_hist) {
    extern __shared__ unsigned char hist_lds[];
    uint64_t *col = reinterpret_cast<uint64_t *>(hist_lds);                  // [2 NW][HIST_TILE]
    unsigned *bins = reinterpret_cast<unsigned *>(col + 2 * NW * HIST_TILE);  // [nbins]
    const int tid = int(threadIdx.x);
    const int F = flags[DESIGN_FINITE];
    const int ti = int(blockIdx.x), row0 = ti * HIST_TILE;
    const int tj0 = max(int(blockIdx.y) * HIST_GROUP, ti), tj1 = (int(blockIdx.y) + 1) * HIST_GROUP;
    if (row0 >= F || tj0 >= tj1 || tj0 * HIST_TILE >= F) return;   // uniform
    for (int k = tid; k < nbins; k += HIST_TILE) bins[k] = 0;
    const int qi = row0 + tid;
    uint64_t a[MAX_PW] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (qi < F) {
#pragma unroll
        for (int w = 0; w < DS_MAX_WORDS; w++)
            if (w < NW) {
                a[w] = rp[size_t(w) * M + qi];
                a[DS_MAX_WORDS + w] = rp[size_t(NW + w) * M + qi];
            }
    }
    int last = 0;
    unsigned run = 0;   // pairs at distance `last` not yet in bins
    for (int tj = tj0; tj < tj1 && tj * HIST_TILE < F; tj++) {
        const int col0 = tj * HIST_TILE, nc = min(HIST_TILE, F - col0);
        __syncthreads();   // the tile before is read; bins are zeroed
        if (tid < nc)
            for (int pw = 0; pw < 2 * NW; pw++) col[pw * HIST_TILE + tid] = rp[size_t(pw) * M + col0 + tid];
        __syncthreads();
        if (qi < F) {
            // each pair once: the column's rank above the row's
            for (int c = tj == ti ? tid + 1 : 0; c < nc; c++) {
                int dist = 0;
#pragma unroll
                for (int w = 0; w < DS_MAX_WORDS; w++)
                    if (w < NW)
                        dist += ds_word_dist(a[w], a[DS_MAX_WORDS + w], col[w * HIST_TILE + c],
                                             col[(NW + w) * HIST_TILE + c]);
                if (dist != last) {
                    if (run) atomicAdd(&bins[last], run);
                    last = dist;
                    run = 0;
                }
                run++;
            }
        }
    }
    if (run) atomicAdd(&bins[last], run);
    __syncthreads();
    for (int k = tid; k < nbins; k += HIST_TILE)
        if (bins[k]) atomicAdd(&pair_hist[k], (unsigned long long)bins[k]);
}

// n_walkers[d]: the walkers with a pick in design d (an entry counts iff it is its walker's first there)
__global__ void __launch_bounds__(256) design_walkers_kernel(const int32_t *member_of, const int32_t *src_of, int M,
                                                             int cap, int32_t *n_walkers) {
    const int e = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (e >= M) return;
    const int k = src_of[e] % cap;   // the walker's picks are the entries e - k .. e
    if (ds_first_of_walker(member_of + (e - k), k)) atomicAdd(&n_walkers[member_of[e]], 1);
}

// one workgroup per design: its leader's walker, record row, score and sequence
__global__ void __launch_bounds__(DSW) design_gather_kernel(const int32_t *leaders, const int *state,
                                                            const int32_t *src_of, int cap, int N,
                                                            const int32_t *pick_rows, const double *pick_scores,
                                                            const char *pick_seqs, int32_t *walkers, int32_t *rows,
                                                            double *scores, char *seqs) {
    const int d = int(blockIdx.x), lane = int(threadIdx.x);
    if (d >= state[0]) return;
    const int s = src_of[leaders[d]];
    if (lane == 0) {
        walkers[d] = s / cap;
        rows[d] = pick_rows[s];
        scores[d] = pick_scores[s];
    }
    for (int p = lane; p < N; p += DSW) seqs[size_t(d) * N + p] = pick_seqs[size_t(s) * N + p];
}

}  // namespace

int design_sort_blocks(int M) { return (M + SORT_TILE - 1) / SORT_TILE; }

hipError_t launch_design_offsets(const int *n_picks, int W, int *offset, int *total, hipStream_t stream) {
    hipLaunchKernelGGL(design_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, n_picks, offset, W, total);
    return hipGetLastError();
}

hipError_t launch_design_pack(const char *seqs, const double *scores, int N, int n_slots, const int *n_picks,
                              const int *offset, int cap, int M, uint64_t *planes, uint64_t *keys, int32_t *idx,
                              int32_t *src_of, int *flags, hipStream_t stream) {
    if (n_slots <= 0 || M <= 0) return hipSuccess;
    hipLaunchKernelGGL(design_pack_kernel, dim3((n_slots + PACK_WAVES - 1) / PACK_WAVES), dim3(PACK_WAVES * DSW), 0,
                       stream, seqs, scores, N, n_slots, n_picks, offset, cap, M, planes, keys, idx, src_of, flags);
    return hipGetLastError();
}

hipError_t launch_design_order(uint64_t *keys, int32_t *idx, uint64_t *keys_tmp, int32_t *idx_tmp, int M, int *hist,
                               hipStream_t stream) {
    if (M <= 0) return hipSuccess;
    const int nb = design_sort_blocks(M);
    for (int pass = 0; pass < 8; pass++) {   // an even number of passes: the result is back in keys / idx
        hipLaunchKernelGGL(radix_hist_kernel, dim3(nb), dim3(SORT_THREADS), 0, stream, keys, M, 8 * pass, hist);
        hipLaunchKernelGGL(design_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, hist, hist, 256 * nb,
                           static_cast<int *>(nullptr));
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nb), dim3(SORT_THREADS), 0, stream, keys, idx, M, 8 * pass, hist,
                           keys_tmp, idx_tmp);
        uint64_t *k = keys;
        keys = keys_tmp;
        keys_tmp = k;
        int32_t *i = idx;
        idx = idx_tmp;
        idx_tmp = i;
    }
    return hipGetLastError();
}

hipError_t launch_design_select(const DesignArgs &a, hipStream_t stream) {
    if (a.M <= 0) return hipSuccess;
    const int NW = ds_words(a.N), M = a.M, blocks = (M + 255) / 256;
    hipLaunchKernelGGL(design_rank_planes_kernel, dim3(blocks), dim3(256), 0, stream, a.planes, a.order, M, 2 * NW,
                       a.rank_planes);
    for (int q0 = 0; q0 < M; q0 += SEL_TILE) {
        hipLaunchKernelGGL(design_resolve_kernel, dim3(1), dim3(SEL_TILE), 0, stream, a.rank_planes, M, NW, q0, a.flags,
                           a.radius, a.K, a.member_rank, a.state, a.leader_rank, a.lead_planes);
        const int rest = M - (q0 + SEL_TILE);
        if (rest > 0)
            hipLaunchKernelGGL(design_cover_kernel, dim3((rest + 255) / 256), dim3(256), 0, stream, a.rank_planes, M,
                               NW, q0 + SEL_TILE, a.flags, a.radius, a.K, a.member_rank, a.state, a.lead_planes);
    }
    hipLaunchKernelGGL(design_finish_kernel, dim3(blocks), dim3(256), 0, stream, a.order, M, a.flags, a.member_rank,
                       a.state, a.leader_rank, a.member_of, a.sizes, a.leaders);
    return hipGetLastError();
}

hipError_t launch_design_hist(const DesignArgs &a, unsigned long long *pair_hist, hipStream_t stream) {
    if (a.M <= 1) return hipSuccess;
    const int NW = ds_words(a.N), nt = (a.M + HIST_TILE - 1) / HIST_TILE;
    const size_t lds = size_t(2 * NW) * HIST_TILE * sizeof(uint64_t) + size_t(a.N + 1) * sizeof(unsigned);
    hipLaunchKernelGGL(design_hist_kernel, dim3(nt, (nt + HIST_GROUP - 1) / HIST_GROUP), dim3(HIST_TILE), lds, stream,
                       a.rank_planes, a.M, NW, a.N + 1, a.flags, pair_hist);
    return hipGetLastError();
}

hipError_t launch_design_walkers(const DesignArgs &a, const int32_t *src_of, int cap, int32_t *n_walkers,
                                 hipStream_t stream) {
    if (a.M <= 0) return hipSuccess;
    hipLaunchKernelGGL(design_walkers_kernel, dim3((a.M + 255) / 256), dim3(256), 0, stream, a.member_of, src_of, a.M,
                       cap, n_walkers);
    return hipGetLastError();
}

hipError_t launch_design_gather(const DesignArgs &a, const int32_t *src_of, int cap, const int32_t *pick_rows,
                                const double *pick_scores, const char *pick_seqs, int32_t *walkers, int32_t *rows,
                                double *scores, char *seqs, hipStream_t stream) {
    if (a.M <= 0) return hipSuccess;
    hipLaunchKernelGGL(design_gather_kernel, dim3(a.K), dim3(DSW), 0, stream, a.leaders, a.state, src_of, cap, a.N,
                       pick_rows, pick_scores, pick_seqs, walkers, rows, scores, seqs);
    return hipGetLastError();
}

}  // namespace adx
