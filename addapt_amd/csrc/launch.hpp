// Host interface of the engine's translation units: every function that
// crosses a file is declared here, once.  Each .hip file and the C ABI (api_*)
// include it; none declares another file's function by hand.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>

#include "dev_types.hpp"

namespace adx {

// LDS one workgroup may take (gfx950: 160 KiB per CU)
constexpr int LDS_LIMIT = 160 * 1024;

// Raise `kernel`'s dynamic-LDS limit to `bytes` (grow-only, one record per
// kernel).  no_static_lds: the kernel carves LDS from address 0, so static LDS
// in front of the dynamic block is an error.
template <class K>
inline hipError_t configure_dynamic_lds(K kernel, size_t bytes, bool no_static_lds = false) {
    static std::map<const void *, size_t> configured;
    static std::mutex guard;   // contexts may launch from several host threads
    const std::lock_guard<std::mutex> lock(guard);
    const void *k = reinterpret_cast<const void *>(kernel);
    size_t &have = configured[k];
    if (bytes <= have) return hipSuccess;
    if (no_static_lds) {
        hipFuncAttributes fa;
        hipError_t e = hipFuncGetAttributes(&fa, k);
        if (e != hipSuccess) return e;
        if (fa.sharedSizeBytes != 0) return hipErrorInvalidKernelFile;
    }
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
    if (e == hipSuccess) have = bytes;
    return e;
}

// ---- fold_rows.hip: lanes = terms fold (score_kernel) and bppm_kernel
enum class RowsK { MinPlus16, MinPlusP2, MinPlus512, SumProdP2, SumProd768, SumProd512 };
const char *rows_kernel_name(RowsK k);
size_t lds_bytes(const KArgs &ka);
int rows_lockstep(const KArgs &ka);        // 2: apo and holo fold in lockstep (their LDS fits one CU), else 1
bool rows_one_per_cu(const KArgs &ka);     // the one-variant tables leave no room for a second workgroup
hipError_t launch_score_rows(RowsK k, const KArgs &ka, const uint8_t *seqs, int W, double *scores, double *terms,
                             float *dG, const int *mask, hipStream_t stream, int grid = 0);
size_t bppm_lds_bytes(const KArgs &ka, bool *gout);
size_t bppm_scratch_bytes(const KArgs &ka, int W);
hipError_t launch_bppm_rows(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, double *full, int ld,
                            double *pair_p, char *scratch, hipStream_t stream, bool reuse);

// ---- mfe_cells.hip, mfe_pair.hip
size_t mfe_cells_lds(const KArgs &ka);
hipError_t launch_mfe_cells(const KArgs &ka, const uint8_t *seqs, int W, float *gout, const int *mask,
                            hipStream_t stream);
bool mfe_pair_covers(const KArgs &ka);
// grid > 0: that many workgroups instead of one per resident slot (ADX_PAIR_GRID, dispatch.hip)
hipError_t launch_mfe_pair(const KArgs &ka, const uint8_t *seqs, int W, float *gout, const int *mask,
                           hipStream_t stream, int grid = 0);

// ---- mfe_trace.hip: MFE structures (fill + traceback, one workgroup per sequence)
size_t mfe_trace_slice_ints(const KArgs &ka);   // ints of HBM scratch per workgroup
int mfe_trace_chunk(const KArgs &ka, int W);    // sequences per launch, so the scratch stays bounded
hipError_t launch_mfe_trace(const KArgs &ka, int variant, const uint8_t *seqs, int W, int *scratch, int chunk,
                            char *structures, float *energies, hipStream_t stream);

// ---- mfe_subopt.hip: Zuker suboptimal structures (inside + outside MFE fill, then
// selection and traceback; one workgroup per sequence).  Sequences w0 .. w0 + n of
// `seqs`; phase 0 fills the scratch slices and writes mfe, n_within and (optional)
// pair_energy, phase 1 reads the same slices and writes the list.  Outputs are
// device buffers indexed by the sequence's position in `seqs`.
struct SuboptOut {
    int *n_found, *n_within;   // [W]
    float *mfe;                // [W] kcal/mol, +inf: the constraint admits nothing
    char *structures;          // [W][max_structs][L], '.' beyond n_found
    float *energies;           // [W][max_structs], +inf beyond n_found
    int *seeds;                // [W][max_structs][2], 1-based, 0 beyond n_found
    float *pair_energy;        // [W][L][L] kcal/mol, +inf where no structure holds the pair (optional)
};
size_t mfe_subopt_slice_ints(const KArgs &ka);   // ints of HBM scratch per workgroup
int mfe_subopt_chunk(const KArgs &ka, int W);    // sequences per launch, so the scratch stays bounded
hipError_t launch_mfe_subopt(const KArgs &ka, int variant, const uint8_t *seqs, int w0, int n, int *scratch, int phase,
                             int delta_dcal, int max_structs, const SuboptOut &out, hipStream_t stream);

// ---- pf_sample.hip: structures drawn from the ensemble (FP64 fill of n sequences
// from w0 into `scratch`, then one wave per sample: samples [k0, k0 + nk) of each,
// structures[n][nk][variant length]; *flag is raised by a sample that met a loop bound)
struct SamplePlan {
    int seqs, samples;   // per launch, so that tables plus device-side output stay bounded
};
size_t pf_sample_slice_doubles(const KArgs &ka);   // doubles of HBM scratch per sequence
SamplePlan pf_sample_plan(const KArgs &ka, int L, int W, int n_samples);
// slice_doubles: the stride between the sequences' slices (0: pf_sample_slice_doubles; the fill
// writes that many doubles at the head of each)
hipError_t launch_pf_fill(const KArgs &ka, int variant, const uint8_t *seqs, int w0, int n, double *scratch,
                          float *energies, hipStream_t stream, size_t slice_doubles = 0);
hipError_t launch_pf_sample(const KArgs &ka, int variant, const uint8_t *seqs, int w0, int n, double *scratch,
                            int k0, int nk, uint64_t seed, char *structures, int *flag, hipStream_t stream);

// ---- pf_access.hip: unpaired-region probabilities P_u(i,j) (the FP64 outside pass over
// the tables launch_pf_fill left for these n sequences in `scratch`, slices of
// pf_access_slice_doubles).  Outputs are device buffers of one launch, indexed by the
// sequence's position in it.
struct AccessOut {
    int max_len, n_regions;
    const int *regions;     // [n_regions][2] first (0-based, folded coordinates), length
    double *profile;        // [n][max_len][L]: row u-1, column i-1 = the window of length u at i (optional)
    double *region_probs;   // [n][n_regions] (optional)
    double *pair_probs;     // [n][L][L] symmetric (optional)
};
// doubles of HBM scratch per sequence: the fill's 3 cells + Nmax + 2, the adjoints'
// 3 cells and the Nmax x Nmax run table, 8 (6 cells + Nmax^2 + Nmax + 2) bytes
size_t pf_access_slice_doubles(const KArgs &ka);
int pf_access_chunk(const KArgs &ka, int W, size_t out_doubles);   // sequences per launch: slices + outputs stay bounded
hipError_t launch_pf_access(const KArgs &ka, int variant, const uint8_t *seqs, int w0, int n, double *scratch,
                            const AccessOut &out, hipStream_t stream);

// ---- struct_eval.hip: energies, probabilities and status bytes of given structures,
// one wave per (sequence, structure) item.  Sequences w0 .. w0 + n of `seqs`, n_per
// structures each: structure k of sequence b at structures + b * seq_stride + k * L
// (seq_stride 0: one list shared by every sequence), outputs at out0 + b * n_per + k.
// TE: energy-valued tables (the MFE image), E: the convention's EvalTab.  probs
// (optional, PF problems only) reads the totals launch_pf_fill left for these n
// sequences in `fill`; status is optional.
hipError_t launch_struct_eval(const KArgs &ka, const DevTables *TE, const EvalTab *E, int variant,
                              const uint8_t *seqs, int w0, int n, int n_per, const char *structures,
                              size_t seq_stride, const double *fill, size_t out0, double *energies, double *probs,
                              uint8_t *status, hipStream_t stream);

// ---- ensemble_struct.hip: centroid and MEA structures of n sequences from their
// pair-probability matrices probs[n][L][L] (launch_bppm's `full`, ld = L):
// centroid, mea = n * L chars, stats = n * 3 doubles (mea, centroid_dist, diversity)
size_t ensemble_struct_slice_doubles(int L);   // doubles of HBM scratch per sequence (M and w)
int ensemble_struct_chunk(int L, int W);       // sequences per launch: matrices + slices stay bounded
hipError_t launch_ensemble_struct(const double *probs, int L, int n, double gamma, double *scratch, char *centroid,
                                  char *mea, double *stats, hipStream_t stream);

// ---- pf_cells.hip, pf_ring.hip
size_t pf_cells_lds(const KArgs &ka);
hipError_t launch_pf_cells(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, float *gout,
                           hipStream_t stream);
size_t pf_ring_lds(const KArgs &ka);
size_t pf_ring_scratch_floats(const KArgs &ka, int W);
hipError_t launch_pf_ring(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, float *gout,
                          float *qscr, hipStream_t stream);

// ---- outside_cells.hip, outside_ring.hip
size_t outside_cells_lds(const KArgs &ka);
hipError_t launch_outside_cells(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, double *pair_p,
                                int sp_score, hipStream_t stream);
size_t outside_ring_lds(const KArgs &ka);
hipError_t launch_outside_ring(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, double *pair_p,
                               hipStream_t stream);

// ---- dispatch.hip: which kernel folds a workload
bool pf_ring_layout(const KArgs &ka);      // the context's stored tables take the ring's slot layout
const char *inside_kernel_name(const KArgs &ka);
const char *outside_kernel_name(const KArgs &ka);
bool window_defers(const KArgs &ka);
hipError_t launch_score_m(const KArgs &ka, const uint8_t *seqs, int W, double *scores, double *terms,
                          float *dG, const int *mask, hipStream_t stream);
hipError_t launch_score(const KArgs &ka, const uint8_t *seqs, int W, double *scores, double *terms, float *dG,
                        hipStream_t stream);
hipError_t launch_bppm(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, double *full, int ld,
                       double *pair_p, char *scratch, hipStream_t stream);
hipError_t launch_outside_m(const KArgs &ka, const uint8_t *seqs, int W, const int *mask, hipStream_t stream);
hipError_t launch_combine(const KArgs &ka, int W, const int *mask, double *scores, double *terms,
                          hipStream_t stream);

// ---- traj_pick.hip: each trajectory's peaks (traj_pick_core.hpp) and the sequences at them.
// Picking runs on chunks of trajectories [w0, w0 + nw) so that the trajectory-major
// copy of their keys stays bounded: keys = traj_pick_key_words(S, chunk) uint64,
// bad = chunk ints.  scores: S * W doubles, step-major; n_picks[W] (-1: a non-finite
// score), steps[W * cap] ascending, pick_scores[W * cap] optional; the caller
// checks window >= 1 and cap >= ceil(S / window).
int traj_pick_chunk(int S, int n_traj);
size_t traj_pick_key_words(int S, int chunk);
hipError_t launch_traj_pick(const double *scores, int W, int S, int window, int cap, int w0, int nw, uint64_t *keys,
                            int *bad, int *n_picks, int32_t *steps, double *pick_scores, hipStream_t stream);
struct ReplayArgs {
    const uint8_t *seq0;        // W * N codes: the walkers' sequences before the first recorded step
    const int32_t *pos;         // the record, step-major [r * W + w]: freely mutable position chosen,
    const int8_t *base;         //   base code chosen,
    const int32_t *outcome;     //   outcome
    int W, N, rows;             // rows recorded
    const int *posmap;          // [N] position -> index into the closure lists (-1: not freely mutable)
    const int *clo_off, *clo_pos;
    const uint8_t *clo_par;
    const uint8_t *lower;       // [N] 1: the template's base is lower case (frozen)
    const int *n_picks;         // [W]
    const int32_t *steps;       // [W * cap] ascending record rows
    int cap;
    char *seqs;                 // [W * cap * N] the sequence at each pick (optional)
    unsigned long long *counts; // [N * 4] A, C, G, U over all picks, added to (optional)
};
hipError_t launch_traj_replay(const ReplayArgs &a, hipStream_t stream);

// ---- traj_autocorr.hip: per-position autocorrelation of sequence trajectories (traj_autocorr_core.hpp).
// The kept steps of every changeable position are packed into two bit planes (low and high
// bit of code - 1), [walker][position][plane][ta_words(kept)] uint64, for chunks of walkers
// [w0, w0 + nw) so that the planes stay bounded: traj_autocorr_plane_words(kept, P, chunk).
// The lag kernel adds each (walker, position, lag)'s matches to pos_matches[P * (max_lag + 1)]
// (by index into the packed positions) and to walker_matches[W * (max_lag + 1)] (optional);
// the caller zeroes both and checks 0 <= max_lag <= kept - 1.
int traj_autocorr_chunk(int kept, int P, int n_traj);
size_t traj_autocorr_plane_words(int kept, int P, int chunk);
struct AutocorrPackArgs {
    const uint8_t *seq0;        // the record, as ReplayArgs
    const int32_t *pos;
    const int8_t *base;
    const int32_t *outcome;
    int W, N, rows;
    int discard;                // rows replayed but not kept (< rows)
    const int *posmap;
    const int *clo_off, *clo_pos;
    const uint8_t *clo_par;
    const int *chg;             // [P] the changeable positions, ascending
    const uint8_t *changeable;  // [N] 1: in chg
    int P;
    int w0, nw;                 // the chunk
    int nwords;                 // ta_words(rows - discard)
    unsigned long long *planes;
    unsigned long long *base_counts;     // [N * 4] A, C, G, U over the kept steps, added to (optional)
    unsigned long long *outcome_counts;  // [W * 4] outcomes 0..3 over the kept steps, written (optional)
};
hipError_t launch_autocorr_pack(const AutocorrPackArgs &a, hipStream_t stream);
// codes[(r * W + w) * P + p], S steps; *bad is set to 1 at a code outside 1..4
hipError_t launch_autocorr_pack_codes(const uint8_t *codes, int W, int S, int P, int w0, int nw, uint64_t *planes,
                                      int *bad, hipStream_t stream);
hipError_t launch_autocorr_lags(const uint64_t *planes, int nw, int P, int kept, int max_lag, int w0,
                                unsigned long long *pos_matches, unsigned long long *walker_matches,
                                hipStream_t stream);

// ---- design_select.hip: distinct designs by greedy Hamming selection (design_select_core.hpp).
// M entries are packed into two bit planes, planes[(plane * ds_words(N) + word) * M + entry],
// ordered by a radix sort of (key, entry) and selected in rank order; everything runs on one
// stream and reads the counts it needs (flags, state) from the device.  The caller zeroes
// flags, state and sizes, sets member_rank to -1 and checks N <= 255, radius >= 0, 1 <= K <= M.
constexpr int DESIGN_BAD = 0, DESIGN_FINITE = 1;   // flags: a bad character seen; entries with a finite score
int design_sort_blocks(int M);                     // hist = 256 * design_sort_blocks(M) ints
// offset[w] = the sum of max(n_picks[v], 0) over v < w, *total = over all walkers
hipError_t launch_design_offsets(const int *n_picks, int W, int *offset, int *total, hipStream_t stream);
// Sequences seqs[slot * N ..] with scores[slot].  n_picks == nullptr: slot = entry, n_slots = M.
// Else slot = walker * cap + k is an entry iff k < n_picks[walker], entry offset[walker] + k, and
// src_of[entry] = slot.  keys = the sort keys, idx = the identity, both M long.
hipError_t launch_design_pack(const char *seqs, const double *scores, int N, int n_slots, const int *n_picks,
                              const int *offset, int cap, int M, uint64_t *planes, uint64_t *keys, int32_t *idx,
                              int32_t *src_of, int *flags, hipStream_t stream);
// sorts (keys, idx) in place; keys_tmp / idx_tmp: M each
hipError_t launch_design_order(uint64_t *keys, int32_t *idx, uint64_t *keys_tmp, int32_t *idx_tmp, int M, int *hist,
                               hipStream_t stream);
struct DesignArgs {
    int M, N, radius, K;
    const uint64_t *planes;     // entry order
    const int32_t *order;       // [M] rank -> entry (launch_design_order's idx)
    uint64_t *rank_planes;      // as planes, in rank order (written by select, read by hist)
    int *flags;                 // [2]
    int *state;                 // [3]; state[0] = the number of designs
    int32_t *member_rank;       // [M] by rank
    int32_t *leader_rank;       // [K]
    uint64_t *lead_planes;      // [2 * ds_words(N) * K] the leaders' planes
    int32_t *member_of;         // [M] by entry
    int32_t *sizes, *leaders;   // [K]
};
hipError_t launch_design_select(const DesignArgs &a, hipStream_t stream);
// after launch_design_select: pair_hist[N + 1], added to
hipError_t launch_design_hist(const DesignArgs &a, unsigned long long *pair_hist, hipStream_t stream);
// the record's glue: n_walkers[K] added to; the leaders' walker, record row, score and sequence
hipError_t launch_design_walkers(const DesignArgs &a, const int32_t *src_of, int cap, int32_t *n_walkers,
                                 hipStream_t stream);
hipError_t launch_design_gather(const DesignArgs &a, const int32_t *src_of, int cap, const int32_t *pick_rows,
                                const double *pick_scores, const char *pick_seqs, int32_t *walkers, int32_t *rows,
                                double *scores, char *seqs, hipStream_t stream);

// ---- mc_step.hip
hipError_t launch_steps(const KArgs &ka, const StepArgs &st, hipStream_t stream, hipEvent_t *evs);
hipError_t launch_rescore(const KArgs &ka, const StepArgs &st, double *tv, hipStream_t stream);

}  // namespace adx
