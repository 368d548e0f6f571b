/*
 * addapt_gpu.h -- C ABI of the MI355X (gfx950) fold -> score -> accept engine.
 *
 * Plain C, plain pointers and sizes, status codes, no exceptions, no torch
 * types.  Library: addapt_amd/_lib/libaddapt_gpu.so (built by
 * __graft_entry__.build()).  All calls are synchronous; one context per GPU
 * per host thread; calls on one context must be serialised by the caller.
 *
 * Two layers, both replacing the reference's FFI into ViennaRNA
 * (/root/reference/src/scoring.cc:6-11 includes, 37-103 call sites):
 *
 *  (1) the per-fold layer adx_fold_* -- one entry point per ViennaRNA symbol
 *      the reference binds, for code that keeps addapt's RnaFold interface
 *      (scoring.hh:42-55, ViennaRnaFold scoring.cc:17-103);
 *
 *  (2) the batched Monte Carlo layer adx_ctx_* / adx_walkers_* / adx_run_steps
 *      / adx_score_batch -- thousands of independent walkers in lockstep;
 *      each step of MonteCarlo::apply (sampling.cc:55-99) is three launches
 *      on one stream, no host round trip: propose (move + thermostat + RNG),
 *      fold + score of the changed walkers, Metropolis accept (plus the
 *      outside pass when base-pair terms are scored).
 */
#ifndef ADDAPT_GPU_H
#define ADDAPT_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADX_ABI_VERSION 4

typedef enum adx_status {
    ADX_OK = 0,
    ADX_EINVAL = 1,      /* bad argument / malformed input */
    ADX_EHIP = 2,        /* HIP runtime error */
    ADX_ECONSTRAINT = 3, /* malformed dot-bracket constraint */
    ADX_EPARAM = 4,      /* energy-parameter file could not be read */
    ADX_ENOMEM = 5,      /* allocation failed */
    ADX_EMOVE = 6,       /* mutation move failed (sampling.cc:256,265,279) */
    ADX_ESTATE = 7,      /* call out of order (e.g. run before walkers_init) */
    ADX_ENODEV = 8,      /* no gfx950 device visible */
    ADX_EUNSUPPORTED = 9 /* feature not available on the GPU path */
} adx_status;

/* Thread-local message for the last non-OK status. */
const char *adx_last_error(void);
int adx_abi_version(void);

/* ------------------------------------------------------------------------
 * Energy parameters (ViennaRNA 2.0 parameter-file layout).  Replaces the
 * implicit vrna_md_set_default() model (scoring.cc:80-83): 37 C, dangles=2,
 * special hairpins, TURN=3, MAXLOOP=30.
 * ---------------------------------------------------------------------- */
typedef struct adx_params adx_params;
adx_status adx_params_load(const char *par_path, adx_params **out);
void adx_params_free(adx_params *p);
/* kT at 37 C in kcal/mol (= fc->exp_params->kT / 1000, scoring.cc:69,91). */
double adx_kT(void);
/* Free energy (kcal/mol) of one structure under the loaded model. */
adx_status adx_eval_structure(const adx_params *p, const char *seq, const char *structure,
                              double *energy_kcal);

/* ------------------------------------------------------------------------
 * (1) Per-fold layer: one-to-one with the ViennaRNA calls in scoring.cc.
 * ---------------------------------------------------------------------- */
typedef struct adx_fold adx_fold;
/* vrna_md_set_default + vrna_fold_compound(seq, &md, VRNA_OPTION_PF)
 * (scoring.cc:79-88); with_bppm mirrors md.compute_bpp (scoring.cc:82-83).
 * The sequence is upper-cased as ViennaRnaFold's constructor does (:28). */
adx_status adx_fold_create(const adx_params *p, const char *seq, int with_bppm, int device,
                           adx_fold **out);
/* vrna_sc_add_hi_motif(fc, seq, fold, energy, VRNA_OPTION_DEFAULT) (:92-100) */
adx_status adx_fold_add_motif(adx_fold *f, const char *motif_seq, const char *motif_fold,
                              double energy_kcal);
/* vrna_constraints_add(fc, db, DB_DEFAULT | DB_ENFORCE_BP) (:61-62) */
adx_status adx_fold_add_constraint(adx_fold *f, const char *dot_bracket);
/* vrna_pf(fc, NULL) (:58, :65): ensemble free energy (kcal/mol, float) */
adx_status adx_fold_pf(adx_fold *f, float *energy_kcal);
/* vrna_mfe(fc, NULL) (fold.h, included at scoring.cc:9, never called by the
 * reference): minimum free energy (kcal/mol, float; integer dcal arithmetic;
 * +inf when the constraint admits no structure), with the ligand motif
 * entering as c(i,j) = min(c(i,j), round(100*(E_motif + bonus))) at every site
 * where the motif can form.  Energy only; adx_fold_mfe_structure adds the
 * structure. */
adx_status adx_fold_mfe(adx_fold *f, float *energy_kcal);
/* vrna_mfe with backtracking: structure = strlen(seq)+1 bytes, NUL-terminated
 * dot-bracket of one optimal structure (ties broken in a fixed order; a formed
 * ligand motif appears as the motif's own fold); all '.' and +inf when the
 * constraint admits no structure.  Filled and traced on the GPU. */
adx_status adx_fold_mfe_structure(adx_fold *f, char *structure, float *energy_kcal);
/* RNAsubopt --zuker / mfold's energy dot plot: the structures within delta_kcal
 * of the minimum, at most one per base pair, for the compound (motif,
 * constraint).  An MFE outside pass on the GPU gives through(i,j), the energy of
 * the best structure that holds the pair (i,j) -- the MFE under that forced pair
 * -- for every pair at once.  Pairs are ordered by (through, i, j) ascending;
 * repeatedly the first pair that no listed structure holds yet and whose
 * through <= MFE + round(100 delta) dcal seeds the next structure (the optimal
 * one through it, ties broken in a fixed order), until max_structs are listed or
 * no pair is left.  The open chain is never listed.  Outputs:
 *   n_found         structures listed
 *   n_pairs_within  pairs with through <= MFE + delta (optional)
 *   mfe_kcal        the minimum (+inf and n_found 0 when the constraint admits nothing)
 *   structures      max_structs * (strlen(seq) + 1) bytes, each NUL-terminated;
 *                   all '.' beyond n_found
 *   energies        [max_structs] kcal/mol, non-decreasing; +inf beyond n_found
 *   seeds           [max_structs][2] the seeding pair, 1-based; 0 beyond n_found (optional)
 *   pair_energy     [L * L] through as float kcal/mol, symmetric, +inf where no
 *                   structure holds the pair (optional, NULL)
 * delta_kcal < 0 (or not finite) or max_structs < 1: ADX_EINVAL. */
adx_status adx_fold_subopt_structures(adx_fold *f, double delta_kcal, int max_structs, int *n_found,
                                      int *n_pairs_within, float *mfe_kcal, char *structures, float *energies,
                                      int *seeds, float *pair_energy);
/* vrna_pbacktrack: n_samples structures drawn from the ensemble the compound
 * describes (motif, constraint).  structures = n_samples * strlen(seq) chars,
 * no terminators; energy_kcal optional (the ensemble energy, as adx_fold_pf).
 * Sample k under `seed` does not depend on n_samples; a formed ligand motif
 * appears as the motif's own fold; all '.' and +inf when the constraint
 * admits no structure.  Filled (FP64) and sampled on the GPU. */
adx_status adx_fold_sample_structures(adx_fold *f, int n_samples, uint64_t seed,
                                      char *structures, float *energy_kcal);
/* RNAeval on the GPU: what the compound's sequence pays for each of n given
 * structures, and how much of its ensemble each is.  structures = n *
 * strlen(seq) chars, no terminators; energies[n] (kcal/mol), probs[n] and
 * status[n] (both optional, NULL).  The compound's motif and constraint are
 * honoured.  convention:
 *   ADX_FOLD_PF   E(s) = -kT ln w(s), w the weight adx_fold_pf's ensemble gives s:
 *                 adx_eval_structure's loops, and per formed motif site (the
 *                 sequence matches, s has the motif's own fold there, the
 *                 constraint admits it) exp(-enc/kT), enc the loops the site
 *                 encloses, replaced by exp(-enc/kT) + exp(-eint/kT)(exp(-beff/kT) - 1)
 *   ADX_FOLD_MFE  the integer dcal arithmetic of adx_fold_mfe: lxc ln(u/30) of a
 *                 loop above 30 truncated, a formed site's enclosed energy
 *                 min(enc, round(100 (eint + beff))), eint the motif's own loops,
 *                 beff = bonus under ADX_MOTIF_ADD and bonus - eint under
 *                 ADX_MOTIF_REPLACE and ADX_MOTIF_AUTO (so round(100 bonus) there);
 *                 in the PF convention beff = bonus under ADD and AUTO
 * status bits per item: ADX_EVAL_MALFORMED (unbalanced, a character outside
 * ".()", a non-canonical pair; energy NaN), ADX_EVAL_HAIRPIN (a hairpin below 3;
 * +inf), ADX_EVAL_EXCLUDED (the constraint excludes it; +inf), ADX_EVAL_BIGLOOP
 * (an interior loop above 30: priced as adx_eval_structure prices it, yet in no
 * fold's ensemble).  status 0 = a member of the ensemble; a string without a
 * pair table (unbalanced, a bad character) reports ADX_EVAL_MALFORMED alone.
 * A bad item never disturbs its neighbours.  probs (ADX_FOLD_PF
 * only): exp(-(E(s) - G)/kT) with G from an FP64 fill on the GPU, 0 for a
 * non-member. */
#define ADX_EVAL_MALFORMED 1
#define ADX_EVAL_HAIRPIN 2
#define ADX_EVAL_EXCLUDED 4
#define ADX_EVAL_BIGLOOP 8
adx_status adx_fold_eval_structures(adx_fold *f, int convention, int n, const char *structures,
                                    double *energies, double *probs, uint8_t *status);
/* Unpaired-region probabilities (RNAplfold -u / RNAup's accessibility) of the
 * ensemble the compound describes (motif, constraint), FP64, from an outside
 * pass over the FP64 fill on the GPU.  With L = strlen(seq) and Z the
 * ensemble's partition function, for every window [i..j], 1 <= i <= j <= L,
 * j - i + 1 <= max_len:
 *   P_u(i, j) = Z(the ensemble restricted to structures with i..j all unpaired) / Z
 * which is what two partition functions give: the compound's own, and one with
 * 'x' merged into the constraint over the window.
 *   probs       max_len * L doubles: row u-1, column i-1 holds the window of
 *               length u starting at i (1-based); columns past L-u are 0
 *   pair_probs  optional (NULL): L * L doubles, symmetric, the pair probabilities
 *   energy_kcal optional: the ensemble energy (+inf: the empty ensemble)
 * A window is exactly 0 where the constraint forces one of its bases to pair
 * ('|', '<', '>', '(', ')'); every entry of probs is NaN when the constraint
 * admits no structure at all (pair_probs too); sequences too short to pair
 * (L < 5) give 1 everywhere.  max_len outside [1, L]: ADX_EINVAL.  Equal
 * inputs give equal bytes. */
adx_status adx_fold_unpaired_probs(adx_fold *f, int max_len, double *probs, double *pair_probs,
                                   float *energy_kcal);
/* What RNAfold -p --MEA prints after the MFE line, for the ensemble the compound
 * describes (motif, constraint), from its pair probabilities P on the GPU:
 *   centroid       the pairs with P > 1/2 (taken in ascending (i, j); a pair that
 *                  shares a base with or crosses one already taken is dropped,
 *                  which exact probabilities never need)
 *   centroid_dist  sum_{i<j} (pair in centroid ? 1 - P : P)
 *   diversity      2 sum_{i<j} P (1 - P)                 (vrna_mean_bp_distance)
 *   MEA            the nested structure over pairs with P > 0 that maximises
 *                  sum_{i unpaired} pu[i] + 2 gamma sum_{pairs} P[i][j],
 *                  pu[i] = 1 - sum_j P[i][j]; mea is that maximum.  gamma = 1 is
 *                  RNAfold's default.
 * All FP64; ties go to a fixed candidate order, so equal inputs give equal bytes. */
typedef struct adx_ensemble_stats {
    double mea;
    double centroid_dist;
    double diversity;
} adx_ensemble_stats;

/* centroid and mea are strlen(seq)+1 bytes each, NUL-terminated; any of
 * centroid, mea, stats may be NULL, not all.  A constraint that admits no
 * structure: both all '.', the statistics NaN.  Fills the probabilities
 * adx_fold_bpp serves as a by-product. */
adx_status adx_fold_ensemble_structures(adx_fold *f, double gamma, char *centroid, char *mea,
                                        adx_ensemble_stats *stats);
/* fc->exp_matrices->probs[fc->iindx[i] - j] with 1-based i < j (:47-50);
 * computed on first use with md.compute_bpp (:41-44). */
adx_status adx_fold_bpp(adx_fold *f, int i, int j, double *prob);
/* vrna_fold_compound_free (:31-35) */
void adx_fold_free(adx_fold *f);

/* ------------------------------------------------------------------------
 * (2) Batched Monte Carlo layer.
 * ---------------------------------------------------------------------- */
#define ADX_APO 0
#define ADX_HOLO 1

#define ADX_TERM_MACROSTATE 0  /* MacrostateProbTerm (scoring.hh:175-192): p = macrostate_prob */
#define ADX_TERM_PAIR 1        /* p = RnaFold::base_pair_prob(i, j) (scoring.cc:37-51) of the
                                  condition's unconstrained fold (outside pass, configs 3-4) */

typedef struct adx_term {
    int condition;             /* ADX_APO / ADX_HOLO */
    int macrostate;            /* index into adx_run_desc.macrostates (ADX_TERM_MACROSTATE) */
    int favorable;             /* 1 = "<name>" (ln p), 0 = "not <name>" (ln(1 - p)) */
    double weight;             /* ScoreTerm weight (scoring.hh:160-168) */
    int kind;                  /* ADX_TERM_MACROSTATE (zero-initialised default) / ADX_TERM_PAIR */
    int pair_i, pair_j;        /* ADX_TERM_PAIR: 0-based device positions, i < j */
} adx_term;

#define ADX_THERMO_FIXED 0     /* FixedThermostat (sampling.cc:305-321) */
#define ADX_THERMO_ANNEAL 1    /* AnnealingThermostat (:324-378) */
#define ADX_THERMO_AUTO 2      /* AutoScalingThermostat (:381-410) */

typedef struct adx_thermostat {
    int kind;
    double t_fixed;
    double t_hi, t_lo;
    int cycle_len;
    double target_rate;
    int period;
    double t_init;
} adx_thermostat;

#define ADX_MOTIF_AUTO 0       /* default (zero-initialised): ADD in partition functions,
                                  REPLACE in MFE folds -- the convention that holds every
                                  reference pin: the rhf(6) ensemble annotations and holo
                                  classes (test_scoring.cc:54-55) and RNAfold's printed holo
                                  MFE -9.22 (test_scoring.cc:152-154, tools/test_seq:9) */
#define ADX_MOTIF_ADD 1        /* opt-in: ligand bonus added to the motif structure's own loop
                                  energies in both fold modes (holo MFE of THEO: -10.92) */
#define ADX_MOTIF_REPLACE 2    /* opt-in: motif structure's total energy := bonus, both modes */

#define ADX_FOLD_PF 0          /* MacrostateProbTerm over vrna_pf ensembles (scoring.cc:53-71) */
#define ADX_FOLD_MFE 1         /* the same terms over minimum free energies:
                                  p = exp(-(E_mfe(constrained) - E_mfe(free)) / kT) */

typedef struct adx_context_desc { /* Context (model.hh:139-157) */
    const char *before;
    const char *after;
} adx_context_desc;

typedef struct adx_run_desc {
    const adx_params *params;
    const char *sequence;            /* template Device sequence; upper = mutable */
    int n_macrostates;
    const char *const *macrostates;  /* each strlen(sequence) chars */
    int n_terms;
    const adx_term *terms;
    const char *aptamer_seq;         /* NULL: no aptamer (holo folds like apo) */
    const char *aptamer_fold;
    double aptamer_energy_kcal;      /* kT*ln(Kd/1M) (scoring.cc:91-99) */
    int motif_mode;                  /* ADX_MOTIF_AUTO (default, 0) / _ADD / _REPLACE */
    int n_contexts;                  /* 0 = none; else map (name) order */
    const adx_context_desc *contexts;
    adx_thermostat thermostat;
    int device;                      /* HIP device ordinal */
    int fold_mode;                   /* ADX_FOLD_PF (default, zero-initialised) / ADX_FOLD_MFE */
} adx_run_desc;

typedef struct adx_ctx adx_ctx;

typedef struct adx_info {
    int length;          /* N (raw device length) */
    int n_variants;      /* partition functions per scored step */
    int n_terms;         /* score terms per context */
    int n_mutable;       /* freely mutable positions */
    int max_walkers;
    double scale_per_nt; /* pf scaling used by the FP32 kernels */
} adx_info;

adx_status adx_ctx_create(const adx_run_desc *desc, adx_ctx **out);
void adx_ctx_destroy(adx_ctx *ctx);
adx_status adx_ctx_info(const adx_ctx *ctx, adx_info *info);

/* W walkers; seqs = W*N chars (NULL: every walker starts from the template),
 * seeds = W uint32 (std::mt19937(seed) per walker, addapt.cc:89).  Computes
 * the initial score of each walker (sampling.cc:40). */
adx_status adx_walkers_init(adx_ctx *ctx, int n_walkers, const char *seqs,
                            const uint32_t *seeds);

/* Optional per-step trace, host arrays of steps*W entries (step-major). */
typedef struct adx_trace {
    int32_t *position;       /* freely-mutable position chosen */
    char *base;              /* base chosen */
    int32_t *outcome;        /* 0 REJECT 1 WORSENED 2 UNCHANGED 3 IMPROVED */
    double *temperature;
    double *proposed_score;  /* NaN on ACCEPT_UNCHANGED */
    double *current_score;   /* after the step */
    double *random_threshold;
    double *term_values;     /* steps*W*n_terms*max(1,n_contexts), proposed; NaN if unchanged */
} adx_trace;

/* Advance every walker by `steps` MC steps (fused mutate + fold + score +
 * Metropolis); the step counter persists across calls (thermostat index). */
adx_status adx_run_steps(adx_ctx *ctx, int steps, adx_trace *trace);

/* Device time (ms) of the last adx_run_steps / adx_score_batch, measured with
 * HIP events on the context's stream. */
adx_status adx_last_kernel_ms(const adx_ctx *ctx, double *ms);
/* Average duration of the score kernel (the fold -> score launch, the dominant
 * kernel) over the launches of the last adx_run_steps, from HIP events recorded
 * on the context's stream around each launch. */
adx_status adx_last_score_kernel_ms(const adx_ctx *ctx, double *avg_ms, int *launches);
/* The same window split per launch (averages, ms): the inside folds (fold ->
 * energies or scores) and, when score terms read base-pair probabilities, the
 * outside pass on the stored inside tables (0 otherwise); the inside share is
 * the window minus its outside pass. */
adx_status adx_last_kernel_split_ms(const adx_ctx *ctx, double *inside_ms, double *outside_ms);
/* Names of the fold kernel(s) and of the outside pass ("" without pair terms)
 * the last adx_run_steps launched, from the engine's own dispatch choice. */
adx_status adx_last_kernel_names(const adx_ctx *ctx, char *inside, int inside_len, char *outside, int outside_len);

adx_status adx_walkers_download(adx_ctx *ctx, char *seqs, double *scores, int64_t *counters);

/* Fold and score every walker's CURRENT configuration from scratch with the
 * MC step's own kernels (the same inside, outside and combine launches as
 * adx_run_steps, no stored tables read), adopt the fresh tables and write the
 * fresh scores[W] (and term_values[W*n_terms*max(1,n_contexts)], optional).
 * The stored scores are left alone: a caller compares the two to check that
 * incremental refolds equal scratch folds bit for bit.  adx_walkers_init
 * computes the walkers' first scores this way (sampling.cc:40).
 * State the call overwrites: each walker's table slot pointer (cur_slot flips
 * to the fresh tables) and valid byte (set), the proposal buffers of the last
 * step (proposed sequences and scores, changed flags, the launch-order list)
 * and, with base-pair terms, the pair-probability and per-variant energy
 * scratch -- so read a step's proposals before rescoring. */
adx_status adx_walkers_rescore(adx_ctx *ctx, double *scores, double *term_values);

/* Replica exchange (BASELINE config 5): copy the walkers' configurations --
 * sequence codes (W*N bytes, 1..4 = A,C,G,U) and scores (W doubles) -- to or
 * from caller-owned DEVICE buffers on the context's GPU (e.g. torch tensors
 * swapped between ranks over RCCL).  RNG streams, counters and thermostat
 * state stay with the walker slot: a swap moves configurations between
 * temperatures.  An imported walker folds from scratch until one of its
 * proposals is accepted; from then on it refolds incrementally on that
 * proposal's tables.
 *
 * adx_walkers_export / adx_walkers_import are synchronous: export returns with
 * the buffers written; the caller's own writes to the buffers must be complete
 * (its stream synchronized) before adx_walkers_import. */
adx_status adx_walkers_export(adx_ctx *ctx, void *dev_seqs, void *dev_scores);
adx_status adx_walkers_import(adx_ctx *ctx, const void *dev_seqs, const void *dev_scores);
/* Stream-ordered forms, no host synchronisation: `stream` / `producer_stream`
 * is the caller's HIP stream that reads / writes the buffers (e.g. torch's
 * current stream; NULL is the null stream -- a valid stream, not "none").
 * The copies run on the context's stream after the work already queued on the
 * caller's stream, and the caller's stream waits for the copies before its
 * later work (so it may read the exported buffers, and overwrite the imported
 * ones, right away).  Use the synchronous pair above for "no stream". */
adx_status adx_walkers_export_on(adx_ctx *ctx, void *dev_seqs, void *dev_scores, void *stream);
adx_status adx_walkers_import_after(adx_ctx *ctx, const void *dev_seqs, const void *dev_scores,
                                    void *producer_stream);
/* Temperature of an ADX_THERMO_FIXED context (one rung of a replica ladder). */
adx_status adx_set_temperature(adx_ctx *ctx, double t);

/* Parity entry point: score W sequences (W*N chars) without moving.
 * scores[W]; term_values[W*n_terms*max(1,n_contexts)] (optional);
 * dG[W*n_variants] ensemble energies (kcal/mol, float, optional). */
adx_status adx_score_batch(adx_ctx *ctx, int n_walkers, const char *seqs, double *scores,
                           double *term_values, float *dG);

/* Base-pair probability matrices of W sequences (W*N chars) for one
 * (context, condition) unconstrained fold: probs = W * L * L doubles, L the
 * folded (context-padded) length, row-major, symmetric, zero diagonal --
 * probs[w*L*L + (i-1)*L + (j-1)] = fc->exp_matrices->probs[iindx[i]-j]
 * (scoring.cc:47-50).  context = 0 without contexts. */
adx_status adx_bppm_batch(adx_ctx *ctx, int n_walkers, const char *seqs, int condition, int context,
                          double *probs);

/* MFE structures of W sequences (W*N chars) for variant v (adx_variant_desc):
 * structures = W*L chars (L = the variant's folded, context-padded length; no
 * terminators), energies[W] (kcal/mol, optional) -- bit for bit the variant's
 * column of adx_score_batch's dG.  ADX_FOLD_MFE contexts only (a partition-
 * function context holds Boltzmann factors, not energies: ADX_EUNSUPPORTED;
 * use adx_fold_mfe_structure there).  Walker state, the stored tables and the
 * next step's results are not touched. */
adx_status adx_mfe_structure_batch(adx_ctx *ctx, int n_walkers, const char *seqs, int variant,
                                   char *structures, float *energies);

/* The same for the walkers' current sequences, read on the device
 * (ADX_ESTATE before adx_walkers_init). */
adx_status adx_walkers_mfe_structures(adx_ctx *ctx, int variant, char *structures, float *energies);

/* Zuker suboptimal structures (adx_fold_subopt_structures) of W sequences (W*N
 * chars) for variant v (adx_variant_desc), with the variant's context padding,
 * constraint and motif.  Per sequence w: n_found[w], n_pairs_within[w]
 * (optional), mfe_kcal[w], structures = W * max_structs * L chars (L = the
 * variant's folded length; no terminators), energies = W * max_structs, seeds =
 * W * max_structs * 2 (optional), pair_energy = W * L * L floats (optional, NULL).
 * The results of a sequence depend on nothing else.  ADX_FOLD_MFE contexts only
 * (ADX_EUNSUPPORTED on a partition-function context; use
 * adx_fold_subopt_structures there).  Walker state, the stored tables and the
 * next step's results are not touched. */
adx_status adx_subopt_structures_batch(adx_ctx *ctx, int n_walkers, const char *seqs, int variant, double delta_kcal,
                                       int max_structs, int *n_found, int *n_pairs_within, float *mfe_kcal,
                                       char *structures, float *energies, int *seeds, float *pair_energy);

/* The same for the walkers' current sequences, read on the device
 * (ADX_ESTATE before adx_walkers_init). */
adx_status adx_walkers_subopt_structures(adx_ctx *ctx, int variant, double delta_kcal, int max_structs, int *n_found,
                                         int *n_pairs_within, float *mfe_kcal, char *structures, float *energies,
                                         int *seeds, float *pair_energy);

/* Device time (ms, HIP events) of the context's last suboptimal-structures call:
 * the inside + outside fill and the selection with its tracebacks. */
adx_status adx_last_subopt_ms(const adx_ctx *ctx, double *fill_ms, double *select_ms);

/* W sequences, variant v of a PF context: structures = W * n_samples * L chars
 * (sequence-major, then sample; L = the variant's folded, context-padded
 * length), energies[W] optional (the variant's ensemble energies, an FP64
 * fill independent of adx_score_batch's dG).  Sample k of sequence w under
 * `seed` depends on nothing else.  ADX_FOLD_PF contexts only
 * (ADX_EUNSUPPORTED on an MFE context).  Touches no walker state. */
adx_status adx_sample_structures_batch(adx_ctx *ctx, int n_walkers, const char *seqs, int variant,
                                       int n_samples, uint64_t seed, char *structures, float *energies);

/* The same for the walkers' current sequences, read on the device; w = walker
 * index (ADX_ESTATE before adx_walkers_init). */
adx_status adx_walkers_sample_structures(adx_ctx *ctx, int variant, int n_samples, uint64_t seed,
                                         char *structures, float *energies);

/* Device time (ms, HIP events) of the context's last sampling call: the FP64
 * fill and the sampling kernel. */
adx_status adx_last_sample_ms(const adx_ctx *ctx, double *fill_ms, double *sample_ms);

/* Centroid and MEA structures (adx_fold_ensemble_structures) of W sequences
 * (W*N chars) for the (context, condition) unconstrained fold, addressed as
 * adx_bppm_batch addresses it: centroid, mea = W*L chars, no terminators;
 * stats[W]; any of the three may be NULL, not all.  probs = W*L*L doubles,
 * optional (NULL): the matrices the structures were computed from, as
 * adx_bppm_batch lays them out.  The matrices stay on the device between the
 * outside pass and the structure kernel.  ADX_FOLD_PF contexts only
 * (ADX_EUNSUPPORTED on an MFE context).  Walker state, the stored tables and
 * the next step's results are not touched. */
adx_status adx_ensemble_structures_batch(adx_ctx *ctx, int n_walkers, const char *seqs, int condition,
                                         int context, double gamma, char *centroid, char *mea,
                                         adx_ensemble_stats *stats, double *probs);

/* The same for the walkers' current sequences, read on the device
 * (ADX_ESTATE before adx_walkers_init). */
adx_status adx_walkers_ensemble_structures(adx_ctx *ctx, int condition, int context, double gamma,
                                           char *centroid, char *mea, adx_ensemble_stats *stats,
                                           double *probs);

/* Device time (ms, HIP events) of the context's last ensemble-structures call:
 * the outside pass and the structure kernel. */
adx_status adx_last_ensemble_ms(const adx_ctx *ctx, double *bppm_ms, double *struct_ms);

/* Energies, ensemble probabilities and status bytes (adx_fold_eval_structures)
 * of given structures for variant v (adx_variant_desc), in the convention of
 * the context's fold mode and with the variant's context padding, constraint
 * and motif: n_seqs sequences (n_seqs*N chars), n_per_seq structures each.
 * structures = n_seqs * n_per_seq * L chars (sequence-major; L = the variant's
 * folded, context-padded length), the layout adx_sample_structures_batch writes
 * and, with n_per_seq = 1, adx_mfe_structure_batch's.  energies, probs and
 * status are n_seqs * n_per_seq, sequence-major; probs and status optional
 * (NULL); probs on an MFE context: ADX_EUNSUPPORTED.  Walker state, the stored
 * tables and the next step's results are not touched. */
adx_status adx_eval_structures_batch(adx_ctx *ctx, int n_seqs, const char *seqs, int variant, int n_per_seq,
                                     const char *structures, double *energies, double *probs, uint8_t *status);

/* n_structs target structures (n_structs * L chars, shared by all walkers) on
 * the walkers' current sequences, read on the device: outputs are W * n_structs,
 * walker-major (ADX_ESTATE before adx_walkers_init). */
adx_status adx_walkers_eval_structures(adx_ctx *ctx, int variant, int n_structs, const char *structures,
                                       double *energies, double *probs, uint8_t *status);

/* Device time (ms, HIP events) of the context's last eval-structures call: the
 * FP64 fill (0 without probs) and the eval kernel. */
adx_status adx_last_eval_ms(const adx_ctx *ctx, double *fill_ms, double *eval_ms);

/* Unpaired-region probabilities (adx_fold_unpaired_probs) of n_seqs sequences
 * (n_seqs*N chars) under variant v (adx_variant_desc), with the variant's
 * context padding, constraint and motif; L = the variant's folded,
 * context-padded length, the coordinates of the sampled structures.
 *   profile       n_seqs * max_len * L doubles (per sequence the layout of
 *                 adx_fold_unpaired_probs), or NULL
 *   regions       n_regions (first, length) pairs, first 0-based in the folded
 *                 coordinates; a region may be longer than max_len
 *   region_probs  n_seqs * n_regions doubles, sequence-major, or NULL; an entry
 *                 equals the profile's entry of the same window, bit for bit
 *   energies      n_seqs ensemble energies, optional
 * profile and region_probs may not both be NULL; with profile NULL max_len may
 * be 0.  ADX_EUNSUPPORTED on an MFE context; ADX_EINVAL for a bad variant,
 * max_len outside [1, L] (0 only without a profile), a region outside the
 * sequence or of length < 1.  Walker state, the stored tables and the next
 * step's results are not touched. */
adx_status adx_unpaired_probs_batch(adx_ctx *ctx, int n_seqs, const char *seqs, int variant, int max_len,
                                    int n_regions, const int *regions, double *profile, double *region_probs,
                                    float *energies);

/* The same on the walkers' current sequences, read on the device: only the
 * requested numbers cross to the host (with regions alone W * n_regions
 * doubles).  Outputs are walker-major (ADX_ESTATE before adx_walkers_init). */
adx_status adx_walkers_unpaired_probs(adx_ctx *ctx, int variant, int max_len, int n_regions, const int *regions,
                                      double *profile, double *region_probs, float *energies);

/* Device time (ms, HIP events) of the context's last unpaired-probs call: the
 * FP64 inside fill and the outside pass with its window sums. */
adx_status adx_last_unpaired_ms(const adx_ctx *ctx, double *fill_ms, double *outside_ms);

/* ------------------------------------------------------------------------
 * Picking each trajectory's best steps on the device (what the reference's
 * pick_seqs script does with a trajectory file).  For one trajectory of S
 * scores c[0..S) (c[r] = the current score after step r) and a window >= 1:
 *   T      the 75th percentile of c (linear interpolation, numpy's default)
 *   peaks  repeat: of the steps not yet blocked take the largest score (the
 *          lowest step among equals); stop when none is left or it is not
 *          >= T; else record it and block [max(i - window, 0), min(i + window, S))
 * so picks are at least `window` steps apart and there are at most
 * ceil(S / window) of them.  A trajectory with a NaN or an infinity is not
 * picked: its count is -1.
 * ---------------------------------------------------------------------- */

/* Stateless: pick from caller-supplied trajectories (scores = n_steps * n_traj
 * doubles, step-major: scores[r * n_traj + w]).  n_picks[n_traj] (-1:
 * non-finite scores); steps = n_traj * cap int32, ascending, the first
 * n_picks[w] of trajectory w's cap valid.  cap < ceil(n_steps / window) or
 * window < 1: ADX_EINVAL naming the needed cap. */
adx_status adx_pick_scores(int device, int n_traj, int n_steps, const double *scores, int window,
                           int cap, int *n_picks, int32_t *steps);

/* The pick record: from adx_record_begin on, consecutive adx_run_steps calls
 * keep each step's current score and move (17 bytes per walker and step) on
 * the device, up to max_steps steps in all; a call that would exceed
 * max_steps returns ADX_ESTATE before it launches anything (the walkers are
 * untouched).  adx_record_begin allocates and snapshots the walkers'
 * sequences (ADX_ENOMEM leaves no record and nothing allocated; ADX_ESTATE
 * before adx_walkers_init; a second begin starts over).  adx_walkers_init and
 * adx_walkers_import* during a record change sequences outside the log, and a
 * failed adx_run_steps leaves rows unwritten: either marks the record broken
 * (adx_record_picks: ADX_ESTATE) until the next adx_record_begin.  Rescoring
 * and the structure calls do not disturb it.  adx_record_end frees it. */
adx_status adx_record_begin(adx_ctx *ctx, int max_steps);
adx_status adx_record_end(adx_ctx *ctx);
/* Picks of the steps recorded so far (may be called more than once, with
 * different windows).  Per walker w, n_picks[w] picks (-1: non-finite scores)
 * in ascending step order, the first n_picks[w] of its cap entries valid:
 * steps[W * cap] the context's global 0-based step index of each pick;
 * scores[W * cap] the current score there; seqs = W * cap * N chars, the
 * walker's sequence after that step (as adx_walkers_download writes it);
 * base_counts = N * 4 int64, how often A, C, G, U stand at each position over
 * all walkers' picks.  scores, seqs and base_counts are optional (NULL).
 * cap < ceil(recorded steps / window) or window < 1: ADX_EINVAL naming the
 * needed cap; before adx_record_begin or with nothing recorded: ADX_ESTATE. */
adx_status adx_record_picks(adx_ctx *ctx, int window, int cap, int *n_picks, int64_t *steps,
                            double *scores, char *seqs, int64_t *base_counts);
/* Device time (ms, HIP events) of the context's last adx_record_picks: the
 * picking kernels and the replay kernel. */
adx_status adx_last_pick_ms(const adx_ctx *ctx, double *pick_ms, double *replay_ms);

/* ------------------------------------------------------------------------
 * The per-position autocorrelation of sequence trajectories on the device
 * (what the reference's auto_corr tool computes from a trajectory file): the
 * measure of the pick window.  For one series x[0..S) of bases and a lag k,
 *   m(k) = #{ i in [0, S - k) : x[i + k] == x[i] },
 * the autocorrelation being m(k) / (S - k).  The calls return the integer
 * counts, summed over trajectories or over positions; the caller divides.
 * A lag may be at most S - 1 (else ADX_EINVAL naming that lag).
 * ---------------------------------------------------------------------- */

/* Stateless: codes = n_steps * n_traj * n_pos bytes, step-major
 * (codes[(r * n_traj + w) * n_pos + p], values 1..4, else ADX_EINVAL).
 * pos_matches = n_pos * (max_lag + 1) int64 summed over trajectories;
 * traj_matches = n_traj * (max_lag + 1) int64 summed over positions (optional). */
adx_status adx_autocorr_codes(int device, int n_traj, int n_steps, int n_pos, const uint8_t *codes,
                              int max_lag, int64_t *pos_matches, int64_t *traj_matches);

/* The same over the steps recorded so far (adx_record_begin), the first
 * `discard` dropped: x[i] is the base after recorded row discard + i, the
 * sequence adx_record_picks returns for that step, S' = rows - discard.
 * A position is changeable if it is in the closure list of a freely mutable
 * position (the position itself and the partners that get its complement);
 * every other position matches at every step.
 * pos_matches = N * (max_lag + 1), summed over walkers; optional (NULL):
 * walker_matches = W * (max_lag + 1) summed over the changeable positions,
 * base_counts = N * 4 (A, C, G, U over the kept steps of all walkers),
 * outcome_counts = W * 4 (kept steps; order of adx_trace.outcome),
 * changeable = N flags, *n_changeable.
 * max_lag < 0, discard < 0, discard >= rows or max_lag > S' - 1: ADX_EINVAL;
 * before adx_record_begin, with nothing recorded or on a broken record:
 * ADX_ESTATE, as adx_record_picks.  May be repeated and interleaved with
 * adx_record_picks; touches neither the walkers nor the record. */
adx_status adx_record_autocorr(adx_ctx *ctx, int max_lag, int discard, int64_t *pos_matches,
                               int64_t *walker_matches, int64_t *base_counts, int64_t *outcome_counts,
                               unsigned char *changeable, int *n_changeable);
/* Device time (ms, HIP events) of the context's last adx_record_autocorr:
 * packing the bit planes (with the replay) and the lag kernel. */
adx_status adx_last_autocorr_ms(const adx_ctx *ctx, double *pack_ms, double *lag_ms);

/* Host arithmetic only, no GPU: the correlation time of a pooled curve.
 * a_k = matches[k] / (n_series * (kept_steps - k)); *tau = the least k >= 1
 * with a_k - baseline <= (1 - baseline) / e; -1 if no lag up to max_lag does
 * (the curve has not decayed: ask for more lags); 0 if baseline >= 1 (nothing
 * ever changed).  For a record the baseline is the chance that two
 * independent draws match: the mean over the changeable positions of
 * sum_c f_pc^2, f_pc = base_counts[p][c] / (W * S'). */
adx_status adx_autocorr_time(const int64_t *matches, int max_lag, int64_t n_series, int64_t kept_steps,
                             double baseline, int *tau);

/* ------------------------------------------------------------------------
 * Distinct designs from scored sequences on the device: the sequence-space
 * twin of the pick rule (picks are the best steps at least `window` steps
 * apart in time, designs the best entries more than `radius` mutations apart
 * in sequence).  For M entries (N bases A, C, G, U in either case, and a
 * score), a radius r >= 0 and a cap K >= 1:
 *   distance   the Hamming distance, bases compared case-insensitively
 *   order      score descending (==: -0.0 ties with +0.0), ties by the lower
 *              entry index; an entry with a non-finite score takes no part
 *              (member_of = -1, counted nowhere)
 *   selection  while fewer than K designs exist and an uncovered entry is
 *              left: the first uncovered entry in order becomes the leader of
 *              design d = 0, 1, ..., and every uncovered entry within r of it,
 *              itself included, is covered by d (member_of = d).  So an entry
 *              leads iff no earlier leader is within r of it, and otherwise
 *              belongs to the lowest-numbered leader within r; entries still
 *              uncovered when K is reached keep -1.  r = 0 removes exact
 *              duplicates; r >= N makes one design.
 *   pair_hist  [d], d = 0..N: the unordered pairs of finite-score entries at
 *              distance d; the sum is F (F - 1) / 2 for F such entries.  It
 *              shows how concentrated the entries are and what radius makes
 *              sense, as the autocorrelation does for the window.
 * All of it is integer work: equal inputs give equal bytes.
 * ---------------------------------------------------------------------- */

/* Stateless: seqs = n_seqs * length chars, no terminators; scores[n_seqs].
 * leaders, sizes = max_designs int32 each, the first *n_designs valid: the
 * leader's entry index and the number of entries the design covers.
 * member_of = n_seqs int32 and pair_hist = (length + 1) int64 are optional
 * (NULL; the all-pairs pass is skipped without pair_hist).  n_seqs < 1, length
 * outside 1..255, radius < 0, max_designs < 1 or a character outside
 * ACGU / acgu: ADX_EINVAL. */
adx_status adx_select_designs(int device, int n_seqs, int length, const char *seqs,
                              const double *scores, int radius, int max_designs,
                              int *n_designs, int32_t *leaders, int32_t *sizes,
                              int32_t *member_of, int64_t *pair_hist);

/* The same over the picks of the steps recorded so far (adx_record_begin):
 * the entries are what adx_record_picks returns for `window` (with its own
 * cap, ceil(recorded steps / window)), walker-major and then by ascending
 * step, so equal scores go to the lower walker and then the lower step;
 * walkers with a count of -1 contribute nothing.  Picks, sequences and the
 * selection stay on the device; only the designs and the histogram cross.
 * Per design, max_designs entries each, the first *n_designs valid: walkers,
 * steps (global 0-based, as adx_record_picks), scores and seqs (max_designs * N
 * chars, no terminators) of its leader; sizes, the picks it covers; n_walkers,
 * the distinct walkers among them (a pick counts iff no earlier pick of its
 * walker has the same design: the evidence of independent rediscovery).
 * *n_picks_total = the number of entries; pair_hist = (N + 1) int64.  Every
 * output but n_designs is optional (NULL).  A record in which no walker has a
 * pick gives *n_designs = 0 and ADX_OK.  window < 1, radius < 0 or
 * max_designs < 1: ADX_EINVAL; before adx_record_begin, with nothing recorded
 * or on a broken record: ADX_ESTATE, as adx_record_picks.  May be repeated and
 * interleaved with adx_record_picks and adx_record_autocorr; touches neither
 * the walkers nor the record. */
adx_status adx_record_designs(adx_ctx *ctx, int window, int radius, int max_designs,
                              int *n_designs, int32_t *walkers, int64_t *steps,
                              double *scores, char *seqs, int32_t *sizes,
                              int32_t *n_walkers, int64_t *n_picks_total, int64_t *pair_hist);
/* Device time (ms, HIP events) of the context's last adx_record_designs:
 * packing, ordering and selecting (with the leaders' gather), and the
 * all-pairs histogram (0 without pair_hist).  The picking and replay before
 * them are not included. */
adx_status adx_last_design_ms(const adx_ctx *ctx, double *select_ms, double *hist_ms);

/* Variant v of the score: which (context, condition, macrostate or -1). */
adx_status adx_variant_desc(const adx_ctx *ctx, int v, int *context, int *condition,
                            int *macrostate);

#ifdef __cplusplus
}
#endif
#endif
