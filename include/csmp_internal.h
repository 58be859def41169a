/*
 * csmp_internal.h -- measurement and test hooks of libcsmp.so.  NOT part of the drop-in boundary: nothing a host of the
 * reference's API (mp / omp / gomp / sp, the Update functors) needs is declared here, and the Julia wrapper binds none of it.
 * bench.py, tools/ and tests/ bind these through compressedsensing.jl_amd/_lib.py (INTERNAL_SIGNATURES).
 */
#ifndef CSMP_INTERNAL_H
#define CSMP_INTERNAL_H
#include "csmp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* on = 1: every sweep launch is bracketed by HIP events on the ctx stream; on = n > 1: every
 * n-th launch only (an event pair costs a few microseconds of stream time); 0 = off. */
int csmp_profile_enable(csmp_ctx *ctx, int on);
/* number of sweep launches timed and the sum of their durations (ms); reset != 0 clears */
int csmp_profile_read(csmp_ctx *ctx, int64_t *sweep_launches, double *sweep_ms, int reset);
/* the timed launches of this context and of the second pipeline of csmp_omp_batch (its twin) as ONE window: launches from the first
 * to the last sampled one on each stream, the time from the earliest start event to the latest end event, the mean duration of a
 * sampled launch, the number of streams that carried timed launches.  Before csmp_profile_read, which consumes the events. */
int csmp_profile_window(csmp_ctx *ctx, int64_t *launches, double *window_ms, double *mean_launch_ms, int *streams);
/* average reading (ms) of an event pair with nothing between its two records: the share of a timed launch's bracket that is the
 * bracket itself */
int csmp_profile_overhead(csmp_ctx *ctx, int reps, double *avg_ms);
/* what the library holds at this moment, process-wide: bytes and blocks of device memory, bytes of page-locked host memory, host ranges
 * registered with the device, events, streams.  Every one is zero when no context exists (tests/test_gpu_leaks.py).  Any pointer may be NULL. */
int csmp_live_resources(int64_t *device_bytes, int64_t *device_blocks, int64_t *pinned_bytes, int64_t *registered_ranges, int64_t *events,
                        int64_t *streams);
/* sweep bandwidth probe: `reps` product sweeps (argmaxinner!(P), src/matchingpursuit.jl:181-185) of a random residual,
 * bracketed by one HIP event pair on the ctx stream; returns the average ms per sweep.  variant 0: the product kernel.  Variants
 * 1 .. 3 time the passes of csmp_omp_batch's grouped scheduler alone, as it launches them -- 1: the shared pass of group_max residuals
 * (k_sweep_multi); 2: the wide pass of 2 * group_max residuals (k_sweep_wide, Float32), nontemporal loads; 3: the wide pass with
 * default-policy loads (what the scheduler runs).  1 .. 3 store every member's c; 4 and 5 are 1 and 3 without c stores, as csmp_omp_batch's
 * grouped scheduler launches them.  CSMP_TUNE_GROUP_MAX and CSMP_TUNE_TICK_GRID set their members and grid. */
int csmp_bench_sweep(csmp_ctx *ctx, int variant, int reps, double *avg_ms);
/* the N-pass of csmp_ard_weights alone, on the directions W = A_S L^-T the LAST csmp_ard_weights call of this context left behind (k of
 * them): `reps` runs bracketed by one HIP event pair, the average ms of one.  variant 0: k_ard_forms, the fused kernel the library runs.
 * variant 1: the yardstick -- the existing k_fr_rebuild_lds launched once per block of 128 directions on rho2 = |a_j|^2 (k_fr_colnorm2),
 * then a root kernel.  max_diff (may be NULL): max_j |w_j(fused) - w_j(split)|.  CSMP_ESTATE: no such call has been made. */
int csmp_bench_ard_forms(csmp_ctx *ctx, int variant, int reps, double eps, double *avg_ms, double *max_diff);
/* G = A A' of the resident dictionary by k_rowgram and its reduction alone (csmp_bp forms it once per dictionary and keeps it): M x M
 * doubles, column-major and exactly symmetric, to host (loc = CSMP_HOST) or device memory (CSMP_DEVICE).  Nothing of the context changes. */
int csmp_bp_rowgram(csmp_ctx *ctx, double *G_out, int loc);
/* C0 = A diag(gamma) A' of the resident dictionary by the weighted k_rowgram and its reduction alone (the first stage of a csmp_sbl
 * update): M x M doubles, column-major and exactly symmetric.  gamma: size(A,2) doubles.  loc says where gamma and C_out live
 * (CSMP_HOST / CSMP_DEVICE).  The column splits are csmp_bp_rowgram's.  Nothing of the context changes. */
int csmp_sbl_rowgram(csmp_ctx *ctx, const double *gamma, double *C_out, int loc);
/* k_sbl_forms alone (the N-pass of a csmp_sbl update) on directions of the caller's:  s_j = sum_d (w_d' a_j)^2,  q_j = sum_d (w_d' a_j) t_d
 * for every atom j, w_d = column d of W, d = 0 .. M - 1.  W: column-major with leading dimension ldw, a multiple of 64 that is at least
 * M, UPPER TRIANGULAR: of column d the kernel uses the rows 0 .. d and nothing else -- with D = d / 128, the 64-row blocks from row
 * 128 (D + 1) on are never read, and inside the blocks that are read an entry below the diagonal counts as zero whatever it holds.
 * t: M doubles; s, q: size(A,2) doubles.  loc says where all four live; a device W starts on a 16-byte boundary.  CSMP_EDIM: ldw. */
int csmp_sbl_forms(csmp_ctx *ctx, const double *W, int64_t ldw, const double *t, double *s, double *q, int loc);
/* the three stages of one csmp_sbl update on the gamma and b the LAST csmp_sbl call of this context left behind, each bracketed by HIP
 * events: the weighted Gram matrix and its reduction; the assembly, the factorisation, L^-T and t = L^-1 b; k_sbl_forms.  The averages
 * (ms) of `reps` runs after one warm-up run; gamma is not updated.  Any pointer may be NULL.  CSMP_ESTATE: no such call has been made. */
int csmp_bench_sbl(csmp_ctx *ctx, double sigma2, int reps, double *gram_ms, double *factor_ms, double *forms_ms);
/* k_fsbl_score and k_fsbl_pick alone (the N-pass of a csmp_fsbl / csmp_rmps step) on a state of the caller's: alpha (+inf = inactive), S
 * and Q, size(A,2) doubles each in host memory.  mode: 1 fsbl's delta, 2 the acquisition value, 3 rmps' deletion value (the MINIMUM is
 * picked), 4 the update value.  values: every atom's value, size(A,2) doubles; pick, value: the first arg-max (arg-min) and its value;
 * action: what the drivers would apply to it, 0 nothing, 1 add, 2 delete, 3 re-estimate.  pick, value and action may be NULL.
 * CSMP_EINVAL: a value that is NaN, or an infinite maximum. */
int csmp_fsbl_score(csmp_ctx *ctx, const double *alpha, const double *S, const double *Q, int mode, double *values, int64_t *pick,
                    double *value, int *action);
/* the rank-one step sqc(i, gamma) alone -- k_fsbl_col, v = C^-1 a_i, k_fsbl_rank1, w = A'v and the S / Q update of the next N-pass -- on a
 * state of the caller's, updated in place in host memory: Cinv, size(A,1)^2 doubles, column-major and symmetric; S and Q, size(A,2)
 * doubles.  gamma: the change of atom i's prior variance, finite and not zero. */
int csmp_fsbl_sqc(csmp_ctx *ctx, double *Cinv, double *S, double *Q, int64_t i, double gamma);
/* the parts of one greedy step on the state the LAST csmp_fsbl / csmp_rmps call of this context left behind, each bracketed by HIP
 * events: the N-pass with the pending S / Q update and the pick; the column and v = C^-1 a_i; the rank-one update of C^-1; the product
 * sweep w = A'v.  Every run adds the prior variance 1 to atom 0.  The averages (ms) of `reps` runs after one warm-up run.  Any pointer may
 * be NULL.  CSMP_ESTATE: no such call has been made. */
int csmp_bench_fsbl(csmp_ctx *ctx, int reps, double *score_ms, double *colgemv_ms, double *rank1_ms, double *sweep_ms);
/* what configure_sweep chose for the resident dictionary: loads per unit of k_sweep_gen (16 / 8 / 4); phases the residual is
 * staged in (1: one LDS image); workgroups of a stand-alone sweep and of the sweep inside the tick kernel; dynamic LDS bytes;
 * dynamic = 1: the columns are handed out at run time (k_sweep_dyn and the DYN tick), 0: split statically; columns_per_unit: 2 or 4
 * where the stand-alone sweep takes short columns several at a time (k_sweep_short), else 1.  Any pointer may be NULL. */
int csmp_sweep_config(const csmp_ctx *ctx, int *unit_loads, int *phases, int *workgroups, int *tick_workgroups, int64_t *lds_bytes, int *dynamic,
                      int *columns_per_unit);
/* signals one shared sweep of csmp_omp_batch's grouped scheduler serves for the resident dictionary (k_sweep_multi: one LDS image of
 * the residual per signal, at most 4); 0 = no shared sweep for this dictionary (a phased or dynamic sweep): that scheduler is not used */
int csmp_sweep_group(const csmp_ctx *ctx, int *group_max);
/* signals one PASS of that scheduler serves: 2 * group_max where wide groups are on (k_sweep_wide: two workgroups with group_max images
 * each read the same bytes of A), else group_max */
int csmp_sweep_group_wide(const csmp_ctx *ctx, int *group_wide);
/* measurement overrides of that choice, applied to the resident dictionary at once and to later ones: 0 = automatic */
#define CSMP_TUNE_SWEEP_GRID 2   /* workgroups of the product sweep */
#define CSMP_TUNE_SWEEP_UNIT 3   /* loads per unit (16, 8 or 4) */
#define CSMP_TUNE_TICK_GRID 4    /* sweep workgroups inside the tick kernel of csmp_omp_batch */
#define CSMP_TUNE_SWEEP_DYN 9     /* 1: the product sweep hands its columns out at run time (k_sweep_dyn; one LDS image, grids up to 512 workgroups); n = 2..64: only the last 1 / n of a workgroup's columns, after a static head; default 0: the static split */
#define CSMP_TUNE_PIPELINES 12    /* 1: csmp_omp_batch keeps one pipeline of three signals; 2: two pipelines side by side whatever the sizes (rounds of 3 + 3 signals, the remainder 1 + 1); 3: two pipelines of three GROUPS of signals, each group's sweeps one shared pass over A (k_sweep_multi); default 0: 3 where a shared pass serves two or more signals, else 2, from two signals and a 4-MiB dictionary on; 3 falls back to 2 where no shared sweep exists.  csmp_mp_batch: 1 keeps one stream, 2 and 3 take two whatever the size; a round with a single group runs its halves on the two streams under 2 and the whole group on one under 3 */
#define CSMP_TUNE_GROUP_MAX 20    /* largest group of the grouped scheduler (CSMP_TUNE_PIPELINES 3); 0 = as many residual images as the LDS holds, at most 4 */
#define CSMP_TUNE_GROUP_WIDE 21   /* 1: no wide groups (every pass serves at most group_max signals); 2: wide groups, the three of a round on ONE pipeline (a measurement: slower); default 0: batches of more signals than that run groups of up to 2 * group_max wherever the grouped scheduler has group_max = 4 images per workgroup on a Float32 dictionary and CSMP_TUNE_GROUP_MAX is 0.  CSMP_TUNE_TICK_GRID overrides the wide pass's grid too, rounded down to a multiple of 16 */
#define CSMP_TUNE_ROWGRAM_SCALAR 22 /* 1: k_rowgram (csmp_bp, csmp_bp_rowgram) loads the dictionary with scalar loads, as for columns that start on no 16-byte boundary (the library's own copy always does: tests reach that instantiation here); the same bits */
#define CSMP_TUNE_SBL_SCALAR 25   /* 1: csmp_sbl's kernels that read the dictionary (the weighted k_rowgram, k_sbl_forms; csmp_sbl_rowgram and csmp_sbl_forms too) load it with scalar loads, as for columns that start on no 16-byte boundary; the same bits */
#define CSMP_TUNE_FSBL_SCALAR 26  /* 1: k_fsbl_col (csmp_fsbl, csmp_rmps, csmp_fsbl_sqc) loads the picked column with scalar loads, as for columns that start on no 16-byte boundary; the same bits */
#define CSMP_TUNE_PASS_C 23      /* 1: the shared passes of csmp_omp_batch's grouped scheduler store every member's c = A'r, which nothing reads there; default 0: they store none (csmp_mp_batch's passes always do).  The same results */
#define CSMP_TUNE_GROUP_SPLIT 24  /* how the grouped scheduler cuts a batch into WIDE groups (host/batch_plan.hpp: narrow_last_groups).  Default 0: ceil(nsig / group_wide) groups, the last one of group_max signals -- a narrow pass -- where that takes no pass more (18 signals: 8 + 6 + 4); 1: as even as possible (6 + 6 + 6); 2, 3: measurements (7 + 7 + 4, 8 + 8 + 2).  The same results */
#define CSMP_TUNE_TICK_ORDER 10   /* 1: the tick kernel's sweep workgroups are dispatched ahead of its append stages' */
#define CSMP_TUNE_CLAIM_POOLS 11  /* the dynamic sweep: column pools a workgroup may claim from (its own first) */
#define CSMP_TUNE_PAIR_LDS_KIB 13 /* dynamic LDS (KiB) requested by the ticks of two pipelines side by side: above 80 = one workgroup per CU (default 81), 1 = what the kernels need */
#define CSMP_TUNE_PAIR_SPLIT 14   /* 1: two pipelines side by side keep the fused tick (append stages + sweep in ONE launch under the large LDS request); default 0: two launches per tick */
#define CSMP_TUNE_SWEEP_LDS_KIB 15 /* dynamic LDS (KiB) the stand-alone product sweep REQUESTS when that is more than it uses: above 80 = one workgroup per CU, 54 = two */
#define CSMP_TUNE_SWEEP_SHORT 16  /* 1: the stand-alone sweep keeps one column per unit for every shape (default 0: columns of up to four 1-KiB chunks go two or four to a unit, k_sweep_short) */
#define CSMP_TUNE_PHASE_ROWS 17   /* the phased sweep (a residual longer than the LDS): most rows of one stage; 0 = as many as the LDS holds */
#define CSMP_TUNE_SCREEN_STATIC 19 /* 1: the screened (image) sweeps deal their column groups out statically; default 0: by ticket counters (measured: 12 % faster for a lone 2-GiB sweep, level with three solves in flight) */
#define CSMP_TUNE_FAIL_ALLOC 18   /* test hook: the n-th device allocation of solver state from now fails for real (hipMalloc of an impossible size: hipErrorOutOfMemory stays pending); 0 = off */
#define CSMP_TUNE_REBUILD_DIRECT 8 /* 1: the oblivious start of csmp_srr forms Q'A with its directions read from L2 per wave (k_fr_rebuild), not staged in the LDS */
#define CSMP_TUNE_SWAP_REFUSE 7 /* 1: every exchange of csmp_ompr on the inverse Gram matrix fails its guard: the fallback to the QR path runs */
#define CSMP_TUNE_DIAG_SPLIT 6   /* 1: kernels that fuse independent parts run one launch per part (same results; a kernel trace shows the parts) */
#define CSMP_TUNE_BATCH_BUDGET_MIB 5 /* csmp_omp_batch_mfma: HBM (MiB) its per-signal state may take -- a test's stand-in for a full device */
int csmp_tune(csmp_ctx *ctx, int key, int64_t value);

/* layout of the last csmp_omp_batch_mfma call: signal columns of one screening launch (the batch
 * padded to whole 256-signal tiles) and the number of streams used (1: the screening GEMM and the per-signal
 * kernels alternate on the context's stream) */
int csmp_batch_layout(const csmp_ctx *ctx, int64_t *screen_signals, int *streams);
/* name of the screening kernel the last csmp_omp_batch_mfma call ran ("none": the exact sweeps served it) */
const char *csmp_batch_screen_kernel(const csmp_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
