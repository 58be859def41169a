/*
 * csmp.h -- C ABI of libcsmp.so: the MI355X (gfx950) matching-pursuit path of
 * CompressedSensing.jl (mp / omp / gomp / sp and their step primitives).
 *
 * The reference is pure Julia and has no FFI seam of its own; the seam is the set of methods
 * dispatched on AbstractMatchingPursuit plus the UpdatableQR API they call.
 * Each entry point below names the reference interface it replaces (paths relative to the
 * reference repository).  A Julia host binds these with `ccall` (see INTEGRATION.md and
 * compressedsensing.jl_amd/julia/CompressedSensingAMD.jl); the Python host mirror binds them
 * with ctypes (compressedsensing.jl_amd/_lib.py).
 *
 * Conventions
 *   - A: dense column-major, M rows (signal length) x N columns (atoms), leading dimension ldA
 *     in elements, element type CSMP_F32 or CSMP_F64.  NOTE the reference names these
 *     `n, m = size(A)` (src/matchingpursuit.jl:20); BASELINE.json uses m=rows, n=cols.
 *   - All selection arithmetic is Float64 on the exactly promoted dictionary values, so an f32
 *     dictionary yields the support a Float64 run of the reference would select on the same values.
 *   - Results follow SparseVector{Float64,Int64} (src/matchingpursuit.jl:76): indices sorted
 *     ascending (0-BASED here; the Julia wrapper adds 1), values aligned, nnz may be < k.
 *   - Every call returns a status (0 = ok, negative = error);
 *     csmp_last_error() gives the text of an error.
 *   - A ctx is bound to one GPU and one HIP stream and is not thread-safe (the reference is
 *     single-threaded too).  Caller owns every buffer passed in; the library owns device memory
 *     behind the opaque ctx.  `loc` says where a caller buffer lives: CSMP_HOST or CSMP_DEVICE.
 */
#ifndef CSMP_H
#define CSMP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CSMP_OK 0
#define CSMP_EINVAL (-1) /* eps < 0 (reference: throw("eps has to be non-negative"), src/matchingpursuit.jl:74,127), bad argument */
#define CSMP_EDIM (-2)   /* length(b) != size(A,1) and the like */
#define CSMP_ERANGE (-3) /* 2k > M for SP (reference: error(...), src/twostage.jl:55); k out of range */
#define CSMP_EHIP (-4)   /* HIP runtime failure / no gfx950 device */
#define CSMP_ESTATE (-5) /* no dictionary set / no solver begun */
#define CSMP_ENOMEM (-6)
#define CSMP_ERCCL (-7)  /* RCCL could not be loaded, or a communicator / collective call failed */
#define CSMP_EIO (-8)    /* a dictionary file could not be read or written */
#define CSMP_F32 0
#define CSMP_F64 1
#define CSMP_HOST 0
#define CSMP_DEVICE 1
#define CSMP_HOST_STREAMED 2 /* csmp_set_dictionary / csmp_set_dictionary_file only: the dictionary stays in host memory (below) */

#define CSMP_ALGO_MP 0
#define CSMP_ALGO_OMP 1
#define CSMP_ALGO_GOMP 2
#define CSMP_ALGO_FR 3 /* update!(P::FR, x): src/forward.jl:88-95 */
#define CSMP_ALGO_SP 4   /* SP(A,b,k), update!(P::SP, x): src/twostage.jl:42-83 */
#define CSMP_ALGO_OMPR 5 /* OMPR(A,b,k), update!(P::OMPR, x) with eta = 1: src/twostage.jl:110-180 */

/* why a solve stopped early (csmp_solver_state: *stop) */
#define CSMP_STOP_NONE 0
#define CSMP_STOP_EPS 1    /* norm(residual) < eps: src/matchingpursuit.jl:79,132 */
#define CSMP_STOP_STAG 2   /* arg-max atom already selected: src/matchingpursuit.jl:66 */
#define CSMP_STOP_FULL 4   /* nnz(x) == size(A,1): src/matchingpursuit.jl:63,117 */

typedef struct csmp_ctx csmp_ctx;

/* ------------------------------------------------------------------ lifetime */
int csmp_version(void);
int csmp_create(csmp_ctx **out, int device_id);
int csmp_destroy(csmp_ctx *ctx);
const char *csmp_last_error(const csmp_ctx *ctx); /* ctx may be NULL: last create error */
/* borrow a caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int csmp_set_stream(csmp_ctx *ctx, void *hip_stream);
int csmp_sync(csmp_ctx *ctx);
/* name (<=255 chars), compute-unit count and total HBM bytes of the bound device */
int csmp_device_info(csmp_ctx *ctx, char *name, int name_len, int *compute_units, int64_t *hbm_bytes);

/* ------------------------------------------------------------------ dictionary
 * Replaces the `A` field of MP/OMP/GOMP/SP (src/matchingpursuit.jl:10-24,44-60,95-114;
 * src/twostage.jl:42-61).  Uploaded once, stays resident in HBM.  A CSMP_DEVICE pointer that is
 * 16-byte aligned with M and ldA multiples of 16 bytes is borrowed without a copy.
 * The entries must be FINITE.  The sweeps pad a column's last load by re-reading its own last 16 bytes against zeros of the
 * residual image (no predicate in the load stream): an Inf or NaN there gives 0 * Inf = NaN for THAT column's product, where
 * the reference's mul! would leave an Inf -- no other column is touched, and a column with a non-finite entry has no
 * meaningful correlation in the reference either. */
int csmp_set_dictionary(csmp_ctx *ctx, const void *A, int64_t M, int64_t N, int64_t ldA, int dtype, int loc);
/* A dictionary LARGER THAN HBM (not in the reference, whose A is whatever the host's memory holds):
 * loc = CSMP_HOST_STREAMED leaves A in HOST memory, page-locked and mapped into the device's address space, and every kernel that
 * reads A -- the sweeps, the column gathers of the appends -- reads it over the host link (PCIe 5 x16: ~50 GB/s against
 * 6.6 TB/s from HBM; the results are those of the resident dictionary, bit for bit).  A 16-byte aligned array with M and ldA
 * multiples of 16 bytes is registered where it lies (hipHostRegister: no second copy; the caller keeps it alive and unchanged
 * until the context is destroyed or given another dictionary); anything else is copied into page-locked memory of the library's.
 *
 * Dictionary files: a 64-byte header ("CSMPDICT", u32 version 1, u32 dtype, i64 M, i64 N, i64 ld, 24 zero bytes) followed by
 * the N columns, ld elements each (M rounded up to 16 bytes, zero padded), little-endian.  csmp_dictionary_file_write writes one
 * from host memory; csmp_set_dictionary_file reads one to where it will live -- HBM (loc = CSMP_DEVICE: chunked upload, the file
 * never sits in host memory whole) or mapped host memory (loc = CSMP_HOST_STREAMED). */
int csmp_dictionary_file_write(const char *path, const void *A, int64_t M, int64_t N, int64_t ldA, int dtype);
int csmp_dictionary_file_info(const char *path, int64_t *M, int64_t *N, int *dtype);
int csmp_set_dictionary_file(csmp_ctx *ctx, const char *path, int loc);
/* A second context on the same GPU that borrows (does not copy) src's resident dictionary: the reference's P
 * objects are independent of one another and share only A -- P1 = OMP(A, b1); P2 = OMP(A, b2)
 * (src/matchingpursuit.jl:44-60) -- so every step-level solver (csmp_solver_begin) that must live beside
 * another one gets a clone.  A dictionary the library copied (host pointer, or an unaligned device pointer) is reference
 * counted: it lives until the last context holding it is destroyed or given another dictionary, whatever the order.  A
 * BORROWED device pointer (zero-copy, see csmp_set_dictionary) stays the caller's to keep alive. */
int csmp_clone(csmp_ctx *src, csmp_ctx **out);

/* ------------------------------------------------------------------ drivers (synchronous)
 * b: length M, element type b_dtype, host memory.  idx/val/order: caller arrays of capacity
 * given per function; *nnz receives the count.  order (may be NULL): atoms in selection order. */

/* mp(A,b,k,x): src/matchingpursuit.jl:26-40.  x0 = optional warm start (idx0 sorted or not).
 * idx/val capacity k + nnz0. */
int csmp_mp(csmp_ctx *ctx, const void *b, int b_dtype, int64_t k, const int64_t *idx0, const double *val0,
            int64_t nnz0, int64_t *idx, double *val, int64_t *nnz);

/* omp(A,b,eps,k): src/matchingpursuit.jl:62-82 (update! :62-70).  The caller supplies eps
 * (the Julia/Python wrappers default it to eps(eltype(A)): :85,89).  Capacity k. */
int csmp_omp(csmp_ctx *ctx, const void *b, int b_dtype, int64_t k, double eps, int64_t *idx, double *val,
             int64_t *nnz, int64_t *order);

/* gomp(A,b,l,eps,k): src/matchingpursuit.jl:116-139, including the remainder step :134-137.
 * Capacity k + l. */
int csmp_gomp(csmp_ctx *ctx, const void *b, int b_dtype, int64_t l, int64_t k, double eps, int64_t *idx,
              double *val, int64_t *nnz, int64_t *order);

/* sp(A,b,k,delta;maxiter): src/twostage.jl:54-107.  maxiter < 0 selects the default 16k.
 * Capacity 2k.  *iters (may be NULL) = number of update! calls made. */
int csmp_sp(csmp_ctx *ctx, const void *b, int b_dtype, int64_t k, double delta, int64_t maxiter, int64_t *idx,
            double *val, int64_t *nnz, int64_t *iters);

/* ompr(A,b,k,delta;maxiter): OMP with replacement, src/twostage.jl:110-202, with x starting empty
 * (the support is filled by oblivious_acquisition!, src/matchingpursuit.jl:207-216).  maxiter < 0
 * selects the default size(A,1).  Capacity k.  *iters (may be NULL) = number of update! calls. */
int csmp_ompr(csmp_ctx *ctx, const void *b, int b_dtype, int64_t k, double delta, int64_t maxiter, int64_t *idx,
              double *val, int64_t *nnz, int64_t *iters);

/* ompr_batch: csmp_ompr(ctx, B[:, s], k, delta_s, maxiter) for every column of B, the update!s of up to sweep_group signals -- group_wide
 * where wide groups are granted -- in lockstep: ONE shared pass reads the dictionary for all members of a group, one launch of each
 * kernel of the exchange chain serves all of them, and the host reads one landing per tick (host/ompr_batch.hpp).
 * Every result is the single call's bit for bit -- support, coefficients, iteration count -- whatever the batch size, the group
 * size and the order in which freed slots are refilled.
 * B: ldB x nsig, column-major, host or device memory (b_loc); idx, val: k x nsig, nnz, iters: nsig, HOST memory (csmp_omp_batch's
 * layout: signal s's entries from s * k, nnz[s] of them written); iters and flags may be NULL.  delta: ndelta = 1 threshold for all
 * signals or ndelta = nsig, one per column.  maxiter < 0 selects size(A,1), as csmp_ompr.
 * flags[s]: CSMP_OMPR_SOLVED_ALONE -- the signal left its group (an exchange the guard refused, an arg-max inside the support, an
 * acquisition short of k atoms: the steps off the inverse Gram matrix's fast path) and was solved from the start by csmp_ompr.
 * The whole call is the loop over csmp_ompr where the dictionary has no shared pass (or csmp_tune switched it off), for nsig < 2, with
 * CSMP_OPT_SCREENED_SWEEP on, on a host-streamed dictionary and for k > 4095: the same results.
 * CSMP_EINVAL: NULL arguments, k < 1, nsig < 0, ndelta neither 1 nor nsig, a NaN delta, a bad b_dtype or b_loc.  CSMP_EDIM: ldB <
 * size(A,1).  CSMP_ERANGE: k > min(size(A)).  CSMP_ESTATE: no dictionary.  CSMP_ENOMEM: a member's buffers could not be allocated;
 * the context and the library stay usable.  nsig == 0: CSMP_OK, the device is not touched. */
#define CSMP_OMPR_SOLVED_ALONE 1
int csmp_ompr_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k,
                    const double *delta, int64_t ndelta, int64_t maxiter,
                    int64_t *idx, double *val, int64_t *nnz, int64_t *iters, int *flags);

/* fr(A,b,max_eps,min_delta,k) = ols = oomp = ormp: forward regression / orthogonal least squares,
 * src/forward.jl:44-54 (forward_step! :56-73, forward_δ! :75-82, ols_rescaling! :99-114), with x
 * starting empty.  Each step adds the atom maximising <a_j,r>^2 / (|a_j|^2 - |Q_S' a_j|^2); stops
 * when norm(r) <= max_eps, when the best score does not exceed min_delta^2, or at k atoms / nnz = M.
 * Capacity k.  (Any M: columns whose two LDS images, 16 M bytes, exceed the LDS -- M beyond ~10 000 -- are swept once per image.) */
int csmp_fr(csmp_ctx *ctx, const void *b, int b_dtype, int64_t k, double max_eps, double min_delta, int64_t *idx,
            double *val, int64_t *nnz, int64_t *order);
/* P.δ² of the most recent forward-regression step (src/forward.jl:11,75-82; foba reads its maximum,
 * src/stepwise.jl:52): delta2 receives N Float64 scores (host). */
int csmp_fr_scores(csmp_ctx *ctx, double *delta2);

/* srr(A,b,k,delta; maxiter,initialization,l): stepwise regression with replacement, src/twostage.jl:3-33,
 * x starting empty.  initialization 1 = oblivious_acquisition! (src/matchingpursuit.jl:207-216),
 * 2 = k forward-regression steps; each iteration takes l forward steps (src/forward.jl:56-73) and then
 * backward steps (src/backward.jl:51-83) until k atoms remain.  maxiter < 0 selects the default 4k.
 * Capacity k + l (at most 4095).  *iters (may be NULL) = iterations made. */
int csmp_srr(csmp_ctx *ctx, const void *b, int b_dtype, int64_t k, double delta, int64_t maxiter, int initialization,
             int64_t l, int64_t *idx, double *val, int64_t *nnz, int64_t *iters);
/* srr with initialization = 3 (random_acquisition!, src/matchingpursuit.jl:195-204; src/twostage.jl:14-16): init[0..k) are the k
 * distinct atoms of the initial support (0-based, any order).  The reference draws them with sample(1:n, k, replace = false) from
 * the host language's RNG; here the host draws and passes them, everything after the draw is the reference's.  The same call is
 * the warm start srr(A, b, k, delta, x) of a full support, nnz(x) == k (src/twostage.jl:7-9: P is built on x.nzind and the
 * acquisition of k - nnz(x) = 0 further atoms changes nothing). */
int csmp_srr_from(csmp_ctx *ctx, const void *b, int b_dtype, int64_t k, double delta, int64_t maxiter, const int64_t *init,
                  int64_t l, int64_t *idx, double *val, int64_t *nnz, int64_t *iters);

/* rmp(A,b,delta,maxiter) (src/stepwise.jl:5-26), rmp(A,b,k) (:32-43) and foba(A,b,delta) (:47-56), x
 * starting empty: loops over forward_step! (src/forward.jl:56-73) and backward_step!
 * (src/backward.jl:51-67) of the StepwiseRegression object.  kmax (<= 0: min(M, N, 4095)) is the largest
 * support the forward stage may build; reaching it below min(M,N) is CSMP_ERANGE.  Capacity of idx/val:
 * kmax.  maxiter < 0 selects the default 1. */
int csmp_rmp_delta(csmp_ctx *ctx, const void *b, int b_dtype, double delta, int64_t maxiter, int64_t kmax,
                   int64_t *idx, double *val, int64_t *nnz);
int csmp_rmp_k(csmp_ctx *ctx, const void *b, int b_dtype, int64_t k, int64_t kmax, int64_t *idx, double *val,
               int64_t *nnz);
int csmp_foba(csmp_ctx *ctx, const void *b, int b_dtype, double delta, int64_t kmax, int64_t *idx, double *val,
              int64_t *nnz);

/* br(A,b,max_eps,max_delta,k) = fbr (src/backward.jl:27-35,154-162) and, with lace != 0,
 * lace(A,b,eps,delta,k) (:233-270): backward regression from the least-squares solution on all N <= M
 * columns (N <= 4095).  Infinite thresholds are passed as HUGE_VAL.  Capacity of idx/val: N. */
int csmp_br(csmp_ctx *ctx, const void *b, int b_dtype, double max_eps, double max_delta, int64_t k, int lace,
            int64_t *idx, double *val, int64_t *nnz);

/* Many independent signals sharing the resident dictionary: omp(A, B[:,s], eps, k) for
 * s = 0..nsig-1 (the loop a caller of the reference writes around omp; signals are independent,
 * SURVEY.md section 8e).  B: M x nsig column-major (ldB elements) on host or device (b_loc);
 * outputs idx (k x nsig, int64, unused tail = -1), val (k x nsig, f64, unused tail = 0),
 * nnz (nsig) on host or device (out_loc).  All signals are enqueued back to back without host
 * synchronisation; the call then synchronises ONCE (to verify the per-signal factorisation flags,
 * see DESIGN.md "optimistic chain") and returns with the results complete. */
int csmp_omp_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k,
                   double eps, int64_t *idx, double *val, int64_t *nnz, int out_loc);

/* fr(A, B[:,s], max_eps, min_delta, k) for s = 0..nsig-1 (src/forward.jl:44-54 in the caller's loop): same
 * conventions, pipelining and single synchronisation as csmp_omp_batch. */
int csmp_fr_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k,
                  double max_eps, double min_delta, int64_t *idx, double *val, int64_t *nnz, int out_loc);

/* mp(A, B[:,s], k) for s = 0..nsig-1 (src/matchingpursuit.jl:26-40 in the caller's loop), x starting from 0: the conventions of
 * csmp_omp_batch (B on host or device, idx / val: k x nsig with unused tails -1 / 0, nnz: nsig, outputs on host or device).  Every
 * signal takes k steps; atoms may repeat, so nnz[s] <= k.  Signal s's output is csmp_mp's, bit for bit: ascending atoms, the
 * increments of one atom added in step order, no entry for an atom whose increments were all exactly zero.  No factorisation is
 * kept, so k is bound neither by M nor by the append kernels' capacity.  Warm starts stay with csmp_mp.
 * Up to eight signals (Float32 dictionaries; four on Float64) share ONE pass over the dictionary per step, and two such groups run
 * side by side on two streams; with out_loc == CSMP_DEVICE the call only enqueues work (csmp_sync).  The signals go one after the
 * other through csmp_mp's own launches -- same results, no gain -- where the resident dictionary has no shared pass (columns
 * longer than the LDS holds, i.e. phased sweeps, and the internal dynamic-sweep measurement switch), with CSMP_OPT_SCREENED_SWEEP
 * on, with CSMP_OPT_PIPELINE 0, and for nsig == 1.  nsig == 0 returns CSMP_OK and touches nothing. */
int csmp_mp_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k, int64_t *idx,
                  double *val, int64_t *nnz, int out_loc);

/* somp(A, B, eps, k; p): simultaneous OMP (S-OMP: Tropp, Gilbert and Strauss 2006) for columns of B that share ONE support -- trials
 * of one experiment, frames of one scene, channels of one array.  omp's driver (src/matchingpursuit.jl:62-82) with the residual
 * matrix R in place of r: a step scores every atom by s_j = sum_l |<a_j, r_l>|^p, p = 1 or 2 (the correlations are the sweeps' bits,
 * added in column order), takes the arg-max (the lowest index among equals) under omp's guards -- the support smaller than
 * size(A,1) and than k, the atom not in it yet: a pick inside the support ends the solve --, appends that atom to ONE CGS2
 * factorisation (the append chain with its second Gram-Schmidt pass) and projects every residual off the new direction; from the
 * second step on the solve ends once ||R||_F < eps.  At the end R_fac X_S = Z is solved for all columns.  One column is omp.
 * B: ldB x nsig, column-major, host or device memory (b_loc).  Outputs in host or device memory (out_loc): idx (k), the support in
 * ascending order; val (ldval x nsig, ldval >= k), row i the coefficients of atom idx[i] in every column, entries that are exactly
 * zero included; order (k, may be NULL), the atoms in the order they were picked; resnorm (nsig, may be NULL), ||r_l|| of every
 * column.  Unused tails of idx and order are -1, of val 0.  nnz and passes (may be NULL) are HOST scalars: the size of the support
 * (the steps taken), and the passes over the dictionary that ran.  The call returns with the work done.
 * The residuals go through the shared pass of csmp_mp_batch in chunks of up to group_wide columns (8 on Float32 dictionaries, 4 on
 * Float64; csmp_tune group_max / group_wide apply): ceil(nsig / group_wide) passes a step, ONE append a step whatever nsig is.  Where
 * the resident dictionary has no shared pass (phased sweeps, the dynamic-sweep switch, a host-streamed dictionary) a step takes
 * one sweep per column: the same results.  CSMP_OPT_SCREENED_SWEEP is ignored: the sweeps are exact.  nsig is bounded by device
 * memory only, 8 (size(A,1) + size(A,2) + k) bytes a column.  The same bits on every run, for every chunking.
 * CSMP_EINVAL: NULL arguments, k < 1, nsig < 0, eps negative or NaN, p neither 1 nor 2, ldB < size(A,1), ldval < k, a bad b_dtype,
 * b_loc or out_loc.  CSMP_ERANGE: k > min(size(A)).  CSMP_ESTATE: no dictionary.  CSMP_ENOMEM: the columns' buffers could not be
 * allocated; everything is freed, the context stays usable.  nsig == 0: CSMP_OK, nothing is written. */
int csmp_somp(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k, double eps, int p,
              int64_t *idx, double *val, int64_t ldval, int64_t *nnz, int64_t *order, double *resnorm, int64_t *passes,
              int out_loc);

/* gomp(A, B[:,s], l, eps, k) for s = 0..nsig-1 (src/matchingpursuit.jl:116-139 in the caller's loop), 1 <= l <= k: the conventions
 * of csmp_omp_batch (idx / val: k x nsig).  TWO solves are in flight, one on the context's stream and one on an internal clone's,
 * out of phase: a signal's short stages (top-l selection, the l-column panel append) run under the other signal's dictionary
 * sweep.  Results are csmp_gomp's, signal by signal.  One synchronisation at the end. */
int csmp_gomp_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t l, int64_t k,
                    double eps, int64_t *idx, double *val, int64_t *nnz, int out_loc);

/* sp(A, B[:,s], k, delta; maxiter) for s = 0..nsig-1 (src/twostage.jl:87-101 in the caller's loop).  B: HOST matrix M x nsig
 * (ldB elements); idx / val: k x nsig host arrays (tail -1 / 0), nnz and iters (may be NULL): nsig.  Up to
 * CSMP_OPT_SOLVES_IN_FLIGHT solves run at once, each on its own context (this one and internal clones) and stream, all driven by
 * the CALLING thread: a Subspace Pursuit solve is two dictionary sweeps and a chain of short kernels with a handful of host
 * decisions (which atoms join, which leave, whether to go on); a solve whose pending device phase has not finished is skipped and
 * another one advanced, so one signal's chain runs under another's sweeps.  Signal s is solved by the very job csmp_sp runs:
 * identical results.  No threads are started; the ctx must not be used by another thread while the call runs. */
int csmp_sp_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int64_t k, double delta, int64_t maxiter,
                  int64_t *idx, double *val, int64_t *nnz, int64_t *iters);

/* The same contract, solved by the batched variant (BASELINE configs 3/4): the residual sweeps of
 * all signals become ONE MFMA GEMM per step (A' [r_1 .. r_B] on 16-bit images -- binary16 by default, bf16 or int8 by option --,
 * f32 accumulate) that only SCREENS: per signal the candidates whose screened value could still be the exact maximum are rescored in
 * Float64 from the f32/f64 master dictionary, and a certificate (exact best > an upper bound on the exact value of
 * every atom that was not rescored) guards every step: a signal that fails it once is re-solved by the exact path
 * before returning, so a certified result equals csmp_omp_batch's.  The error bound behind the certificate is
 * chosen by CSMP_OPT_BATCH_CERT (below).  Dictionaries of more than 8192 rows, and support capacities min(k, M) whose per-signal
 * vectors exceed the LDS (about 5000 columns at M = 4096), are solved by csmp_omp_batch's exact sweeps (same results;
 * the internal csmp_batch_screen_kernel then reports "none").  The per-signal state is two k x k Float64 factors: a batch
 * whose state does not fit the free HBM is solved in chunks of whole 256-signal tiles (csmp_batch_stats adds them up).  With out_loc == CSMP_DEVICE this call still
 * synchronises once (to read the per-signal certificates). */
int csmp_omp_batch_mfma(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k,
                        double eps, int64_t *idx, double *val, int64_t *nnz, int out_loc);
/* statistics of the last csmp_omp_batch_mfma call: signals, how many were re-solved exactly (and
 * why), and -- when profiling is enabled -- the number and total duration (ms) of screening GEMMs */
int csmp_batch_stats(csmp_ctx *ctx, int64_t *signals, int64_t *resolved_exactly, int64_t *uncertain, int64_t *illcond,
                     int64_t *screen_launches, double *screen_ms);
/* ------------------------------------------------------------------ options
 * The reference passes every behavioural choice as an argument (src/matchingpursuit.jl:88-91,145-148;
 * src/twostage.jl:87); those are arguments here too.  The choices that exist only on this side of the boundary are
 * per-context options ("Config / flags").  The library reads NO environment variable.  A clone
 * (csmp_clone) starts from its parent's values (the resident Gram matrix excepted: 8 N^2 bytes per context are asked for, not
 * inherited).  Unknown keys and out-of-range values: CSMP_EINVAL.  (Keys 5-8 of rounds 2-3 -- a test switch and three choices with
 * one sane value each -- are gone: the library takes the default they had.) */
#define CSMP_OPT_BATCH_CERT 1      /* certificate of csmp_omp_batch_mfma (and of the screened sweeps, CSMP_OPT_SCREENED_SWEEP).
                                      1 (default): rigorous -- a deterministic bound on the screen's error (unit roundoff of both
                                      operands' images, Float32 accumulation, key truncation) with the largest column norm: a
                                      passed certificate PROVES the pick; no residual, however constructed, can slip through
                                      (tests: test_batched_certificate_against_adversarial_residuals).
                                      0 (opt-in, UNSAFE): statistical -- 8 standard deviations of independent roundings + a
                                      coherent term; narrower windows (fewer rescored candidates, int8 operands allowed), holds
                                      for generic data, NOT a proof: a residual aligned with the rounding errors of a near-tied
                                      atom passes the certificate with the WRONG atom and nothing reports it (the library's own
                                      adversarial test constructs 24 such signals out of 24).  Not measured in the default bench
                                      line; use it only where a wrong pick on a crafted input is acceptable */
#define CSMP_OPT_BATCH_GRAM 2      /* 1: csmp_omp_batch_mfma keeps G = A'A resident (Float64, 8 N^2 bytes: 32 GiB at N = 65536;
                                      built on first use, 2 M N^2 / 2 flops on the Float64 matrix cores) and takes A_S'a from it
                                      instead of streaming the support's columns: half the append traffic.  0 (default) frees it */
#define CSMP_OPT_BATCH_WINDOW 3    /* capacity of the rescoring window, 1..128; 0 (default) = 64 statistical / 128 rigorous */
#define CSMP_OPT_PIPELINE 4        /* csmp_omp_batch / csmp_fr_batch: 1 (default) three signals in flight, 0 one at a time */
#define CSMP_OPT_SOLVES_IN_FLIGHT 9 /* csmp_sp_batch: solves in flight (contexts on their own streams, one host thread), 1..4, default 3 */
#define CSMP_OPT_SCREENED_SWEEP 10 /* csmp_mp, csmp_omp(_batch), csmp_gomp(_batch) (l <= 16), csmp_sp(_batch) and csmp_ompr (k <= 4096): 0 (default) every sweep
                                      reads the f32/f64 dictionary (exact, 4 / 8 bytes per element).  1 / 3 / 2: the sweep reads an IMAGE of the
                                      dictionary and only SCREENS -- the best candidates are rescored in Float64 from the master dictionary under the
                                      batched variant's certificate (CSMP_OPT_BATCH_CERT; gomp: the whole top-l set and its order are certified; sp:
                                      every acquisition's top-k SET), and a solve (sp: an acquisition) with an uncertified step is repeated with the
                                      exact sweep before the call returns: results are those of option 0.
                                      3: the binary16 image (2 bytes per element under one power-of-two scale, f32 accumulate): with the rigorous
                                      certificate (the default) its bound is 2^-11 |a||r| -- narrow enough to certify (nearly) every step on the
                                      benchmark dictionaries: a PROVABLY exact solve at half the bytes per atom.
                                      1: the bf16 image (2 bytes, bound 2^-8 |a||r|: under the rigorous certificate most solves fall back; useful with
                                      CSMP_OPT_BATCH_CERT = 0).  2: the int8 image where the dictionary is flat (max|A| <= 8 rms of its entries;
                                      otherwise the bf16 image): 1 byte per element under one step max|A|/127, the residual quantised per sweep,
                                      exact integer accumulation; statistical certificate only.
                                      Costs the image (2 Mk N or Mk N bytes) beside the dictionary.  Default off: the headline path stays the
                                      exact sweep ("Screened single-signal sweep"). */
#define CSMP_OPT_BATCH_SCREEN 11   /* csmp_omp_batch_mfma: operands of the screening GEMM.
                                      3 (default): binary16 images (v_mfma_f32_16x16x32_f16; the dictionary and every residual under
                                      exact power-of-two scales): the same rate and bytes as bf16 with eleven significand bits --
                                      the rigorous bound is 2^-10 |a||r| instead of 2^-7 |a||r|, windows as narrow as bf16's
                                      statistical ones.  0: bf16 images (v_mfma_f32_16x16x32_bf16), the form of rounds 1-3.
                                      1: int8 images -- the dictionary under one step max|A|/127, every residual under its own -- on
                                      v_mfma_i32_16x16x64_i8 (half the K-loop, exact integer accumulation); 2: int8 where the
                                      dictionary is flat (max|A| <= 8 x the root mean square of its entries), binary16 otherwise.
                                      The int8 screen has a statistical certificate only: it runs under CSMP_OPT_BATCH_CERT = 0;
                                      under the rigorous certificate 1 and 2 run binary16.  Only the image in use is built
                                      (2 M N bytes; int8: M N). */
int csmp_set_option(csmp_ctx *ctx, int key, int64_t value);
int csmp_get_option(csmp_ctx *ctx, int key, int64_t *value);

/* screened solves (CSMP_OPT_SCREENED_SWEEP) made through this ctx and how many of them had to be repeated with the exact sweep
 * (a step whose certificate failed); reset != 0 zeroes both counters.  Measurement / tests. */
int csmp_screened_stats(csmp_ctx *ctx, int64_t *solves, int64_t *fallbacks, int reset);

/* ------------------------------------------------------------------ step-level API
 * Mirrors the Update functors: P = OMP(A,b,k) / MP(A,b) / GOMP(A,b,l) / FR(A,b) then update!(P,x)
 * (src/CompressedSensing.jl:22-23; src/matchingpursuit.jl:26,62,116; src/forward.jl:88-95).  The solver state
 * (residual, on-device QR, support) lives in the ctx. */
int csmp_solver_begin(csmp_ctx *ctx, int algo, const void *b, int b_dtype, int64_t kcap,
                      const int64_t *idx0, const double *val0, int64_t nnz0);
/* CSMP_ALGO_SP / CSMP_ALGO_OMPR: kcap is the k of SP(A,b,k) (2k <= M or CSMP_ERANGE: src/twostage.jl:55) / OMPR(A,b,k).  The
 * solver owns x.  SP: (idx0, val0) is the x the host would hand to update! -- any vector of at most 2k atoms; its values count (the
 * acquisition starts from residual!(P, x), :68).  OMPR: x starts empty (nnz0 = 0): its factorisation does (:124-129).
 * one update!: MP/OMP ignore l; GOMP adds the l best atoms; SP / OMPR: update!(P, x) (:75-83 / :134-180, eta = 1), which requires
 * nnz(x) == k -- otherwise CSMP_ESTATE with the reference's message "nnz(x) = .. != .. = k" (:76, :135) */
int csmp_solver_step(csmp_ctx *ctx, int64_t l);
/* SP: sp_acquisition!(P, x, k) (src/twostage.jl:67-72) -- the k atoms best correlated with the residual of x join it, least squares
 * on the union.  OMPR / OMP / GOMP: oblivious_acquisition!(P, x, k) (src/matchingpursuit.jl:207-216) -- the same with the
 * updatable QR (OMPR: on the empty x, k = the k of OMPR(A,b,k): how ompr fills the support, src/twostage.jl:190). */
int csmp_solver_acquire(csmp_ctx *ctx, int64_t k);
/* dropindex!(x, AiQR, i) (src/util.jl:137-161): atom leaves the support of an OMP/GOMP solver -- Givens
 * down-date of the on-device QR (remove_column!), residual and coefficients follow.  No-op if absent.
 * Any capacity: up to 1023 columns one workgroup walks R, up to 4095 the rotations come from the explicit inverse, beyond that the
 * factorisation is rebuilt from the columns that stay. */
int csmp_solver_remove(csmp_ctx *ctx, int64_t atom);
/* current x (sorted), ||b - A x||_2, selection order, stop reason.  Any pointer may be NULL. */
int csmp_solver_state(csmp_ctx *ctx, int64_t *idx, double *val, int64_t *nnz, double *resnorm,
                      int64_t *order, int *stop);

/* ------------------------------------------------------------------ one signal, columns sharded over GPUs
 * SURVEY.md section 8e/8f-4 (not in the reference: its omp takes one b and one A, src/matchingpursuit.jl:73-82).
 * Each rank's ctx holds columns [col_offset, col_offset + N) of the global dictionary and a full replica of
 * the solver state.  A solve: csmp_solver_begin(ctx, CSMP_ALGO_OMP, b, ...) on every rank; then k times
 *     csmp_shard_sweep (argmaxinner!(P), :181-185, over the local columns; t > 0: the driver's residual test :79)
 *     -> the caller's all_gather of ONE record per rank (csmp_shard_record_bytes each, device memory)
 *     -> csmp_shard_append (global arg-max, ties to the lower global index; update!'s guards :63,66;
 *        add_column! and the residual update on the winner's column, which travels inside its record);
 * then csmp_solver_state (indices are global; identical on every rank).  Nothing synchronises with the host
 * between those calls: with csmp_set_stream they are stream-ordered with the collective. */
int csmp_shard_config(csmp_ctx *ctx, int64_t col_offset);
int64_t csmp_shard_record_bytes(const csmp_ctx *ctx);
int csmp_shard_sweep(csmp_ctx *ctx, double eps, int check_eps, void *rec_dev);
int csmp_shard_append(csmp_ctx *ctx, const void *recs_dev, int nrec);

/* ------------------------------------------------------------------ many signals sharded over GPUs
 * SURVEY.md section 8e, BASELINE configs[3]: signals are independent given A (the loop a caller of the reference writes around
 * omp, src/matchingpursuit.jl:73-82), so rank r -- ONE PROCESS PER GPU, A replicated -- solves the contiguous block
 * [lo, hi) = csmp_shard_range(nsig, r, world) and ONE collective moves the results: per signal a row of 2k + 1 Float64
 * [idx_0..idx_{k-1} | val_0..val_{k-1} | nnz].
 *
 * csmp_omp_sharded does all of it inside the library: the block's solves (method 0: csmp_omp_batch, 1: csmp_omp_batch_mfma),
 * the packing on the device, ONE ncclAllGather over xGMI on the context's stream (device memory to device memory), and the
 * unpacking into global signal order.  B: THIS RANK'S block, M x (hi - lo) column-major (ldB elements), host or device (b_loc);
 * idx / val (k x nsig, tail -1 / 0) and nnz (nsig): ALL signals, on every rank, host or device (out_loc).  nsig is the
 * global count and must be the same on every rank; the call is collective.
 * The communicator: rank 0 calls csmp_comm_id (ncclGetUniqueId, CSMP_COMM_ID_BYTES of host memory), the host passes those
 * bytes to the other ranks by whatever started them (a file, a socket, Julia's Distributed, torch.distributed's store), and
 * every rank calls csmp_comm_init(ctx, id, rank, world) (ncclCommInitRank on the ctx's GPU; collective).  The host language
 * needs no collective library of its own.  RCCL is bound lazily (librccl.so.1) by these calls only.  csmp_destroy frees the
 * communicator; csmp_comm_free does it earlier. */
#define CSMP_COMM_ID_BYTES 128
int csmp_comm_id(void *id);
int csmp_comm_init(csmp_ctx *ctx, const void *id, int rank, int world);
int csmp_comm_free(csmp_ctx *ctx);
int csmp_omp_sharded(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k, double eps,
                     int method, int64_t *idx, double *val, int64_t *nnz, int out_loc);
/* The device-side halves of that exchange on their own, stream-ordered on the ctx (device pointers throughout): rows of 2k + 1 Float64
 * from a block's results (idx, val: k x nloc; nnz: nloc; `rows` >= nloc rows are written, the surplus zeroed -- every rank packs
 * ceil(nsig / world) rows so that the blocks gather), and the gathered world x rows x (2k + 1) array into idx / val (k x nsig) and nnz
 * (nsig) in global signal order.  For a host that keeps results on the device under a collective of its own. */
int csmp_pack_block_device(csmp_ctx *ctx, const int64_t *idx, const double *val, const int64_t *nnz, int64_t k, int64_t nloc,
                           int64_t rows, double *packed);
int csmp_unpack_gathered_device(csmp_ctx *ctx, const double *gathered, int64_t k, int64_t nsig, int world, int64_t *idx, double *val,
                                int64_t *nnz);
/* The same wire layout for hosts that bring their own collective (torch.distributed all_gather in sharded.py's gloo tests and
 * single-signal solver families; MPI): host memory, no ctx. */
int csmp_shard_range(int64_t nsig, int rank, int world, int64_t *lo, int64_t *hi);
int csmp_pack_results(const int64_t *idx, const double *val, const int64_t *nnz, int64_t k, int64_t nsig, double *packed);
int csmp_unpack_results(const double *packed, int64_t k, int64_t nsig, int64_t *idx, double *val, int64_t *nnz);

/* ------------------------------------------------------------------ l1-regularised least squares
 * ista(A,b,w,x; maxiter, stepsize): src/basispursuit.jl:164-183, and FISTA (Beck-Teboulle) on the same objective -- the
 * reference's own fista (:186-204) does not run.  Convention, the reference's exactly: the objective is
 * ||b - A x||^2 + sum_j w_j |x_j|, one iteration is  g = A'(b - A y);  x+ = shrinkage(y + 2 stepsize g, w stepsize)  with
 * shrinkage(u, a) = sign(u) max(|u| - a, 0) (:144), and there is no stopping rule: exactly maxiter iterations.  accel = 0 (ISTA):
 * y = x.  accel = 1 (FISTA): t_1 = 1, t+ = (1 + sqrt(1 + 4 t^2)) / 2, y+ = x+ + ((t - 1) / t+) (x+ - x), y_1 = x_0.
 * w, nw: nw = 1 is one weight lambda for every atom (ista(A,b,lambda::Real,...), :164), nw = size(A,2) one weight per atom;
 * anything else: CSMP_EDIM.  w is a host array; the weights are non-negative and finite.
 * idx0 / val0 / nnz0: the warm start x_0 (indices 0-based, in any order); nnz0 = 0: x_0 = 0.  maxiter = 0 returns the warm start.
 * x: the DENSE result, Float64[size(A,2)]; an exact zero is a structural zero of the reference's result (dropzeros!, :180).
 * x_loc says where x AND b live: CSMP_HOST, or CSMP_DEVICE (both device pointers; the call still returns with the work done).
 * resnorm (may be NULL): ||b - A x||_2 of the returned x.
 * Arithmetic: Float64 on the exactly promoted dictionary values; x, y and the residual are Float64.  The same call returns the
 * same bits every time.  CSMP_EINVAL: maxiter < 0, a stepsize that is not finite and positive, a negative or non-finite weight,
 * a warm-start index out of range or repeated.  CSMP_ESTATE: no dictionary -- and a host-streamed dictionary
 * (CSMP_HOST_STREAMED), which this entry does not serve: every iteration reads the dictionary up to twice. */
int csmp_ista(csmp_ctx *ctx, const void *b, int b_dtype, const double *w, int64_t nw,
              const int64_t *idx0, const double *val0, int64_t nnz0,
              int64_t maxiter, double stepsize, int accel,
              double *x, int x_loc, double *resnorm);

/* ista_batch: csmp_ista for every column of B on shared launches.  The pass over the dictionary for c = A'r is the same for every
 * signal: a group of up to eight signals (the groups of csmp_mp_batch and csmp_bp_batch: csmp_tune group_max / group_wide apply) takes
 * its iterations together, four launches a step however many members it has -- one launch each for the residual's two steps
 * (r = b - A y over every member's own list), one shared pass over A, one launch for the update.  Every signal runs exactly maxiter
 * iterations (there is no stopping rule), so the signals are taken in ascending order, a group at a time, and nothing waits for the
 * device between a group's first launch and its results.
 * Contract: column s of X and resnorm[s] are those of csmp_ista(ctx, B[:, s], w_s, x0_s, maxiter, stepsize, accel, ...), BIT FOR BIT,
 * whatever nsig and the group sizes are.
 * B: size(A,1) x nsig, column-major, leading dimension ldB >= size(A,1), CSMP_F32 or CSMP_F64, on the host or the device (b_loc).
 * X: size(A,2) x nsig doubles, leading dimension ldX >= size(A,2), on the host or the device (x_loc); column s receives the dense
 * result of signal s, rows beyond size(A,2) are not touched.
 * w, nw, ldw: a host array; nw = 1 (one weight for every atom) or size(A,2) (one per atom), as csmp_ista.  ldw = 0: the nw weights
 * are shared by all signals.  ldw >= nw: w is nw x nsig with leading dimension ldw and column s belongs to signal s -- one lambda
 * per signal (nw = 1, ldw = 1) or one weight vector per signal: a regularisation path is the same b in every column.
 * X0, ldX0: NULL starts every signal from zero.  Otherwise a dense size(A,2) x nsig matrix of doubles where X lives (x_loc), leading
 * dimension ldX0 >= size(A,2): column s is the warm start of signal s, the dense vector csmp_ista builds from idx0 / val0.
 * X0 == X with ldX0 == ldX continues a run in place; any other overlap of X0 and X is the caller's error and is not detected.
 * resnorm: a host array of nsig entries, or NULL.  maxiter = 0 returns the warm start (or zeros) and resnorm[s] = ||b_s - A x0_s||,
 * which is ||b_s|| for a zero start.  nsig = 0: CSMP_OK, nothing is touched.
 * A dictionary without a shared pass (csmp_sweep_config: group 0), CSMP_OPT_SCREENED_SWEEP switched on and nsig = 1 take csmp_ista's
 * own launches signal by signal: the same outputs.
 * Memory beside csmp_ista's, kept by the context until csmp_set_dictionary: per member of a group 3 size(A,2) + the list
 * (1.5 size(A,2)) doubles and the residual's partials -- 18 MiB + 128 MiB for eight members at 4096 x 65536.
 * CSMP_EINVAL: nsig < 0, null pointers, a dtype / location that is neither, accel other than 0 or 1, maxiter < 0, a stepsize that is
 * not positive and finite, a negative or non-finite weight (in any column), ldw < 0 or 0 < ldw < nw.  CSMP_EDIM: ldB < size(A,1),
 * ldX < size(A,2), ldX0 < size(A,2), nw other than 1 or size(A,2).  CSMP_ESTATE: no dictionary, or a host-streamed one (as csmp_ista).
 * CSMP_ENOMEM: a buffer could not be allocated; no partial buffers are left behind and the context stays usable.  Everything is
 * validated before any device work.  A refused call writes nothing. */
int csmp_ista_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                    const double *w, int64_t nw, int64_t ldw, const double *X0, int64_t ldX0,
                    int64_t maxiter, double stepsize, int accel, double *X, int64_t ldX, int x_loc,
                    double *resnorm);

/* ista_joint: ISTA / FISTA on the row-sparse (l2,1, "group lasso over rows", MMV) objective
 *     ||B - A X||_F^2 + sum_j w_j ||X[j, :]||_2
 * for columns of B that share ONE support -- the convex counterpart of csmp_somp.  One iteration, alpha = stepsize, t_j = w_j alpha:
 *     R = B - A Y;  C = A'R;  U = Y + 2 alpha C;  n_j = sqrt(sum_l U[j,l]^2), added in column order l = 0, 1, ...;
 *     X+[j,:] = 0 exactly where !(n_j > t_j), else (1 - t_j / n_j) U[j,:].
 * accel = 0 (ISTA): Y+ = X+.  accel = 1 (FISTA): Y+ = X+ + beta (X+ - X) with csmp_ista's recurrence, t_1 = 1, Y_1 = X_0.  Exactly
 * maxiter iterations, no stopping rule, nothing read back in between; maxiter = 0 returns the warm start.
 * B: size(A,1) x nsig, column-major, leading dimension ldB >= size(A,1), CSMP_F32 or CSMP_F64, on the host or the device (b_loc).
 * w, nw: a host array; nw = 1 (one lambda) or size(A,2) (one weight per ROW of X); non-negative and finite.
 * X0, ldX0: NULL starts from zero.  Otherwise a dense size(A,2) x nsig matrix of doubles where X lives (x_loc), ldX0 >= size(A,2).
 * X0 == X with ldX0 == ldX continues a run in place; any other overlap of X0 and X is the caller's error and is not detected.
 * X: size(A,2) x nsig doubles, leading dimension ldX >= size(A,2), on the host or the device (x_loc); rows beyond size(A,2) are not
 * touched.  nrows (may be NULL): the number of non-zero rows of X.  resnorm (may be NULL): a host array, ||b_l - A x_l||_2 per column
 * (||b_l|| for maxiter = 0 without a warm start).  nsig = 0: CSMP_OK, nothing is touched.
 * One column is csmp_ista: nsig = 1 takes csmp_ista's own launches and returns its bits.  More columns: the passes for C are
 * csmp_somp's (chunks of up to group_wide columns on the shared pass, csmp_tune group_max / group_wide apply; one sweep per column for
 * a dictionary without a shared pass; CSMP_OPT_SCREENED_SWEEP is ignored), and the residual reads every live column of A ONCE for a
 * chunk of up to eight columns of B, because there is one list for all of them.
 * Arithmetic: Float64 on the exactly promoted dictionary values, no floating-point atomics, every sum in a fixed order: the same call
 * returns the same bits every time, whatever the chunks are, and equal columns of B give equal columns of X.
 * Memory: the call's own, released when it returns -- 8 (2 size(A,1) + 4 size(A,2)) bytes a column (size(A,1) rounded up to 256 rows)
 * and one chunk's partial sums of the residual (128 MiB at 4096 x 65536); nsig is bounded by memory only.
 * CSMP_EINVAL: nsig < 0, null pointers, a dtype / location that is neither, accel other than 0 or 1, maxiter < 0, a stepsize that is
 * not positive and finite, a negative or non-finite weight.  CSMP_EDIM: ldB < size(A,1), ldX < size(A,2), ldX0 < size(A,2), nw other
 * than 1 or size(A,2).  CSMP_ERANGE: nsig > 2^22.  CSMP_ESTATE: no dictionary, or a host-streamed one (as csmp_ista).  CSMP_ENOMEM: a
 * buffer could not be allocated; no partial buffers are left behind and the context stays usable.  Everything is validated before
 * any device work.  A refused call writes nothing. */
int csmp_ista_joint(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                    const double *w, int64_t nw, const double *X0, int64_t ldX0,
                    int64_t maxiter, double stepsize, int accel,
                    double *X, int64_t ldX, int x_loc, int64_t *nrows, double *resnorm);

/* ------------------------------------------------------------------ reweighted l1
 * candes_weights! / ard_weights! / basispursuit_reweighting: src/basispursuit.jl:18-74 (bp_candes, bp_ard; bpd_candes, bpd_ard :102-124),
 * with ista / fista as the inner solver (the reference's own inner solvers, bp and bpd, are csmp_bp and csmp_bpd below: neither needs
 * an LP or SOCP solver).
 *
 * ard_weights!(w, A, x, eps, iter) (:49-65): `iter` times over,  d = |x| ./ w;  K = eps I + A diag(d) A';
 * w_j = sqrt(max(a_j' K^-1 a_j, 0)) for every atom.  x, w_in, w_out: N doubles each, all three in host memory (loc = CSMP_HOST) or all
 * three in device memory (CSMP_DEVICE; the call still returns with the work done); w_out may be w_in.  Only the support S of x
 * enters K: with k = |S|, G = A_S'A_S and L L' = eps diag(w_S ./ |x_S|) + G,  a_j' K^-1 a_j = (|a_j|^2 - |L^-1 A_S' a_j|^2) / eps;
 * k = 0 gives w_j = |a_j| / sqrt(eps).  Float64 on the exactly promoted dictionary values, every sum in a fixed order: the same call
 * returns the same bits every time.
 * CSMP_EINVAL: a null pointer, eps that is not positive and finite, iter < 1, a weight that is zero (the reference: "weights cannot
 * be zero", :50-52), negative or not finite, an x that is not finite.  CSMP_ERANGE: nnz(x) > min(M, CSMP_ARD_KMAX) -- a basic
 * solution of bp has at most M non-zeros.  CSMP_ESTATE: no dictionary, or a host-streamed one (as csmp_ista).  CSMP_ENOMEM: a buffer
 * could not be allocated; nothing of it is left behind, and the next call starts afresh. */
#define CSMP_ARD_KMAX 1024
int csmp_ard_weights(csmp_ctx *ctx, const double *x, const double *w_in, double eps, int64_t iter, double *w_out, int loc);

/* basispursuit_reweighting (:18-31) on  ||b - A x||^2 + lambda sum_j w_j |x_j|:  x = solve(w = 1);  then for i = 2 .. outer_maxiter:
 * w from x -- scheme CSMP_REWEIGHT_CANDES: w_j = 1 / (|x_j| + eps) (:33-39); CSMP_REWEIGHT_ARD: ard_weights!(w, A, x, eps, ard_iter)
 * on the w of the previous outer iteration, from ones (ard_function, :67) --;  xs = solve(lambda w), WARM-STARTED from x (the
 * reference's bp has no warm start; ista has, and a cold start would spend the inner iterations on getting back to x);
 * norm(xs - x) < min_decrease: return xs;  else x = xs.  solve = csmp_ista with the caller's maxiter, stepsize and accel.
 * outer_maxiter = 1 is the plain csmp_ista call with the one weight lambda, bit for bit.
 * x: the dense result, N doubles; x_loc says where b, x and w_out live (as csmp_ista).  w_out (may be NULL): the last weights (ones
 * when no reweighting took place).  outer_done (may be NULL): the number of solves done, 1 .. outer_maxiter.  resnorm (may be NULL):
 * ||b - A x||_2 of the returned x.  x and w stay on the device between the solves; the host reads one step norm per outer iteration.
 * CSMP_EINVAL: a scheme that is neither, eps not positive and finite, ard_iter < 1, outer_maxiter < 1, a negative or NaN
 * min_decrease, a negative or non-finite lambda, weights that come out NaN or Inf (:36-38), and csmp_ista's.  CSMP_ERANGE: an
 * iterate with more than CSMP_ARD_KMAX non-zeros under CSMP_REWEIGHT_ARD (an iterate of ista is no basic solution and may have more
 * than M: the k x k form holds for any k, eps diag(w_S ./ |x_S|) keeps it positive definite).  CSMP_ESTATE, CSMP_ENOMEM: as above. */
#define CSMP_REWEIGHT_CANDES 0
#define CSMP_REWEIGHT_ARD 1
int csmp_ista_reweighted(csmp_ctx *ctx, const void *b, int b_dtype, double lambda, int scheme, double eps, int64_t ard_iter,
                         int64_t outer_maxiter, double min_decrease, int64_t maxiter, double stepsize, int accel,
                         double *x, int x_loc, double *w_out, int64_t *outer_done, double *resnorm);

/* ------------------------------------------------------------------ basis pursuit
 * basispursuit(A, b[, w]) = bp: src/basispursuit.jl:1-16.  min sum_j w_j |x_j| subject to A x = b, by ADMM on the split x = z -- no
 * LP solver: with G = A A' = R'R (formed and factorised ONCE per dictionary, kept by the context until csmp_set_dictionary), the scaled
 * dual u, the penalty rho, shrink(t, a) = sign(t) max(|t| - a, 0), and p = A z, q = A u carried as M-vectors, one iteration is
 *     e = p - q - b;   y = G^-1 e;   c = A' y;   t = z - c;   z+ = shrink(t, w / rho);   u+ = t - z+;
 *     r = b - A z+;   p+ = b - r;   q+ = p - G y - p+
 * -- one pass over A, one over the non-zeros of z+, three M x M matrix-vector products.  Start: z = u = 0.  Every check_every
 * iterations the host reads ||u+ - u|| (primal residual) and rho ||z+ - z|| (dual residual) and stops when both are < tol; reaching
 * maxiter is not an error.  The result is z: exactly sparse; the feasible but dense x of the iteration is not returned.
 * w, nw: nw = 1 is one weight for every atom, nw = size(A,2) one weight per atom; anything else: CSMP_EDIM.  w is a host array; the
 * weights are non-negative and finite.
 * x: the DENSE result, Float64[size(A,2)]; x_loc says where x AND b live: CSMP_HOST, or CSMP_DEVICE (the call still returns with the
 * work done).  iterations, resnorm (||b - A z||_2 of the returned z), flags: may be NULL.  flags: CSMP_BP_CONVERGED -- both residuals
 * passed tol at a check; CSMP_BP_FACTORED -- this call formed and factorised A A' (the first on a dictionary).
 * Memory: G, M x M doubles, and the augmented matrix of the factorisation, (2 M)^2 doubles with M rounded up to 64 -- 128 MiB + 512 MiB
 * at M = 4096.
 * CSMP_EINVAL: null pointers, a b_dtype / x_loc that is neither, rho or tol not positive and finite, maxiter < 0, check_every < 1, a
 * negative or non-finite weight, and "bp: A A' is not positive definite to working precision" (A without full row rank: a pivot of the
 * factorisation below 4 M eps of its diagonal entry).  CSMP_EDIM: size(A,1) > size(A,2).  CSMP_ERANGE: more than 2^19 rows.
 * CSMP_ESTATE: no dictionary -- and a host-streamed dictionary (CSMP_HOST_STREAMED), as csmp_ista.  CSMP_ENOMEM: a buffer could not be
 * allocated; nothing of G or its factor is left behind, and the next call starts afresh. */
#define CSMP_BP_CONVERGED 1
#define CSMP_BP_FACTORED 2
int csmp_bp(csmp_ctx *ctx, const void *b, int b_dtype, const double *w, int64_t nw,
            double rho, int64_t maxiter, double tol, int64_t check_every,
            double *x, int x_loc, int64_t *iterations, double *resnorm, int *flags);

/* bp_batch: csmp_bp for every column of B, the signals in lockstep on shared launches.  Everything an iteration of csmp_bp reads in
 * bulk -- the dictionary, R^-1, R^-T, G -- is the same for every signal: a group of up to eight signals (the groups of csmp_mp_batch:
 * csmp_tune group_max / group_wide apply) takes its iterations together, eight launches a step however many are live -- three M x M
 * products with one read of each matrix for all right-hand sides, one shared pass over A, one launch each for the update, the
 * residual's two steps and the M-vector step.  Solves end at different iterations: a finished signal's slot is refilled with the next
 * column at the following multiple of check_every.
 * Contract: column s of X, iterations[s], resnorm[s] and the CSMP_BP_CONVERGED bit of flags[s] are those of
 * csmp_bp(ctx, B[:, s], ...) with the same w, rho, maxiter, tol, check_every, BIT FOR BIT, whatever nsig and the group sizes are.
 * CSMP_BP_FACTORED is set in flags[0] only, and only when this call formed the factor (what a loop over csmp_bp would report).
 * B: size(A,1) x nsig, column-major, leading dimension ldB >= size(A,1), CSMP_F32 or CSMP_F64, on the host or the device (b_loc).
 * X: size(A,2) x nsig doubles, leading dimension ldX >= size(A,2), on the host or the device (x_loc); column s receives the exactly
 * sparse z of signal s, rows beyond size(A,2) are not touched.  w, nw: csmp_bp's, a host array, shared by all signals.  iterations,
 * resnorm, flags: host arrays of nsig entries, each may be NULL.  maxiter = 0: every column zero, iterations 0, resnorm ||b||.
 * A dictionary without a shared pass (csmp_sweep_config: group 0), CSMP_OPT_SCREENED_SWEEP switched on and nsig = 1 take csmp_bp's
 * own solve signal by signal: the same outputs.
 * Memory beside csmp_bp's, kept by the context until csmp_set_dictionary: per member of a group 2 size(A,2) + the list (1.5 size(A,2))
 * doubles and the residual's partials -- 8 MiB + 128 MiB for eight members at 4096 x 65536.
 * CSMP_EDIM: ldB < size(A,1), ldX < size(A,2), a w of another length, size(A,1) > size(A,2).  CSMP_EINVAL: nsig < 0, null pointers, a
 * dtype / location that is neither, csmp_bp's knobs and weights, A A' not positive definite.  nsig = 0: CSMP_OK, nothing is touched.
 * CSMP_ERANGE, CSMP_ESTATE: csmp_bp's.  CSMP_ENOMEM: a buffer could not be allocated; no partial buffers are left behind and the
 * context stays usable. */
int csmp_bp_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                  const double *w, int64_t nw, double rho, int64_t maxiter, double tol, int64_t check_every,
                  double *X, int64_t ldX, int x_loc, int64_t *iterations, double *resnorm, int *flags);

/* bp_joint: row-sparse basis pursuit (the l2,1 "MMV" programme every joint recovery guarantee is stated for)
 *     min sum_j w_j ||X[j, :]||_2   subject to   A X = B
 * for columns of B that share ONE support -- csmp_bp with matrices in place of vectors; the equality-constrained companion of
 * csmp_ista_joint and the convex counterpart of csmp_somp.  No lambda, no step size.  With Z, U of size(A,2) x nsig, P = A Z, Q = A U, E,
 * Y of size(A,1) x nsig, t_j = w_j / rho, one iteration is
 *     E = P - Q - B;   Y = G^-1 E  (V = R^-T E, Y = R^-1 V);   C = A' Y;   T = Z - C;
 *     n_j = sqrt(sum_l T[j,l]^2), added by fma in column order l = 0, 1, ...;
 *     Z+[j,:] = 0 exactly where !(n_j > t_j), else (1 - t_j / n_j) T[j,:];   U+ = T - Z+;
 *     R = B - A Z+;   P+ = B - R;   Q+ = P - G Y - P+
 * Start: Z = U = 0.  Every check_every iterations the host reads ||U+ - U||_F and rho ||Z+ - Z||_F and stops when both are < tol: ONE
 * rule for all columns, so there is one iterations and one converged; reaching maxiter is not an error.  The result is Z: exactly
 * row-sparse, every column with the same non-zero rows.
 * B: size(A,1) x nsig, column-major, leading dimension ldB >= size(A,1), CSMP_F32 or CSMP_F64, on the host or the device (b_loc).
 * w, nw: a host array; nw = 1 (one weight) or size(A,2) (one weight per ROW of X); non-negative and finite.
 * X: size(A,2) x nsig doubles, leading dimension ldX >= size(A,2), on the host or the device (x_loc); rows beyond size(A,2) are not
 * touched.  iterations, nrows (the number of non-zero rows of X), flags (CSMP_BP_CONVERGED, CSMP_BP_FACTORED as csmp_bp_batch's
 * flags[0]): one number each, may be NULL.  resnorm (may be NULL): a host array of nsig entries, ||b_l - A z_l||_2 from the last R.
 * nsig = 0: CSMP_OK, nothing is touched.  maxiter = 0: X = 0, iterations 0, not converged, resnorm ||b_l||.
 * One column is csmp_bp: nsig = 1 takes csmp_bp's own solve and returns its bits.  More columns: the three M x M products read R^-1,
 * R^-T and G once per chunk of up to eight columns; the passes for C are csmp_somp's (chunks of up to group_wide columns on the shared
 * pass, csmp_tune group_max / group_wide apply; one sweep per column for a dictionary without a shared pass;
 * CSMP_OPT_SCREENED_SWEEP is ignored); the residual is csmp_ista_joint's, one read of every live column of A per chunk of up to
 * eight columns of B.
 * Arithmetic: Float64 on the exactly promoted dictionary values, no floating-point atomics, every sum in a fixed order: the same call
 * returns the same bits every time, whatever the chunks are, and equal columns of B give equal columns of X.  With zero weights
 * nothing is shrunk and column s runs csmp_bp(B[:, s], w = 0)'s arithmetic bit for bit.
 * Memory: the factor of A A' is csmp_bp's, kept by the context until csmp_set_dictionary.  The columns live in the call's own arrays,
 * all allocated or none, released when it returns -- 8 (8 size(A,1) + 4 size(A,2)) bytes a column (size(A,1) rounded up to 256 rows)
 * and one chunk's partial sums of the residual (128 MiB at 4096 x 65536); nsig is bounded by memory only.
 * CSMP_EINVAL: nsig < 0, null pointers, a dtype / location that is neither, rho or tol not positive and finite, maxiter < 0,
 * check_every < 1, a negative or non-finite weight, A A' not positive definite.  CSMP_EDIM: ldB < size(A,1), ldX < size(A,2), nw other
 * than 1 or size(A,2), size(A,1) > size(A,2).  CSMP_ERANGE: nsig > 2^22, more than 2^19 rows.  CSMP_ESTATE: no dictionary, or a
 * host-streamed one (as csmp_bp).  CSMP_ENOMEM: a buffer could not be allocated; no partial buffers are left behind and the context
 * stays usable.  Everything is validated before any device work.  A refused call writes nothing. */
int csmp_bp_joint(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                  const double *w, int64_t nw, double rho, int64_t maxiter, double tol, int64_t check_every,
                  double *X, int64_t ldX, int x_loc, int64_t *iterations, int64_t *nrows, double *resnorm, int *flags);

/* bp_candes / bp_ard: basispursuit_reweighting (:18-31) with csmp_bp's solve:  x = solve(w = 1);  then for i = 2 .. outer_maxiter:  w from x
 * (scheme, eps, ard_iter: as csmp_ista_reweighted; CSMP_REWEIGHT_ARD takes supports of up to min(size(A,1), CSMP_ARD_KMAX) atoms);
 * xs = solve(w), WARM-STARTED from the z, u, p, q of the previous solve;  norm(xs - x) < min_decrease: return xs;  else x = xs.
 * rho, maxiter, tol, check_every: csmp_bp's, for every solve.  x, x_loc, w_out, outer_done, resnorm: as csmp_ista_reweighted.
 * Errors: csmp_bp's and csmp_ista_reweighted's (CSMP_ERANGE: an iterate with more non-zeros than CSMP_REWEIGHT_ARD takes). */
int csmp_bp_reweighted(csmp_ctx *ctx, const void *b, int b_dtype, int scheme, double eps, int64_t ard_iter,
                       int64_t outer_maxiter, double min_decrease, double rho, int64_t maxiter, double tol, int64_t check_every,
                       double *x, int x_loc, double *w_out, int64_t *outer_done, double *resnorm);

/* ------------------------------------------------------------------ basis pursuit denoising
 * basis_pursuit_denoising(A, b, delta[, w]) = bpd: src/basispursuit.jl:76-100.  min sum_j w_j |x_j| subject to ||A x - b||_2 <= delta,
 * the form for data that carry noise -- no SOCP solver: graph-form ADMM.  Block one is (x, s) on the subspace s = A x, block two (z, v)
 * with sum w|z| + the indicator of ||v - b|| <= delta; scaled duals u (of x = z) and lam (of s = v), penalty rho.  With
 * K = I + A A' = R'R (formed and factorised ONCE per dictionary, kept by the context until csmp_set_dictionary; A A' itself is a
 * temporary), shrink(t, a) = sign(t) max(|t| - a, 0), and p = A z, q = A u carried as M-vectors, one iteration is
 *     e = v - lam - p + q;   y = K^-1 e;   c = A' y;   t = z + c;   z+ = shrink(t, w / rho);   u+ = t - z+;
 *     r = b - A z+;   p+ = b - r;   q+ = p + (e - y) - p+                  (A A' y = (K - I) y = e - y)
 *     h = v - y - b;   v+ = b + h min(1, delta / ||h||)  (v+ = b + h where ||h|| <= delta, ||h|| = 0 included);   lam+ = v - y - v+
 * -- one pass over A, one over the non-zeros of z+, two triangular M x M matrix-vector products (csmp_bp has a full one besides).
 * Start: z = u = 0, v = lam = 0.  Every check_every iterations the host reads sqrt(||u+ - u||^2 + ||lam+ - lam||^2) (primal residual)
 * and rho sqrt(||z+ - z||^2 + ||v+ - v||^2) (dual residual) and stops when both are < tol; reaching maxiter is not an error.  The result
 * is z: exactly sparse.  delta = 0 is allowed: the ball is the point b, and the method is another route to csmp_bp's answer.
 * rho: unlike csmp_bp, 1 is a poor choice here; the bindings' default is 100.
 * K is positive definite for EVERY dictionary: size(A,1) > size(A,2) and rank-deficient A, which csmp_bp refuses, are served.
 * w, nw: nw = 1 is one weight for every atom, nw = size(A,2) one weight per atom; anything else: CSMP_EDIM.  w is a host array; the
 * weights are non-negative and finite.
 * x: the DENSE result, Float64[size(A,2)]; x_loc says where x AND b live: CSMP_HOST, or CSMP_DEVICE (the call still returns with the
 * work done).  iterations, resnorm (||b - A z||_2 of the returned z), flags: may be NULL.  flags: CSMP_BPD_CONVERGED -- both residuals
 * passed tol at a check; CSMP_BPD_FACTORED -- this call formed and factorised K (the first on a dictionary).  The factor is apart from
 * csmp_bp's: a context may hold both, and neither call invalidates the other's.
 * Memory: the augmented matrix of the factorisation, (2 M)^2 doubles with M rounded up to 64 -- 512 MiB at M = 4096 -- and, during the
 * factorising call only, A A' (M x M doubles) and k_rowgram's partials.
 * CSMP_EINVAL: null pointers, a b_dtype / x_loc that is neither, delta negative or not finite, rho or tol not positive and finite,
 * maxiter < 0, check_every < 1, a negative or non-finite weight, and "bpd: the factorisation of I + A A' met a pivot that is not
 * positive" (non-finite entries of A or a fault of the factorisation, never a property of a finite A).  CSMP_EDIM: nw.  CSMP_ERANGE: more
 * than 2^19 rows.  CSMP_ESTATE: no dictionary -- and a host-streamed dictionary (CSMP_HOST_STREAMED), as csmp_ista.  CSMP_ENOMEM: a
 * buffer could not be allocated; nothing of the factor is left behind, and the next call starts afresh. */
#define CSMP_BPD_CONVERGED 1
#define CSMP_BPD_FACTORED 2
int csmp_bpd(csmp_ctx *ctx, const void *b, int b_dtype, double delta, const double *w, int64_t nw,
             double rho, int64_t maxiter, double tol, int64_t check_every,
             double *x, int x_loc, int64_t *iterations, double *resnorm, int *flags);

/* bpd_batch: csmp_bpd for every column of B, the signals in lockstep on shared launches -- csmp_bp_batch's scheme for data that carry
 * noise.  Everything an iteration of csmp_bpd reads in bulk -- the dictionary, R^-1, R^-T of K = I + A A' -- is the same for every
 * signal: a group of up to eight signals (the groups of csmp_mp_batch: csmp_tune group_max / group_wide apply) takes its iterations
 * together, eight launches a step however many are live -- two triangular M x M products with one read of each triangle for all
 * right-hand sides, one shared pass over A, one launch each for the update, the residual's two steps and the two steps of the
 * M-vector stage (the projection on every member's own ball).  Solves end at different iterations: a finished signal's slot is
 * refilled with the next column at the following multiple of check_every.
 * Contract: column s of X, iterations[s], resnorm[s] and the CSMP_BPD_CONVERGED bit of flags[s] are those of
 * csmp_bpd(ctx, B[:, s], delta[s], ...) with the same w, rho, maxiter, tol, check_every, BIT FOR BIT, whatever nsig and the group
 * sizes are.  CSMP_BPD_FACTORED is set in flags[0] only, and only when this call formed the factor (what a loop over csmp_bpd would
 * report).  No flag is added to csmp_bpd's two.
 * delta, ndelta: a host array; ndelta = 1 is one radius for every signal, ndelta = nsig one radius per signal (noise levels differ
 * from measurement to measurement); anything else: CSMP_EDIM.  Every delta is non-negative and finite.
 * B: size(A,1) x nsig, column-major, leading dimension ldB >= size(A,1), CSMP_F32 or CSMP_F64, on the host or the device (b_loc).
 * X: size(A,2) x nsig doubles, leading dimension ldX >= size(A,2), on the host or the device (x_loc); column s receives the exactly
 * sparse z of signal s, rows beyond size(A,2) are not touched.  w, nw: csmp_bpd's, a host array, shared by all signals.  iterations,
 * resnorm, flags: host arrays of nsig entries, each may be NULL.  maxiter = 0: every column zero, iterations 0, resnorm ||b||.
 * A dictionary without a shared pass (csmp_sweep_config: group 0), CSMP_OPT_SCREENED_SWEEP switched on and nsig = 1 take csmp_bpd's
 * own solve signal by signal: the same outputs.  size(A,1) > size(A,2) and rank-deficient dictionaries are served, as csmp_bpd
 * serves them.
 * Memory beside csmp_bpd's, kept by the context until csmp_set_dictionary: per member of a group 2 size(A,2) + the list
 * (1.5 size(A,2)) doubles, the residual's partials and eight M-vectors -- 8 MiB + 128 MiB for eight members at 4096 x 65536.
 * CSMP_EDIM: ldB < size(A,1), ldX < size(A,2), a w or a delta of another length.  CSMP_EINVAL: nsig < 0, null pointers, a dtype /
 * location that is neither, a negative or non-finite delta, csmp_bpd's knobs and weights.  nsig = 0: CSMP_OK, nothing is touched.
 * CSMP_ERANGE, CSMP_ESTATE: csmp_bpd's.  CSMP_ENOMEM: a buffer could not be allocated; no partial buffers are left behind and the
 * context stays usable.  A refused call writes nothing to X, iterations, resnorm or flags. */
int csmp_bpd_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                   const double *delta, int64_t ndelta, const double *w, int64_t nw, double rho,
                   int64_t maxiter, double tol, int64_t check_every, double *X, int64_t ldX, int x_loc,
                   int64_t *iterations, double *resnorm, int *flags);

/* bpd_candes / bpd_ard: bpd_reweighting (:102-124) with csmp_bpd's solve:  x = solve(w = 1);  then for i = 2 .. outer_maxiter:  w from x
 * (scheme, eps, ard_iter: as csmp_ista_reweighted; CSMP_REWEIGHT_ARD takes supports of up to min(size(A,1), CSMP_ARD_KMAX) atoms);
 * xs = solve(w), WARM-STARTED from the z, u, p, q, v, lam of the previous solve;  norm(xs - x) < min_decrease: return xs;  else x = xs.
 * The reference's defaults: eps = delta (bpd_candes), eps = delta^2 (bpd_ard), min_decrease = 1e-4.
 * delta, rho, maxiter, tol, check_every: csmp_bpd's, for every solve.  x, x_loc, w_out, outer_done, resnorm: as csmp_ista_reweighted.
 * Errors: csmp_bpd's and csmp_ista_reweighted's (CSMP_ERANGE: an iterate with more non-zeros than CSMP_REWEIGHT_ARD takes). */
int csmp_bpd_reweighted(csmp_ctx *ctx, const void *b, int b_dtype, double delta, int scheme, double eps, int64_t ard_iter,
                        int64_t outer_maxiter, double min_decrease, double rho, int64_t maxiter, double tol, int64_t check_every,
                        double *x, int x_loc, double *w_out, int64_t *outer_done, double *resnorm);

/* ------------------------------------------------------------------ sparse Bayesian learning
 * sbl(A, b, sigma2) and update!(::SBL): src/sbl.jl:1-51, for a scalar noise variance sigma2 (a matrix Sigma is not served; fsbl and
 * rmps, :57-437, are csmp_fsbl and csmp_rmps below).  The reference factorises the N x N matrix A'A / sigma2 + Gamma^-1 in every update; this is
 * the same update in the Woodbury form, on the M x M matrix
 *     C = sigma2 I + A Gamma A' = L L',   Gamma = diag(gamma)
 * -- positive definite for EVERY dictionary, so size(A,1) > size(A,2) is served.  For every atom j
 *     s_j = |L^-1 a_j|^2;   q_j = (L^-1 a_j)' (L^-1 b);   x_j = gamma_j q_j;   gamma_j+ = gamma_j q_j^2 / s_j + 1e-14
 * (B^-1 = Gamma - Gamma A' C^-1 A Gamma, so 1 - diag(B^-1)_j / gamma_j = gamma_j s_j and B^-1 A' b / sigma2 = Gamma A' C^-1 b: :26-35
 * exactly, without the cancellation in 1 - diag / gamma).  A zero column has s_j = 0: x_j = 0 and gamma_j+ = 1e-14.  One update is two
 * M x M x N products on the Float64 matrix cores (A Gamma A', and the projections of every atom on the columns of L^-T, of which the
 * triangle's zero half is skipped), one M x M Cholesky factorisation and ONE host read.
 * The loop is sbl's (:38-51): from gamma = gamma_in (NULL: ones), after every update stop when ||gamma_old - gamma||_2 < min_change (the
 * reference's default: 1e-6), at the latest after maxiter updates (the reference's default: 128 size(A,2)); reaching maxiter is not an
 * error.  maxiter = 1 is update!: gamma_out of one call is the gamma_in of the next.
 * x: the DENSE result of the last update, Float64[size(A,2)]; gamma_in (may be NULL), gamma_out (may be NULL; may be gamma_in):
 * Float64[size(A,2)].  loc says where b, x, gamma_in and gamma_out live: CSMP_HOST, or CSMP_DEVICE (the call still returns with the
 * work done).  iterations (updates done), flags: may be NULL.  flags: CSMP_SBL_CONVERGED -- the last update moved gamma by less than
 * min_change.
 * Memory, kept by the context until csmp_set_dictionary, apart from csmp_bp's and csmp_bpd's factors (no call here reads or invalidates
 * them): the augmented matrix of the factorisation, (2 M)^2 doubles with M rounded up to 64, A Gamma A' and its column-split partials
 * (M x M doubles each; one split where the upper 128 x 128 tiles alone fill the device) -- 512 MiB + 128 MiB + 128 MiB at 4096 x 65536
 * -- and four vectors of size(A,2) doubles.
 * CSMP_EINVAL: null pointers, a b_dtype / loc that is neither, sigma2 not positive and finite, min_change negative or NaN, maxiter < 1,
 * an entry of gamma_in that is not positive and finite, "sbl: sigma2 I + A Gamma A' is not positive definite to working precision" (a
 * pivot of the factorisation below 4 M eps of its diagonal entry: csmp_bp's rule), and a gamma that comes out negative or not finite.
 * CSMP_ERANGE: more than 2^19 rows.  CSMP_ESTATE: no dictionary -- and a host-streamed dictionary (CSMP_HOST_STREAMED), as csmp_ista.
 * CSMP_ENOMEM: a buffer could not be allocated; none of them is left behind, and the next call starts afresh. */
#define CSMP_SBL_CONVERGED 1
int csmp_sbl(csmp_ctx *ctx, const void *b, int b_dtype, double sigma2, int64_t maxiter, double min_change,
             const double *gamma_in, double *x, double *gamma_out, int loc, int64_t *iterations, int *flags);

/* ------------------------------------------------------------------ greedy sparse Bayesian learning
 * fsbl(A, b, sigma2) and rmps(A, b, sigma2): src/sbl.jl:57-437, for a scalar noise variance sigma2 (a matrix Sigma, the sigma2-optimising
 * rmps and the unused rmp_acquisition_value are not served).  Every step changes the prior precision alpha_i of ONE atom (+inf =
 * inactive; all atoms start there).  The state is alpha, C^-1 (size(A,1)^2 doubles, I / sigma2 at the start),
 *     S_j = a_j' C^-1 a_j   and   Q_j = a_j' C^-1 b      (|a_j|^2 / sigma2 and (A'b)_j / sigma2 at the start),
 * and per atom f = alpha / (alpha - S) (1 where inactive), s = S f, q = Q f, relevant = s < q^2, alpha* = s^2 / (q^2 - s).  The actions on
 * a picked atom i: add (alpha_i = alpha*, gam = 1 / alpha*), delete (gam = -1 / alpha_i, alpha_i = +inf), re-estimate (gam = 1 / alpha* -
 * 1 / alpha_i, alpha_i = alpha*), each followed by the rank-one step
 *     v = C^-1 a_i;  den = 1 / gam + S_i;  C^-1 -= v v' / den;  w = A'v;  S -= w^2 / den;  Q -= w Q_i / den.
 * One step is an N-pass that applies the previous step's S / Q update and evaluates every atom, ONE host read (the decision), one
 * M x M matrix-vector product, one streaming update of C^-1 and one product sweep over A.
 * csmp_fsbl, a pass (:165-176): delta_j = delta_add (inactive, relevant), delta_del (active, not relevant), delta_upd (active, relevant)
 * or 0; i = the first arg-max; where delta_i > 0 the matching action.  After the pass in which max delta < min_increase the loop stops
 * (the reference's default: 1e-6), at the latest after maxiter passes (the reference's default: 2 size(A,2)); reaching maxiter is not an
 * error.  maxiter = 1 is update!(::FSBL): alpha_out of one call is the alpha_in of the next.
 * csmp_rmps, an outer iteration (:389-404): at most maxiter_acquisition additions of the first arg-max of delta_add while it is > 0; stop
 * where alpha has not changed since the last check; at most maxiter_deletion turns, each the deletion of the first arg-min of q^2 / s over
 * the active atoms that are not relevant where that is < 1, else the re-estimation of the arg-max of delta_upd where that is > 0, the
 * stage ending once that value (0 where nothing was done) is < min_increase; stop where alpha has not changed.  The reference's defaults:
 * size(A,1) for the three caps.
 * x: the posterior mean, Float64[size(A,2)], exactly 0 on the inactive atoms and Q_j / alpha_j on the active ones -- in exact arithmetic
 * what the reference's solve (A_a'A_a / sigma2 + diag alpha_a) x_a = A_a'b / sigma2 gives.  alpha_in (may be NULL: all +inf): a warm
 * start, entries positive or +inf; the state is rebuilt from I / sigma2 by one rank-one step per finite entry, in index order.  alpha_out
 * (may be NULL; may be alpha_in).  loc says where b, x, alpha_in and alpha_out live: CSMP_HOST, or CSMP_DEVICE (the call still returns
 * with the work done).  history (host memory, may be NULL): the pairs (action, index) of the applied steps, the first history_cap of
 * them, 2 history_cap words; actions: 1 add, 2 delete, 3 re-estimate.  iterations: passes done (csmp_fsbl), steps applied (csmp_rmps).
 * flags: CSMP_FSBL_CONVERGED / CSMP_RMPS_CONVERGED -- a stopping rule ended the run, not a cap.  iterations, flags: may be NULL.
 * Memory, kept by the context until csmp_set_dictionary, apart from csmp_sbl's buffers and csmp_bp's and csmp_bpd's factors (no call here
 * reads or invalidates them): C^-1, size(A,1)^2 doubles -- 128 MiB at 4096 rows -- and five vectors of size(A,2) doubles.
 * CSMP_EINVAL: null pointers, a b_dtype / loc that is neither, sigma2 not positive and finite, min_increase negative or NaN, a cap < 1,
 * an entry of alpha_in that is not positive (or NaN), and a value of the marginal likelihood's change that is not finite.  CSMP_ERANGE:
 * more than 2^19 rows.  CSMP_ESTATE: no dictionary -- and a host-streamed dictionary (CSMP_HOST_STREAMED), as csmp_sbl.  CSMP_ENOMEM:
 * the size(A,1)^2 doubles of C^-1 or a vector could not be allocated; none of them is left behind, and the next call starts afresh. */
#define CSMP_FSBL_CONVERGED 1
#define CSMP_RMPS_CONVERGED 1
int csmp_fsbl(csmp_ctx *ctx, const void *b, int b_dtype, double sigma2, int64_t maxiter, double min_increase,
              const double *alpha_in, double *x, double *alpha_out, int loc,
              int64_t *history, int64_t history_cap, int64_t *iterations, int *flags);
int csmp_rmps(csmp_ctx *ctx, const void *b, int b_dtype, double sigma2, int64_t maxiter, int64_t maxiter_acquisition,
              int64_t maxiter_deletion, double min_increase, const double *alpha_in, double *x, double *alpha_out, int loc,
              int64_t *history, int64_t history_cap, int64_t *iterations, int *flags);

/* fsbl_batch / rmps_batch: csmp_fsbl / csmp_rmps for every column of B in lockstep on shared launches.  The product sweep w = A'v of a
 * greedy step -- the one read of the dictionary, two thirds of a step at 4096 x 65536 -- is the same read for every signal: a group of up
 * to eight signals (the groups of csmp_mp_batch and csmp_bp_batch: csmp_tune group_max / group_wide apply) takes its steps together.
 * One tick of the group is five launches (the N-pass, the decisions, a_i, C^-1 a_i and the rank-one update of every member), ONE read
 * of all decision records and one shared pass over A for the members that acted; C^-1 stays per signal.  The signals end at different
 * steps: a slot whose signal is done takes the next unsolved one in ascending order.
 * Contract: column s of X, column s of alpha_out, iterations[s], flags[s] and signal s's history are those of
 * csmp_fsbl(ctx, B[:, s], sigma2_s, maxiter, min_increase, alpha_in[:, s], ...) -- of csmp_rmps likewise --, BIT FOR BIT, whatever nsig,
 * the group sizes and the order the slots are refilled in.
 * B: size(A,1) x nsig, column-major, leading dimension ldB >= size(A,1), CSMP_F32 or CSMP_F64, on the host or the device (b_loc); read only.
 * sigma2, nsigma2: a host array of nsigma2 = 1 (one noise variance for every signal) or nsigma2 = nsig (one per signal) values.
 * X: size(A,2) x nsig doubles, leading dimension ldX >= size(A,2), on the host or the device (x_loc); rows beyond size(A,2) are not
 * touched.  alpha_in: NULL (every signal starts with all atoms inactive) or size(A,2) x nsig doubles where X lives, leading dimension
 * ld_alpha_in >= size(A,2), entries positive or +inf; column s is the warm start of signal s.  alpha_out: NULL or size(A,2) x nsig doubles
 * where X lives, ld_alpha_out >= size(A,2); it may be alpha_in itself (with the same leading dimension).
 * history (host memory, may be NULL): 2 history_cap nsig words; signal s's pairs (action, index) start at 2 history_cap s and are cut at
 * history_cap as in the single call.  iterations, flags: host arrays of nsig entries, or NULL.  nsig = 0: CSMP_OK, nothing is touched.
 * A dictionary without a shared pass (csmp_sweep_config: group 0), CSMP_OPT_SCREENED_SWEEP switched on and nsig = 1 take csmp_fsbl's /
 * csmp_rmps's own launches signal by signal: the same outputs.
 * Memory beside csmp_fsbl's, kept by the context until csmp_set_dictionary: per member of a group C^-1, size(A,1)^2 doubles, and five
 * vectors of size(A,2) doubles -- 1 GiB + 20 MiB for eight members at 4096 x 65536.
 * CSMP_EINVAL: nsig < 0, null pointers, a dtype / location that is neither, nsigma2 other than 1 or nsig, a sigma2 that is not positive
 * and finite, min_increase negative or NaN, a cap < 1, history_cap < 0, an entry of alpha_in that is not positive (or NaN) -- and, during
 * the run, a value of the marginal likelihood's change that is not finite (the message names the signal).  CSMP_EDIM: ldB < size(A,1);
 * ldX, ld_alpha_in or ld_alpha_out < size(A,2).  CSMP_ESTATE: no dictionary, or a host-streamed one.  CSMP_ERANGE: more than 2^19 rows.
 * CSMP_ENOMEM: the members' buffers, R x size(A,1)^2 doubles and the vectors, could not be allocated; none of them is left behind and the
 * context stays usable.  R is the group's size (eight where wide groups are on and nsig exceeds a narrow group, else up to four): the
 * call does NOT fall back to fewer members -- where R matrices do not fit beside the dictionary, the loop over csmp_fsbl / csmp_rmps,
 * which keeps one, is the caller's way.  Everything is validated before any device work.  A refused call writes nothing. */
int csmp_fsbl_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                    const double *sigma2, int64_t nsigma2, int64_t maxiter, double min_increase,
                    const double *alpha_in, int64_t ld_alpha_in, double *X, int64_t ldX,
                    double *alpha_out, int64_t ld_alpha_out, int x_loc,
                    int64_t *history, int64_t history_cap, int64_t *iterations, int *flags);
int csmp_rmps_batch(csmp_ctx *ctx, const void *B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                    const double *sigma2, int64_t nsigma2, int64_t maxiter, int64_t maxiter_acquisition,
                    int64_t maxiter_deletion, double min_increase,
                    const double *alpha_in, int64_t ld_alpha_in, double *X, int64_t ldX,
                    double *alpha_out, int64_t ld_alpha_out, int x_loc,
                    int64_t *history, int64_t history_cap, int64_t *iterations, int *flags);

/* ------------------------------------------------------------------ dictionary analysis
 * colnorms(A): src/util.jl:2.  norms[j] = ||a_j||_2 of every column of the resident dictionary, N doubles, to host memory
 * (out_loc = CSMP_HOST) or device memory (CSMP_DEVICE; the call still returns with the work done).  Float64 on the exactly
 * promoted dictionary values; a zero column gives 0.
 * CSMP_EINVAL: a null ctx or norms, an out_loc that is neither.  CSMP_ESTATE: no dictionary -- and a host-streamed dictionary
 * (CSMP_HOST_STREAMED), which the analysis entries do not serve.  CSMP_ENOMEM: the N doubles could not be allocated; nothing
 * is left behind. */
int csmp_colnorms(csmp_ctx *ctx, double *norms, int out_loc);              /* N doubles, CSMP_HOST or CSMP_DEVICE */

/* coherence(A) / babel(A,k) / cumbabel(A,k): src/util.jl:96-115.  mu[m-1] = mu_1(m), m = 1..k, the Babel function: for every
 * column i form g = |A' a_i| and set g[i] = 0 -- the self entry does not count, and it stays in the vector as a zero, so with
 * k = N the last term added is that zero --, sort the k largest entries of g in descending order, take their running sums
 * s_i(1..k); mu_1(m) = max_i s_i(m).  babel(A,k) = mu[k-1], coherence(A) = mu[0].  The inner products are raw, as in the
 * reference, which assumes unit-norm columns and does not divide.
 * normalize = 1 (an addition): every entry is |<a_i, a_j>| / (||a_i|| ||a_j||), the coherence of a dictionary that has not been
 * normalised; a zero column contributes 0.  normalize = 0: the reference's values.
 * pair (may be NULL; an addition): the two columns (i, j), i < j, 0-based, that attain mu_1(1); among equal values the lowest i
 * wins, then the lowest j (tie-break); (-1, -1) when N = 1.  mu and pair are host arrays of k doubles and 2 int64.
 * Float64 on the exactly promoted dictionary values, every sum in a fixed order: the same call returns the same bits every time.
 * The N x N Gram matrix is never held: the device keeps one strip of 128 rows of it (1 KiB per column of the dictionary).
 * CSMP_EINVAL: a null ctx or mu, a normalize that is neither 0 nor 1.  CSMP_ERANGE: k < 1 or k > min(N, CSMP_BABEL_KMAX).
 * CSMP_ESTATE: no dictionary -- and a host-streamed dictionary (CSMP_HOST_STREAMED): the call is N passes over the dictionary,
 * which would cross the host link each time (as csmp_ista).  CSMP_ENOMEM: a buffer could not be allocated; nothing is left
 * behind, and the next call starts afresh. */
#define CSMP_BABEL_KMAX 1024
int csmp_cumbabel(csmp_ctx *ctx, int64_t k, int normalize, double *mu, int64_t *pair);  /* mu: k doubles (host); pair: 2 int64 (host) or NULL */

/* ------------------------------------------------------------------ primitives
 * argmaxinner!(P) / argmaxinner!(P,k): src/matchingpursuit.jl:181-193.  r: length-M Float64
 * host vector.  abs_corr (may be NULL): receives |A' r| (length N).  top_idx/top_val: the
 * topk atoms, descending by |<a_i, r>|, ties by ascending index (partialsortperm, :192). */
int csmp_sweep(csmp_ctx *ctx, const double *r, double *abs_corr, int64_t topk, int64_t *top_idx, double *top_val);

/* A[:, cols] \ b by the on-device QR: the UpdatableQR solve pinned by test/forward.jl:23-28
 * ("P.AiQR \ y ~ A[:, nzind] \ y").  cols in any order; coef aligned with cols. */
int csmp_lstsq(csmp_ctx *ctx, const int64_t *cols, int64_t ncols, const void *b, int b_dtype, double *coef);

#ifdef __cplusplus
}
#endif
#endif
