// host/mp_batch.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_mp_batch -- Matching Pursuit for every column of B on the shared pass of the grouped scheduler (host/omp.hpp).
// ------------------------------------------------------------------------------------------ mp batch
// MP keeps no factorisation: a step is the sweep, the arg-max and one AXPY on a column.  A GROUP of up to group_wide signals takes
// its steps together, two launches each: the shared pass csmp_omp_batch's grouped scheduler launches (shared_pass_launch, host/omp.hpp,
// with eps = 0, check_eps = 0, skipmask = 0: MP never stops early) reads A once for all members, then k_mp_group does
// k_select's and k_mp_update's work for every member.  Member m of a group lives in solver slot 3 m (the slots of group 0 of the
// grouped scheduler).  TWO groups run side by side, the second on the twin context and stream, so that one group's short launch
// falls under the other group's pass; a round is one group per pipeline (mp_batch_plan, host/batch_plan.hpp).  The twin, the slots
// of both contexts, the fork and the join of the streams are batch_pipelines' (host/batch_io.hpp), a lone signal's solve is mp_solve
// (host/forward.hpp); this file keeps the group's step, the emit launch and the round loop.  Every signal's
// arithmetic is csmp_mp's -- the pass gives sweep_body_gen's bits per member, the arg-max order is k_select's, the update is
// k_mp_update's expression, the output rule is mp_collect's (k_mp_emit) -- so the results are csmp_mp's bit for bit.
// A round with one group only (a batch of 2 .. group_wide signals, the last round of an odd number of groups): the group whole on one
// stream, or its halves on two?  csmp_tune pipelines 2 takes the halves and 3 the whole group, whatever this says.
// Measured at 4096 x 65536 f32, k = 256, atoms/s of a whole call (six calls each, the two forms alternated): 2 signals whole 11.87e3,
// halves 6.68e3; 4 signals 22.96e3 / 13.27e3; 8 signals 34.8e3 / 26.1e3.  The extra pass costs far more than the hidden short launch
// gives back: the group stays whole.
constexpr bool kMpSplitLone = false;
template <typename TA>
static int mp_group_step(csmp_ctx* ctx, int size, int nblk, int nblk_wide, size_t lds_sweep) {
    CHECK(shared_pass_launch<TA>(ctx, 0, size, 0.0, 0, 0, nblk, nblk_wide, lds_sweep, true));  // (eps, check_eps, skipmask: MP never stops early; need_c: k_mp_group reads c)
    const bool wide = size > kGroupMax;
    MpGroup g;
    g.n = size;
    for (int m = 0; m < kWideMax; ++m) {
        const Solver& s = *slot_ptr(ctx, 3 * std::min(m, size - 1));
        g.r[m] = s.r; g.cvec[m] = s.cvec; g.pval[m] = s.pval; g.pidx[m] = s.pidx; g.st[m] = s.st; g.sel[m] = s.sel; g.z[m] = s.z;
        g.cap[m] = s.kcap;
        g.nblk[m] = wide ? nblk_wide / 2 : nblk;  // (the pass's partials: one per stream)
    }
    const int wgs = ((int)ctx->M + 255) / 256;
    hipLaunchKernelGGL(k_mp_group<TA>, dim3((unsigned)(size * wgs)), dim3(256), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld, (int)ctx->M, ctx->N, g, wgs);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// the logs of the `size` signals from `first`, in the context's slots 0, 3, 6, ... (slot 0 active), into their output columns
static int mp_emit(csmp_ctx* ctx, const BatchIO& io, int64_t first, int size) {
    MpEmit e;
    e.n = size;
    for (int m = 0; m < kWideMax; ++m) {
        const int mm = std::min(m, size - 1);
        const Solver& s = *slot_ptr(ctx, 3 * mm);
        e.sel[m] = s.sel; e.z[m] = s.z; e.st[m] = s.st;
        e.keep[m] = s.cands; e.acc[m] = s.coef;  // (scratch of kcap entries each; nothing reads them between solves)
        e.idx[m] = io.d_idx + (first + mm) * io.k; e.val[m] = io.d_val + (first + mm) * io.k; e.nnz[m] = io.d_nnz + (first + mm);
    }
    hipLaunchKernelGGL(k_mp_emit, dim3((unsigned)size), dim3(256), 0, ctx->stream, e, (int)io.k);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// One signal through csmp_mp's own solve (mp_solve, host/forward.hpp: mp_step; with CSMP_OPT_SCREENED_SWEEP mp_step_screened, an
// uncertified solve repeated with the exact sweep) and the emit kernel: the path of a dictionary without a shared pass, of the
// screened sweeps, of a lone signal
static int mp_solve_one(csmp_ctx* ctx, const BatchIO& io, int64_t sgn) {
    CHECK(mp_solve(ctx, io.k, [&]() -> int { return io.init(ctx, sgn); }));
    return mp_emit(ctx, io, sgn, 1);
}

static int mp_batch_impl(csmp_ctx* ctx, BatchIO& io) {
    const int64_t nsig = io.nsig, k = io.k;
    if (k > ((int64_t)1 << 28)) return fail(ctx, CSMP_ERANGE, "mp_batch: k too large");
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    auto ensure = [&](csmp_ctx* c) -> int {  // c's active slot ready for a solve of this batch
        const int rc = solver_ensure(c, (int)k, 1, false);  // MP keeps no factorisation: k is bound neither by M nor by qr_max_cols()
        c->s.begun = false;
        return rc;
    };
    CHECK(ensure(ctx));
    CHECK(io.stage(false));
    // The shared pass where the resident dictionary has one and the sweeps are exact; a lone signal keeps csmp_mp's launches.
    const bool grouped = ctx->pipeline && ctx->sweep_group >= 1 && !screened_on(ctx) && nsig >= 2;
    if (!grouped) {
        int rc = CSMP_OK;
        for (int64_t sgn = 0; sgn < nsig && rc == CSMP_OK; ++sgn) rc = mp_solve_one(ctx, io, sgn);
        return io.done(rc);
    }
    // Two pipelines where csmp_omp_batch takes them (batch_two_pipelines, host/batch_io.hpp).  Member m of a group is slot 3 m: the
    // narrow groups' sweep_group slots, and group_wide of them where the batch has more signals than a narrow pass serves.
    const bool two = batch_two_pipelines(ctx);
    const int wide_members = ctx->group_wide > ctx->sweep_group && nsig > ctx->sweep_group && !ctx->wide_refused ? ctx->group_wide : 0;
    auto run_plan = [&](csmp_ctx* tw, bool wide) -> int {
        csmp_ctx* cs[2] = {ctx, tw};
        // the grids and the LDS request of the passes: the grouped scheduler's (pipe_begin) -- one workgroup per CU
        const size_t excl = (size_t)(ctx->tune_pair_lds_kib > 0 ? ctx->tune_pair_lds_kib : kPairLdsKiB) * 1024;
        const int members = wide ? wide_members : ctx->sweep_group;
        for (const MpRound& r : mp_batch_plan(nsig, members, !two, ctx->tune_pipelines == 2 || (ctx->tune_pipelines != 3 && kMpSplitLone))) {
            for (int p = 0; p < 2; ++p) {  // every member's signal into its slot
                csmp_ctx* c = cs[p];
                for (int m = 0; m < r.g[p].size; ++m) {
                    activate_slot(c, 3 * m);
                    CHECK(twin_rc(ctx, c, io.init(c, r.g[p].first + m)));
                }
                if (r.g[p].size > 0) activate_slot(c, 0);
            }
            for (int64_t t = 0; t < k; ++t)
                for (int p = 0; p < 2; ++p) {
                    if (r.g[p].size == 0) continue;
                    csmp_ctx* c = cs[p];
                    const int nblk = pipe_nblk(c, c->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid), nw = wide_nblk(c);
                    CHECK(twin_rc(ctx, c, c->dtype == CSMP_F32 ? mp_group_step<float>(c, r.g[p].size, nblk, nw, excl)
                                                               : mp_group_step<double>(c, r.g[p].size, nblk, nw, excl)));
                }
            for (int p = 0; p < 2; ++p)
                if (r.g[p].size > 0) CHECK(twin_rc(ctx, cs[p], mp_emit(cs[p], io, r.g[p].first, r.g[p].size)));
        }
        return CSMP_OK;
    };
    return io.done(batch_pipelines(ctx, two, ctx->sweep_group, wide_members, 3, ensure, run_plan));
}

extern "C" int csmp_mp_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k, int64_t* idx,
                             double* val, int64_t* nnz, int out_loc) {
    if (!ctx) return CSMP_EINVAL;
    BatchIO io(ctx, B, b_dtype, ldB, nsig, b_loc, k, idx, val, nnz, out_loc);
    CHECK(io.check());
    if (nsig == 0) return CSMP_OK;
    return mp_batch_impl(ctx, io);
}
