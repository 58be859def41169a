// host/mp_batch.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_mp_batch -- Matching Pursuit for every column of B on the shared pass of the grouped scheduler (host/omp.hpp).
// ------------------------------------------------------------------------------------------ mp batch
// MP keeps no factorisation: a step is the sweep, the arg-max and one AXPY on a column.  A GROUP of up to group_wide signals takes
// its steps together, two launches each: the shared pass csmp_omp_batch's grouped scheduler launches (multi_members + multi_launch /
// wide_launch with eps = 0, check_eps = 0, skipmask = 0: MP never stops early) reads A once for all members, then k_mp_group does
// k_select's and k_mp_update's work for every member.  Member m of a group lives in solver slot 3 m (the slots of group 0 of the
// grouped scheduler).  TWO groups run side by side, the second on the twin context and stream, so that one group's short launch
// falls under the other group's pass; a round is one group per pipeline (mp_batch_plan, host/batch_plan.hpp).  Every signal's
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
    MultiSweep<TA> p;
    p.A = (const TA*)ctx->dA; p.ld = ctx->ld; p.Mv = ctx->Mv; p.N = ctx->N;
    const bool wide = size > kGroupMax;
    p.eps = 0.0; p.check_eps = 0; p.skipmask = 0; p.nblk = wide ? nblk_wide : nblk; p.KP = ctx->sweep_KP;
    multi_members<TA>(ctx, p, 0, size);
    const bool timed = prof_pick(ctx);  // (one sampled launch per shared pass, as group_pipe_launch's)
    if (timed) CHECK(prof_mark(ctx));
    const size_t lds = std::max(sweep_multi_lds_bytes(p.KP, p.n), lds_sweep);
    HIPCHECK(wide ? wide_launch<TA>(ctx, p, lds) : multi_launch<TA>(ctx, p, lds));
    if (timed) CHECK(prof_mark(ctx));
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

// One signal through csmp_mp's own launches (mp_step; with CSMP_OPT_SCREENED_SWEEP mp_step_screened, an uncertified solve repeated
// with the exact sweep) and the emit kernel: the path of a dictionary without a shared pass, of the screened sweeps, of a lone signal
static int mp_solve_one(csmp_ctx* ctx, const BatchIO& io, int64_t sgn) {
    bool screened = screened_on(ctx);
    if (screened) CHECK(screened_ensure(ctx));
    ctx->scr_lone = true;  // (one solve at a time: reset on every way out below)
    struct LoneReset {
        csmp_ctx* c;
        ~LoneReset() { c->scr_lone = false; }
    } lone_reset{ctx};
    for (int attempt = 0; attempt < 2; ++attempt) {
        CHECK(io.init(ctx, sgn));
        for (int64_t t = 0; t < io.k; ++t) {
            if (screened) {
                Solver& s = ctx->s;
                if (s.jh >= s.kcap) return fail(ctx, CSMP_ERANGE, "mp: more steps than the capacity this solver was begun with");
                s.jh += 1;
                CHECK(mp_step_screened(ctx));
            } else {
                CHECK(mp_step(ctx));
            }
        }
        if (!screened) break;
        DevState hs;
        HIPCHECK(hipMemcpyAsync(&hs, ctx->s.st, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        ctx->scr_solves += 1;
        if (hs.uncertain == 0) break;
        ctx->scr_fallbacks += 1;
        screened = false;
    }
    return mp_emit(ctx, io, sgn, 1);
}

static int mp_batch_impl(csmp_ctx* ctx, BatchIO& io) {
    const int64_t nsig = io.nsig, k = io.k;
    if (k > ((int64_t)1 << 28)) return fail(ctx, CSMP_ERANGE, "mp_batch: k too large");
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    CHECK(solver_ensure(ctx, (int)k, 1, false));  // MP keeps no factorisation: k is bound neither by M nor by qr_max_cols()
    ctx->s.begun = false;
    CHECK(io.stage(false));
    // The shared pass where the resident dictionary has one and the sweeps are exact; a lone signal keeps csmp_mp's launches.
    const bool grouped = ctx->pipeline && ctx->sweep_group >= 1 && !screened_on(ctx) && nsig >= 2;
    if (!grouped) {
        int rc = CSMP_OK;
        for (int64_t sgn = 0; sgn < nsig && rc == CSMP_OK; ++sgn) rc = mp_solve_one(ctx, io, sgn);
        return io.done(rc);
    }
    // Two pipelines as csmp_omp_batch takes them (batch_schedule): csmp_tune pipelines 1 keeps one stream, 2 and 3 take two whatever
    // the size, automatic: dictionaries of 4 MiB and more.
    const size_t dict_bytes = (size_t)ctx->Mv * (size_t)ctx->N * (ctx->dtype == CSMP_F32 ? 4 : 8);
    const bool two = ctx->tune_pipelines != 1 && (ctx->tune_pipelines >= 2 || dict_bytes >= ((size_t)4 << 20));
    int members = ctx->sweep_group;
    const int wide_members = ctx->group_wide > ctx->sweep_group && nsig > ctx->sweep_group && !ctx->wide_refused ? ctx->group_wide : 0;
    csmp_ctx* tw = nullptr;
    auto on = [&](csmp_ctx* c, int rc) -> int {  // (a twin's failure is reported on the caller's context)
        if (rc != CSMP_OK && c != ctx) ctx->err = c->err;
        return rc;
    };
    auto ensure_slots = [&](csmp_ctx* c, int from, int to) -> int {  // the slots of members from .. to - 1
        int rc = CSMP_OK;
        for (int m = from; m < to && rc == CSMP_OK; ++m) {
            activate_slot(c, 3 * m);
            rc = solver_ensure(c, (int)k, 1, false);
            c->s.begun = false;
        }
        activate_slot(c, 0);
        return on(c, rc);
    };
    auto each_member = [&](csmp_ctx* c, const PlanGroup& g, auto&& f) -> int {
        int rc = CSMP_OK;
        for (int m = 0; m < g.size && rc == CSMP_OK; ++m) {
            activate_slot(c, 3 * m);
            rc = f(c, g.first + m);
        }
        activate_slot(c, 0);
        return on(c, rc);
    };
    auto run_plan = [&]() -> int {  // (every way out of here once the twin exists passes the drain below)
        CHECK(ensure_slots(ctx, 1, members));
        if (two) {
            CHECK(twins_ensure(ctx, 1));
            tw = ctx->twins[0];
            tw->prof = ctx->prof;  // (csmp_profile_*: the second pipeline's passes are sampled like the first's)
            tw->prof_every = ctx->prof_every;
            CHECK(ensure_slots(tw, 0, members));
        }
        if (wide_members > 0) {
            // the slots beyond the narrow groups': all of them on both contexts, or none -- a device that cannot hold them runs the
            // groups of sweep_group members it has the slots for (batch_impl's rule)
            csmp_ctx* cs[2] = {ctx, tw};
            int r3 = CSMP_OK;
            for (csmp_ctx* c : cs) {
                if (!c || r3 != CSMP_OK) continue;
                c->tune_fail_alloc = ctx->tune_fail_alloc;  // (the test hook counts on through the twin's allocations)
                r3 = ensure_slots(c, members, wide_members);
                ctx->tune_fail_alloc = c->tune_fail_alloc;
                if (c != ctx) c->tune_fail_alloc = 0;
            }
            if (r3 == CSMP_OK) {
                members = wide_members;
            } else {
                ctx->wide_refused = true;
                for (csmp_ctx* c : cs) {
                    if (!c) continue;
                    (void)hipStreamSynchronize(c->stream);
                    for (int m = members; m < wide_members; ++m) {
                        activate_slot(c, 3 * m);
                        solver_free(c->s);
                    }
                    activate_slot(c, 0);
                    c->err.clear();
                }
                (void)hipGetLastError();
            }
        }
        if (two) {
            if (!ctx->ev_twin) HIPCHECK(hipEventCreateWithFlags(&ctx->ev_twin, hipEventDisableTiming));
            if (!tw->ev_twin) HIPCHECK(hipEventCreateWithFlags(&tw->ev_twin, hipEventDisableTiming));
            // (the twin starts behind everything this context's stream holds: the caller's buffers, the slots' allocation)
            HIPCHECK(hipEventRecord(ctx->ev_twin, ctx->stream));
            HIPCHECK(hipStreamWaitEvent(tw->stream, ctx->ev_twin, 0));
        }
        // the grids and the LDS request of the passes: the grouped scheduler's (pipe_begin) -- one workgroup per CU
        csmp_ctx* cs[2] = {ctx, tw};
        const size_t excl = (size_t)(ctx->tune_pair_lds_kib > 0 ? ctx->tune_pair_lds_kib : kPairLdsKiB) * 1024;
        auto init = [&](csmp_ctx* c, int64_t sgn) -> int { return io.init(c, sgn); };
        for (const MpRound& r : mp_batch_plan(nsig, members, !two, ctx->tune_pipelines == 2 || (ctx->tune_pipelines != 3 && kMpSplitLone))) {
            for (int p = 0; p < 2; ++p)
                if (r.g[p].size > 0) CHECK(each_member(cs[p], r.g[p], init));
            for (int64_t t = 0; t < k; ++t)
                for (int p = 0; p < 2; ++p) {
                    if (r.g[p].size == 0) continue;
                    csmp_ctx* c = cs[p];
                    const int nblk = pipe_nblk(c, c->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid), nw = wide_nblk(c);
                    CHECK(on(c, c->dtype == CSMP_F32 ? mp_group_step<float>(c, r.g[p].size, nblk, nw, excl)
                                                      : mp_group_step<double>(c, r.g[p].size, nblk, nw, excl)));
                }
            for (int p = 0; p < 2; ++p)
                if (r.g[p].size > 0) CHECK(on(cs[p], mp_emit(cs[p], io, r.g[p].first, r.g[p].size)));
        }
        if (two) {  // this context's stream goes on behind the twin's last launch
            HIPCHECK(hipEventRecord(tw->ev_twin, tw->stream));
            HIPCHECK(hipStreamWaitEvent(ctx->stream, tw->ev_twin, 0));
        }
        return CSMP_OK;
    };
    const int rc = run_plan();
    activate_slot(ctx, 0);
    if (tw) activate_slot(tw, 0);
    if (rc != CSMP_OK && tw) {  // (a failed enqueue: both streams drained before anything is released)
        (void)hipStreamSynchronize(tw->stream);
        (void)hipStreamSynchronize(ctx->stream);
    }
    return io.done(rc);
}

extern "C" int csmp_mp_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k, int64_t* idx,
                             double* val, int64_t* nnz, int out_loc) {
    if (!ctx) return CSMP_EINVAL;
    BatchIO io(ctx, B, b_dtype, ldB, nsig, b_loc, k, idx, val, nnz, out_loc);
    CHECK(io.check());
    if (nsig == 0) return CSMP_OK;
    return mp_batch_impl(ctx, io);
}
