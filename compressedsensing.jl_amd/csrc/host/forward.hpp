// host/forward.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// forward regression (OLS) sweeps and drivers; the omp / fr batch drivers (batch_impl: the schedule, the rounds and the re-solves, on
// the two-pipeline scaffold of host/batch_io.hpp); mp (mp_solve: the one MP solve csmp_mp and csmp_mp_batch's lone signals share).
// ------------------------------------------------------------------------------------------ forward regression (OLS)
// one pass of k_fr_sweep (csmp_forward.hpp): nq = -1 first step (norms), 0 scores only, 1 / 2 directions
struct FrPass {
    int nq = 1;
    const double* q1 = nullptr;  // null with nq >= 1: the last Q column, looked up on the device
    double s1 = -1.0;
    const double* q2 = nullptr;
    double s2 = 1.0;
    int64_t qstride = 0;  // nq == 4: the directions are q1 + d*qstride
    const int* unmark = nullptr;
    int update_only = 0;
};

template <typename TA, int U, bool FULL, int NQ>
static hipError_t fr_sweep_launch_t(csmp_ctx* ctx, const FrPass& ps, int grid, size_t lds, double max_eps, int skipmask) {
    Solver& s = ctx->s;
    auto kern = k_fr_sweep<TA, U, FULL, NQ>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kSweepThreads), lds, ctx->stream, (const TA*)ctx->dA, ctx->ld, ctx->Mv, ctx->N,
                       (const double*)s.r, (const double*)s.Q, s.ldq, ps.q1, ps.s1, ps.q2, ps.s2, ps.unmark, ps.update_only, s.rho2,
                       s.dvec, s.pval, s.pidx, (const int*)s.sel, s.st, max_eps, skipmask);
    return hipGetLastError();
}
template <typename TA, int U, bool FULL>
static hipError_t fr_sweep_launch_nq(csmp_ctx* ctx, const FrPass& ps, int grid, size_t lds, double max_eps, int skipmask) {
    switch (ps.nq) {
        case -1: return fr_sweep_launch_t<TA, U, FULL, -1>(ctx, ps, grid, lds, max_eps, skipmask);
        case 0: return fr_sweep_launch_t<TA, U, FULL, 0>(ctx, ps, grid, lds, max_eps, skipmask);
        case 1: return fr_sweep_launch_t<TA, U, FULL, 1>(ctx, ps, grid, lds, max_eps, skipmask);
        case 2: return fr_sweep_launch_t<TA, U, FULL, 2>(ctx, ps, grid, lds, max_eps, skipmask);
        default: return hipErrorInvalidValue;
    }
}
template <typename TA>
static hipError_t fr_sweep_launch(csmp_ctx* ctx, const FrPass& ps, int U, bool full, int grid, size_t lds, double max_eps, int skipmask) {
    if (!full) return fr_sweep_launch_nq<TA, 4, false>(ctx, ps, grid, lds, max_eps, skipmask);
    if (U == 16) return fr_sweep_launch_nq<TA, 16, true>(ctx, ps, grid, lds, max_eps, skipmask);
    return fr_sweep_launch_nq<TA, 8, true>(ctx, ps, grid, lds, max_eps, skipmask);
}

// block size of the forward-regression sweep: 16 or 8 chunks when they tile M exactly, else the
// predicated 4-chunk kernel
static void fr_config(const csmp_ctx* ctx, int nq, int& U, bool& full, size_t& lds, int& grid) {
    const int vec = ctx->dtype == CSMP_F32 ? 4 : 2;
    const int rows = kWave * vec;
    U = 4;
    full = false;
    if (ctx->Mv % rows == 0) {
        const int nchunk = ctx->Mv / rows;
        // Measured at 4096 x 65536 f32 (profiles/r01_bench_fr_line.json): 8-chunk blocks on one workgroup per CU
        // 168 us, 16-chunk blocks on 3/4 of the CUs (the OMP sweep's optimum) 173 us -- with a second LDS image
        // to read per chunk, the extra waves hide more than the extra DRAM streams cost.
        // With TWO directions the three images leave room for one workgroup per CU only: four waves, and what hides the DRAM latency
        // is the loads each of them keeps in flight -- 16-chunk blocks on 15/16 of the CUs 175 us, 8-chunk blocks on all of them 187
        // (16 on all: 184, on 7/8: 176, on 3/4: 194; profiles/r05_bench_srr_kernel_stats.csv).
        const int umax = ctx->tune_sweep_U == 16 ? 16 : ctx->tune_sweep_U == 8 ? 8 : nq == 2 ? 16 : 8;  // (csmp_tune: measurement override)
        for (int u : {16, 8})
            if (u <= umax && nchunk % u == 0) {
                U = u;
                full = true;
                break;
            }
    }
    lds = fr_sweep_lds_bytes(ctx->Mv, vec, U, nq);
    const int cus = ctx->prop.multiProcessorCount;
    int64_t g = U == 16 ? (int64_t)cus * (nq == 2 ? 15 : 12) / 16 : (int64_t)cus;  // (nq < 2 with 16-chunk blocks: as the OMP sweep, configure_sweep)
    if (ctx->tune_sweep_grid > 0) g = std::min<int64_t>(ctx->tune_sweep_grid, (int64_t)cus * 8);
    const int64_t groups = (ctx->N + (kSweepThreads / kWave) - 1) / (kSweepThreads / kWave);
    grid = (int)std::max<int64_t>(1, std::min<int64_t>(g, groups));
}

// A column whose LDS images (the residual and up to two directions: 24 M bytes) exceed the LDS takes the tall path: the same pass
// as separate launches (csmp_forward.hpp, k_fr_combine)
static bool fr_tall(const csmp_ctx* ctx, int nq) {
    int U, grid; bool full; size_t lds;
    fr_config(ctx, nq, U, full, lds, grid);
    return lds > 160 * 1024 - 512;
}
static int fr_combine_grid(const csmp_ctx* ctx) {  // (its partials land in pval / pidx: cus * 8 + 8 entries, solver_alloc)
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(2048, ctx->prop.multiProcessorCount * 8 + 8), (ctx->N + 255) / 256));
}

static int fr_ensure(csmp_ctx* ctx) {
    Solver& s = ctx->s;
    int U; bool full; size_t lds;
    fr_config(ctx, 1, U, full, lds, s.fr_grid);
    if (fr_tall(ctx, 2)) {  // (some pass of some solver on this dictionary will take the tall path: srr's two directions at the latest)
        if (!s.frg1) CHECK(dmalloc(ctx, &s.frg1, (size_t)ctx->N));
        if (!s.frg2) CHECK(dmalloc(ctx, &s.frg2, (size_t)ctx->N));
        if (!s.frq) CHECK(dmalloc(ctx, &s.frq, (size_t)s.Mpad));
    }
    if (!s.rho2) CHECK(dmalloc(ctx, &s.rho2, (size_t)ctx->N));
    if (!s.dvec) CHECK(dmalloc(ctx, &s.dvec, (size_t)ctx->N));
    return CSMP_OK;
}

// forward_δ! on a tall dictionary: g = A'q per direction and c = A'r by the product sweep, then k_fr_combine
static int launch_fr_pass_tall(csmp_ctx* ctx, const FrPass& ps, double max_eps, int skipmask) {
    Solver& s = ctx->s;
    const int M = (int)ctx->M;
    if (ps.nq >= 1) {
        const double* q1 = ps.q1;
        if (!q1) {
            hipLaunchKernelGGL(k_fr_lastq, dim3((s.Mpad + 255) / 256), dim3(256), 0, ctx->stream, (const double*)s.Q, s.ldq, (const DevState*)s.st, s.Mpad, M, s.frq);
            HIPCHECK(hipGetLastError());
            q1 = s.frq;
        }
        CHECK(launch_sweep(ctx, q1, 0.0, 0, skipmask, s.frg1));
    }
    if (ps.nq == 2) CHECK(launch_sweep(ctx, ps.q2, 0.0, 0, skipmask, s.frg2));
    if (ps.nq < 0) {
        const unsigned grid = (unsigned)((ctx->N + 3) / 4);
        if (ctx->dtype == CSMP_F32)
            hipLaunchKernelGGL(k_fr_colnorm2<float>, dim3(grid), dim3(256), 0, ctx->stream, (const float*)ctx->dA, ctx->ld, M, ctx->N, s.frg1);
        else
            hipLaunchKernelGGL(k_fr_colnorm2<double>, dim3(grid), dim3(256), 0, ctx->stream, (const double*)ctx->dA, ctx->ld, M, ctx->N, s.frg1);
        HIPCHECK(hipGetLastError());
    }
    CHECK(launch_sweep(ctx, s.r, 0.0, 0, skipmask));  // (last: the sweep's prologue leaves ||r||^2 in the control block)
    const dim3 grid((unsigned)fr_combine_grid(ctx));
    s.fr_grid = (int)grid.x;  // (the arg-max partials the append reads are k_fr_combine's)
#define FR_COMBINE(NQ)                                                                                                                      \
    hipLaunchKernelGGL(k_fr_combine<NQ>, grid, dim3(256), 0, ctx->stream, ctx->N, (const double*)s.cvec, (const double*)s.frg1, ps.s1,       \
                       (const double*)s.frg2, ps.s2, ps.unmark, ps.update_only, s.rho2, s.dvec, s.pval, s.pidx, (const int*)s.sel, s.st, max_eps, \
                       skipmask)
    switch (ps.nq) {
        case -1: FR_COMBINE(-1); break;
        case 0: FR_COMBINE(0); break;
        case 1: FR_COMBINE(1); break;
        default: FR_COMBINE(2); break;
    }
#undef FR_COMBINE
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// forward_δ! + the residual-norm guard of forward_step! (src/forward.jl:59-61,75-82)
static int launch_fr_pass(csmp_ctx* ctx, const FrPass& ps, double max_eps, int skipmask) {
    if (fr_tall(ctx, ps.nq)) return launch_fr_pass_tall(ctx, ps, max_eps, skipmask);
    int U, grid; bool full; size_t lds;
    fr_config(ctx, ps.nq, U, full, lds, grid);
    ctx->s.fr_grid = grid;  // (the partials of THIS pass: a dictionary near the LDS limit mixes fused and tall passes)
    const bool timed = !ps.update_only && prof_pick(ctx);
    if (timed) CHECK(prof_mark(ctx));
    hipError_t e = ctx->dtype == CSMP_F32 ? fr_sweep_launch<float>(ctx, ps, U, full, grid, lds, max_eps, skipmask)
                                          : fr_sweep_launch<double>(ctx, ps, U, full, grid, lds, max_eps, skipmask);
    HIPCHECK(e);
    if (timed) CHECK(prof_mark(ctx));
    return CSMP_OK;
}
static int launch_fr_sweep(csmp_ctx* ctx, bool first, double max_eps, int skipmask) {
    FrPass ps;
    ps.nq = first ? -1 : 1;
    return launch_fr_pass(ctx, ps, max_eps, skipmask);
}

// forward_step!(P, x, max_ε, min_δ): src/forward.jl:56-73
static int fr_step(csmp_ctx* ctx, bool first, double max_eps, double min_d2, bool optimistic) {
    const int skip = STOP_EPS | STOP_STAG | STOP_FULL | STOP_REORTH;
    CHECK(launch_fr_sweep(ctx, first, max_eps, skip));
    return launch_append(ctx, 3, 0, skip, optimistic, min_d2, ctx->s.fr_grid);
}

// One tick of a pipeline of three forward-regression signals (tick_pipe_launch, host/omp.hpp, with the OLS sweep: k_tick_fr,
// the qr1 stage in mode 3)
template <typename TA, int U, int NQ>
static hipError_t tick_fr_launch_t(csmp_ctx* ctx, const TickFr<TA>& sw, const TickQr1<TA>& q1, const TickQr2& q2, int G, size_t lds,
                                   double min_d2) {
    auto kern = k_tick_fr<TA, U, NQ>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(2 * G + sw.nblk), dim3(kSweepThreads), lds, ctx->stream, sw, q1, q2, G, min_d2);
    return hipGetLastError();
}
template <typename TA>
static int fr_pipe_launch(Pipe& fp, int64_t n) {
    csmp_ctx* ctx = fp.ctx;
    const int skip = STOP_EPS | STOP_STAG | STOP_FULL | STOP_REORTH;
    const TickStages t = tick_stages(n, fp.k, fp.size);
    if (!t.az && !t.ay && !t.ax) return CSMP_OK;
    Solver &z = *slot_ptr(ctx, t.z), &y = *slot_ptr(ctx, t.y), &x = *slot_ptr(ctx, t.x);
    const int G = ctx->s.G;
    const int jh1 = t.ay ? qr1_advance(y) : 0;
    TickFr<TA> sw;
    sw.A = (const TA*)ctx->dA; sw.ld = ctx->ld; sw.Mv = ctx->Mv; sw.N = ctx->N;
    sw.r = z.r; sw.Q = z.Q; sw.ldq = z.ldq; sw.rho2 = z.rho2; sw.dvec = z.dvec; sw.pval = z.pval; sw.pidx = z.pidx;
    sw.sel = z.sel; sw.st = z.st; sw.max_eps = fp.eps; sw.skipmask = skip; sw.nblk = fp.nblk; sw.active = t.az ? 1 : 0;
    auto q1 = tick_qr1_params<TA>(ctx, y, skip, fp.nblk, jh1, t.ay ? 1 : 0);
    q1.mode = 3;
    const auto q2 = tick_qr2_params(ctx, x, x.jh_last, 1, t.ax ? 1 : 0);
    const double d2 = fp.min_d2;
    const bool timed = t.az && t.ay && t.ax && prof_pick(ctx);
    if (timed) CHECK(prof_mark(ctx));
    const hipError_t e = fp.U == 16 ? (t.tz == 0 ? tick_fr_launch_t<TA, 16, -1>(ctx, sw, q1, q2, G, fp.lds, d2) : tick_fr_launch_t<TA, 16, 1>(ctx, sw, q1, q2, G, fp.lds, d2))
                                    : (t.tz == 0 ? tick_fr_launch_t<TA, 8, -1>(ctx, sw, q1, q2, G, fp.lds, d2) : tick_fr_launch_t<TA, 8, 1>(ctx, sw, q1, q2, G, fp.lds, d2));
    HIPCHECK(e);
    if (timed) CHECK(prof_mark(ctx));
    return CSMP_OK;
}
// fr(A, b, max_ε, min_δ, k) = ols = oomp = ormp, x starting empty: src/forward.jl:44-54
extern "C" int csmp_fr(csmp_ctx* ctx, const void* b, int b_dtype, int64_t k, double max_eps, double min_delta, int64_t* idx,
                       double* val, int64_t* nnz, int64_t* order) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || k < 0) return fail(ctx, CSMP_EINVAL, "fr: b == NULL or k < 0");
    if (max_eps != max_eps || min_delta != min_delta) return fail(ctx, CSMP_EINVAL, "fr: max_eps / min_delta is NaN");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    HIPCHECK(hipSetDevice(ctx->dev));
    const int kc = (int)std::max<int64_t>(1, std::min<int64_t>(k, ctx->M));
    CHECK(solver_ensure(ctx, kc, (int)std::max<int64_t>(k, 1)));
    CHECK(fr_ensure(ctx));
    ctx->s.begun = false;
    const double min_d2 = min_delta * min_delta;  // :64
    for (int pass = 0; pass < 2; ++pass) {  // optimistic append chain, repeated with re-orthogonalisation if flagged (see csmp_omp)
        const bool optimistic = pass == 0;
        CHECK(upload_b(ctx, b, b_dtype));
        for (int64_t t = 0; t < k; ++t) {
            CHECK(fr_step(ctx, t == 0, max_eps, min_d2, optimistic));
            if ((t + 1) % kPollSteps == 0 && t + 1 < k) {
                bool stopped = false;
                CHECK(solver_poll(ctx, &stopped));
                if (stopped) break;
            }
        }
        CHECK(launch_finish(ctx, ctx->s.out_idx, ctx->s.out_val, ctx->s.out_nnz, ctx->s.out_order, ctx->s.outcap));
        DevState hs;
        HIPCHECK(hipMemcpyAsync(&hs, ctx->s.st, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        if (!(hs.done & STOP_REORTH)) {
            break;
        }
    }
    CHECK(download_result(ctx, ctx->s.outcap, idx, val, nnz, order));
    return CSMP_OK;
}

// ------------------------------------------------------------------------------------------ omp / fr batch
// Optimistic two-kernel append chains for every signal, no host synchronisation.  Signals are taken three at a time through the
// tick kernel (k_tick): one launch per atom carries the sweep of one signal and the two short append stages of the other two, so
// the latency-bound chain is hidden underneath the HBM-bound sweep.  Bit-identical to the one-at-a-time path.
static BatchSchedule batch_schedule(const csmp_ctx* ctx, bool isfr, int64_t nsig, int kc) {
    // (the tick kernel carries the LDS form of the append stages: supports beyond qr_max_cols() go one signal at a time through
    // launch_append, whose spill kernels have no such bound)
    if (!ctx->pipeline || nsig < 2 || kc > qr_max_cols()) return BatchSchedule::Signals;
    if (isfr) {  // the tick kernel exists for the exact-tiling FR sweeps only
        int U, g; bool full; size_t l;
        fr_config(ctx, 1, U, full, l, g);
        if (!full || fr_tall(ctx, 1)) return BatchSchedule::Signals;
    }
    // TWO pipelines: the second half of the triples runs on a twin context and stream beside the first.  The sweeps of the two then
    // share the HBM, out of step with one another: the last workgroups of one tick, its launch boundary and the staging of its
    // residual image fall under the other pipeline's stream instead of leaving the memory system idle (DESIGN.md section 0, round 6:
    // 6.03e3 -> 6.46e3 atoms/s with 192 sweep workgroups each).
    // From two signals on and where batch_two_pipelines (host/batch_io.hpp) says so: by size, or as csmp_tune(CSMP_TUNE_PIPELINES) asks.
    // (forward regression too: its ticks under the same LDS request -- one workgroup per CU -- 6.28e3 -> 6.57e3 atoms/s at the benchmark
    // shape; without the request 6.47e3.  With the sweep body as round 5 left it the same pairing had measured 5.99e3 against 5.96e3.)
    constexpr int64_t kPairMinSignals = 2;
    if (nsig < kPairMinSignals || !batch_two_pipelines(ctx)) return BatchSchedule::One;
    // GROUPED (omp only): each pipeline's three slots become three groups of up to sweep_group signals whose sweeps share one pass over
    // A (group_pipe_launch).  csmp_tune(CSMP_TUNE_PIPELINES, 3) forces it; automatic wherever two pipelines run and a pass serves two or
    // more signals.  Supports beyond qr_max_cols(), screened sweeps (csmp_omp_batch) and fr keep the schedules above.
    if (!isfr && ctx->sweep_group >= 1 && (ctx->tune_pipelines == 3 || (ctx->tune_pipelines == 0 && ctx->sweep_group >= 2)))
        return BatchSchedule::Grouped;
    return BatchSchedule::Pairs;
}

constexpr int kPairLdsKiB = 81;  // dynamic LDS of a tick of two pipelines side by side: more than half a CU's 160 KiB = one workgroup per CU
// A pipeline of a round on context c: its groups, its sweep grid and its LDS requests
static void pipe_begin(Pipe& p, csmp_ctx* c, const PlanGroup g[3], RoundForm form, bool isfr, int64_t k, double eps, double min_d2) {
    p.ctx = c;
    for (int q = 0; q < 3; ++q) p.size[q] = g[q].size;
    p.k = k;
    p.eps = eps;
    p.min_d2 = min_d2;
    activate_slot(c, 0);
    const size_t qr_lds = qr_lds_bytes((int)std::min<int64_t>(k, c->s.kcap));  // (jh never exceeds k here)
    // Two pipelines: ONE workgroup per CU (an LDS request above half of the 160 KiB): the workgroups of the two pipelines' launches
    // then QUEUE for the CUs instead of all being resident at once, and the dispatcher hands a CU that a workgroup of one tick has left
    // to the next workgroup in line -- of the other pipeline's tick, whose sweep does not depend on this one.  The chip is never waiting
    // for the slowest workgroups of a launch (they finish 139 ... 160 us into a 157-us sweep), for a launch boundary or for a residual
    // image.
    const size_t excl = form == RoundForm::One ? 0 : (size_t)(c->tune_pair_lds_kib > 0 ? c->tune_pair_lds_kib : kPairLdsKiB) * 1024;
    if (isfr) {
        bool full;
        size_t flds;
        fr_config(c, 1, p.U, full, flds, p.nblk);
        p.lds = std::max({flds, qr_lds, excl});
        return;
    }
    // Measured at 4096 x 65536 f32: 8-chunk load blocks on ONE workgroup per CU (the append stages of the other two signals share
    // those CUs) 160.4 us per tick; 16-chunk blocks on 176 workgroups (11/12 of the stand-alone sweep's optimum of 192) 162.6 us.
    p.nblk = pipe_nblk(c, form == RoundForm::One ? c->tick_grid : form == RoundForm::Grouped && c->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid);  // (tick_grid: configure_sweep)
    if (form == RoundForm::Grouped) {
        p.nblk_wide = wide_nblk(c);
        p.lds = qr_lds;
        p.lds_sweep = excl;
    } else if (form == RoundForm::One || c->tune_pair_split == 1) {  // (pair_split 1, a measurement: the fused tick under the large request)
        p.lds = std::max({c->sweep_lds, qr_lds, excl});
    } else {  // a tick of two pipelines is two launches: the append stages under what THEY need, the sweep one workgroup per CU
        p.lds = qr_lds;
        p.lds_sweep = std::max(c->sweep_lds, excl);
    }
}
// One round of the plan: pipeline A on ctx, in the pair and grouped forms pipeline B on the twin beside it
template <typename TA>
static int run_round(const PlanRound& r, csmp_ctx* ctx, csmp_ctx* tw, bool isfr, int64_t k, double eps, double min_d2) {
    Pipe a, b;
    pipe_begin(a, ctx, r.g[0], r.form, isfr, k, eps, min_d2);
    Pipe* pb = nullptr;
    if (r.form != RoundForm::One) {
        pipe_begin(b, tw, r.g[1], r.form, isfr, k, eps, min_d2);
        pb = &b;
    }
    if (r.form == RoundForm::Grouped) return pipe_ticks<group_pipe_launch<TA>>(a, pb);
    return isfr ? pipe_ticks<fr_pipe_launch<TA>>(a, pb) : pipe_ticks<tick_pipe_launch<TA>>(a, pb);
}

// omp (isfr false: p1 = eps) or fr (isfr true: p1 = max_eps, p2 = min_delta^2) for every column of B
static int batch_impl(csmp_ctx* ctx, BatchIO& io, bool isfr, double eps, double p2) {
    const int64_t nsig = io.nsig, k = io.k;
    HIPCHECK(hipSetDevice(ctx->dev));
    const int kc = (int)std::max<int64_t>(1, std::min<int64_t>(k, ctx->M));
    CHECK(solver_ensure(ctx, kc, (int)k));
    if (isfr) CHECK(fr_ensure(ctx));
    ctx->s.begun = false;
    CHECK(io.stage(false));
    int rc = CSMP_OK;
    activate_slot(ctx, 0);
    if (ctx->s.sigcap < nsig) {
        HIPCHECK(sync_all(ctx));
        dfree(ctx->s.sigflags);
        ctx->s.sigcap = 0;
        CHECK(dmalloc(ctx, &ctx->s.sigflags, (size_t)nsig));
        ctx->s.sigcap = (int)nsig;
    }
    int* const sigflags = ctx->s.sigflags;  // (a pointer VALUE: ctx->s itself is swapped by activate_slot)
    auto init = [&](csmp_ctx* c, int64_t sgn) -> int { return io.init(c, sgn); };  // signal sgn into c's active slot
    auto finish = [&](csmp_ctx* c, int64_t sgn) -> int { return io.emit(c, sgn, sigflags + sgn); };
    auto solve_one = [&](int64_t sgn, bool optimistic) -> int {  // (optimistic false: the exact re-solve, omp_solve_exact's for omp)
        return batch_solve(ctx, io, sgn, sigflags + sgn, [&](int64_t t) {
            return isfr ? fr_step(ctx, t == 0, eps, p2, optimistic) : omp_step(ctx, eps, t > 0, optimistic);
        });
    };
    const BatchSchedule sched = batch_schedule(ctx, isfr, nsig, kc);
    const bool twin = sched == BatchSchedule::Pairs || sched == BatchSchedule::Grouped;
    const int nslots = sched == BatchSchedule::Grouped ? 3 * ctx->sweep_group : 3;
    // wide groups: passes of up to group_wide members where the batch has more signals than a narrow pass serves, on 3 * group_wide slots
    const int nslots_wide = sched == BatchSchedule::Grouped && ctx->group_wide > ctx->sweep_group && nsig > ctx->sweep_group && !ctx->wide_refused ? 3 * ctx->group_wide : 0;
    auto ensure = [&](csmp_ctx* c) -> int {  // c's active slot ready for a chain of this batch
        CHECK(solver_ensure(c, kc, (int)k));
        return isfr ? fr_ensure(c) : CSMP_OK;
    };
    auto run_plan = [&](csmp_ctx* tw, bool wide) -> int {
        // f(context, signal) for every member of a round with its slot active: A's groups, then B's, group by group, member by member
        auto each_member = [&](const PlanRound& r, auto&& f) -> int {
            csmp_ctx* cs[2] = {ctx, tw};
            for (int p = 0; p < 2; ++p)
                for (int g = 0; g < 3; ++g)
                    for (int m = 0; m < r.g[p][g].size; ++m) {
                        activate_slot(cs[p], g + 3 * m);
                        CHECK(twin_rc(ctx, cs[p], f(cs[p], r.g[p][g].first + m)));
                    }
            return CSMP_OK;
        };
        // The end of a round: ONE finish launch per context for all its members (k_finish_group) -- member by member in stream order
        // the single waves ran behind each other, twelve of ~150 us on pipeline A at 18 signals and k = 256, after the last pass.
        // Supports beyond the single-wave form (kcap > 256: launch_finish's block back substitution) keep one launch_finish each.
        auto finish_round = [&](const PlanRound& r) -> int {
            csmp_ctx* cs[2] = {ctx, tw};
            for (int p = 0; p < 2; ++p) {
                if (!cs[p]) continue;
                activate_slot(cs[p], 0);  // (slot_ptr)
                GroupFinish a;
                a.n = 0;
                a.outcap = (int)k;
                bool group = true;
                for (int g = 0; g < 3; ++g)
                    for (int m = 0; m < r.g[p][g].size; ++m) {
                        const Solver& sv = *slot_ptr(cs[p], g + 3 * m);
                        group = group && finish_groupable(sv) && a.n < kFinishGroupMax;
                        if (!group) continue;
                        const int64_t sgn = r.g[p][g].first + m;
                        a.m[a.n++] = io.member(sv, sgn, sigflags + sgn);
                    }
                if (!group) {  // one launch_finish per member, as ever
                    PlanRound own = r;
                    for (int g = 0; g < 3; ++g) own.g[1 - p][g].size = 0;
                    CHECK(each_member(own, finish));
                } else if (a.n > 0) {
                    CHECK(twin_rc(ctx, cs[p], launch_finish_group(cs[p], a)));
                }
            }
            return CSMP_OK;
        };
        // Wide groups keep the plan's dealing over both pipelines (18 signals: groups 0 and 2 on A, 1 on B).  Measured on the benchmark,
        // atoms/s at 18 / 20 signals, two runs each: 2 + 1 on 256 workgroups 26 087, 26 176 / 27 622, 27 735; three groups on ONE pipeline
        // (csmp_tune group_wide 2) 25 257, 25 071 / 26 958, 27 060 -- its append launches have no other pipeline's sweep to run under.
        const int members = wide ? ctx->group_wide : ctx->sweep_group;
        // ... and end on a group of sweep_group signals, a narrow pass, where that costs no pass more (narrow_last_groups, host/batch_plan.hpp;
        // 18 signals: 8 + 6 + 4, the 8 and the 4 on A, the 6 on B)
        for (const PlanRound& r : batch_plan(nsig, sched, members, wide && ctx->tune_group_wide == 2, wide ? ctx->sweep_group : 0, ctx->tune_group_split)) {
            CHECK(each_member(r, init));
            CHECK(ctx->dtype == CSMP_F32 ? run_round<float>(r, ctx, tw, isfr, k, eps, p2) : run_round<double>(r, ctx, tw, isfr, k, eps, p2));
            CHECK(finish_round(r));
        }
        return CSMP_OK;
    };
    if (sched == BatchSchedule::Signals) {
        for (int64_t sgn = 0; sgn < nsig && rc == CSMP_OK; ++sgn) rc = solve_one(sgn, true);
    } else {
        rc = batch_pipelines(ctx, twin, nslots, nslots_wide, 1, ensure, run_plan);
    }
    // ... then ONE synchronisation: a signal whose support failed the DGKS test (flagged on the
    // device, nothing committed for the failing column) is solved again with the full chain
    if (rc == CSMP_OK) {
        std::vector<int> hf((size_t)nsig);
        HIPCHECK(hipMemcpyAsync(hf.data(), sigflags, (size_t)nsig * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        for (int64_t sgn = 0; sgn < nsig && rc == CSMP_OK; ++sgn)
            if (hf[sgn] & STOP_REORTH) rc = solve_one(sgn, false);
    }
    return io.done(rc);
}

extern "C" int csmp_omp_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k,
                              double eps, int64_t* idx, double* val, int64_t* nnz, int out_loc) {
    if (!ctx) return CSMP_EINVAL;
    if (!(eps >= 0.0)) return fail(ctx, CSMP_EINVAL, "eps has to be non-negative");
    BatchIO io(ctx, B, b_dtype, ldB, nsig, b_loc, k, idx, val, nnz, out_loc);
    CHECK(io.check());
    if (screened_on(ctx) && nsig > 0) return omp_batch_screened(ctx, io, eps);
    return batch_impl(ctx, io, false, eps, 0.0);
}

// fr(A, B[:,s], max_eps, min_delta, k) for every column of B: the forward-regression sweeps of three signals
// at a time are pipelined against one another's append stages exactly like csmp_omp_batch's
extern "C" int csmp_fr_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k,
                             double max_eps, double min_delta, int64_t* idx, double* val, int64_t* nnz, int out_loc) {
    if (!ctx) return CSMP_EINVAL;
    if (max_eps != max_eps || min_delta != min_delta) return fail(ctx, CSMP_EINVAL, "fr_batch: max_eps / min_delta is NaN");
    BatchIO io(ctx, B, b_dtype, ldB, nsig, b_loc, k, idx, val, nnz, out_loc);
    CHECK(io.check());
    return batch_impl(ctx, io, true, max_eps, min_delta * min_delta);
}

// warm start: support/values -> device lists, r = b - A x
static int upload_support(csmp_ctx* ctx, const int64_t* idx0, const double* val0, int64_t nnz0) {
    Solver& s = ctx->s;
    std::vector<int> hi((size_t)nnz0);
    for (int64_t t = 0; t < nnz0; ++t) {
        if (idx0[t] < 0 || idx0[t] >= ctx->N) return fail(ctx, CSMP_ERANGE, "warm start: index out of range");
        hi[t] = (int)idx0[t];
    }
    HIPCHECK(hipMemcpyAsync(s.cands, hi.data(), (size_t)nnz0 * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipMemcpyAsync(s.coef, val0, (size_t)nnz0 * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    const int grid = ((int)ctx->M + 255) / 256;
    if (ctx->dtype == CSMP_F32)
        hipLaunchKernelGGL(k_residual<float>, dim3(grid), dim3(256), 0, ctx->stream, (const float*)ctx->dA, ctx->ld, (int)ctx->M,
                           (const int*)s.cands, (const double*)s.coef, (const int*)nullptr, (int)nnz0, (const double*)s.b, s.r);
    else
        hipLaunchKernelGGL(k_residual<double>, dim3(grid), dim3(256), 0, ctx->stream, (const double*)ctx->dA, ctx->ld, (int)ctx->M,
                           (const int*)s.cands, (const double*)s.coef, (const int*)nullptr, (int)nnz0, (const double*)s.b, s.r);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// MP bookkeeping on the host side of the boundary: the device returns the k (atom, <a,r>) pairs in
// step order; x[i] += d is replayed in that order (same summation order as src/matchingpursuit.jl:29)
static int mp_collect(csmp_ctx* ctx, const int64_t* idx0, const double* val0, int64_t nnz0, int64_t* idx, double* val,
                      int64_t* nnz) {
    Solver& s = ctx->s;
    DevState hs;
    HIPCHECK(hipMemcpyAsync(&hs, s.st, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    const int n = hs.nsel;
    std::vector<int> hsel((size_t)std::max(n, 1));
    std::vector<double> hz((size_t)std::max(n, 1));
    HIPCHECK(hipMemcpy(hsel.data(), s.sel, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hz.data(), s.z, (size_t)n * 8, hipMemcpyDeviceToHost));
    std::vector<std::pair<int64_t, double>> x;
    for (int64_t t = 0; t < nnz0; ++t) x.push_back({idx0[t], val0[t]});
    std::sort(x.begin(), x.end(), [](auto& a, auto& c) { return a.first < c.first; });
    for (int t = 0; t < n; ++t) {
        auto it = std::lower_bound(x.begin(), x.end(), (int64_t)hsel[t], [](auto& a, int64_t v) { return a.first < v; });
        if (it != x.end() && it->first == hsel[t])
            it->second += hz[t];
        else if (hz[t] != 0.0)  // SparseVector setindex! does not store a structural zero
            x.insert(it, {(int64_t)hsel[t], hz[t]});
    }
    for (size_t t = 0; t < x.size(); ++t) {
        if (idx) idx[t] = x[t].first;
        if (val) val[t] = x[t].second;
    }
    if (nnz) *nnz = (int64_t)x.size();
    return CSMP_OK;
}

static int mp_step(csmp_ctx* ctx) {
    Solver& s = ctx->s;
    if (s.jh >= s.kcap) return fail(ctx, CSMP_ERANGE, "mp: more steps than the capacity this solver was begun with");
    s.jh += 1;  // (MP: steps taken; the log of (atom, coefficient) pairs holds kcap of them)
    CHECK(launch_sweep(ctx, ctx->s.r, 0.0, 0, 0));
    CHECK(launch_select(ctx, 0, 0));
    return launch_mp_update(ctx);
}

// One MP solve of k steps on the active slot.  load() puts the signal there (and a warm start's support); it runs again before a
// repeat.  CSMP_OPT_SCREENED_SWEEP: the sweeps read the image, every pick is certified (host/screened.hpp); a solve with an
// uncertified pick is repeated with the exact sweep.  The log of (atom, coefficient) pairs stays on the device: csmp_mp reads it
// with mp_collect, csmp_mp_batch's lone signals with mp_emit (host/mp_batch.hpp).  scr_lone is set for the steps only: it is reset
// before the caller's output step, which launches no pick kernel.
template <typename Load>
static int mp_solve(csmp_ctx* ctx, int64_t k, Load&& load) {
    bool screened = screened_on(ctx);
    if (screened) CHECK(screened_ensure(ctx));
    LoneGuard lone_guard(ctx);  // (one solve at a time)
    for (int attempt = 0; attempt < 2; ++attempt) {
        CHECK(load());
        for (int64_t t = 0; t < k; ++t) {
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
    return CSMP_OK;
}

extern "C" int csmp_mp(csmp_ctx* ctx, const void* b, int b_dtype, int64_t k, const int64_t* idx0, const double* val0,
                       int64_t nnz0, int64_t* idx, double* val, int64_t* nnz) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || k < 0 || nnz0 < 0 || (nnz0 > 0 && (!idx0 || !val0))) return fail(ctx, CSMP_EINVAL, "mp: bad arguments");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    HIPCHECK(hipSetDevice(ctx->dev));
    CHECK(solver_ensure(ctx, (int)std::max<int64_t>(std::max(k, nnz0), 1), 1, false));  // MP keeps no factorisation
    ctx->s.begun = false;
    CHECK(mp_solve(ctx, k, [&]() -> int {
        CHECK(upload_b(ctx, b, b_dtype));
        return nnz0 > 0 ? upload_support(ctx, idx0, val0, nnz0) : CSMP_OK;
    }));
    return mp_collect(ctx, idx0, val0, nnz0, idx, val, nnz);
}
