// host/omp.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// the tick pipeline (three signals in flight), the grouped scheduler with the shared pass of a group (shared_pass_launch: csmp_mp_batch
// launches it too) and the omp driver.
// ------------------------------------------------------------------------------------------ tick kernel (3 signals in flight)
template <typename TA>
static TickSweep<TA> tick_sweep_params(csmp_ctx* ctx, Solver& s, double eps, int check_eps, int skipmask, int nblk, int active) {
    TickSweep<TA> p;
    p.claim = p.claim_next = nullptr;
    p.npools = ctx->claim_pools | (ctx->tune_sweep_dyn << 16);
    if (active && ctx->sweep_dyn) claim_sets(s, p.claim, p.claim_next);
    p.A = (const TA*)ctx->dA; p.ld = ctx->ld; p.Mv = ctx->Mv; p.N = ctx->N;
    p.r = s.r; p.cvec = s.cvec; p.pval = s.pval; p.pidx = s.pidx; p.st = s.st;
    p.eps = eps; p.check_eps = check_eps; p.skipmask = skipmask; p.nblk = nblk; p.active = active; p.KP = ctx->sweep_KP;
    p.pcap = ctx->sweep_pcap;
    return p;
}
template <typename TA>
static TickQr1<TA> tick_qr1_params(csmp_ctx* ctx, const Solver& s, int skipmask, int nblk_sweep, int jh, int active) {
    TickQr1<TA> p;
    p.A = (const TA*)ctx->dA; p.ld = ctx->ld; p.M = (int)ctx->M;
    p.Q = s.Q; p.ldq = s.ldq; p.st = s.st; p.avec = s.avec; p.P1 = s.P1;
    p.G = s.G; p.kcap = s.kcap; p.jpad = qr_jpad(jh); p.mode = 1;
    p.pval = s.pval; p.pidx = s.pidx; p.nblk_sweep = nblk_sweep;
    p.cands = s.cands; p.ncands = s.ncands; p.which = 0; p.sel = s.sel; p.skipmask = skipmask;
    p.r = s.r; p.P1s = s.P1s; p.jh = jh; p.active = active;
    return p;
}
static TickQr2 tick_qr2_params(csmp_ctx* ctx, const Solver& s, int jh, int optimistic, int active) {
    TickQr2 p;
    p.Q = s.Q; p.ldq = s.ldq; p.st = s.st; p.avec = s.avec; p.r = s.r;
    p.P1 = s.P1; p.P1s = s.P1s; p.G = s.G;
    p.W1 = s.W1; p.vvec = s.vvec; p.P2 = s.P2; p.P2s = s.P2s; p.R = s.R; p.z = s.z; p.sel = s.sel;
    p.kcap = s.kcap; p.jpad = qr_jpad(jh); p.force_reorth = 0; p.jh = jh; p.optimistic = optimistic;
    p.active = active;
    return p;
}

template <typename TA, int U, bool PH, bool STEADY = false, bool DYN = false>
static hipError_t tick_launch_t(csmp_ctx* ctx, const TickSweep<TA>& sw, const TickQr1<TA>& q1, const TickQr2& q2, int G, size_t lds) {
    auto kern = k_tick<TA, U, PH, STEADY, DYN>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(2 * G + sw.nblk), dim3(DYN ? kSweepDynThreads : kSweepThreads), lds, ctx->stream, sw, q1, q2, G, ctx->tick_sweep_first ? 1 : 0);
    return hipGetLastError();
}
// steady: all three stages of this tick are live (the launches the bench's roofline is quoted on)
template <typename TA, int U, bool PH, bool DYN = false>
static hipError_t tick_launch_s(csmp_ctx* ctx, const TickSweep<TA>& sw, const TickQr1<TA>& q1, const TickQr2& q2, int G, size_t lds, bool steady) {
    return steady ? tick_launch_t<TA, U, PH, true, DYN>(ctx, sw, q1, q2, G, lds) : tick_launch_t<TA, U, PH, false, DYN>(ctx, sw, q1, q2, G, lds);
}
template <typename TA>
static hipError_t tick_launch(csmp_ctx* ctx, const TickSweep<TA>& sw, const TickQr1<TA>& q1, const TickQr2& q2, int G, size_t lds, bool steady) {
    if (ctx->sweep_ph) return tick_launch_s<TA, 8, true>(ctx, sw, q1, q2, G, lds, steady);
    if (ctx->sweep_dyn) {
        switch (ctx->sweep_U) {
            case 16: return tick_launch_s<TA, 16, false, true>(ctx, sw, q1, q2, G, lds, steady);
            case 8: return tick_launch_s<TA, 8, false, true>(ctx, sw, q1, q2, G, lds, steady);
            default: return tick_launch_s<TA, 4, false, true>(ctx, sw, q1, q2, G, lds, steady);
        }
    }
    switch (ctx->sweep_U) {
        case 16: return tick_launch_s<TA, 16, false>(ctx, sw, q1, q2, G, lds, steady);
        case 8: return tick_launch_s<TA, 8, false>(ctx, sw, q1, q2, G, lds, steady);
        default: return tick_launch_s<TA, 4, false>(ctx, sw, q1, q2, G, lds, steady);
    }
}

// ------------------------------------------------------------------------------------------ batch pipelines (host/batch_plan.hpp)
// One pipeline of a batch round (batch_impl, host/forward.hpp): its context, with slot 0 active, the sizes of its three groups
// (member m of group g is solver slot g + 3 m) and what its launches ask for (pipe_begin).  The chains of a batch are optimistic:
// batch_impl solves a signal that failed the DGKS test again, alone.
struct Pipe {
    csmp_ctx* ctx = nullptr;
    int size[3] = {0, 0, 0};
    int64_t k = 0;
    double eps = 0.0;     // omp's eps, fr's max_eps
    double min_d2 = 0.0;  // (fr)
    int nblk = 0;         // sweep workgroups
    int nblk_wide = 0;    // workgroups of a wide pass (groups of more than kGroupMax members): a multiple of 16, nblk_wide / 2 column streams
    int U = 8;            // (fr: the sweep's block size)
    size_t lds = 0;       // the request of the launch that carries the append stages (and the sweep, where lds_sweep == 0)
    size_t lds_sweep = 0; // > 0: the sweep is a launch of its own and asks for at least this
};
static Solver* slot_ptr(csmp_ctx* ctx, int q) { return q == 0 ? &ctx->s : &ctx->park[q]; }
// the qr1 stage takes the next column of the solver's factorisation: its column count, kept for the qr2 stage of the next tick
static int qr1_advance(Solver& s) {
    const int jh = std::min(s.jh, s.kcap);
    s.jh_last = jh;
    if (s.jh < s.kcap) s.jh += 1;
    return jh;
}
// the sweep workgroups of a pipeline launched on `grid`: a csmp_tune override first, never more than the column groups of A nor
// than the arg-max partials hold (pval / pidx: solver_alloc)
static int pipe_nblk(const csmp_ctx* ctx, int64_t grid) {
    const int64_t groups = (ctx->N + (kSweepThreads / kWave) - 1) / (kSweepThreads / kWave);
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ctx->tick_nblk > 0 ? ctx->tick_nblk : grid, groups),
                                                      ctx->prop.multiProcessorCount * 8 + 8));
}
// the workgroups of a wide pass: kWideTickGrid or the csmp_tune override, under pipe_nblk's limits, rounded down to a multiple of 16
static int wide_nblk(const csmp_ctx* ctx) { return std::max(16, pipe_nblk(ctx, kWideTickGrid) / 16 * 16); }

// one tick of a pipeline of three signals (k_tick): the sweep of one, the qr1 and qr2 stages of the other two
template <typename TA>
static int tick_pipe_launch(Pipe& tp, int64_t n) {
    csmp_ctx* ctx = tp.ctx;
    const int skip = STOP_EPS | STOP_STAG | STOP_FULL | STOP_REORTH;
    const TickStages t = tick_stages(n, tp.k, tp.size);
    if (!t.az && !t.ay && !t.ax) return CSMP_OK;
    Solver &z = *slot_ptr(ctx, t.z), &y = *slot_ptr(ctx, t.y), &x = *slot_ptr(ctx, t.x);
    const int G = ctx->s.G;
    const int jh1 = t.ay ? qr1_advance(y) : 0;
    const auto sw = tick_sweep_params<TA>(ctx, z, tp.eps, t.tz > 0 ? 1 : 0, skip, tp.nblk, t.az ? 1 : 0);
    const auto q1 = tick_qr1_params<TA>(ctx, y, skip, tp.nblk, jh1, t.ay ? 1 : 0);
    const auto q2 = tick_qr2_params(ctx, x, x.jh_last, 1, t.ax ? 1 : 0);
    // steady: all three stages live (one pipeline: the launches the roofline is quoted on).  Two pipelines: a tick's sweep is a
    // launch of its own, the same work whatever the other stages do -- every one of them counts, the fill and drain ticks' too
    const bool steady = tp.lds_sweep > 0 ? t.az : (t.az && t.ay && t.ax);
    const bool timed = steady && prof_pick(ctx);
    if (tp.lds_sweep > 0) {
        // the append stages first, in a launch of their own that asks for what they need (it shares the CUs with the OTHER pipeline's
        // sweep), then the sweep alone with the large LDS request that keeps its workgroups one to a CU (pipe_begin)
        if (t.ay || t.ax) {
            auto sw0 = sw;
            sw0.active = 0;
            sw0.nblk = 0;
            HIPCHECK(tick_launch<TA>(ctx, sw0, q1, q2, G, tp.lds, false));
        }
        if (t.az) {
            auto q10 = q1;
            auto q20 = q2;
            q10.active = 0;
            q20.active = 0;
            if (timed) CHECK(prof_mark(ctx));
            HIPCHECK(tick_launch<TA>(ctx, sw, q10, q20, 0, tp.lds_sweep, steady));
            if (timed) CHECK(prof_mark(ctx));
        }
        return CSMP_OK;
    }
    if (timed) CHECK(prof_mark(ctx));
    HIPCHECK(tick_launch<TA>(ctx, sw, q1, q2, G, tp.lds, steady));
    if (timed) CHECK(prof_mark(ctx));
    return CSMP_OK;
}

// ------------------------------------------------------------------------------------------ grouped scheduler (shared sweeps)
// The rotation of tick_pipe_launch with three GROUPS of up to ctx->sweep_group signals in place of three signals: at tick n the
// members of the sweep group sweep in ONE launch that reads A once for all of them (k_sweep_multi), and the k_qr1 stages of one group
// and the k_qr2 stages of another run in ONE append launch (k_append_group), small enough to share the CUs with the other pipeline's
// sweep.  Every signal's own chain -- sweep, qr1, qr2 in three consecutive ticks -- is the one tick_pipe_launch runs, so every
// signal gets the same bits.
template <typename TA, int U, int R>
static hipError_t multi_launch_t(csmp_ctx* ctx, const MultiSweep<TA>& p, size_t lds) {
    constexpr bool w4 = Vec<TA>::n == 2;  // Float64: round 7's four-wave body (csmp_kernels.hpp)
    auto kern = [] {
        if constexpr (w4) return k_sweep_multi_w4<TA, U, R>;
        else return k_sweep_multi<TA, 4, R>;
    }();
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(w4 ? kSweepThreads : kMultiThreads), lds, ctx->stream, p);
    return hipGetLastError();
}
template <typename TA, int U>
static hipError_t multi_launch_u(csmp_ctx* ctx, const MultiSweep<TA>& p, size_t lds) {
    switch (p.n) {
        case 1: return multi_launch_t<TA, U, 1>(ctx, p, lds);
        case 2: return multi_launch_t<TA, U, 2>(ctx, p, lds);
        case 3: return multi_launch_t<TA, U, 3>(ctx, p, lds);
        default: return multi_launch_t<TA, U, 4>(ctx, p, lds);
    }
}
// The wide pass (k_sweep_wide, Float32): p.n + p.n1 members on p.nblk workgroups, a multiple of 16; R is the larger half, p.n.
// nt: the ring's loads nontemporal; kWideNt is what the scheduler runs.  Default-policy loads: a nontemporal load gives up the reuse
// the second half lives on (csmp_bench_sweep variants 2 / 3 against 1, 4096 x 65536 f32, grid 256, a narrow pass = 1: 4 + 4 members
// nt 1.58, default 1.33; 3 + 3 members nt 1.54, default 1.23 -- profiles/r09_wide_sweep.txt).
template <typename TA, bool NT>
static hipError_t wide_launch_nt(csmp_ctx* ctx, const MultiSweep<TA>& p, size_t lds) {
    if constexpr (Vec<TA>::n == 2) return hipErrorInvalidValue;  // (Float64 dictionaries keep groups of kGroupMax)
    else {
        auto go = [&](auto kern) {
            if (lds > 64 * 1024) {
                hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) return e;
            }
            hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(kMultiThreads), lds, ctx->stream, p);
            return hipGetLastError();
        };
        if (p.nblk < 16 || p.nblk % 16 != 0 || p.n1 < 1 || p.n1 > p.n || p.n > kGroupMax) return hipErrorInvalidValue;
        switch (p.n) {
            case 1: return go(k_sweep_wide<TA, 4, 1, NT>);
            case 2: return go(k_sweep_wide<TA, 4, 2, NT>);
            case 3: return go(k_sweep_wide<TA, 4, 3, NT>);
            default: return go(k_sweep_wide<TA, 4, 4, NT>);
        }
    }
}
constexpr bool kWideNt = false;
template <typename TA>
static hipError_t wide_launch(csmp_ctx* ctx, const MultiSweep<TA>& p, size_t lds, bool nt = kWideNt) {
    return nt ? wide_launch_nt<TA, true>(ctx, p, lds) : wide_launch_nt<TA, false>(ctx, p, lds);
}
// what a pass reads and writes of ONE member: its residual, where its c goes, its arg-max partials, its control block
struct PassMember {
    const double* r; double* cvec; double* pval; int* pidx; DevState* st;
};
static PassMember slot_member(csmp_ctx* ctx, int q) {
    const Solver& s = *slot_ptr(ctx, q);
    return PassMember{s.r, s.cvec, s.pval, s.pidx, s.st};
}
// the `size` members member(0), member(1), ... as a pass's entries: up to kGroupMax of them the narrow pass's [0, n); more, the wide
// pass's halves [0, n) and [kGroupMax, kGroupMax + n1).  Entries past a half's members repeat its last one (the narrow pass never
// reads them; the wide pass stages their image and masks them).  need_c false: EVERY cvec entry null -- the pass stages and stores
// no c (sweep_body_multi, sweep_body_multi_w4).
template <typename TA, typename Member>
static void multi_members_of(MultiSweep<TA>& p, int size, bool need_c, Member&& member) {
    const bool wide = size > kGroupMax;
    p.n = wide ? (size + 1) / 2 : size;
    p.n1 = wide ? size / 2 : 0;
    for (int e = 0; e < kWideMax; ++e) {
        const int h = e / kGroupMax, i = e % kGroupMax;
        const int m = h == 0 || !wide ? std::min(i, p.n - 1) : p.n + std::min(i, p.n1 - 1);
        const PassMember s = member(m);
        p.r[e] = s.r; p.cvec[e] = need_c ? s.cvec : nullptr; p.pval[e] = s.pval; p.pidx[e] = s.pidx; p.st[e] = s.st;
    }
}
// the schedulers' members: [first, first + size) step 3 of the slots from slot0
template <typename TA>
static void multi_members(csmp_ctx* ctx, MultiSweep<TA>& p, int slot0, int size, bool need_c) {
    multi_members_of<TA>(p, size, need_c, [&](int m) { return slot_member(ctx, slot0 + 3 * m); });
}
// Float32: the 512-thread pair body, whose unit is its own (4 loads per column); Float64: the four-wave body on ctx->sweep_U
template <typename TA>
static hipError_t multi_launch(csmp_ctx* ctx, const MultiSweep<TA>& p, size_t lds) {
    if constexpr (Vec<TA>::n == 2) {
        switch (ctx->sweep_U) {
            case 16: return multi_launch_u<TA, 16>(ctx, p, lds);
            case 8: return multi_launch_u<TA, 8>(ctx, p, lds);
            default: return multi_launch_u<TA, 4>(ctx, p, lds);
        }
    }
    return multi_launch_u<TA, 4>(ctx, p, lds);
}
// The shared pass of a group: the `size` members in the slots slot0, slot0 + 3, ... sweep in ONE launch that reads A once for all of
// them -- the narrow pass on nblk workgroups, for more than kGroupMax members (more than a workgroup has images) the wide pass on
// nblk_wide, two workgroups per read of A -- under an LDS request of at least lds_sweep.  group_pipe_launch's sweep stage and a
// step of csmp_mp_batch's groups (mp_group_step, host/mp_batch.hpp).  need_c: the pass writes every member's c = A'r to its slot's
// cvec.  k_mp_group reads c there; the grouped OMP scheduler's append stage (k_append_group: qr1_body) takes its atom from the
// pass's partials and k_finish_group reads R, z and the selection, so its passes store none (2.4 GB a call of 18 signals, k = 256, at
// N = 65536) unless csmp_tune pass_c asks for them.  shared_pass_launch_of: the same launch for members that live elsewhere
// (csmp_somp's columns, host/somp.hpp).
template <typename TA, typename Member>
static int shared_pass_launch_of(csmp_ctx* ctx, int size, double eps, int check_eps, int skipmask, int nblk, int nblk_wide, size_t lds_sweep,
                                 bool need_c, Member&& member) {
    MultiSweep<TA> p;
    p.A = (const TA*)ctx->dA; p.ld = ctx->ld; p.Mv = ctx->Mv; p.N = ctx->N;
    const bool wide = size > kGroupMax;
    p.eps = eps; p.check_eps = check_eps; p.skipmask = skipmask; p.nblk = wide ? nblk_wide : nblk; p.KP = ctx->sweep_KP;
    multi_members_of<TA>(p, size, need_c, member);
    // ONE sampled launch per shared pass: it reads A once, whatever the group size
    const bool timed = prof_pick(ctx);
    if (timed) CHECK(prof_mark(ctx));
    const size_t lds = std::max(sweep_multi_lds_bytes(p.KP, p.n), lds_sweep);
    HIPCHECK(wide ? wide_launch<TA>(ctx, p, lds) : multi_launch<TA>(ctx, p, lds));
    if (timed) CHECK(prof_mark(ctx));
    return CSMP_OK;
}
template <typename TA>
static int shared_pass_launch(csmp_ctx* ctx, int slot0, int size, double eps, int check_eps, int skipmask, int nblk, int nblk_wide,
                              size_t lds_sweep, bool need_c) {
    return shared_pass_launch_of<TA>(ctx, size, eps, check_eps, skipmask, nblk, nblk_wide, lds_sweep, need_c,
                                     [&](int m) { return slot_member(ctx, slot0 + 3 * m); });
}
template <typename TA>
static int group_pipe_launch(Pipe& gp, int64_t n) {
    csmp_ctx* ctx = gp.ctx;
    const int skip = STOP_EPS | STOP_STAG | STOP_FULL | STOP_REORTH;
    const TickStages t = tick_stages(n, gp.k, gp.size);
    if (t.ay || t.ax) {
        GroupAppend<TA> a;
        a.n2 = t.ax ? gp.size[t.x] : 0;
        a.n1 = t.ay ? gp.size[t.y] : 0;
        for (int m = 0; m < a.n2; ++m) {
            const Solver& s = *slot_ptr(ctx, t.x + 3 * m);
            a.q2[m] = tick_qr2_params(ctx, s, s.jh_last, 1, 1);
        }
        for (int m = 0; m < a.n1; ++m) {
            Solver& s = *slot_ptr(ctx, t.y + 3 * m);
            const int jh1 = qr1_advance(s);
            a.q1[m] = tick_qr1_params<TA>(ctx, s, skip, a.n1 > kGroupMax ? gp.nblk_wide / 2 : gp.nblk, jh1, 1);  // (the sweep's partials: one per stream)
        }
        const int G = ctx->s.G;
        auto kern = k_append_group<TA>;
        if (gp.lds > 64 * 1024) HIPCHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gp.lds));
        hipLaunchKernelGGL(kern, dim3((a.n1 + a.n2) * G), dim3(kSweepThreads), gp.lds, ctx->stream, a, G);
        HIPCHECK(hipGetLastError());
    }
    if (t.az) CHECK(shared_pass_launch<TA>(ctx, t.z, gp.size[t.z], gp.eps, t.tz > 0 ? 1 : 0, skip, gp.nblk, gp.nblk_wide, gp.lds_sweep,
                                          ctx->tune_pass_c == 1));
    return CSMP_OK;
}

// A round's 3k + 2 ticks on one pipeline, or on two side by side (b: the twin's, its own stream) with the launches of every tick
// enqueued A first, then B.  launch: tick_pipe_launch, group_pipe_launch or fr_pipe_launch (host/forward.hpp).
template <int (*launch)(Pipe&, int64_t)>
static int pipe_ticks(Pipe& a, Pipe* b) {
    for (int64_t n = 0; n < 3 * a.k + 2; ++n) {
        CHECK(launch(a, n));
        if (b) CHECK(twin_rc(a.ctx, b->ctx, launch(*b, n)));
    }
    return CSMP_OK;
}

// ------------------------------------------------------------------------------------------ drivers
extern "C" int csmp_omp(csmp_ctx* ctx, const void* b, int b_dtype, int64_t k, double eps, int64_t* idx, double* val,
                        int64_t* nnz, int64_t* order) {
    if (!ctx) return CSMP_EINVAL;
    if (!(eps >= 0.0)) return fail(ctx, CSMP_EINVAL, "eps has to be non-negative");  // src/matchingpursuit.jl:74
    if (!b || k < 0) return fail(ctx, CSMP_EINVAL, "omp: b == NULL or k < 0");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    HIPCHECK(hipSetDevice(ctx->dev));
    const int kc = (int)std::max<int64_t>(1, std::min<int64_t>(k, ctx->M));  // UpdatableQR(T, n, k): :58
    CHECK(solver_ensure(ctx, kc, (int)std::max<int64_t>(k, 1)));
    ctx->s.begun = false;
    // CSMP_OPT_SCREENED_SWEEP: first with the bf16-image sweep + certified picks (csmp_screened.hpp); a solve in which a pick
    // could not be certified is repeated with the exact sweep.
    // Within an attempt: optimistic two-kernel append chain first; if any column failed the DGKS test (flagged on the
    // device, nothing committed) the solve is repeated with the second Gram-Schmidt pass enabled
    bool screened = screened_on(ctx);
    if (screened) CHECK(screened_ensure(ctx));
    LoneGuard lone_guard(ctx);  // (csmp_omp is one solve at a time)
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool uncertain = false;
        for (int pass = 0; pass < 2; ++pass) {
            const bool optimistic = pass == 0;
            CHECK(upload_b(ctx, b, b_dtype));
            for (int64_t t = 0; t < k; ++t) {
                CHECK(screened ? omp_step_screened(ctx, eps, t > 0, optimistic) : omp_step(ctx, eps, t > 0, optimistic));
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
            uncertain = screened && hs.uncertain > 0;
            if (!(hs.done & STOP_REORTH)) {
                break;
            }
        }
        if (screened) {
            ctx->scr_solves += 1;
            ctx->scr_fallbacks += uncertain ? 1 : 0;
        }
        if (!uncertain) break;
        screened = false;
    }
    CHECK(download_result(ctx, ctx->s.outcap, idx, val, nnz, order));
    return CSMP_OK;
}
