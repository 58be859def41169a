// host/ista_batch.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_ista_batch -- csmp_ista for every column of B, the members of a group on shared launches.
// ------------------------------------------------------------------------------------------ ista batch
// An iteration of csmp_ista reads the dictionary once for c = A'r and once more, over the columns of the list, for r = b - A y.  The
// first read is the same for every signal: a GROUP of up to R members (R = group_wide where the batch has more signals than
// sweep_group and wide groups are on, else sweep_group) takes its iterations together, FOUR launches a step whatever the number of
// members, in ista_iterate's order: the group forms of k_ista_axpy and k_ista_resum (csmp_bp.hpp), the shared pass of
// csmp_mp_batch's groups with the members' r as its residuals, and k_ista_update_group.  Every member runs exactly maxiter
// iterations, so there is no plan: the signals are taken in ascending order, R at a time, a remainder forms a narrower group, and
// nothing waits for the device between a group's first launch and its results.  Member m lives in solver slot 3 m (b, r, c, the
// pass's partials and control block) and in its share of IstaBatchBuf (x, y, its weights, the list, the axpy's partials, a norm).
// Every member's arithmetic is csmp_ista's: the pass gives the single sweep's bits per member, the group forms call the single
// kernels' bodies, the FISTA coefficient is the host's Float64 value of the same recurrence, a member starts as ista_solve does: the
// results are csmp_ista's bit for bit.  One pipeline, on the context's own stream; csmp_ista's IstaBuf is left alone.
static int istab_ensure(csmp_ctx* ctx, int R) {
    IstaBatchBuf& t = ctx->istab;
    const int P = ista_parts_max(ctx);
    if (t.xy && t.R >= R && t.N == ctx->N && t.Mv == ctx->Mv && t.P == P) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    istab_free(t);
    IstaBatchBuf n;
    const size_t N = (size_t)ctx->N, Rr = (size_t)R;
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.xy, 2 * N * Rr));
        CHECK(dmalloc(ctx, &n.w, N * Rr));
        CHECK(dmalloc(ctx, &n.lidx, N * Rr));
        CHECK(dmalloc(ctx, &n.lval, N * Rr));
        CHECK(dmalloc(ctx, &n.seg_cnt, (size_t)kIstaMaxSegs * Rr));
        CHECK(dmalloc(ctx, &n.nnz, Rr));
        CHECK(dmalloc(ctx, &n.part, (size_t)P * (size_t)ctx->Mv * Rr));
        CHECK(dmalloc(ctx, &n.nrm, Rr));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        istab_free(n);
        return rc;
    }
    n.R = R;
    n.N = ctx->N;
    n.Mv = ctx->Mv;
    n.P = P;
    t = n;
    return CSMP_OK;
}

// member m's pointers
struct IstabMember {
    double *x, *y, *w, *lval, *part, *nrm;
    int *lidx, *seg_cnt;
    unsigned* nnz;
};
static IstabMember istab_member(const csmp_ctx* ctx, int m) {
    const IstaBatchBuf& t = ctx->istab;
    const size_t N = (size_t)t.N, mm = (size_t)m;
    IstabMember r;
    r.x = t.xy + 2 * N * mm;
    r.y = r.x + N;
    r.w = t.w + N * mm;
    r.lidx = t.lidx + N * mm;
    r.lval = t.lval + N * mm;
    r.seg_cnt = t.seg_cnt + (size_t)kIstaMaxSegs * mm;
    r.nnz = t.nnz + mm;
    r.part = t.part + (size_t)t.P * (size_t)t.Mv * mm;
    r.nrm = t.nrm + mm;
    return r;
}

// bp_pass_members (host/bp_batch.hpp) with the residual where csmp_ista keeps it: member i's solver slot's r is entry i's residual
template <typename TA>
static void ista_pass_members(csmp_ctx* ctx, MultiSweep<TA>& p, int L) {
    const bool wide = L > kGroupMax;
    p.n = wide ? (L + 1) / 2 : L;
    p.n1 = wide ? L / 2 : 0;
    for (int e = 0; e < kWideMax; ++e) {
        const int h = e / kGroupMax, i = e % kGroupMax;
        const int m = h == 0 || !wide ? std::min(i, p.n - 1) : p.n + std::min(i, p.n1 - 1);
        const Solver& s = *slot_ptr(ctx, 3 * m);
        p.r[e] = s.r; p.cvec[e] = s.cvec; p.pval[e] = s.pval; p.pidx[e] = s.pidx; p.st[e] = s.st;
    }
}

// The arguments of one call and the launches of a group: members 0 .. L) of the group are slots 0 .. L)
struct IstaBatchRun {
    csmp_ctx* ctx;
    const char* dB;  // B on the device
    int b_dtype;
    int64_t ldB;
    const double* w;
    int64_t nw, ldw;
    const double* X0;
    int64_t ldX0, maxiter;
    double stepsize;
    int accel;
    double* X;
    int64_t ldX;
    int x_loc;
    double* resnorm;

    int init(int64_t sig) const {  // signal sig into the ACTIVE slot: b, r = b, the control block
        const char* col = dB + (size_t)sig * (size_t)ldB * (b_dtype == CSMP_F32 ? 4 : 8);
        ctx->s.begun = false;
        return b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)col) : init_from_device_t<double>(ctx, (const double*)col);
    }
    hipMemcpyKind out_kind() const { return x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost; }
    hipMemcpyKind in_kind() const { return x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }
    // csmp_ista's own solve of one signal on slot 0 (no shared pass, the screened sweeps, a lone signal)
    int solve_one(int64_t sig) const {
        CHECK(init(sig));
        return ista_solve(ctx, w + sig * ldw, nw, X0 ? X0 + sig * ldX0 : nullptr, in_kind(), maxiter, stepsize, accel, X + sig * ldX, x_loc,
                          resnorm ? resnorm + sig : nullptr);
    }

    // r_m = b_m - A[:, list_m] values_m of every member: the group forms of ista_launch_residual
    template <typename TA>
    int residual(const BpGroup& G, int L) const {
        const int M = (int)ctx->M;
        const int64_t seg_len = ista_seg_len(ctx->N);
        const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
        hipLaunchKernelGGL(k_ista_axpy_group<TA>, dim3(ctx->istab.P, ista_row_blocks(ctx), (unsigned)L), dim3(kIstaThreads), 0, ctx->stream,
                           (const TA*)ctx->dA, ctx->ld, ctx->Mv, nseg, seg_len, G);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(k_ista_resum_group, dim3((M + kWave - 1) / kWave, 1, (unsigned)L), dim3(kIstaThreads), 0, ctx->stream, ctx->Mv, M,
                           ctx->istab.P, G);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    int update(const BpGroup& G, const IstaGroupW& W, int L, double alpha, double beta, int flags) const {
        const int64_t seg_len = ista_seg_len(ctx->N);
        const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
        hipLaunchKernelGGL(k_ista_update_group, dim3(nseg, 1, (unsigned)L), dim3(kIstaThreads), 0, ctx->stream, G, W, nw, ctx->N, seg_len, alpha, beta,
                           flags);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    // the shared pass: mp_group_step's grids and LDS request, c = A'r of every member to its slot's cvec
    template <typename TA>
    int pass(int L) const {
        const bool wide = L > kGroupMax;
        MultiSweep<TA> p;
        p.A = (const TA*)ctx->dA; p.ld = ctx->ld; p.Mv = ctx->Mv; p.N = ctx->N;
        p.eps = 0.0; p.check_eps = 0; p.skipmask = 0; p.KP = ctx->sweep_KP;
        p.nblk = wide ? wide_nblk(ctx) : pipe_nblk(ctx, ctx->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid);
        ista_pass_members<TA>(ctx, p, L);
        const size_t excl = (size_t)(ctx->tune_pair_lds_kib > 0 ? ctx->tune_pair_lds_kib : kPairLdsKiB) * 1024;
        const size_t lds = std::max(sweep_multi_lds_bytes(p.KP, p.n), excl);
        HIPCHECK(wide ? wide_launch<TA>(ctx, p, lds) : multi_launch<TA>(ctx, p, lds));
        return CSMP_OK;
    }

    // The signals sig0 .. sig0 + L) from entry to results (slot 0 active on entry and on return)
    template <typename TA>
    int group(int64_t sig0, int L) {
        const size_t nbytes = (size_t)ctx->N * sizeof(double);
        BpGroup G{};
        IstaGroupW W{};
        G.n = L;
        for (int i = 0; i < kBpGroupMax; ++i) {
            const int m = std::min(i, L - 1);
            const IstabMember b = istab_member(ctx, m);
            const Solver& s = *slot_ptr(ctx, 3 * m);
            G.c[i] = s.cvec; G.z[i] = b.x; G.u[i] = b.y; G.lidx[i] = b.lidx; G.seg_cnt[i] = b.seg_cnt; G.lval[i] = b.lval;
            G.part[i] = b.part; G.nnz[i] = b.nnz; G.b[i] = s.b; G.r[i] = s.r;
            W.w[i] = ldw > 0 ? b.w : ctx->istab.w;  // (shared weights: member 0's share, written once per call)
        }
        for (int m = 0; m < L; ++m) {  // as ista_solve starts: b and r = b, the weights, the warm start or x = y = 0
            const int64_t sig = sig0 + m;
            activate_slot(ctx, 3 * m);
            const int rc = init(sig);
            activate_slot(ctx, 0);
            CHECK(rc);
            const IstabMember b = istab_member(ctx, m);
            if (ldw > 0) HIPCHECK(hipMemcpyAsync(b.w, w + sig * ldw, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            if (X0) HIPCHECK(hipMemcpyAsync(b.y, X0 + sig * ldX0, nbytes, in_kind(), ctx->stream));
            else HIPCHECK(hipMemsetAsync(b.x, 0, 2 * nbytes, ctx->stream));  // (y follows x)
        }
        bool listed = false;  // the lists (and r) belong to the current y
        if (X0) {
            CHECK(update(G, W, L, 0.0, 0.0, ISTA_INIT | ISTA_LIST_X));
            listed = true;
        }
        double tk = 1.0;
        for (int64_t it = 1; it <= maxiter; ++it) {  // ista_iterate, four launches a step
            if (listed) CHECK(residual<TA>(G, L));
            CHECK(pass<TA>(L));
            const double tn = (1.0 + std::sqrt(1.0 + 4.0 * tk * tk)) / 2.0;
            const double beta = accel ? (tk - 1.0) / tn : 0.0;
            tk = tn;
            CHECK(update(G, W, L, stepsize, beta, (accel ? ISTA_ACCEL : 0) | (it == maxiter ? ISTA_LIST_X : 0)));
            listed = true;
        }
        // retirement: ||r|| as residual_norm takes it, x to the signal's column, one read of all norms
        if (resnorm && listed) CHECK(residual<TA>(G, L));
        const int M = (int)ctx->M;
        for (int m = 0; m < L; ++m) {
            const IstabMember b = istab_member(ctx, m);
            if (resnorm) hipLaunchKernelGGL(k_norm2, dim3(1), dim3(256), 0, ctx->stream, (const double*)slot_ptr(ctx, 3 * m)->r, M, b.nrm);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpyAsync(X + (sig0 + m) * ldX, b.x, nbytes, out_kind(), ctx->stream));
        }
        if (resnorm) {
            double nrm[kBpGroupMax] = {};
            PinFetch f(ctx);
            CHECK(f.begin(sizeof nrm));
            CHECK(f.add(nrm, ctx->istab.nrm, (size_t)L * sizeof(double)));
            CHECK(f.wait());
            for (int m = 0; m < L; ++m) resnorm[sig0 + m] = std::sqrt(nrm[m]);
        }
        return CSMP_OK;
    }
};

static int ista_nomem(csmp_ctx* ctx, int rc) {
    if (rc == CSMP_EHIP) return fail(ctx, CSMP_ENOMEM, "ista_batch: no device memory for the iterates (" + ctx->err + ")");
    return rc;
}

extern "C" int csmp_ista_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, const double* w, int64_t nw,
                               int64_t ldw, const double* X0, int64_t ldX0, int64_t maxiter, double stepsize, int accel, double* X, int64_t ldX,
                               int x_loc, double* resnorm) {
    if (!ctx) return CSMP_EINVAL;
    if (nsig < 0) return fail(ctx, CSMP_EINVAL, "ista_batch: nsig has to be non-negative");
    if (!w || (nsig > 0 && (!B || !X))) return fail(ctx, CSMP_EINVAL, "ista_batch: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if ((b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) || (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE))
        return fail(ctx, CSMP_EINVAL, "ista_batch: b_loc / x_loc must be CSMP_HOST or CSMP_DEVICE");
    if (accel != 0 && accel != 1) return fail(ctx, CSMP_EINVAL, "ista_batch: accel must be 0 (ISTA) or 1 (FISTA)");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, "ista_batch: a host-streamed dictionary is not served");
    if (ldB < ctx->M) return fail(ctx, CSMP_EDIM, "ista_batch: ldB < size(A, 1)");
    if (ldX < ctx->N) return fail(ctx, CSMP_EDIM, "ista_batch: ldX < size(A, 2)");
    if (X0 && ldX0 < ctx->N) return fail(ctx, CSMP_EDIM, "ista_batch: ldX0 < size(A, 2)");
    if (nw != 1 && nw != ctx->N) return fail(ctx, CSMP_EDIM, "ista_batch: length(w) must be 1 or size(A, 2)");
    if (ldw < 0 || (ldw > 0 && ldw < nw)) return fail(ctx, CSMP_EINVAL, "ista_batch: ldw must be 0 (shared weights) or at least nw");
    if (maxiter < 0) return fail(ctx, CSMP_EINVAL, "ista_batch: maxiter has to be non-negative");
    if (!std::isfinite(stepsize) || !(stepsize > 0.0)) return fail(ctx, CSMP_EINVAL, "ista_batch: stepsize has to be positive and finite");
    for (int64_t s = 0; s < (ldw > 0 ? nsig : 1); ++s)
        for (int64_t i = 0; i < nw; ++i) {
            const double v = w[s * ldw + i];
            if (!std::isfinite(v) || v < 0.0) return fail(ctx, CSMP_EINVAL, "ista_batch: the weights have to be non-negative and finite");
        }
    if (nsig == 0) return CSMP_OK;
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    // The shared pass where the resident dictionary has one and the sweeps are exact; a lone signal keeps csmp_ista's launches.
    const bool grouped = ctx->pipeline && ctx->sweep_group >= 1 && !screened_on(ctx) && nsig >= 2;
    {
        int rc = solver_ensure(ctx, 1, 1, false);
        if (rc == CSMP_OK && !grouped) rc = ista_ensure(ctx);
        CHECK(ista_nomem(ctx, rc));
    }
    IstaBatchRun run{};
    run.ctx = ctx; run.dB = (const char*)B; run.b_dtype = b_dtype; run.ldB = ldB; run.w = w; run.nw = nw; run.ldw = ldw; run.X0 = X0; run.ldX0 = ldX0;
    run.maxiter = maxiter; run.stepsize = stepsize; run.accel = accel; run.X = X; run.ldX = ldX; run.x_loc = x_loc; run.resnorm = resnorm;
    DevTmp tB;  // a host caller's B on the device
    if (b_loc == CSMP_HOST) {
        const size_t bytes = (size_t)ldB * (size_t)nsig * (b_dtype == CSMP_F32 ? 4 : 8);
        CHECK(ista_nomem(ctx, tB.alloc(ctx, bytes)));
        HIPCHECK(hipMemcpy(tB.p, B, bytes, hipMemcpyHostToDevice));
        run.dB = (const char*)tB.p;
    }
    auto finish = [&](int rc) -> int {
        activate_slot(ctx, 0);
        (void)hipStreamSynchronize(ctx->stream);  // (on every way out: the temporaries and the caller's buffers are at rest)
        return rc;
    };
    if (!grouped) {
        int rc = CSMP_OK;
        for (int64_t s = 0; s < nsig && rc == CSMP_OK; ++s) rc = run.solve_one(s);
        return finish(rc);
    }
    const int wide_members = ctx->group_wide > ctx->sweep_group && nsig > ctx->sweep_group && !ctx->wide_refused ? ctx->group_wide : 0;
    auto ensure = [&](csmp_ctx* c) -> int {
        const int rc = solver_ensure(c, 1, 1, false);
        c->s.begun = false;
        return rc;
    };
    auto enqueue = [&](csmp_ctx*, bool granted) -> int {
        const int R = (int)std::min<int64_t>(granted ? wide_members : ctx->sweep_group, nsig);
        CHECK(istab_ensure(ctx, R));
        if (ldw == 0) HIPCHECK(hipMemcpyAsync(ctx->istab.w, w, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        for (int64_t s0 = 0; s0 < nsig; s0 += R) {
            const int L = (int)std::min<int64_t>(R, nsig - s0);
            CHECK(ctx->dtype == CSMP_F32 ? run.group<float>(s0, L) : run.group<double>(s0, L));
        }
        return CSMP_OK;
    };
    return finish(ista_nomem(ctx, batch_pipelines(ctx, false, ctx->sweep_group, wide_members, 3, ensure, enqueue)));
}
