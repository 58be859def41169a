// host/bp_batch.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_bp_batch -- csmp_bp for every column of B, the members of a group in lockstep on shared launches.
// ------------------------------------------------------------------------------------------ bp batch
// Every byte an iteration of csmp_bp reads in bulk -- the dictionary, R^-1, R^-T, G -- is the same for every signal.  A GROUP of up to
// R members (R = group_wide where the batch has more signals than sweep_group and wide groups are on, else sweep_group) takes its
// iterations together, EIGHT launches a step whatever the number of live members: three k_bp_gemm (one read of each matrix for all
// right-hand sides), the shared pass of csmp_mp_batch's groups with the members' y as its residuals, and the group forms of
// k_bp_update, k_ista_axpy, k_ista_resum, k_bp_pq (csmp_bp.hpp).  Member m lives in solver slot 3 m (b, r, c, the pass's partials
// and control block) and in its share of BpBatchBuf (everything else csmp_bp keeps per solve); G, its factor and the weights are
// csmp_bp's own (bp_prepare).  The members end at different iterations: bp_lockstep (host/bp_batch_plan.hpp) says who runs, who is
// checked -- one read of all res pairs per interval -- and who leaves.  Every member's arithmetic is csmp_bp's: k_bp_gemm repeats
// k_bp_gemv's operations per right-hand side, the pass gives the single sweep's bits per member, the group forms call the single
// kernels' bodies, a slot starts as bp_start does: the results are csmp_bp's bit for bit.  One pipeline, on the context's own stream.
static int bpb_ensure(csmp_ctx* ctx, int R) {
    BpBatchBuf& t = ctx->bpb;
    const int P = ista_parts_max(ctx), Mp = ctx->bp.Mp;
    if (t.zu && t.R >= R && t.N == ctx->N && t.Mv == ctx->Mv && t.P == P && t.Mp == Mp) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    bpb_free(t);
    BpBatchBuf n;
    const size_t N = (size_t)ctx->N, Rr = (size_t)R;
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.zu, 2 * N * Rr));
        CHECK(dmalloc(ctx, &n.lidx, N * Rr));
        CHECK(dmalloc(ctx, &n.lval, N * Rr));
        CHECK(dmalloc(ctx, &n.seg_cnt, (size_t)kIstaMaxSegs * Rr));
        CHECK(dmalloc(ctx, &n.nnz, Rr));
        CHECK(dmalloc(ctx, &n.part, (size_t)P * (size_t)ctx->Mv * Rr));
        CHECK(dmalloc(ctx, &n.vec, (size_t)6 * Mp * Rr));
        CHECK(dmalloc(ctx, &n.rpart, (size_t)2 * kIstaMaxSegs * Rr));
        CHECK(dmalloc(ctx, &n.res, 2 * Rr));
        CHECK(dmalloc(ctx, &n.nrm, Rr));
        HIPCHECK(hipMemsetAsync(n.vec, 0, (size_t)6 * Mp * Rr * sizeof(double), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        bpb_free(n);
        return rc;
    }
    n.R = R;
    n.N = ctx->N;
    n.Mv = ctx->Mv;
    n.P = P;
    n.Mp = Mp;
    t = n;
    return CSMP_OK;
}

// member m's pointers
struct BpbMember {
    double *z, *u, *lval, *part, *rpart, *res, *nrm, *p, *q, *e, *v, *y, *g;
    int *lidx, *seg_cnt;
    unsigned* nnz;
};
static BpbMember bpb_member(const csmp_ctx* ctx, int m) {
    const BpBatchBuf& t = ctx->bpb;
    const size_t N = (size_t)t.N, mm = (size_t)m;
    BpbMember r;
    r.z = t.zu + 2 * N * mm;
    r.u = r.z + N;
    r.lidx = t.lidx + N * mm;
    r.lval = t.lval + N * mm;
    r.seg_cnt = t.seg_cnt + (size_t)kIstaMaxSegs * mm;
    r.nnz = t.nnz + mm;
    r.part = t.part + (size_t)t.P * (size_t)t.Mv * mm;
    double* vec = t.vec + (size_t)6 * t.Mp * mm;
    r.p = vec; r.q = vec + t.Mp; r.e = vec + 2 * t.Mp; r.v = vec + 3 * t.Mp; r.y = vec + 4 * t.Mp; r.g = vec + 5 * t.Mp;
    r.rpart = t.rpart + (size_t)2 * kIstaMaxSegs * mm;
    r.res = t.res + 2 * mm;
    r.nrm = t.nrm + mm;
    return r;
}

static hipError_t bp_gemm_launch(csmp_ctx* ctx, int L, const double* mat, int64_t ld, int M, int mode, const BpGemm& g) {
    const dim3 gv((unsigned)((M + 3) / 4));  // a wave per column
    switch (L) {
        case 1: hipLaunchKernelGGL(k_bp_gemm<1>, gv, dim3(256), 0, ctx->stream, mat, ld, M, mode, g); break;
        case 2: hipLaunchKernelGGL(k_bp_gemm<2>, gv, dim3(256), 0, ctx->stream, mat, ld, M, mode, g); break;
        case 3: hipLaunchKernelGGL(k_bp_gemm<3>, gv, dim3(256), 0, ctx->stream, mat, ld, M, mode, g); break;
        case 4: hipLaunchKernelGGL(k_bp_gemm<4>, gv, dim3(256), 0, ctx->stream, mat, ld, M, mode, g); break;
        case 5: hipLaunchKernelGGL(k_bp_gemm<5>, gv, dim3(256), 0, ctx->stream, mat, ld, M, mode, g); break;
        case 6: hipLaunchKernelGGL(k_bp_gemm<6>, gv, dim3(256), 0, ctx->stream, mat, ld, M, mode, g); break;
        case 7: hipLaunchKernelGGL(k_bp_gemm<7>, gv, dim3(256), 0, ctx->stream, mat, ld, M, mode, g); break;
        case 8: hipLaunchKernelGGL(k_bp_gemm<8>, gv, dim3(256), 0, ctx->stream, mat, ld, M, mode, g); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// multi_members' sibling (host/omp.hpp): the pass's entries from a LIST of members -- slots[i]'s y is entry i's residual, its solver
// slot's cvec, partials and control block the rest.  Up to kGroupMax members the narrow pass's [0, n); more, the wide pass's halves.
template <typename TA>
static void bp_pass_members(csmp_ctx* ctx, MultiSweep<TA>& p, const int* slots, int L) {
    const bool wide = L > kGroupMax;
    p.n = wide ? (L + 1) / 2 : L;
    p.n1 = wide ? L / 2 : 0;
    for (int e = 0; e < kWideMax; ++e) {
        const int h = e / kGroupMax, i = e % kGroupMax;
        const int at = h == 0 || !wide ? std::min(i, p.n - 1) : p.n + std::min(i, p.n1 - 1);
        const int m = slots[at];
        const Solver& s = *slot_ptr(ctx, 3 * m);
        p.r[e] = bpb_member(ctx, m).y; p.cvec[e] = s.cvec; p.pval[e] = s.pval; p.pidx[e] = s.pidx; p.st[e] = s.st;
    }
}

// One step of the live members slots[0 .. L), in slot order: eight launches (slot 0 active)
template <typename TA>
static int bp_group_step(csmp_ctx* ctx, const int* slots, int L, int64_t nw, double rho) {
    BpBuf& t = ctx->bp;
    const int M = (int)ctx->M, np = t.np, npa = 2 * np;
    const double* T = t.Gm + (size_t)np * npa;  // R^-T, lower
    const double* Ri = t.Gm + np;               // R^-1, upper
    BpGemm g1, g2, g3;
    BpGroup G;
    G.n = L;
    for (int i = 0; i < kBpGroupMax; ++i) {
        const int m = slots[std::min(i, L - 1)];
        const BpbMember b = bpb_member(ctx, m);
        const Solver& s = *slot_ptr(ctx, 3 * m);
        g1.x[i] = b.e; g1.out[i] = b.v;
        g2.x[i] = b.v; g2.out[i] = b.y;
        g3.x[i] = b.y; g3.out[i] = b.g;
        G.c[i] = s.cvec; G.z[i] = b.z; G.u[i] = b.u; G.lidx[i] = b.lidx; G.seg_cnt[i] = b.seg_cnt; G.lval[i] = b.lval; G.rpart[i] = b.rpart;
        G.part[i] = b.part; G.nnz[i] = b.nnz; G.b[i] = s.b; G.r[i] = s.r; G.g[i] = b.g; G.p[i] = b.p; G.q[i] = b.q; G.e[i] = b.e;
    }
    HIPCHECK(bp_gemm_launch(ctx, L, Ri, (int64_t)npa, M, (int)BP_UPPER, g1));
    HIPCHECK(bp_gemm_launch(ctx, L, T, (int64_t)npa, M, (int)BP_LOWER, g2));
    HIPCHECK(bp_gemm_launch(ctx, L, t.G, (int64_t)M, M, (int)BP_FULL, g3));
    {  // the shared pass: mp_group_step's grids and LDS request, c = A'y of every member to its slot's cvec
        const bool wide = L > kGroupMax;
        MultiSweep<TA> p;
        p.A = (const TA*)ctx->dA; p.ld = ctx->ld; p.Mv = ctx->Mv; p.N = ctx->N;
        p.eps = 0.0; p.check_eps = 0; p.skipmask = 0; p.KP = ctx->sweep_KP;
        p.nblk = wide ? wide_nblk(ctx) : pipe_nblk(ctx, ctx->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid);
        bp_pass_members<TA>(ctx, p, slots, L);
        const size_t excl = (size_t)(ctx->tune_pair_lds_kib > 0 ? ctx->tune_pair_lds_kib : kPairLdsKiB) * 1024;
        const size_t lds = std::max(sweep_multi_lds_bytes(p.KP, p.n), excl);
        HIPCHECK(wide ? wide_launch<TA>(ctx, p, lds) : multi_launch<TA>(ctx, p, lds));
    }
    const int64_t seg_len = ista_seg_len(ctx->N);
    const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
    const unsigned uL = (unsigned)L;
    hipLaunchKernelGGL(k_bp_update_group, dim3(nseg, 1, uL), dim3(kIstaThreads), 0, ctx->stream, G, (const double*)ctx->ista.w, nw, rho, ctx->N, seg_len);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ista_axpy_group<TA>, dim3(ctx->bpb.P, ista_row_blocks(ctx), uL), dim3(kIstaThreads), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld,
                       ctx->Mv, nseg, seg_len, G);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ista_resum_group, dim3((M + kWave - 1) / kWave, 1, uL), dim3(kIstaThreads), 0, ctx->stream, ctx->Mv, M, ctx->bpb.P, G);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_bp_pq_group, dim3((M + 255) / 256, 1, uL), dim3(256), 0, ctx->stream, M, G);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// The arguments of one call and bp_lockstep's callbacks
struct BpBatchRun {
    csmp_ctx* ctx;
    const char* dB;  // B on the device
    int b_dtype;
    int64_t ldB, nw;
    double rho, tol;
    int64_t maxiter, check_every;
    double* X;
    int64_t ldX;
    int x_loc;
    int64_t* iterations;
    double* resnorm;
    int* flags;

    int init(int64_t sig) const {  // signal sig into the ACTIVE slot: b, r = b, the control block
        const char* col = dB + (size_t)sig * (size_t)ldB * (b_dtype == CSMP_F32 ? 4 : 8);
        ctx->s.begun = false;
        return b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)col) : init_from_device_t<double>(ctx, (const double*)col);
    }
    hipMemcpyKind out_kind() const { return x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost; }
    void record(int64_t sig, int64_t iters, bool conv, double norm) const {
        if (iterations) iterations[sig] = iters;
        if (resnorm) resnorm[sig] = norm;
        if (flags) flags[sig] = conv ? CSMP_BP_CONVERGED : 0;
    }
    // csmp_bp's own solve of one signal on slot 0 (no shared pass, the screened sweeps, a lone signal)
    int solve_one(int64_t sig) const {
        CHECK(init(sig));
        CHECK(bp_start(ctx));
        int64_t iters = 0;
        bool conv = false;
        CHECK(bp_iterate(ctx, nw, rho, maxiter, tol, check_every, &iters, &conv));
        double nr = 0.0;
        if (resnorm) CHECK(residual_norm(ctx, &nr));
        HIPCHECK(hipMemcpyAsync(X + sig * ldX, ctx->ista.x, (size_t)ctx->N * sizeof(double), out_kind(), ctx->stream));
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        record(sig, iters, conv, nr);
        return CSMP_OK;
    }

    // bp_lockstep's callbacks ---------------------------------------------------------------
    int enter(int slot, int64_t sig) {  // as bp_start: z = u = 0, p = q = 0, e = -b, r = b
        activate_slot(ctx, 3 * slot);
        const int rc = init(sig);
        activate_slot(ctx, 0);
        CHECK(rc);
        const BpbMember b = bpb_member(ctx, slot);
        const int M = (int)ctx->M;
        HIPCHECK(hipMemsetAsync(b.z, 0, (size_t)2 * (size_t)ctx->N * sizeof(double), ctx->stream));  // (u follows z)
        hipLaunchKernelGGL(k_bp_start, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, (const double*)slot_ptr(ctx, 3 * slot)->b, M, b.p, b.q, b.e);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    int step(const int* slots, int n) {
        return ctx->dtype == CSMP_F32 ? bp_group_step<float>(ctx, slots, n, nw, rho) : bp_group_step<double>(ctx, slots, n, nw, rho);
    }
    int check(const int* slots, int n, bool* converged) {  // csmp_bp's test on every checked member: one read of all res pairs
        const int64_t seg_len = ista_seg_len(ctx->N);
        const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
        for (int i = 0; i < n; ++i) {
            const BpbMember b = bpb_member(ctx, slots[i]);
            hipLaunchKernelGGL(k_bp_fold, dim3(1), dim3(256), 0, ctx->stream, (const double*)b.rpart, nseg, b.res);
        }
        HIPCHECK(hipGetLastError());
        double res[2 * kBpPlanMaxMembers];
        {
            PinFetch f(ctx);
            CHECK(f.begin(sizeof res));
            CHECK(f.add(res, ctx->bpb.res, (size_t)2 * ctx->bpb.R * sizeof(double)));
            CHECK(f.wait());
        }
        for (int i = 0; i < n; ++i) {
            const double* r2 = res + 2 * slots[i];
            converged[i] = std::sqrt(r2[0]) < tol && rho * std::sqrt(r2[1]) < tol;
        }
        return CSMP_OK;
    }
    int retire(const BpPlanRetired* who, int n) {  // ||r|| as residual_norm takes it, z to the signal's column, the outputs
        const int M = (int)ctx->M;
        for (int i = 0; i < n; ++i) {
            const BpbMember b = bpb_member(ctx, who[i].slot);
            if (resnorm) hipLaunchKernelGGL(k_norm2, dim3(1), dim3(256), 0, ctx->stream, (const double*)slot_ptr(ctx, 3 * who[i].slot)->r, M, b.nrm);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpyAsync(X + who[i].sig * ldX, b.z, (size_t)ctx->N * sizeof(double), out_kind(), ctx->stream));
        }
        double nrm[kBpPlanMaxMembers] = {};
        if (resnorm) {
            PinFetch f(ctx);
            CHECK(f.begin(sizeof nrm));
            CHECK(f.add(nrm, ctx->bpb.nrm, (size_t)ctx->bpb.R * sizeof(double)));
            CHECK(f.wait());
        }
        for (int i = 0; i < n; ++i) record(who[i].sig, who[i].iterations, who[i].converged, std::sqrt(nrm[who[i].slot]));
        return CSMP_OK;
    }
};

extern "C" int csmp_bp_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, const double* w, int64_t nw,
                             double rho, int64_t maxiter, double tol, int64_t check_every, double* X, int64_t ldX, int x_loc,
                             int64_t* iterations, double* resnorm, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (nsig < 0) return fail(ctx, CSMP_EINVAL, "bp_batch: nsig has to be non-negative");
    if (!w || (nsig > 0 && (!B || !X))) return fail(ctx, CSMP_EINVAL, "bp_batch: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if ((b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) || (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE))
        return fail(ctx, CSMP_EINVAL, "bp_batch: b_loc / x_loc must be CSMP_HOST or CSMP_DEVICE");
    CHECK(bp_entry(ctx, "bp_batch"));
    if (ldB < ctx->M) return fail(ctx, CSMP_EDIM, "bp_batch: ldB < size(A, 1)");
    if (ldX < ctx->N) return fail(ctx, CSMP_EDIM, "bp_batch: ldX < size(A, 2)");
    if (nw != 1 && nw != ctx->N) return fail(ctx, CSMP_EDIM, "bp_batch: length(w) must be 1 or size(A, 2)");
    CHECK(bp_check_knobs(ctx, "bp_batch", rho, maxiter, tol, check_every));
    for (int64_t i = 0; i < nw; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(ctx, CSMP_EINVAL, "bp_batch: the weights have to be non-negative and finite");
    if (nsig == 0) return CSMP_OK;
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    bool did = false;
    CHECK(bp_prepare(ctx, &did));
    BpBatchRun run{};
    run.ctx = ctx; run.dB = (const char*)B; run.b_dtype = b_dtype; run.ldB = ldB; run.nw = nw; run.rho = rho; run.tol = tol;
    run.X = X; run.ldX = ldX; run.x_loc = x_loc; run.iterations = iterations; run.resnorm = resnorm; run.flags = flags;
    run.maxiter = maxiter; run.check_every = check_every;
    DevTmp tB;  // a host caller's B on the device
    if (b_loc == CSMP_HOST) {
        const size_t bytes = (size_t)ldB * (size_t)nsig * (b_dtype == CSMP_F32 ? 4 : 8);
        CHECK(bp_nomem(ctx, tB.alloc(ctx, bytes)));
        HIPCHECK(hipMemcpy(tB.p, B, bytes, hipMemcpyHostToDevice));
        run.dB = (const char*)tB.p;
    }
    HIPCHECK(hipMemcpyAsync(ctx->ista.w, w, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    auto finish = [&](int rc) -> int {
        activate_slot(ctx, 0);
        (void)hipStreamSynchronize(ctx->stream);  // (on every way out: the temporaries and the caller's buffers are at rest)
        if (rc == CSMP_OK && flags && did) flags[0] |= CSMP_BP_FACTORED;
        return rc;
    };
    // The shared pass where the resident dictionary has one and the sweeps are exact; a lone signal keeps csmp_bp's launches.
    const bool grouped = ctx->pipeline && ctx->sweep_group >= 1 && !screened_on(ctx) && nsig >= 2;
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
        CHECK(bpb_ensure(ctx, R));
        const int rc = bp_lockstep(R, nsig, maxiter, check_every, run);
        if (rc < 0) return fail(ctx, CSMP_EINVAL, "bp_batch: no schedule for this group size");
        return rc;
    };
    return finish(bp_nomem(ctx, batch_pipelines(ctx, false, ctx->sweep_group, wide_members, 3, ensure, enqueue)));
}
