// host/bpd_batch.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_bpd_batch -- csmp_bpd for every column of B, the members of a group in lockstep on shared launches.
// ------------------------------------------------------------------------------------------ bpd batch
// csmp_bp_batch's scheme (host/bp_batch.hpp) for the ball-constrained problem.  Everything an iteration of csmp_bpd reads in bulk -- the
// dictionary, R^-1, R^-T of K = I + A A' -- is the same for every signal.  A GROUP of up to R members (csmp_bp_batch's rule for R)
// takes its iterations together, EIGHT launches a step whatever the number of live members: two k_bp_gemm (one read of each triangle
// for all right-hand sides), the shared pass with the members' yn as its residuals, k_bp_update_group, k_ista_axpy_group,
// k_ista_resum_group (csmp_bp.hpp, unchanged) and the group forms of the M-vector stage, k_bpd_pq_group and k_bpd_ball_group
// (csmp_bpd.hpp).  Member m lives in solver slot 3 m (b, r, c, the pass's partials and control block) and in its share of BpdBatchBuf
// (everything else csmp_bpd keeps per solve); the factor and the weights are csmp_bpd's own (bpd_prepare).  Every member has its own
// radius delta.  bp_lockstep (host/bp_batch_plan.hpp) says who runs, who is checked -- one read of all res quadruples per interval --
// and who leaves.  Every member's arithmetic is csmp_bpd's: the results are csmp_bpd's bit for bit.  One pipeline, the context's stream.
static int bpdb_ensure(csmp_ctx* ctx, int R) {
    BpdBatchBuf& t = ctx->bpdb;
    const int P = ista_parts_max(ctx), Mp = ctx->bpd.Mp;
    if (t.zu && t.R >= R && t.N == ctx->N && t.Mv == ctx->Mv && t.P == P && t.Mp == Mp) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    bpdb_free(t);
    BpdBatchBuf n;
    const size_t N = (size_t)ctx->N, Rr = (size_t)R;
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.zu, 2 * N * Rr));
        CHECK(dmalloc(ctx, &n.lidx, N * Rr));
        CHECK(dmalloc(ctx, &n.lval, N * Rr));
        CHECK(dmalloc(ctx, &n.seg_cnt, (size_t)kIstaMaxSegs * Rr));
        CHECK(dmalloc(ctx, &n.nnz, Rr));
        CHECK(dmalloc(ctx, &n.part, (size_t)P * (size_t)ctx->Mv * Rr));
        CHECK(dmalloc(ctx, &n.vec, (size_t)kBpdVecs * Mp * Rr));
        CHECK(dmalloc(ctx, &n.rpart, (size_t)2 * kIstaMaxSegs * Rr));
        CHECK(dmalloc(ctx, &n.mpart, (size_t)3 * kBpdMaxParts * Rr));
        CHECK(dmalloc(ctx, &n.res, 4 * Rr));
        CHECK(dmalloc(ctx, &n.nrm, Rr));
        HIPCHECK(hipMemsetAsync(n.vec, 0, (size_t)kBpdVecs * Mp * Rr * sizeof(double), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        bpdb_free(n);
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

// member m's pointers (the M-vectors in BpdBuf's order)
struct BpdbMember {
    double *z, *u, *lval, *part, *rpart, *mpart, *res, *nrm, *p, *q, *en, *tmp, *yn, *v, *lam, *h;
    int *lidx, *seg_cnt;
    unsigned* nnz;
};
static BpdbMember bpdb_member(const csmp_ctx* ctx, int m) {
    const BpdBatchBuf& t = ctx->bpdb;
    const size_t N = (size_t)t.N, mm = (size_t)m;
    BpdbMember r;
    r.z = t.zu + 2 * N * mm;
    r.u = r.z + N;
    r.lidx = t.lidx + N * mm;
    r.lval = t.lval + N * mm;
    r.seg_cnt = t.seg_cnt + (size_t)kIstaMaxSegs * mm;
    r.nnz = t.nnz + mm;
    r.part = t.part + (size_t)t.P * (size_t)t.Mv * mm;
    double* vec = t.vec + (size_t)kBpdVecs * t.Mp * mm;
    r.p = vec; r.q = vec + t.Mp; r.en = vec + 2 * t.Mp; r.tmp = vec + 3 * t.Mp; r.yn = vec + 4 * t.Mp; r.v = vec + 5 * t.Mp;
    r.lam = vec + 6 * t.Mp; r.h = vec + 7 * t.Mp;
    r.rpart = t.rpart + (size_t)2 * kIstaMaxSegs * mm;
    r.mpart = t.mpart + (size_t)3 * kBpdMaxParts * mm;
    r.res = t.res + 4 * mm;
    r.nrm = t.nrm + mm;
    return r;
}

// bp_pass_members (host/bp_batch.hpp) on BpdBatchBuf: slots[i]'s yn is entry i's residual
template <typename TA>
static void bpd_pass_members(csmp_ctx* ctx, MultiSweep<TA>& p, const int* slots, int L) {
    const bool wide = L > kGroupMax;
    p.n = wide ? (L + 1) / 2 : L;
    p.n1 = wide ? L / 2 : 0;
    for (int e = 0; e < kWideMax; ++e) {
        const int h = e / kGroupMax, i = e % kGroupMax;
        const int at = h == 0 || !wide ? std::min(i, p.n - 1) : p.n + std::min(i, p.n1 - 1);
        const int m = slots[at];
        const Solver& s = *slot_ptr(ctx, 3 * m);
        p.r[e] = bpdb_member(ctx, m).yn; p.cvec[e] = s.cvec; p.pval[e] = s.pval; p.pidx[e] = s.pidx; p.st[e] = s.st;
    }
}

// One step of the live members slots[0 .. L), in slot order: eight launches (slot 0 active).  delta: the radius of every SLOT's ball.
template <typename TA>
static int bpd_group_step(csmp_ctx* ctx, const int* slots, int L, const double* delta, int64_t nw, double rho) {
    BpdBuf& t = ctx->bpd;
    const int M = (int)ctx->M, np = t.np, npa = 2 * np;
    const double* T = t.Gm + (size_t)np * npa;  // R^-T, lower
    const double* Ri = t.Gm + np;               // R^-1, upper
    BpGemm g1, g2;
    BpGroup G;
    BpdGroup Q;
    G.n = Q.n = L;
    for (int i = 0; i < kBpGroupMax; ++i) {
        const int m = slots[std::min(i, L - 1)];
        const BpdbMember b = bpdb_member(ctx, m);
        const Solver& s = *slot_ptr(ctx, 3 * m);
        g1.x[i] = b.en; g1.out[i] = b.tmp;
        g2.x[i] = b.tmp; g2.out[i] = b.yn;
        // (BpGroup's g, p, q, e are k_bp_pq_group's, which does not run here: filled so that no entry is left unset)
        G.c[i] = s.cvec; G.z[i] = b.z; G.u[i] = b.u; G.lidx[i] = b.lidx; G.seg_cnt[i] = b.seg_cnt; G.lval[i] = b.lval; G.rpart[i] = b.rpart;
        G.part[i] = b.part; G.nnz[i] = b.nnz; G.b[i] = s.b; G.r[i] = s.r; G.g[i] = b.yn; G.p[i] = b.p; G.q[i] = b.q; G.e[i] = b.en;
        Q.b[i] = s.b; Q.r[i] = s.r; Q.p[i] = b.p; Q.q[i] = b.q; Q.en[i] = b.en; Q.v[i] = b.v; Q.lam[i] = b.lam; Q.h[i] = b.h; Q.yn[i] = b.yn;
        Q.mpart[i] = b.mpart; Q.delta[i] = delta[m];
    }
    HIPCHECK(bp_gemm_launch(ctx, L, Ri, (int64_t)npa, M, (int)BP_UPPER, g1));
    HIPCHECK(bp_gemm_launch(ctx, L, T, (int64_t)npa, M, (int)BP_LOWER, g2));
    {  // the shared pass: bp_group_step's grids and LDS request, -c = A'yn of every member to its slot's cvec
        const bool wide = L > kGroupMax;
        MultiSweep<TA> p;
        p.A = (const TA*)ctx->dA; p.ld = ctx->ld; p.Mv = ctx->Mv; p.N = ctx->N;
        p.eps = 0.0; p.check_eps = 0; p.skipmask = 0; p.KP = ctx->sweep_KP;
        p.nblk = wide ? wide_nblk(ctx) : pipe_nblk(ctx, ctx->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid);
        bpd_pass_members<TA>(ctx, p, slots, L);
        const size_t excl = (size_t)(ctx->tune_pair_lds_kib > 0 ? ctx->tune_pair_lds_kib : kPairLdsKiB) * 1024;
        const size_t lds = std::max(sweep_multi_lds_bytes(p.KP, p.n), excl);
        HIPCHECK(wide ? wide_launch<TA>(ctx, p, lds) : multi_launch<TA>(ctx, p, lds));
    }
    const int64_t seg_len = ista_seg_len(ctx->N);
    const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
    const int nparts = (M + 255) / 256;  // <= kBpdMaxParts: M <= 2^19 (bpd_entry)
    const unsigned uL = (unsigned)L;
    hipLaunchKernelGGL(k_bp_update_group, dim3(nseg, 1, uL), dim3(kIstaThreads), 0, ctx->stream, G, (const double*)ctx->ista.w, nw, rho, ctx->N, seg_len);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ista_axpy_group<TA>, dim3(ctx->bpdb.P, ista_row_blocks(ctx), uL), dim3(kIstaThreads), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld,
                       ctx->Mv, nseg, seg_len, G);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ista_resum_group, dim3((M + kWave - 1) / kWave, 1, uL), dim3(kIstaThreads), 0, ctx->stream, ctx->Mv, M, ctx->bpdb.P, G);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_bpd_pq_group, dim3(nparts, 1, uL), dim3(256), 0, ctx->stream, M, Q);
    hipLaunchKernelGGL(k_bpd_ball_group, dim3(nparts, 1, uL), dim3(256), 0, ctx->stream, M, nparts, Q);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// The arguments of one call and bp_lockstep's callbacks
struct BpdBatchRun {
    csmp_ctx* ctx;
    const char* dB;  // B on the device
    int b_dtype;
    int64_t ldB, nw;
    const double* delta;  // one radius, or one per signal
    int64_t ndelta;
    double rho, tol;
    int64_t maxiter, check_every;
    double* X;
    int64_t ldX;
    int x_loc;
    int64_t* iterations;
    double* resnorm;
    int* flags;
    double slot_delta[kBpPlanMaxMembers];  // the radius of the signal in every slot

    double delta_of(int64_t sig) const { return delta[ndelta == 1 ? 0 : sig]; }
    int init(int64_t sig) const {  // signal sig into the ACTIVE slot: b, r = b, the control block
        const char* col = dB + (size_t)sig * (size_t)ldB * (b_dtype == CSMP_F32 ? 4 : 8);
        ctx->s.begun = false;
        return b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)col) : init_from_device_t<double>(ctx, (const double*)col);
    }
    hipMemcpyKind out_kind() const { return x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost; }
    void record(int64_t sig, int64_t iters, bool conv, double norm) const {
        if (iterations) iterations[sig] = iters;
        if (resnorm) resnorm[sig] = norm;
        if (flags) flags[sig] = conv ? CSMP_BPD_CONVERGED : 0;
    }
    // csmp_bpd's own solve of one signal on slot 0 (no shared pass, the screened sweeps, a lone signal)
    int solve_one(int64_t sig) const {
        CHECK(init(sig));
        CHECK(bpd_start(ctx));
        int64_t iters = 0;
        bool conv = false;
        CHECK(bpd_iterate(ctx, nw, delta_of(sig), rho, maxiter, tol, check_every, &iters, &conv));
        double nr = 0.0;
        if (resnorm) CHECK(residual_norm(ctx, &nr));
        HIPCHECK(hipMemcpyAsync(X + sig * ldX, ctx->ista.x, (size_t)ctx->N * sizeof(double), out_kind(), ctx->stream));
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        record(sig, iters, conv, nr);
        return CSMP_OK;
    }

    // bp_lockstep's callbacks ---------------------------------------------------------------
    int enter(int slot, int64_t sig) {  // as bpd_start: z = u = 0, p = q = 0, v = lam = 0, en = 0, r = b
        activate_slot(ctx, 3 * slot);
        const int rc = init(sig);
        activate_slot(ctx, 0);
        CHECK(rc);
        slot_delta[slot] = delta_of(sig);
        const BpdbMember b = bpdb_member(ctx, slot);
        const int M = (int)ctx->M;
        HIPCHECK(hipMemsetAsync(b.z, 0, (size_t)2 * (size_t)ctx->N * sizeof(double), ctx->stream));  // (u follows z)
        hipLaunchKernelGGL(k_bpd_start, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, M, b.p, b.q, b.v, b.lam, b.en);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    int step(const int* slots, int n) {
        return ctx->dtype == CSMP_F32 ? bpd_group_step<float>(ctx, slots, n, slot_delta, nw, rho)
                                      : bpd_group_step<double>(ctx, slots, n, slot_delta, nw, rho);
    }
    int check(const int* slots, int n, bool* converged) {  // csmp_bpd's test on every checked member: one read of all res quadruples
        const int64_t seg_len = ista_seg_len(ctx->N);
        const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
        const int nparts = ((int)ctx->M + 255) / 256;
        for (int i = 0; i < n; ++i) {
            const BpdbMember b = bpdb_member(ctx, slots[i]);
            hipLaunchKernelGGL(k_bpd_fold, dim3(1), dim3(256), 0, ctx->stream, (const double*)b.rpart, nseg, (const double*)b.mpart, nparts, b.res);
        }
        HIPCHECK(hipGetLastError());
        double res[4 * kBpPlanMaxMembers];
        {
            PinFetch f(ctx);
            CHECK(f.begin(sizeof res));
            CHECK(f.add(res, ctx->bpdb.res, (size_t)4 * ctx->bpdb.R * sizeof(double)));
            CHECK(f.wait());
        }
        for (int i = 0; i < n; ++i) {
            const double* r4 = res + 4 * slots[i];
            converged[i] = std::sqrt(r4[0] + r4[2]) < tol && rho * std::sqrt(r4[1] + r4[3]) < tol;
        }
        return CSMP_OK;
    }
    int retire(const BpPlanRetired* who, int n) {  // ||r|| as residual_norm takes it, z to the signal's column, the outputs
        const int M = (int)ctx->M;
        for (int i = 0; i < n; ++i) {
            const BpdbMember b = bpdb_member(ctx, who[i].slot);
            if (resnorm) hipLaunchKernelGGL(k_norm2, dim3(1), dim3(256), 0, ctx->stream, (const double*)slot_ptr(ctx, 3 * who[i].slot)->r, M, b.nrm);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpyAsync(X + who[i].sig * ldX, b.z, (size_t)ctx->N * sizeof(double), out_kind(), ctx->stream));
        }
        double nrm[kBpPlanMaxMembers] = {};
        if (resnorm) {
            PinFetch f(ctx);
            CHECK(f.begin(sizeof nrm));
            CHECK(f.add(nrm, ctx->bpdb.nrm, (size_t)ctx->bpdb.R * sizeof(double)));
            CHECK(f.wait());
        }
        for (int i = 0; i < n; ++i) record(who[i].sig, who[i].iterations, who[i].converged, std::sqrt(nrm[who[i].slot]));
        return CSMP_OK;
    }
};

extern "C" int csmp_bpd_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, const double* delta, int64_t ndelta,
                              const double* w, int64_t nw, double rho, int64_t maxiter, double tol, int64_t check_every, double* X, int64_t ldX,
                              int x_loc, int64_t* iterations, double* resnorm, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (nsig < 0) return fail(ctx, CSMP_EINVAL, "bpd_batch: nsig has to be non-negative");
    if (!w || !delta || (nsig > 0 && (!B || !X))) return fail(ctx, CSMP_EINVAL, "bpd_batch: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if ((b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) || (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE))
        return fail(ctx, CSMP_EINVAL, "bpd_batch: b_loc / x_loc must be CSMP_HOST or CSMP_DEVICE");
    CHECK(bpd_entry(ctx, "bpd_batch", 0.0));
    if (ldB < ctx->M) return fail(ctx, CSMP_EDIM, "bpd_batch: ldB < size(A, 1)");
    if (ldX < ctx->N) return fail(ctx, CSMP_EDIM, "bpd_batch: ldX < size(A, 2)");
    if (nw != 1 && nw != ctx->N) return fail(ctx, CSMP_EDIM, "bpd_batch: length(w) must be 1 or size(A, 2)");
    if (ndelta != 1 && ndelta != nsig) return fail(ctx, CSMP_EDIM, "bpd_batch: length(delta) must be 1 or nsig");
    CHECK(bp_check_knobs(ctx, "bpd_batch", rho, maxiter, tol, check_every));
    for (int64_t i = 0; i < nw; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(ctx, CSMP_EINVAL, "bpd_batch: the weights have to be non-negative and finite");
    for (int64_t i = 0; i < ndelta; ++i)
        if (!std::isfinite(delta[i]) || delta[i] < 0.0) return fail(ctx, CSMP_EINVAL, "bpd_batch: every delta has to be non-negative and finite");
    if (nsig == 0) return CSMP_OK;
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    bool did = false;
    CHECK(bpd_prepare(ctx, &did));
    BpdBatchRun run{};
    run.ctx = ctx; run.dB = (const char*)B; run.b_dtype = b_dtype; run.ldB = ldB; run.nw = nw; run.delta = delta; run.ndelta = ndelta; run.rho = rho;
    run.tol = tol; run.X = X; run.ldX = ldX; run.x_loc = x_loc; run.iterations = iterations; run.resnorm = resnorm; run.flags = flags;
    run.maxiter = maxiter; run.check_every = check_every;
    DevTmp tB;  // a host caller's B on the device
    if (b_loc == CSMP_HOST) {
        const size_t bytes = (size_t)ldB * (size_t)nsig * (b_dtype == CSMP_F32 ? 4 : 8);
        CHECK(bpd_nomem(ctx, tB.alloc(ctx, bytes)));
        HIPCHECK(hipMemcpy(tB.p, B, bytes, hipMemcpyHostToDevice));
        run.dB = (const char*)tB.p;
    }
    HIPCHECK(hipMemcpyAsync(ctx->ista.w, w, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    auto finish = [&](int rc) -> int {
        activate_slot(ctx, 0);
        (void)hipStreamSynchronize(ctx->stream);  // (on every way out: the temporaries and the caller's buffers are at rest)
        if (rc == CSMP_OK && flags && did) flags[0] |= CSMP_BPD_FACTORED;
        return rc;
    };
    // The shared pass where the resident dictionary has one and the sweeps are exact; a lone signal keeps csmp_bpd's launches.
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
        CHECK(bpdb_ensure(ctx, R));
        const int rc = bp_lockstep(R, nsig, maxiter, check_every, run);
        if (rc < 0) return fail(ctx, CSMP_EINVAL, "bpd_batch: no schedule for this group size");
        return rc;
    };
    return finish(bpd_nomem(ctx, batch_pipelines(ctx, false, ctx->sweep_group, wide_members, 3, ensure, enqueue)));
}
