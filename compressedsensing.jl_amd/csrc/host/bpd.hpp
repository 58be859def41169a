// host/bpd.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_bpd (basis_pursuit_denoising, src/basispursuit.jl:76-100, by graph-form ADMM) and csmp_bpd_reweighted (bpd_reweighting, :102-115,
// around it).  The factor of K = I + A A' lives in the context's BpdBuf, beside and apart from csmp_bp's factor of A A' (BpBuf): a
// context may hold both.  G = A A' is a temporary of the factorisation; what stays resident is the augmented matrix, (2 np)^2 doubles
// (np = M rounded up to 64): 512 MiB at M = 4096.
// ------------------------------------------------------------------------------------------ basis pursuit denoising
static constexpr int kBpdVecs = 8;  // p, q, en, the triangular products' intermediate, yn, v, lam, h

// The buffers of the context for the resident dictionary: all of them, or none.
static int bpd_ensure(csmp_ctx* ctx) {
    BpdBuf& t = ctx->bpd;
    if (t.Gm && t.M == (int)ctx->M) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    bpd_free(t);
    BpdBuf n;
    const size_t M = (size_t)ctx->M, np = (size_t)bp_np(ctx), npa = 2 * np;
    n.Mp = (int)((M + 255) / 256 * 256);
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.Gm, npa * npa));
        CHECK(dmalloc(ctx, &n.pivref, np));
        CHECK(dmalloc(ctx, &n.Dfac, np * kCholNB));
        CHECK(dmalloc(ctx, &n.vec, (size_t)kBpdVecs * n.Mp));
        CHECK(dmalloc(ctx, &n.rpart, (size_t)2 * kIstaMaxSegs));
        CHECK(dmalloc(ctx, &n.mpart, (size_t)3 * kBpdMaxParts));
        CHECK(dmalloc(ctx, &n.res, (size_t)4));
        CHECK(dmalloc(ctx, &n.st, (size_t)1));
        HIPCHECK(hipMemsetAsync(n.vec, 0, (size_t)kBpdVecs * n.Mp * sizeof(double), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        bpd_free(n);
        return rc;
    }
    n.M = (int)ctx->M;
    n.np = (int)np;
    t = n;
    return CSMP_OK;
}

// G = A A' (a temporary), K = G + I = R'R by the blocked Cholesky of csmp_gram.hpp, augmented by the unit vectors (bp_factor's launches);
// then R^-1 beside R^-T.  One host read: the verdict.
static int bpd_factor(csmp_ctx* ctx) {
    BpdBuf& t = ctx->bpd;
    const int M = (int)ctx->M, np = t.np, npa = 2 * np;
    DevTmp G;
    CHECK(G.alloc(ctx, (size_t)M * (size_t)M * sizeof(double)));
    CHECK(bp_form_gram(ctx, (double*)G.p));
    HIPCHECK(hipMemsetAsync(t.st, 0, sizeof(DevState), ctx->stream));
    hipLaunchKernelGGL(k_bpd_assemble, dim3((unsigned)(((int64_t)npa * npa + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)G.p, M, np, npa,
                       bp_pivot_fraction(ctx), t.Gm, t.pivref);
    HIPCHECK(hipGetLastError());
    const int nsteps = (M + kCholNB - 1) / kCholNB;
    {
        const int left0 = npa - kCholNB;
        hipLaunchKernelGGL(k_chol_row, dim3(std::max(1, (left0 + kCholRowCols - 1) / kCholRowCols)), dim3(kCholThreads), 0, ctx->stream, t.Gm, npa, M, 0,
                           (const double*)t.pivref, t.st, t.Dfac);
    }
    for (int kb = 0; kb + 1 < nsteps; ++kb) {
        const int left = npa - (kb + 1) * kCholNB;
        const int left2 = left - kCholNB;
        const int Tt = (left + kGramTile - 1) / kGramTile;
        const int ntrail = left > kCholNB ? Tt * (Tt + 1) / 2 : 0;
        const int nrow = std::max(1, (left2 + kCholRowCols - 1) / kCholRowCols);
        hipLaunchKernelGGL(k_chol_step, dim3(nrow + ntrail), dim3(kCholThreads), 0, ctx->stream, t.Gm, npa, M, kb, (const double*)t.pivref, t.st, nrow,
                           t.Dfac, np);
    }
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_bp_transpose, dim3((unsigned)((M + 31) / 32), (unsigned)((M + 31) / 32)), dim3(256), 0, ctx->stream,
                       (const double*)(t.Gm + (size_t)np * npa), (int64_t)npa, M, t.Gm + np);
    HIPCHECK(hipGetLastError());
    DevState hs{};
    {  // (the wait also ends every use of G before it is released)
        PinFetch f(ctx);
        CHECK(f.begin(sizeof hs));
        CHECK(f.add(&hs, t.st, sizeof hs));
        CHECK(f.wait());
    }
    t.factored = true;
    t.notpd = (hs.done & STOP_REORTH) != 0;
    return CSMP_OK;
}

static int bpd_nomem(csmp_ctx* ctx, int rc) {
    if (rc == CSMP_EHIP) return fail(ctx, CSMP_ENOMEM, "bpd: no device memory for I + A A' and its factor (" + ctx->err + ")");
    return rc;
}
// everything a solve needs; *did = the call formed and factorised K.  A failed allocation leaves no BpdBuf behind.
static int bpd_prepare(csmp_ctx* ctx, bool* did) {
    *did = false;
    int rc = solver_ensure(ctx, 1, 1, false);
    if (rc == CSMP_OK) rc = ista_ensure(ctx);
    if (rc == CSMP_OK) rc = bpd_ensure(ctx);
    if (rc == CSMP_OK && !ctx->bpd.factored) {
        rc = bpd_factor(ctx);
        if (rc != CSMP_OK) {
            (void)hipStreamSynchronize(ctx->stream);
            bpd_free(ctx->bpd);
        }
        *did = rc == CSMP_OK;
    }
    CHECK(bpd_nomem(ctx, rc));
    // K's smallest eigenvalue is at least 1 whatever the dictionary: this is no verdict on A
    if (ctx->bpd.notpd)
        return fail(ctx, CSMP_EINVAL, "bpd: the factorisation of I + A A' met a pivot that is not positive (non-finite entries of A, or a fault of the "
                                      "factorisation: I + A A' is positive definite for every finite A)");
    return CSMP_OK;
}

static int bpd_entry(csmp_ctx* ctx, const char* who, double delta) {
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, std::string(who) + ": a host-streamed dictionary is not served");
    if (ctx->M > kBpMaxRows) return fail(ctx, CSMP_ERANGE, std::string(who) + ": more than 2^19 rows");
    if (!std::isfinite(delta) || delta < 0.0) return fail(ctx, CSMP_EINVAL, std::string(who) + ": delta has to be non-negative and finite");
    return CSMP_OK;
}

// z = u = 0, v = lam = 0: p = q = 0, en = 0; r = b already (upload_b / init_from_device_t)
static int bpd_start(csmp_ctx* ctx) {
    BpdBuf& t = ctx->bpd;
    IstaBuf& v = ctx->ista;
    const int M = (int)ctx->M;
    HIPCHECK(hipMemsetAsync(v.x, 0, (size_t)ctx->N * sizeof(double), ctx->stream));
    HIPCHECK(hipMemsetAsync(v.y, 0, (size_t)ctx->N * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_bpd_start, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, M, t.vec, t.vec + t.Mp, t.vec + 5 * t.Mp, t.vec + 6 * t.Mp,
                       t.vec + 2 * t.Mp);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// Up to maxiter iterations from the z, u (the context's ista buffers x, y), p, q, v, lam, en and weights as they stand; the launches of an
// interval of check_every iterations are queued without a wait, then the host reads the four sums of the stopping test.  Eight launches
// an iteration, as csmp_bp: two triangular products (bp has those and a full one), the sweep, k_bp_update, the axpy and its resum, and
// the two kernels of the M-vector stage.
static int bpd_iterate(csmp_ctx* ctx, int64_t nw, double delta, double rho, int64_t maxiter, double tol, int64_t check_every, int64_t* iters,
                       bool* converged) {
    BpdBuf& t = ctx->bpd;
    IstaBuf& x = ctx->ista;
    Solver& s = ctx->s;
    const int M = (int)ctx->M, np = t.np, npa = 2 * np;
    double *p = t.vec, *q = t.vec + t.Mp, *en = t.vec + 2 * t.Mp, *tmp = t.vec + 3 * t.Mp, *yn = t.vec + 4 * t.Mp, *v = t.vec + 5 * t.Mp,
           *lam = t.vec + 6 * t.Mp, *h = t.vec + 7 * t.Mp;
    const double* T = t.Gm + (size_t)np * npa;  // R^-T, lower
    const double* Ri = t.Gm + np;               // R^-1, upper
    const int64_t seg_len = ista_seg_len(ctx->N);
    const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
    const int nparts = (M + 255) / 256;  // <= kBpdMaxParts: M <= 2^19 (bpd_entry)
    const dim3 gv((unsigned)((M + 3) / 4)), gm((unsigned)nparts);
    *iters = 0;
    *converged = false;
    for (int64_t it = 1; it <= maxiter; ++it) {
        hipLaunchKernelGGL(k_bp_gemv, gv, dim3(256), 0, ctx->stream, Ri, (int64_t)npa, M, (int)BP_UPPER, (const double*)en, tmp);
        hipLaunchKernelGGL(k_bp_gemv, gv, dim3(256), 0, ctx->stream, T, (int64_t)npa, M, (int)BP_LOWER, (const double*)tmp, yn);
        HIPCHECK(hipGetLastError());
        CHECK(launch_sweep(ctx, yn, 0.0, 0, 0));  // -c
        hipLaunchKernelGGL(k_bp_update, dim3(nseg), dim3(kIstaThreads), 0, ctx->stream, (const double*)s.cvec, (const double*)x.w, nw, rho, x.x, x.y,
                           ctx->N, seg_len, x.lidx, x.lval, x.seg_cnt, t.rpart);
        HIPCHECK(hipGetLastError());
        CHECK(ista_residual(ctx));
        hipLaunchKernelGGL(k_bpd_pq, gm, dim3(256), 0, ctx->stream, (const double*)s.b, (const double*)s.r, (const double*)en, (const double*)yn,
                           (const double*)v, M, p, q, h, t.mpart + 2 * kBpdMaxParts);
        hipLaunchKernelGGL(k_bpd_ball, gm, dim3(256), 0, ctx->stream, (const double*)s.b, (const double*)h, (const double*)yn, (const double*)p,
                           (const double*)q, (const double*)(t.mpart + 2 * kBpdMaxParts), nparts, delta, M, v, lam, en, t.mpart);
        HIPCHECK(hipGetLastError());
        *iters = it;
        if (it % check_every == 0) {
            hipLaunchKernelGGL(k_bpd_fold, dim3(1), dim3(256), 0, ctx->stream, (const double*)t.rpart, nseg, (const double*)t.mpart, nparts, t.res);
            HIPCHECK(hipGetLastError());
            double res[4];
            {
                PinFetch f(ctx);
                CHECK(f.begin(sizeof res));
                CHECK(f.add(res, t.res, sizeof res));
                CHECK(f.wait());
            }
            if (std::sqrt(res[0] + res[2]) < tol && rho * std::sqrt(res[1] + res[3]) < tol) {
                *converged = true;
                break;
            }
        }
    }
    return CSMP_OK;
}

extern "C" int csmp_bpd(csmp_ctx* ctx, const void* b, int b_dtype, double delta, const double* w, int64_t nw, double rho, int64_t maxiter, double tol,
                        int64_t check_every, double* x, int x_loc, int64_t* iterations, double* resnorm, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || !w || !x) return fail(ctx, CSMP_EINVAL, "bpd: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "bpd: x_loc must be CSMP_HOST or CSMP_DEVICE");
    CHECK(bpd_entry(ctx, "bpd", delta));
    if (nw != 1 && nw != ctx->N) return fail(ctx, CSMP_EDIM, "bpd: length(w) must be 1 or size(A, 2)");
    CHECK(bp_check_knobs(ctx, "bpd", rho, maxiter, tol, check_every));
    for (int64_t i = 0; i < nw; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(ctx, CSMP_EINVAL, "bpd: the weights have to be non-negative and finite");
    HIPCHECK(hipSetDevice(ctx->dev));
    bool did = false;
    CHECK(bpd_prepare(ctx, &did));
    CHECK(bp_upload(ctx, b, b_dtype, x_loc));
    HIPCHECK(hipMemcpyAsync(ctx->ista.w, w, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CHECK(bpd_start(ctx));
    int64_t iters = 0;
    bool conv = false;
    CHECK(bpd_iterate(ctx, nw, delta, rho, maxiter, tol, check_every, &iters, &conv));
    if (resnorm) CHECK(residual_norm(ctx, resnorm));  // r = b - A z of the last iteration (r = b where there was none)
    HIPCHECK(hipMemcpyAsync(x, ctx->ista.x, (size_t)ctx->N * sizeof(double), x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                            ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    if (iterations) *iterations = iters;
    if (flags) *flags = (conv ? CSMP_BPD_CONVERGED : 0) | (did ? CSMP_BPD_FACTORED : 0);
    return CSMP_OK;
}

// bpd_reweighting (:102-115) around csmp_bpd's solve.  csmp_bp_reweighted's loop written once more: the solver and its warm start (z, u,
// p, q, v, lam stay as the previous solve left them) differ.
extern "C" int csmp_bpd_reweighted(csmp_ctx* ctx, const void* b, int b_dtype, double delta, int scheme, double eps, int64_t ard_iter,
                                   int64_t outer_maxiter, double min_decrease, double rho, int64_t maxiter, double tol, int64_t check_every, double* x,
                                   int x_loc, double* w_out, int64_t* outer_done, double* resnorm) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || !x) return fail(ctx, CSMP_EINVAL, "bpd_reweighted: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "bpd_reweighted: x_loc must be CSMP_HOST or CSMP_DEVICE");
    if (scheme != CSMP_REWEIGHT_CANDES && scheme != CSMP_REWEIGHT_ARD)
        return fail(ctx, CSMP_EINVAL, "bpd_reweighted: scheme must be CSMP_REWEIGHT_CANDES or CSMP_REWEIGHT_ARD");
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(ctx, CSMP_EINVAL, "bpd_reweighted: eps has to be positive and finite");
    if (ard_iter < 1) return fail(ctx, CSMP_EINVAL, "bpd_reweighted: ard_iter has to be at least 1");
    if (outer_maxiter < 1) return fail(ctx, CSMP_EINVAL, "bpd_reweighted: the outer maxiter has to be at least 1");
    if (!(min_decrease >= 0.0)) return fail(ctx, CSMP_EINVAL, "bpd_reweighted: min_decrease has to be non-negative");
    CHECK(bpd_entry(ctx, "bpd_reweighted", delta));
    CHECK(bp_check_knobs(ctx, "bpd_reweighted", rho, maxiter, tol, check_every));
    HIPCHECK(hipSetDevice(ctx->dev));
    bool did = false;
    CHECK(bpd_prepare(ctx, &did));
    CHECK(rw_nomem(ctx, rw_ensure(ctx), "bpd_reweighted"));
    IstaBuf& t = ctx->ista;
    RwBuf& u = ctx->rw;
    const int64_t N = ctx->N;
    const unsigned gridN = (unsigned)((N + 255) / 256);
    CHECK(bp_upload(ctx, b, b_dtype, x_loc));
    const double one = 1.0;
    HIPCHECK(hipMemcpyAsync(t.w, &one, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CHECK(bpd_start(ctx));
    {  // w = ones(N) (:105): the Candes weights of an "x" of zeros at eps = 1 -- exactly 1.0
        HIPCHECK(hipMemsetAsync(u.info, 0, sizeof(RwInfo), ctx->stream));
        hipLaunchKernelGGL(k_rw_candes, dim3(gridN), dim3(256), 0, ctx->stream, (const double*)t.x, N, 1.0, 1.0, u.w, u.xprev, u.info);
        HIPCHECK(hipGetLastError());
    }
    int64_t iters = 0;
    bool conv = false;
    CHECK(bpd_iterate(ctx, 1, delta, rho, maxiter, tol, check_every, &iters, &conv));  // x = solve(w = 1)
    int64_t done = 1;
    for (int64_t i = 2; i <= outer_maxiter; ++i) {
        HIPCHECK(hipMemcpyAsync(u.xprev, t.x, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        if (scheme == CSMP_REWEIGHT_CANDES) {
            HIPCHECK(hipMemsetAsync(u.info, 0, sizeof(RwInfo), ctx->stream));
            hipLaunchKernelGGL(k_rw_candes, dim3(gridN), dim3(256), 0, ctx->stream, (const double*)t.x, N, eps, 1.0, u.w, t.w, u.info);
            HIPCHECK(hipGetLastError());
        } else {
            CHECK(rw_ard(ctx, t.x, eps, ard_iter, rw_kmax(ctx)));
            hipLaunchKernelGGL(k_rw_scale, dim3(gridN), dim3(256), 0, ctx->stream, (const double*)u.w, N, 1.0, t.w, u.info);
            HIPCHECK(hipGetLastError());
        }
        CHECK(bpd_iterate(ctx, N, delta, rho, maxiter, tol, check_every, &iters, &conv));  // xs = solve(w), warm-started
        done = i;
        hipLaunchKernelGGL(k_rw_stepnorm, dim3(kRwNormParts), dim3(256), 0, ctx->stream, (const double*)t.x, (const double*)u.xprev, N, u.npart);
        HIPCHECK(hipGetLastError());
        double part[kRwNormParts];
        RwInfo info{};
        {  // the outer iteration's one read: the step norm's partials and the weights' verdict
            PinFetch f(ctx);
            CHECK(f.begin(sizeof part + sizeof info + 16));
            CHECK(f.add(part, u.npart, sizeof part));
            CHECK(f.add(&info, u.info, sizeof info));
            CHECK(f.wait());
        }
        if (info.flags & RW_BAD_RESULT) return fail(ctx, CSMP_EINVAL, "bpd_reweighted: weights contain NaN or Inf");
        double n2 = 0.0;
        for (int q = 0; q < kRwNormParts; ++q) n2 += part[q];
        if (std::sqrt(n2) < min_decrease) break;  // norm(xs - x) < min_decrease: return xs (:109)
    }
    if (resnorm) CHECK(residual_norm(ctx, resnorm));
    const hipMemcpyKind out = x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHECK(hipMemcpyAsync(x, t.x, (size_t)N * sizeof(double), out, ctx->stream));
    if (w_out) HIPCHECK(hipMemcpyAsync(w_out, u.w, (size_t)N * sizeof(double), out, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    if (outer_done) *outer_done = done;
    return CSMP_OK;
}
