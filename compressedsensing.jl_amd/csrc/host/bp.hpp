// host/bp.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_bp (basispursuit, src/basispursuit.jl:1-16, by ADMM) and csmp_bp_reweighted (basispursuit_reweighting, :18-31, around it).
// ------------------------------------------------------------------------------------------ basis pursuit
static constexpr int64_t kBpMaxRows = (int64_t)1 << 19;  // the launches over the augmented matrix count (2 np)^2 / 256 workgroups in 32 bits
static int bp_np(const csmp_ctx* ctx) { return (int)((ctx->M + kGramTile - 1) / kGramTile * kGramTile); }
// a pivot of the factorisation has to reach this fraction of its diagonal entry of G: 4 M eps
static double bp_pivot_fraction(const csmp_ctx* ctx) { return 8.0 * (double)ctx->M * 0x1p-53; }

// k_rowgram's column splits: a function of the shape and the device alone, so that the summation order -- and with it every bit of G --
// does not depend on what the context ran before
static void bp_rowgram_split(const csmp_ctx* ctx, int& nsplit, int64_t& cps) {
    const int64_t T = (ctx->M + kRgTile - 1) / kRgTile, ntiles = T * (T + 1) / 2;
    int64_t want = (2 * (int64_t)ctx->prop.multiProcessorCount + ntiles - 1) / ntiles;
    want = std::min<int64_t>(want, std::max<int64_t>(1, ctx->N / kRgMinCols));
    want = std::max<int64_t>(1, std::min<int64_t>(want, kRgMaxSplit));
    cps = ((ctx->N + want - 1) / want + kRgKC - 1) / kRgKC * kRgKC;
    nsplit = (int)((ctx->N + cps - 1) / cps);
}

template <typename TA, bool VEC>
static hipError_t rowgram_t(csmp_ctx* ctx, int nsplit, int64_t cps, double* Gpart) {
    auto kern = k_rowgram<TA, VEC>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rowgram_lds_bytes());
    if (e != hipSuccess) return e;
    const int64_t T = (ctx->M + kRgTile - 1) / kRgTile;
    hipLaunchKernelGGL(kern, dim3((unsigned)(T * (T + 1) / 2), (unsigned)nsplit), dim3(256), rowgram_lds_bytes(), ctx->stream, (const TA*)ctx->dA,
                       ctx->ld, (int)ctx->M, ctx->N, cps, Gpart, (const double*)nullptr);
    return hipGetLastError();
}
// G = A A' into Gdst (M x M doubles, device).  The partials are a temporary of the call.
static int bp_form_gram(csmp_ctx* ctx, double* Gdst) {
    int nsplit;
    int64_t cps;
    bp_rowgram_split(ctx, nsplit, cps);
    const size_t MM = (size_t)ctx->M * (size_t)ctx->M;
    DevTmp part;
    CHECK(part.alloc(ctx, (size_t)nsplit * MM * sizeof(double)));
    // 16-byte loads of a column's rows need the column starts on 16-byte boundaries
    const size_t esz = ctx->dtype == CSMP_F32 ? 4 : 8;
    const bool vec = ((uintptr_t)ctx->dA % 16 == 0) && ((size_t)ctx->ld * esz) % 16 == 0 && !ctx->tune_rowgram_scalar;
    hipError_t e;
    if (ctx->dtype == CSMP_F32) e = vec ? rowgram_t<float, true>(ctx, nsplit, cps, (double*)part.p) : rowgram_t<float, false>(ctx, nsplit, cps, (double*)part.p);
    else e = vec ? rowgram_t<double, true>(ctx, nsplit, cps, (double*)part.p) : rowgram_t<double, false>(ctx, nsplit, cps, (double*)part.p);
    HIPCHECK(e);
    hipLaunchKernelGGL(k_rowgram_reduce, dim3((unsigned)((MM + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)part.p, nsplit, (int)ctx->M, Gdst);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(ctx->stream));  // (the partials are released on return)
    return CSMP_OK;
}

// The buffers of the context for the resident dictionary: all of them, or none.
static int bp_ensure(csmp_ctx* ctx) {
    BpBuf& t = ctx->bp;
    if (t.G && t.M == (int)ctx->M) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    bp_free(t);
    BpBuf n;
    const size_t M = (size_t)ctx->M, np = (size_t)bp_np(ctx), npa = 2 * np;
    n.Mp = (int)((M + 255) / 256 * 256);
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.G, M * M));
        CHECK(dmalloc(ctx, &n.Gm, npa * npa));
        CHECK(dmalloc(ctx, &n.pivref, np));
        CHECK(dmalloc(ctx, &n.Dfac, np * kCholNB));
        CHECK(dmalloc(ctx, &n.vec, (size_t)6 * n.Mp));
        CHECK(dmalloc(ctx, &n.rpart, (size_t)2 * kIstaMaxSegs));
        CHECK(dmalloc(ctx, &n.res, (size_t)2));
        CHECK(dmalloc(ctx, &n.st, (size_t)1));
        HIPCHECK(hipMemsetAsync(n.vec, 0, (size_t)6 * n.Mp * sizeof(double), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        bp_free(n);
        return rc;
    }
    n.M = (int)ctx->M;
    n.np = (int)np;
    t = n;
    return CSMP_OK;
}

// G = A A' and G = R'R by the blocked Cholesky of csmp_gram.hpp, augmented by the unit vectors (rw_factor's launches): block rows
// 0 .. ceil(M / 32) - 1, one launch each; then R^-1 beside R^-T.  One host read: the verdict.
static int bp_factor(csmp_ctx* ctx) {
    BpBuf& t = ctx->bp;
    const int M = (int)ctx->M, np = t.np, npa = 2 * np;
    CHECK(bp_form_gram(ctx, t.G));
    HIPCHECK(hipMemsetAsync(t.st, 0, sizeof(DevState), ctx->stream));
    hipLaunchKernelGGL(k_bp_assemble, dim3((unsigned)(((int64_t)npa * npa + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.G, M, np, npa,
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
    {
        PinFetch f(ctx);
        CHECK(f.begin(sizeof hs));
        CHECK(f.add(&hs, t.st, sizeof hs));
        CHECK(f.wait());
    }
    t.factored = true;
    t.notpd = (hs.done & STOP_REORTH) != 0;
    return CSMP_OK;
}

static int bp_nomem(csmp_ctx* ctx, int rc) {
    if (rc == CSMP_EHIP) return fail(ctx, CSMP_ENOMEM, "bp: no device memory for A A' and its factor (" + ctx->err + ")");
    return rc;
}
// everything a solve needs; *did = the call formed and factorised G.  A failed allocation leaves no BpBuf behind.
static int bp_prepare(csmp_ctx* ctx, bool* did) {
    *did = false;
    int rc = solver_ensure(ctx, 1, 1, false);
    if (rc == CSMP_OK) rc = ista_ensure(ctx);
    if (rc == CSMP_OK) rc = bp_ensure(ctx);
    if (rc == CSMP_OK && !ctx->bp.factored) {
        rc = bp_factor(ctx);
        if (rc != CSMP_OK) {
            (void)hipStreamSynchronize(ctx->stream);
            bp_free(ctx->bp);
        }
        *did = rc == CSMP_OK;
    }
    CHECK(bp_nomem(ctx, rc));
    if (ctx->bp.notpd) return fail(ctx, CSMP_EINVAL, "bp: A A' is not positive definite to working precision");
    return CSMP_OK;
}

static int bp_entry(csmp_ctx* ctx, const char* who) {
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, std::string(who) + ": a host-streamed dictionary is not served");
    if (ctx->M > ctx->N) return fail(ctx, CSMP_EDIM, std::string(who) + ": size(A, 1) > size(A, 2): A A' is singular");
    if (ctx->M > kBpMaxRows) return fail(ctx, CSMP_ERANGE, std::string(who) + ": more than 2^19 rows");
    return CSMP_OK;
}
static int bp_check_knobs(csmp_ctx* ctx, const char* who, double rho, int64_t maxiter, double tol, int64_t check_every) {
    if (!std::isfinite(rho) || !(rho > 0.0)) return fail(ctx, CSMP_EINVAL, std::string(who) + ": rho has to be positive and finite");
    if (!std::isfinite(tol) || !(tol > 0.0)) return fail(ctx, CSMP_EINVAL, std::string(who) + ": tol has to be positive and finite");
    if (maxiter < 0) return fail(ctx, CSMP_EINVAL, std::string(who) + ": maxiter has to be non-negative");
    if (check_every < 1) return fail(ctx, CSMP_EINVAL, std::string(who) + ": check_every has to be at least 1");
    return CSMP_OK;
}

// z = u = 0: p = q = 0, e = -b; r = b already (upload_b / init_from_device_t)
static int bp_start(csmp_ctx* ctx) {
    BpBuf& t = ctx->bp;
    IstaBuf& v = ctx->ista;
    const int M = (int)ctx->M;
    HIPCHECK(hipMemsetAsync(v.x, 0, (size_t)ctx->N * sizeof(double), ctx->stream));
    HIPCHECK(hipMemsetAsync(v.y, 0, (size_t)ctx->N * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_bp_start, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, (const double*)ctx->s.b, M, t.vec, t.vec + t.Mp, t.vec + 2 * t.Mp);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// Up to maxiter iterations from the z, u (the context's ista buffers x, y), p, q, e and weights as they stand; the launches of an
// interval of check_every iterations are queued without a wait, then the host reads the two residual norms.
static int bp_iterate(csmp_ctx* ctx, int64_t nw, double rho, int64_t maxiter, double tol, int64_t check_every, int64_t* iters, bool* converged) {
    BpBuf& t = ctx->bp;
    IstaBuf& v = ctx->ista;
    Solver& s = ctx->s;
    const int M = (int)ctx->M, np = t.np, npa = 2 * np;
    double *p = t.vec, *q = t.vec + t.Mp, *e = t.vec + 2 * t.Mp, *vv = t.vec + 3 * t.Mp, *y = t.vec + 4 * t.Mp, *g = t.vec + 5 * t.Mp;
    const double* T = t.Gm + (size_t)np * npa;  // R^-T, lower
    const double* Ri = t.Gm + np;               // R^-1, upper
    const int64_t seg_len = ista_seg_len(ctx->N);
    const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
    const dim3 gv((unsigned)((M + 3) / 4)), gm((unsigned)((M + 255) / 256));
    *iters = 0;
    *converged = false;
    for (int64_t it = 1; it <= maxiter; ++it) {
        hipLaunchKernelGGL(k_bp_gemv, gv, dim3(256), 0, ctx->stream, Ri, (int64_t)npa, M, (int)BP_UPPER, (const double*)e, vv);
        hipLaunchKernelGGL(k_bp_gemv, gv, dim3(256), 0, ctx->stream, T, (int64_t)npa, M, (int)BP_LOWER, (const double*)vv, y);
        hipLaunchKernelGGL(k_bp_gemv, gv, dim3(256), 0, ctx->stream, (const double*)t.G, (int64_t)M, M, (int)BP_FULL, (const double*)y, g);
        HIPCHECK(hipGetLastError());
        CHECK(launch_sweep(ctx, y, 0.0, 0, 0));
        hipLaunchKernelGGL(k_bp_update, dim3(nseg), dim3(kIstaThreads), 0, ctx->stream, (const double*)s.cvec, (const double*)v.w, nw, rho, v.x, v.y,
                           ctx->N, seg_len, v.lidx, v.lval, v.seg_cnt, t.rpart);
        HIPCHECK(hipGetLastError());
        CHECK(ista_residual(ctx));
        hipLaunchKernelGGL(k_bp_pq, gm, dim3(256), 0, ctx->stream, (const double*)s.b, (const double*)s.r, (const double*)g, M, p, q, e);
        HIPCHECK(hipGetLastError());
        *iters = it;
        if (it % check_every == 0) {
            hipLaunchKernelGGL(k_bp_fold, dim3(1), dim3(256), 0, ctx->stream, (const double*)t.rpart, nseg, t.res);
            HIPCHECK(hipGetLastError());
            double res[2];
            {
                PinFetch f(ctx);
                CHECK(f.begin(sizeof res));
                CHECK(f.add(res, t.res, sizeof res));
                CHECK(f.wait());
            }
            if (std::sqrt(res[0]) < tol && rho * std::sqrt(res[1]) < tol) {
                *converged = true;
                break;
            }
        }
    }
    return CSMP_OK;
}

static int bp_upload(csmp_ctx* ctx, const void* b, int b_dtype, int x_loc) {
    ctx->s.begun = false;
    if (x_loc == CSMP_DEVICE)
        return b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)b) : init_from_device_t<double>(ctx, (const double*)b);
    return upload_b(ctx, b, b_dtype);  // r = b: the residual of z = 0
}

extern "C" int csmp_bp(csmp_ctx* ctx, const void* b, int b_dtype, const double* w, int64_t nw, double rho, int64_t maxiter, double tol,
                       int64_t check_every, double* x, int x_loc, int64_t* iterations, double* resnorm, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || !w || !x) return fail(ctx, CSMP_EINVAL, "bp: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "bp: x_loc must be CSMP_HOST or CSMP_DEVICE");
    CHECK(bp_entry(ctx, "bp"));
    if (nw != 1 && nw != ctx->N) return fail(ctx, CSMP_EDIM, "bp: length(w) must be 1 or size(A, 2)");
    CHECK(bp_check_knobs(ctx, "bp", rho, maxiter, tol, check_every));
    for (int64_t i = 0; i < nw; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(ctx, CSMP_EINVAL, "bp: the weights have to be non-negative and finite");
    HIPCHECK(hipSetDevice(ctx->dev));
    bool did = false;
    CHECK(bp_prepare(ctx, &did));
    CHECK(bp_upload(ctx, b, b_dtype, x_loc));
    HIPCHECK(hipMemcpyAsync(ctx->ista.w, w, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CHECK(bp_start(ctx));
    int64_t iters = 0;
    bool conv = false;
    CHECK(bp_iterate(ctx, nw, rho, maxiter, tol, check_every, &iters, &conv));
    if (resnorm) CHECK(residual_norm(ctx, resnorm));  // r = b - A z of the last iteration (r = b where there was none)
    HIPCHECK(hipMemcpyAsync(x, ctx->ista.x, (size_t)ctx->N * sizeof(double), x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                            ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    if (iterations) *iterations = iters;
    if (flags) *flags = (conv ? CSMP_BP_CONVERGED : 0) | (did ? CSMP_BP_FACTORED : 0);
    return CSMP_OK;
}

// basispursuit_reweighting (:18-31) around csmp_bp's solve.  csmp_ista_reweighted's loop written a second time: the solver, its warm
// start (z, u, p, q stay as the previous solve left them) and the weights' scale differ.
extern "C" int csmp_bp_reweighted(csmp_ctx* ctx, const void* b, int b_dtype, int scheme, double eps, int64_t ard_iter, int64_t outer_maxiter,
                                  double min_decrease, double rho, int64_t maxiter, double tol, int64_t check_every, double* x, int x_loc,
                                  double* w_out, int64_t* outer_done, double* resnorm) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || !x) return fail(ctx, CSMP_EINVAL, "bp_reweighted: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "bp_reweighted: x_loc must be CSMP_HOST or CSMP_DEVICE");
    if (scheme != CSMP_REWEIGHT_CANDES && scheme != CSMP_REWEIGHT_ARD)
        return fail(ctx, CSMP_EINVAL, "bp_reweighted: scheme must be CSMP_REWEIGHT_CANDES or CSMP_REWEIGHT_ARD");
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(ctx, CSMP_EINVAL, "bp_reweighted: eps has to be positive and finite");
    if (ard_iter < 1) return fail(ctx, CSMP_EINVAL, "bp_reweighted: ard_iter has to be at least 1");
    if (outer_maxiter < 1) return fail(ctx, CSMP_EINVAL, "bp_reweighted: the outer maxiter has to be at least 1");
    if (!(min_decrease >= 0.0)) return fail(ctx, CSMP_EINVAL, "bp_reweighted: min_decrease has to be non-negative");
    CHECK(bp_entry(ctx, "bp_reweighted"));
    CHECK(bp_check_knobs(ctx, "bp_reweighted", rho, maxiter, tol, check_every));
    HIPCHECK(hipSetDevice(ctx->dev));
    bool did = false;
    CHECK(bp_prepare(ctx, &did));
    CHECK(rw_nomem(ctx, rw_ensure(ctx), "bp_reweighted"));
    IstaBuf& t = ctx->ista;
    RwBuf& u = ctx->rw;
    const int64_t N = ctx->N;
    const unsigned gridN = (unsigned)((N + 255) / 256);
    CHECK(bp_upload(ctx, b, b_dtype, x_loc));
    const double one = 1.0;
    HIPCHECK(hipMemcpyAsync(t.w, &one, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CHECK(bp_start(ctx));
    {  // w = ones(N) (:21): the Candes weights of an "x" of zeros at eps = 1 -- exactly 1.0
        HIPCHECK(hipMemsetAsync(u.info, 0, sizeof(RwInfo), ctx->stream));
        hipLaunchKernelGGL(k_rw_candes, dim3(gridN), dim3(256), 0, ctx->stream, (const double*)t.x, N, 1.0, 1.0, u.w, u.xprev, u.info);
        HIPCHECK(hipGetLastError());
    }
    int64_t iters = 0;
    bool conv = false;
    CHECK(bp_iterate(ctx, 1, rho, maxiter, tol, check_every, &iters, &conv));  // x = solve(w = 1)
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
        CHECK(bp_iterate(ctx, N, rho, maxiter, tol, check_every, &iters, &conv));  // xs = solve(w), warm-started
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
        if (info.flags & RW_BAD_RESULT) return fail(ctx, CSMP_EINVAL, "bp_reweighted: weights contain NaN or Inf");
        double n2 = 0.0;
        for (int q = 0; q < kRwNormParts; ++q) n2 += part[q];
        if (std::sqrt(n2) < min_decrease) break;  // norm(xs - x) < min_decrease: return xs (:25)
    }
    if (resnorm) CHECK(residual_norm(ctx, resnorm));
    const hipMemcpyKind out = x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHECK(hipMemcpyAsync(x, t.x, (size_t)N * sizeof(double), out, ctx->stream));
    if (w_out) HIPCHECK(hipMemcpyAsync(w_out, u.w, (size_t)N * sizeof(double), out, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    if (outer_done) *outer_done = done;
    return CSMP_OK;
}

// ------------------------------------------------------------------------------------------ measurement (include/csmp_internal.h)
extern "C" int csmp_bp_rowgram(csmp_ctx* ctx, double* G_out, int loc) {
    if (!ctx) return CSMP_EINVAL;
    if (!G_out || (loc != CSMP_HOST && loc != CSMP_DEVICE)) return fail(ctx, CSMP_EINVAL, "bp_rowgram: bad arguments");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, "bp_rowgram: a host-streamed dictionary is not served");
    if (ctx->M > kBpMaxRows) return fail(ctx, CSMP_ERANGE, "bp_rowgram: more than 2^19 rows");
    HIPCHECK(hipSetDevice(ctx->dev));
    const size_t bytes = (size_t)ctx->M * (size_t)ctx->M * sizeof(double);
    if (loc == CSMP_DEVICE) return bp_nomem(ctx, bp_form_gram(ctx, G_out));
    DevTmp G;
    CHECK(bp_nomem(ctx, G.alloc(ctx, bytes)));
    CHECK(bp_nomem(ctx, bp_form_gram(ctx, (double*)G.p)));
    HIPCHECK(hipMemcpyAsync(G_out, G.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    return CSMP_OK;
}
