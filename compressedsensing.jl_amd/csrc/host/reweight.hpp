// host/reweight.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_ard_weights (ard_weights!, src/basispursuit.jl:49-65) and csmp_ista_reweighted (basispursuit_reweighting with candes_function /
// ard_function, :18-44,67-73, around ista / fista).
// ------------------------------------------------------------------------------------------ reweighted l1
static int rw_kmax(const csmp_ctx* ctx) { return (int)std::min<int64_t>(ctx->M, CSMP_ARD_KMAX); }
static int64_t rw_ldw(const csmp_ctx* ctx) { return (ctx->M + kRbRows - 1) / kRbRows * kRbRows; }  // whole row blocks of k_ard_forms
static int64_t rw_ldo(const csmp_ctx* ctx) { return (ctx->M + 15) / 16 * 16; }                    // rows of the gathered columns (k_gather_cols)

// The buffers sized by the dictionary: all of them, or none.
static int rw_ensure(csmp_ctx* ctx) {
    RwBuf& t = ctx->rw;
    if (t.w && t.N == ctx->N) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    rw_free(t);
    RwBuf n;
    const size_t N = (size_t)ctx->N;
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.w, N));
        CHECK(dmalloc(ctx, &n.xprev, N));
        CHECK(dmalloc(ctx, &n.xin, N));
        CHECK(dmalloc(ctx, &n.npart, (size_t)kRwNormParts));
        CHECK(dmalloc(ctx, &n.zeroM, (size_t)ctx->M));
        CHECK(dmalloc(ctx, &n.cols, (size_t)CSMP_ARD_KMAX));
        CHECK(dmalloc(ctx, &n.info, (size_t)1));
        CHECK(dmalloc(ctx, &n.st, (size_t)1));
        HIPCHECK(hipMemsetAsync(n.zeroM, 0, (size_t)ctx->M * sizeof(double), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        rw_free(n);
        return rc;
    }
    n.N = ctx->N;
    t = n;
    return CSMP_OK;
}

static int rw_nomem(csmp_ctx* ctx, int rc, const char* who) {
    if (rc == CSMP_EHIP) return fail(ctx, CSMP_ENOMEM, std::string(who) + ": no device memory for the weights (" + ctx->err + ")");
    return rc;
}

// k_gram's row slices for a support of np columns: a function of the shape alone, so that the summation order -- and with it every
// bit of the result -- does not depend on what the context ran before
static int rw_split_for(const csmp_ctx* ctx, int np) { return gram_split_for(ctx, np, 0, np); }

// The buffers sized by the support (np columns, whole 64-column tiles): all of them, or none of THEM (the dictionary-sized ones stay).
static int rw_ensure_support(csmp_ctx* ctx, int np) {
    RwBuf& t = ctx->rw;
    if (t.np == np) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    rw_free_support(t);
    const int nsplit = rw_split_for(ctx, np), npa = 2 * np;
    const size_t esz = ctx->dtype == CSMP_F32 ? 4 : 8;
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &t.xS, (size_t)np));
        CHECK(dmalloc(ctx, &t.wS, (size_t)np));
        CHECK(dmalloc(ctx, &t.Gs, (size_t)np * np));
        CHECK(dmalloc(ctx, &t.Y, (size_t)np * np));
        CHECK(dmalloc(ctx, &t.Gm, (size_t)npa * npa));
        CHECK(dmalloc(ctx, &t.Gpart, (size_t)nsplit * np * np));
        CHECK(dmalloc(ctx, &t.gdiag, (size_t)np));
        CHECK(dmalloc(ctx, &t.Dfac, (size_t)np * kCholNB));
        CHECK(dmalloc(ctx, &t.rhs_part, (size_t)np * (size_t)((rw_ldo(ctx) + 255) / 256)));
        CHECK(dmalloc(ctx, &t.W, (size_t)rw_ldw(ctx) * (size_t)np));
        CHECK(dmalloc(ctx, &t.Acomp, (size_t)np * (size_t)rw_ldo(ctx) * esz));
        // the DGKS reference of the Cholesky kernels (csmp_gram.hpp): zero -- a pivot fails only by not being positive
        HIPCHECK(hipMemsetAsync(t.gdiag, 0, (size_t)np * sizeof(double), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        rw_free_support(t);
        return rc;
    }
    t.np = np;
    t.nsplit = nsplit;
    return CSMP_OK;
}

template <typename TA, bool VEC>
static hipError_t ard_forms_t(csmp_ctx* ctx, int k, double eps) {
    RwBuf& t = ctx->rw;
    auto kern = k_ard_forms<TA, VEC>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fr_rebuild_lds_bytes());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)((ctx->N + 127) / 128)), dim3(256), fr_rebuild_lds_bytes(), ctx->stream, (const TA*)ctx->dA, ctx->ld,
                       (int)ctx->M, ctx->N, (const double*)t.W, rw_ldw(ctx), k, eps, t.w);
    return hipGetLastError();
}
static int launch_ard_forms(csmp_ctx* ctx, int k, double eps) {
    // 16-byte loads of a column's rows need the column starts on 16-byte boundaries
    const size_t esz = ctx->dtype == CSMP_F32 ? 4 : 8;
    const bool vec = ((uintptr_t)ctx->dA % 16 == 0) && ((size_t)ctx->ld * esz) % 16 == 0;
    hipError_t e;
    if (ctx->dtype == CSMP_F32) e = vec ? ard_forms_t<float, true>(ctx, k, eps) : ard_forms_t<float, false>(ctx, k, eps);
    else e = vec ? ard_forms_t<double, true>(ctx, k, eps) : ard_forms_t<double, false>(ctx, k, eps);
    HIPCHECK(e);
    return CSMP_OK;
}

// G = A_S'A_S of the listed support: the gather and the Gram kernel of the whole-set least squares (csmp_gram.hpp), then the symmetric copy
template <typename TA>
static int rw_gram_t(csmp_ctx* ctx, int k) {
    RwBuf& t = ctx->rw;
    const int np = t.np, M = (int)ctx->M, nsplit = t.nsplit;
    const int64_t ldo = rw_ldo(ctx);
    const int nchunk = (int)((ldo + 255) / 256);
    const int rps = (((M + nsplit - 1) / nsplit + 15) / 16) * 16;
    hipLaunchKernelGGL(k_gather_cols<TA>, dim3((unsigned)nchunk, np), dim3(256), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld, M, (const int*)t.cols, k,
                       (TA*)t.Acomp, ldo, (const double*)t.zeroM, np, t.rhs_part);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_gram<TA>, dim3(np / kGramWgJ, (np + kGramWgI - 1) / kGramWgI, nsplit), dim3(256), 0, ctx->stream, (const TA*)t.Acomp, ldo, np,
                       rps, t.Gpart, 0, (k + kGramWgJ - 1) / kGramWgJ);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_rw_gram_sym, dim3((unsigned)(((int64_t)np * np + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.Gpart, nsplit, k, np,
                       t.Gs);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}
template <typename TA>
static int rw_dirs_t(csmp_ctx* ctx, int k) {
    RwBuf& t = ctx->rw;
    const int np = t.np, npa = 2 * np;
    const int64_t ldw = rw_ldw(ctx);
    hipLaunchKernelGGL(k_rw_dirs<TA>, dim3((unsigned)(ldw / 32), (unsigned)((k + 31) / 32)), dim3(256), 0, ctx->stream, (const TA*)t.Acomp, rw_ldo(ctx),
                       (const double*)(t.Gm + (size_t)np * npa), npa, k, t.W, ldw);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// H = L L' by the blocked Cholesky of csmp_gram.hpp, augmented by the unit vectors: block rows 0 .. ceil(k / 32) - 1, one launch each
static int rw_factor(csmp_ctx* ctx, int k, double eps) {
    RwBuf& t = ctx->rw;
    const int np = t.np, npa = 2 * np;
    hipLaunchKernelGGL(k_rw_assemble, dim3((unsigned)(((int64_t)npa * npa + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.Gs,
                       (const double*)t.xS, (const double*)t.wS, eps, k, np, npa, t.Gm);
    HIPCHECK(hipGetLastError());
    const int nsteps = (k + kCholNB - 1) / kCholNB;
    {
        const int left0 = npa - kCholNB;
        hipLaunchKernelGGL(k_chol_row, dim3(std::max(1, (left0 + kCholRowCols - 1) / kCholRowCols)), dim3(kCholThreads), 0, ctx->stream, t.Gm, npa, k, 0,
                           (const double*)t.gdiag, t.st, t.Dfac);
    }
    for (int kb = 0; kb + 1 < nsteps; ++kb) {
        const int left = npa - (kb + 1) * kCholNB;
        const int left2 = left - kCholNB;
        const int Tt = (left + kGramTile - 1) / kGramTile;
        const int ntrail = left > kCholNB ? Tt * (Tt + 1) / 2 : 0;
        const int nrow = std::max(1, (left2 + kCholRowCols - 1) / kCholRowCols);
        hipLaunchKernelGGL(k_chol_step, dim3(nrow + ntrail), dim3(kCholThreads), 0, ctx->stream, t.Gm, npa, k, kb, (const double*)t.gdiag, t.st, nrow,
                           t.Dfac, np);
    }
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// ard_weights!(w, A, x, eps, iter) on the device: t.w (N weights) is updated in place from x (N doubles, device), for supports of up
// to kmax atoms.  Two host reads:
// the support's size (the launches are sized by it) and the factorisation's verdict.
static int rw_ard(csmp_ctx* ctx, const double* x, double eps, int64_t iter, int kmax) {
    RwBuf& t = ctx->rw;
    HIPCHECK(hipMemsetAsync(t.st, 0, sizeof(DevState), ctx->stream));
    hipLaunchKernelGGL(k_rw_support, dim3(1), dim3(256), 0, ctx->stream, x, (const double*)t.w, ctx->N, kmax, t.cols, t.info);
    HIPCHECK(hipGetLastError());
    RwInfo info{};
    {
        PinFetch f(ctx);
        CHECK(f.begin(sizeof info));
        CHECK(f.add(&info, t.info, sizeof info));
        CHECK(f.wait());
    }
    if (info.flags & RW_BAD_WEIGHT) return fail(ctx, CSMP_EINVAL, "ard_weights: weights cannot be zero (every weight has to be positive and finite)");
    if (info.flags & RW_BAD_X) return fail(ctx, CSMP_EINVAL, "ard_weights: x has to be finite");
    if (info.nnz > kmax)
        return fail(ctx, CSMP_ERANGE, "ard_weights: nnz(x) = " + std::to_string(info.nnz) + " but at most " + std::to_string(kmax) + " are taken");
    const int k = info.nnz;
    const int np = std::max(1, (k + kGramTile - 1) / kGramTile) * kGramTile;
    CHECK(rw_nomem(ctx, rw_ensure_support(ctx, np), "ard_weights"));
    if (k > 0) {
        hipLaunchKernelGGL(k_rw_gather_s, dim3((k + 255) / 256), dim3(256), 0, ctx->stream, x, (const double*)t.w, (const int*)t.cols, k, t.xS, t.wS);
        HIPCHECK(hipGetLastError());
        CHECK(ctx->dtype == CSMP_F32 ? rw_gram_t<float>(ctx, k) : rw_gram_t<double>(ctx, k));
        for (int64_t it = 1; it <= iter; ++it) {
            CHECK(rw_factor(ctx, k, eps));
            if (it < iter) {  // w_S alone: Y = L^-1 G, then the k quadratic forms
                hipLaunchKernelGGL(k_wgemm, dim3((k + 31) / 32, (k + 31) / 32), dim3(256), 0, ctx->stream, (const double*)(t.Gm + (size_t)np * 2 * np),
                                   2 * np, (const double*)t.Gs, np, k, k, t.Y, np);
                HIPCHECK(hipGetLastError());
                hipLaunchKernelGGL(k_rw_inner_w, dim3((k + 3) / 4), dim3(256), 0, ctx->stream, (const double*)t.Gs, (const double*)t.Y, k, np, eps,
                                   (const DevState*)t.st, t.wS);
                HIPCHECK(hipGetLastError());
            }
        }
        CHECK(ctx->dtype == CSMP_F32 ? rw_dirs_t<float>(ctx, k) : rw_dirs_t<double>(ctx, k));
    }
    CHECK(launch_ard_forms(ctx, k, eps));
    DevState hs{};
    {
        PinFetch f(ctx);
        CHECK(f.begin(sizeof hs));
        CHECK(f.add(&hs, t.st, sizeof hs));
        CHECK(f.wait());
    }
    if (hs.done & STOP_REORTH) return fail(ctx, CSMP_EINVAL, "ard_weights: eps diag(w ./ |x|) + A_S'A_S is not positive definite to working precision");
    return CSMP_OK;
}

static int rw_entry(csmp_ctx* ctx, const char* who) {
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, std::string(who) + ": a host-streamed dictionary is not served");
    return CSMP_OK;
}
extern "C" int csmp_ard_weights(csmp_ctx* ctx, const double* x, const double* w_in, double eps, int64_t iter, double* w_out, int loc) {
    if (!ctx) return CSMP_EINVAL;
    if (!x || !w_in || !w_out) return fail(ctx, CSMP_EINVAL, "ard_weights: bad arguments");
    if (loc != CSMP_HOST && loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "ard_weights: loc must be CSMP_HOST or CSMP_DEVICE");
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(ctx, CSMP_EINVAL, "ard_weights: eps has to be positive and finite");
    if (iter < 1) return fail(ctx, CSMP_EINVAL, "ard_weights: iter has to be at least 1");
    CHECK(rw_entry(ctx, "ard_weights"));
    HIPCHECK(hipSetDevice(ctx->dev));
    CHECK(rw_nomem(ctx, rw_ensure(ctx), "ard_weights"));
    RwBuf& t = ctx->rw;
    const size_t bytes = (size_t)ctx->N * sizeof(double);
    const hipMemcpyKind in = loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIPCHECK(hipMemcpyAsync(t.xin, x, bytes, in, ctx->stream));
    HIPCHECK(hipMemcpyAsync(t.w, w_in, bytes, in, ctx->stream));
    CHECK(rw_ard(ctx, t.xin, eps, iter, rw_kmax(ctx)));
    HIPCHECK(hipMemcpyAsync(w_out, t.w, bytes, loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    return CSMP_OK;
}

extern "C" int csmp_ista_reweighted(csmp_ctx* ctx, const void* b, int b_dtype, double lambda, int scheme, double eps, int64_t ard_iter,
                                    int64_t outer_maxiter, double min_decrease, int64_t maxiter, double stepsize, int accel, double* x, int x_loc,
                                    double* w_out, int64_t* outer_done, double* resnorm) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || !x) return fail(ctx, CSMP_EINVAL, "ista_reweighted: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "ista_reweighted: x_loc must be CSMP_HOST or CSMP_DEVICE");
    if (accel != 0 && accel != 1) return fail(ctx, CSMP_EINVAL, "ista_reweighted: accel must be 0 (ISTA) or 1 (FISTA)");
    if (scheme != CSMP_REWEIGHT_CANDES && scheme != CSMP_REWEIGHT_ARD)
        return fail(ctx, CSMP_EINVAL, "ista_reweighted: scheme must be CSMP_REWEIGHT_CANDES or CSMP_REWEIGHT_ARD");
    if (!std::isfinite(lambda) || lambda < 0.0) return fail(ctx, CSMP_EINVAL, "ista_reweighted: lambda has to be non-negative and finite");
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(ctx, CSMP_EINVAL, "ista_reweighted: eps has to be positive and finite");
    if (ard_iter < 1) return fail(ctx, CSMP_EINVAL, "ista_reweighted: ard_iter has to be at least 1");
    if (outer_maxiter < 1) return fail(ctx, CSMP_EINVAL, "ista_reweighted: the outer maxiter has to be at least 1");
    if (!(min_decrease >= 0.0)) return fail(ctx, CSMP_EINVAL, "ista_reweighted: min_decrease has to be non-negative");
    if (maxiter < 0) return fail(ctx, CSMP_EINVAL, "ista_reweighted: maxiter has to be non-negative");
    if (!std::isfinite(stepsize) || !(stepsize > 0.0)) return fail(ctx, CSMP_EINVAL, "ista_reweighted: stepsize has to be positive and finite");
    CHECK(rw_entry(ctx, "ista_reweighted"));
    HIPCHECK(hipSetDevice(ctx->dev));
    {
        int rc = solver_ensure(ctx, 1, 1, false);
        if (rc == CSMP_OK) rc = ista_ensure(ctx);
        if (rc == CSMP_OK) rc = rw_ensure(ctx);
        CHECK(rw_nomem(ctx, rc, "ista_reweighted"));
    }
    Solver& s = ctx->s;
    IstaBuf& t = ctx->ista;
    RwBuf& u = ctx->rw;
    const int64_t N = ctx->N;
    const unsigned gridN = (unsigned)((N + 255) / 256);
    s.begun = false;
    if (x_loc == CSMP_DEVICE)
        CHECK(b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)b) : init_from_device_t<double>(ctx, (const double*)b));
    else
        CHECK(upload_b(ctx, b, b_dtype));  // r = b: the residual of x = 0
    // x = solve(w = 1): the plain csmp_ista call with the one weight lambda
    HIPCHECK(hipMemcpyAsync(t.w, &lambda, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipMemsetAsync(t.x, 0, (size_t)N * sizeof(double), ctx->stream));
    HIPCHECK(hipMemsetAsync(t.y, 0, (size_t)N * sizeof(double), ctx->stream));
    {  // w = ones(N) (:21): lambda = 1 times the Candes weights of an "x" of zeros at eps = 1 -- exactly 1.0
        HIPCHECK(hipMemsetAsync(u.info, 0, sizeof(RwInfo), ctx->stream));
        hipLaunchKernelGGL(k_rw_candes, dim3(gridN), dim3(256), 0, ctx->stream, (const double*)t.x, N, 1.0, 1.0, u.w, u.xprev, u.info);
        HIPCHECK(hipGetLastError());
    }
    bool listed = false;
    CHECK(ista_iterate(ctx, 1, maxiter, stepsize, accel, listed));
    int64_t done = 1;
    for (int64_t i = 2; i <= outer_maxiter; ++i) {
        HIPCHECK(hipMemcpyAsync(u.xprev, t.x, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        if (scheme == CSMP_REWEIGHT_CANDES) {
            HIPCHECK(hipMemsetAsync(u.info, 0, sizeof(RwInfo), ctx->stream));
            hipLaunchKernelGGL(k_rw_candes, dim3(gridN), dim3(256), 0, ctx->stream, (const double*)t.x, N, eps, lambda, u.w, t.w, u.info);
            HIPCHECK(hipGetLastError());
        } else {
            CHECK(rw_ard(ctx, t.x, eps, ard_iter, CSMP_ARD_KMAX));  // (an iterate is no basic solution: its support may exceed M)
            hipLaunchKernelGGL(k_rw_scale, dim3(gridN), dim3(256), 0, ctx->stream, (const double*)u.w, N, lambda, t.w, u.info);
            HIPCHECK(hipGetLastError());
        }
        // xs = solve(lambda w), warm-started from x: y = x, t_1 = 1, the list and r of x
        HIPCHECK(hipMemcpyAsync(t.y, t.x, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        CHECK(ista_launch_update(ctx, N, 0.0, 0.0, ISTA_INIT | ISTA_LIST_X));
        listed = true;
        CHECK(ista_iterate(ctx, N, maxiter, stepsize, accel, listed));
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
        if (info.flags & RW_BAD_RESULT) return fail(ctx, CSMP_EINVAL, "ista_reweighted: weights contain NaN or Inf");
        double n2 = 0.0;
        for (int q = 0; q < kRwNormParts; ++q) n2 += part[q];
        if (std::sqrt(n2) < min_decrease) break;  // norm(xs - x) < min_decrease: return xs (:25)
    }
    if (resnorm) {
        if (listed) CHECK(ista_residual(ctx));
        CHECK(residual_norm(ctx, resnorm));
    }
    const hipMemcpyKind out = x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHECK(hipMemcpyAsync(x, t.x, (size_t)N * sizeof(double), out, ctx->stream));
    if (w_out) HIPCHECK(hipMemcpyAsync(w_out, u.w, (size_t)N * sizeof(double), out, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    if (outer_done) *outer_done = done;
    return CSMP_OK;
}

// ------------------------------------------------------------------------------------------ measurement (include/csmp_internal.h)
template <typename TA, bool VEC>
static hipError_t rw_split_block_t(csmp_ctx* ctx, int d0, int nd, double* rho2) {
    auto kern = k_fr_rebuild_lds<TA, VEC>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fr_rebuild_lds_bytes());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)((ctx->N + 127) / 128)), dim3(256), fr_rebuild_lds_bytes(), ctx->stream, (const TA*)ctx->dA, ctx->ld,
                       (int)ctx->M, ctx->N, (const double*)ctx->rw.W, rw_ldw(ctx), d0, nd, rho2);
    return hipGetLastError();
}
// the N-pass as the EXISTING kernel would run it: |a_j|^2 by k_fr_colnorm2, one k_fr_rebuild_lds launch per block of 128 directions
// (each a read-modify-write of rho2), then the root -- into xprev / xin, scratch outside a solve
static int rw_split_forms(csmp_ctx* ctx, int k, double eps) {
    RwBuf& t = ctx->rw;
    const size_t esz = ctx->dtype == CSMP_F32 ? 4 : 8;
    const bool vec = ((uintptr_t)ctx->dA % 16 == 0) && ((size_t)ctx->ld * esz) % 16 == 0;
    const unsigned grid = (unsigned)((ctx->N + 3) / 4);
    if (ctx->dtype == CSMP_F32)
        hipLaunchKernelGGL(k_fr_colnorm2<float>, dim3(grid), dim3(256), 0, ctx->stream, (const float*)ctx->dA, ctx->ld, (int)ctx->M, ctx->N, t.xprev);
    else
        hipLaunchKernelGGL(k_fr_colnorm2<double>, dim3(grid), dim3(256), 0, ctx->stream, (const double*)ctx->dA, ctx->ld, (int)ctx->M, ctx->N, t.xprev);
    HIPCHECK(hipGetLastError());
    for (int d0 = 0; d0 < k; d0 += kRbDirs) {
        const int nd = std::min(kRbDirs, k - d0);
        hipError_t e;
        if (ctx->dtype == CSMP_F32) e = vec ? rw_split_block_t<float, true>(ctx, d0, nd, t.xprev) : rw_split_block_t<float, false>(ctx, d0, nd, t.xprev);
        else e = vec ? rw_split_block_t<double, true>(ctx, d0, nd, t.xprev) : rw_split_block_t<double, false>(ctx, d0, nd, t.xprev);
        HIPCHECK(e);
    }
    hipLaunchKernelGGL(k_rw_split_root, dim3((unsigned)((ctx->N + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.xprev, ctx->N, eps, t.xin);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

extern "C" int csmp_bench_ard_forms(csmp_ctx* ctx, int variant, int reps, double eps, double* avg_ms, double* max_diff) {
    if (!ctx || reps < 1 || (variant != 0 && variant != 1) || !(eps > 0.0)) return CSMP_EINVAL;
    CHECK(rw_entry(ctx, "bench_ard_forms"));
    RwBuf& t = ctx->rw;
    if (!t.w || t.N != ctx->N || t.np == 0) return fail(ctx, CSMP_ESTATE, "bench_ard_forms: no directions (call csmp_ard_weights first)");
    HIPCHECK(hipSetDevice(ctx->dev));
    RwInfo info{};
    HIPCHECK(hipMemcpy(&info, t.info, sizeof info, hipMemcpyDeviceToHost));
    const int k = std::min(info.nnz, t.np);
    auto run = [&]() -> int { return variant == 0 ? launch_ard_forms(ctx, k, eps) : rw_split_forms(ctx, k, eps); };
    CHECK(run());
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0));
    HIPCHECK(hipEventCreate(&e1));
    HIPCHECK(hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < reps; ++i) CHECK(run());
    HIPCHECK(hipEventRecord(e1, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    float ms0 = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms0, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (avg_ms) *avg_ms = (double)ms0 / reps;
    if (max_diff) {  // the two forms against each other: max |w_fused - w_split|
        CHECK(launch_ard_forms(ctx, k, eps));
        CHECK(rw_split_forms(ctx, k, eps));
        std::vector<double> a((size_t)ctx->N), b((size_t)ctx->N);
        HIPCHECK(hipMemcpyAsync(a.data(), t.w, a.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHECK(hipMemcpyAsync(b.data(), t.xin, b.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        double d = 0.0;
        for (size_t j = 0; j < a.size(); ++j) d = std::max(d, std::fabs(a[j] - b[j]));
        *max_diff = d;
    }
    return CSMP_OK;
}
