// host/sbl.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_sbl (sbl / update!(::SBL), src/sbl.jl:1-51, in the Woodbury form).  One update is the weighted row Gram matrix A Gamma A' and its
// reduction, the blocked Cholesky of C = sigma2 I + A Gamma A' in the augmented form (bp_factor's launches), t = L^-1 b, the N-pass
// k_sbl_forms and the element-wise step -- and ONE host read: the factorisation's verdict, |gam+ - gam|^2 and the verdict on gam+.
// The buffers live in the context's SblBuf, apart from csmp_bp's and csmp_bpd's kept factors: no call here reads or invalidates them.
// ------------------------------------------------------------------------------------------ sparse Bayesian learning
static bool sbl_vec(const csmp_ctx* ctx) {
    // 16-byte loads of a column's rows need the column starts on 16-byte boundaries
    const size_t esz = ctx->dtype == CSMP_F32 ? 4 : 8;
    return ((uintptr_t)ctx->dA % 16 == 0) && ((size_t)ctx->ld * esz) % 16 == 0 && !ctx->tune_sbl_scalar;
}
static int64_t sbl_ldw(const csmp_ctx* ctx) { return (ctx->M + kRbRows - 1) / kRbRows * kRbRows; }  // whole row blocks of k_sbl_forms

template <typename TA, bool VEC>
static hipError_t rowgram_w_t(csmp_ctx* ctx, int nsplit, int64_t cps, double* Gpart, const double* gam) {
    auto kern = k_rowgram<TA, VEC, true>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rowgram_lds_bytes());
    if (e != hipSuccess) return e;
    const int64_t T = (ctx->M + kRgTile - 1) / kRgTile;
    hipLaunchKernelGGL(kern, dim3((unsigned)(T * (T + 1) / 2), (unsigned)nsplit), dim3(256), rowgram_lds_bytes(), ctx->stream, (const TA*)ctx->dA,
                       ctx->ld, (int)ctx->M, ctx->N, cps, Gpart, gam);
    return hipGetLastError();
}
// Gdst = A diag(gam) A' (M x M doubles, full and exactly symmetric) through the nsplit partials in Gpart: bp_rowgram_split's splits, so
// the bits depend on the shape and the device alone.  Two launches, no wait.
static int sbl_gram(csmp_ctx* ctx, const double* gam, int nsplit, int64_t cps, double* Gpart, double* Gdst) {
    const bool vec = sbl_vec(ctx);
    hipError_t e;
    if (ctx->dtype == CSMP_F32) e = vec ? rowgram_w_t<float, true>(ctx, nsplit, cps, Gpart, gam) : rowgram_w_t<float, false>(ctx, nsplit, cps, Gpart, gam);
    else e = vec ? rowgram_w_t<double, true>(ctx, nsplit, cps, Gpart, gam) : rowgram_w_t<double, false>(ctx, nsplit, cps, Gpart, gam);
    HIPCHECK(e);
    const size_t MM = (size_t)ctx->M * (size_t)ctx->M;
    hipLaunchKernelGGL(k_rowgram_reduce, dim3((unsigned)((MM + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)Gpart, nsplit, (int)ctx->M, Gdst);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

template <typename TA, bool VEC>
static hipError_t sbl_forms_t(csmp_ctx* ctx, const double* W, int64_t ldw, const double* t, double* s, double* q) {
    auto kern = k_sbl_forms<TA, VEC>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fr_rebuild_lds_bytes());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)((ctx->N + 127) / 128)), dim3(256), fr_rebuild_lds_bytes(), ctx->stream, (const TA*)ctx->dA, ctx->ld,
                       (int)ctx->M, ctx->N, W, ldw, t, s, q);
    return hipGetLastError();
}
// s, q (N doubles each) from the directions W (upper triangular, leading dimension ldw: whole 64-row blocks) and t.  One launch.
static int sbl_launch_forms(csmp_ctx* ctx, const double* W, int64_t ldw, const double* t, double* s, double* q) {
    const bool vec = sbl_vec(ctx);
    hipError_t e;
    if (ctx->dtype == CSMP_F32) e = vec ? sbl_forms_t<float, true>(ctx, W, ldw, t, s, q) : sbl_forms_t<float, false>(ctx, W, ldw, t, s, q);
    else e = vec ? sbl_forms_t<double, true>(ctx, W, ldw, t, s, q) : sbl_forms_t<double, false>(ctx, W, ldw, t, s, q);
    HIPCHECK(e);
    return CSMP_OK;
}

// The buffers of the context for the resident dictionary: all of them, or none.
static int sbl_ensure(csmp_ctx* ctx) {
    SblBuf& t = ctx->sbl;
    if (t.Gm && t.M == (int)ctx->M && t.N == ctx->N) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    sbl_free(t);
    SblBuf n;
    const size_t M = (size_t)ctx->M, N = (size_t)ctx->N, np = (size_t)bp_np(ctx), npa = 2 * np;
    n.Mp = (int)((M + 255) / 256 * 256);
    bp_rowgram_split(ctx, n.nsplit, n.cps);
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.Gpart, (size_t)n.nsplit * M * M));
        CHECK(dmalloc(ctx, &n.G, M * M));
        CHECK(dmalloc(ctx, &n.Gm, npa * npa));
        CHECK(dmalloc(ctx, &n.pivref, np));
        CHECK(dmalloc(ctx, &n.Dfac, np * kCholNB));
        CHECK(dmalloc(ctx, &n.vec, (size_t)2 * n.Mp));
        CHECK(dmalloc(ctx, &n.gam, N));
        CHECK(dmalloc(ctx, &n.s, N));
        CHECK(dmalloc(ctx, &n.q, N));
        CHECK(dmalloc(ctx, &n.x, N));
        CHECK(dmalloc(ctx, &n.part, (size_t)kSblParts));
        CHECK(dmalloc(ctx, &n.info, (size_t)1));
        CHECK(dmalloc(ctx, &n.st, (size_t)1));
        // (k_sbl_forms reads t up to whole blocks of 128 directions: zeros beyond M, which no kernel writes)
        HIPCHECK(hipMemsetAsync(n.vec, 0, (size_t)2 * n.Mp * sizeof(double), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        sbl_free(n);
        return rc;
    }
    n.M = (int)ctx->M;
    n.N = ctx->N;
    n.np = (int)np;
    t = n;
    return CSMP_OK;
}
static int sbl_nomem(csmp_ctx* ctx, int rc) {
    if (rc == CSMP_EHIP) return fail(ctx, CSMP_ENOMEM, "sbl: no device memory for sigma2 I + A Gamma A' and its factor (" + ctx->err + ")");
    return rc;
}

// C = sigma2 I + G = R'R by the blocked Cholesky of csmp_gram.hpp, augmented by the unit vectors (bp_factor's launches): block rows
// 0 .. ceil(M / 32) - 1, one launch each; then W = R^-1 = L^-T beside R^-T, and t = L^-1 b.  No wait: the verdict is read with the update's.
static int sbl_factor(csmp_ctx* ctx, double sigma2) {
    SblBuf& t = ctx->sbl;
    const int M = (int)ctx->M, np = t.np, npa = 2 * np;
    HIPCHECK(hipMemsetAsync(t.st, 0, sizeof(DevState), ctx->stream));
    hipLaunchKernelGGL(k_sbl_assemble, dim3((unsigned)(((int64_t)npa * npa + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.G, sigma2, M, np,
                       npa, bp_pivot_fraction(ctx), t.Gm, t.pivref);
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
    // t = R^-T b: column c of R^-1 holds row c of R^-T
    hipLaunchKernelGGL(k_bp_gemv, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, ctx->stream, (const double*)(t.Gm + np), (int64_t)npa, M, (int)BP_UPPER,
                       (const double*)t.vec, t.vec + t.Mp);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}
static int sbl_forms(csmp_ctx* ctx) {
    SblBuf& t = ctx->sbl;
    return sbl_launch_forms(ctx, t.Gm + t.np, (int64_t)2 * t.np, t.vec + t.Mp, t.s, t.q);
}

static int sbl_entry(csmp_ctx* ctx, const char* who) {
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, std::string(who) + ": a host-streamed dictionary is not served");
    if (ctx->M > kBpMaxRows) return fail(ctx, CSMP_ERANGE, std::string(who) + ": more than 2^19 rows");
    return CSMP_OK;
}

extern "C" int csmp_sbl(csmp_ctx* ctx, const void* b, int b_dtype, double sigma2, int64_t maxiter, double min_change, const double* gamma_in, double* x,
                        double* gamma_out, int loc, int64_t* iterations, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || !x) return fail(ctx, CSMP_EINVAL, "sbl: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if (loc != CSMP_HOST && loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "sbl: loc must be CSMP_HOST or CSMP_DEVICE");
    if (!std::isfinite(sigma2) || !(sigma2 > 0.0)) return fail(ctx, CSMP_EINVAL, "sbl: sigma2 has to be positive and finite");
    if (!(min_change >= 0.0)) return fail(ctx, CSMP_EINVAL, "sbl: min_change has to be non-negative");
    if (maxiter < 1) return fail(ctx, CSMP_EINVAL, "sbl: maxiter has to be at least 1");
    CHECK(sbl_entry(ctx, "sbl"));
    const int64_t N = ctx->N;
    const int M = (int)ctx->M;
    static const char* kBadGamma = "sbl: every entry of gamma has to be positive and finite";
    if (gamma_in && loc == CSMP_HOST)
        for (int64_t j = 0; j < N; ++j)
            if (!std::isfinite(gamma_in[j]) || !(gamma_in[j] > 0.0)) return fail(ctx, CSMP_EINVAL, kBadGamma);
    HIPCHECK(hipSetDevice(ctx->dev));
    CHECK(sbl_nomem(ctx, sbl_ensure(ctx)));
    SblBuf& t = ctx->sbl;
    const unsigned gridN = (unsigned)((N + 255) / 256), gridM = (unsigned)((M + 255) / 256);
    const hipMemcpyKind in = loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out = loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (loc == CSMP_DEVICE) {
        if (b_dtype == CSMP_F32) hipLaunchKernelGGL(k_sbl_loadb<float>, dim3(gridM), dim3(256), 0, ctx->stream, (const float*)b, M, t.vec);
        else hipLaunchKernelGGL(k_sbl_loadb<double>, dim3(gridM), dim3(256), 0, ctx->stream, (const double*)b, M, t.vec);
        HIPCHECK(hipGetLastError());
    } else {  // through the page-locked slot, as upload_b
        void* pv = nullptr;
        CHECK(pin_get(ctx, 0, (size_t)M * sizeof(double), &pv));
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        double* hb = (double*)pv;
        if (b_dtype == CSMP_F32)
            for (int i = 0; i < M; ++i) hb[i] = (double)((const float*)b)[i];
        else
            memcpy(hb, b, (size_t)M * sizeof(double));
        HIPCHECK(hipMemcpyAsync(t.vec, hb, (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHECK(hipMemsetAsync(t.info, 0, sizeof(SblInfo), ctx->stream));
    if (gamma_in) {
        HIPCHECK(hipMemcpyAsync(t.gam, gamma_in, (size_t)N * sizeof(double), in, ctx->stream));
        if (loc == CSMP_DEVICE) hipLaunchKernelGGL(k_sbl_check, dim3(gridN), dim3(256), 0, ctx->stream, (const double*)t.gam, N, t.info);
    } else {
        hipLaunchKernelGGL(k_sbl_ones, dim3(gridN), dim3(256), 0, ctx->stream, t.gam, N);
    }
    HIPCHECK(hipGetLastError());
    int64_t iters = 0;
    bool conv = false;
    for (int64_t it = 1; it <= maxiter; ++it) {
        CHECK(sbl_gram(ctx, t.gam, t.nsplit, t.cps, t.Gpart, t.G));
        CHECK(sbl_factor(ctx, sigma2));
        CHECK(sbl_forms(ctx));
        hipLaunchKernelGGL(k_sbl_update, dim3(kSblParts), dim3(256), 0, ctx->stream, (const double*)t.s, (const double*)t.q, N, t.gam, t.x, t.part, t.info);
        hipLaunchKernelGGL(k_sbl_fold, dim3(1), dim3(256), 0, ctx->stream, (const double*)t.part, t.info);
        HIPCHECK(hipGetLastError());
        DevState hs{};
        SblInfo info{};
        {  // the update's one read: the factorisation's verdict, the step norm and the verdict on gamma
            PinFetch f(ctx);
            CHECK(f.begin(sizeof hs + sizeof info + 16));
            CHECK(f.add(&hs, t.st, sizeof hs));
            CHECK(f.add(&info, t.info, sizeof info));
            CHECK(f.wait());
        }
        if (info.bad_input) return fail(ctx, CSMP_EINVAL, kBadGamma);
        if (hs.done & STOP_REORTH) return fail(ctx, CSMP_EINVAL, "sbl: sigma2 I + A Gamma A' is not positive definite to working precision");
        if (info.bad_gamma) return fail(ctx, CSMP_EINVAL, "sbl: an update gave a gamma that is negative or not finite");
        iters = it;
        if (std::sqrt(info.dg2) < min_change) {  // norm(gamma_old - gamma) < min_change (:45)
            conv = true;
            break;
        }
    }
    HIPCHECK(hipMemcpyAsync(x, t.x, (size_t)N * sizeof(double), out, ctx->stream));
    if (gamma_out) HIPCHECK(hipMemcpyAsync(gamma_out, t.gam, (size_t)N * sizeof(double), out, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    if (iterations) *iterations = iters;
    if (flags) *flags = conv ? CSMP_SBL_CONVERGED : 0;
    return CSMP_OK;
}

// ------------------------------------------------------------------------------------------ measurement (include/csmp_internal.h)
extern "C" int csmp_sbl_rowgram(csmp_ctx* ctx, const double* gamma, double* C_out, int loc) {
    if (!ctx) return CSMP_EINVAL;
    if (!gamma || !C_out || (loc != CSMP_HOST && loc != CSMP_DEVICE)) return fail(ctx, CSMP_EINVAL, "sbl_rowgram: bad arguments");
    CHECK(sbl_entry(ctx, "sbl_rowgram"));
    HIPCHECK(hipSetDevice(ctx->dev));
    int nsplit;
    int64_t cps;
    bp_rowgram_split(ctx, nsplit, cps);
    const size_t MM = (size_t)ctx->M * (size_t)ctx->M, nbytes = (size_t)ctx->N * sizeof(double);
    DevTmp part, G, gam;
    CHECK(sbl_nomem(ctx, part.alloc(ctx, (size_t)nsplit * MM * sizeof(double))));
    const double* dgam = gamma;
    double* dG = C_out;
    if (loc == CSMP_HOST) {
        CHECK(sbl_nomem(ctx, G.alloc(ctx, MM * sizeof(double))));
        CHECK(sbl_nomem(ctx, gam.alloc(ctx, nbytes)));
        HIPCHECK(hipMemcpyAsync(gam.p, gamma, nbytes, hipMemcpyHostToDevice, ctx->stream));
        dgam = (const double*)gam.p;
        dG = (double*)G.p;
    }
    CHECK(sbl_gram(ctx, dgam, nsplit, cps, (double*)part.p, dG));
    if (loc == CSMP_HOST) HIPCHECK(hipMemcpyAsync(C_out, dG, MM * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));  // (the temporaries are released on return)
    return CSMP_OK;
}

extern "C" int csmp_sbl_forms(csmp_ctx* ctx, const double* W, int64_t ldw, const double* t, double* s, double* q, int loc) {
    if (!ctx) return CSMP_EINVAL;
    if (!W || !t || !s || !q || (loc != CSMP_HOST && loc != CSMP_DEVICE)) return fail(ctx, CSMP_EINVAL, "sbl_forms: bad arguments");
    CHECK(sbl_entry(ctx, "sbl_forms"));
    if (ldw < sbl_ldw(ctx) || ldw % kRbRows != 0) return fail(ctx, CSMP_EDIM, "sbl_forms: ldw has to be a multiple of 64 and at least size(A, 1)");
    if (loc == CSMP_DEVICE && (uintptr_t)W % 16 != 0) return fail(ctx, CSMP_EINVAL, "sbl_forms: W has to start on a 16-byte boundary");
    HIPCHECK(hipSetDevice(ctx->dev));
    const size_t wbytes = (size_t)ldw * (size_t)ctx->M * sizeof(double), mbytes = (size_t)ctx->M * sizeof(double), nbytes = (size_t)ctx->N * sizeof(double);
    // t followed by zeros up to whole blocks of 128 directions, as the kernel reads it
    const size_t tbytes = (size_t)((ctx->M + kRbDirs - 1) / kRbDirs * kRbDirs) * sizeof(double);
    DevTmp dW, dt, ds, dq;
    CHECK(sbl_nomem(ctx, dt.alloc(ctx, tbytes)));
    HIPCHECK(hipMemsetAsync(dt.p, 0, tbytes, ctx->stream));
    HIPCHECK(hipMemcpyAsync(dt.p, t, mbytes, loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    if (loc == CSMP_DEVICE) {
        CHECK(sbl_launch_forms(ctx, W, ldw, (const double*)dt.p, s, q));
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        return CSMP_OK;
    }
    CHECK(sbl_nomem(ctx, dW.alloc(ctx, wbytes)));
    CHECK(sbl_nomem(ctx, ds.alloc(ctx, nbytes)));
    CHECK(sbl_nomem(ctx, dq.alloc(ctx, nbytes)));
    HIPCHECK(hipMemcpyAsync(dW.p, W, wbytes, hipMemcpyHostToDevice, ctx->stream));
    CHECK(sbl_launch_forms(ctx, (const double*)dW.p, ldw, (const double*)dt.p, (double*)ds.p, (double*)dq.p));
    HIPCHECK(hipMemcpyAsync(s, ds.p, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipMemcpyAsync(q, dq.p, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    return CSMP_OK;
}

extern "C" int csmp_bench_sbl(csmp_ctx* ctx, double sigma2, int reps, double* gram_ms, double* factor_ms, double* forms_ms) {
    if (!ctx || reps < 1 || !(sigma2 > 0.0)) return CSMP_EINVAL;
    CHECK(sbl_entry(ctx, "bench_sbl"));
    SblBuf& t = ctx->sbl;
    if (!t.Gm || t.M != (int)ctx->M || t.N != ctx->N) return fail(ctx, CSMP_ESTATE, "bench_sbl: no gamma (call csmp_sbl first)");
    HIPCHECK(hipSetDevice(ctx->dev));
    hipEvent_t ev[4];
    for (auto& e : ev) HIPCHECK(hipEventCreate(&e));
    double sum[3] = {0.0, 0.0, 0.0};
    int rc = CSMP_OK;
    for (int i = 0; i <= reps && rc == CSMP_OK; ++i) {  // (run 0 warms up)
        auto run = [&]() -> int {
            HIPCHECK(hipEventRecord(ev[0], ctx->stream));
            CHECK(sbl_gram(ctx, t.gam, t.nsplit, t.cps, t.Gpart, t.G));
            HIPCHECK(hipEventRecord(ev[1], ctx->stream));
            CHECK(sbl_factor(ctx, sigma2));
            HIPCHECK(hipEventRecord(ev[2], ctx->stream));
            CHECK(sbl_forms(ctx));
            HIPCHECK(hipEventRecord(ev[3], ctx->stream));
            HIPCHECK(hipStreamSynchronize(ctx->stream));
            for (int k = 0; k < 3; ++k) {
                float ms = 0.f;
                HIPCHECK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
                if (i > 0) sum[k] += ms;
            }
            return CSMP_OK;
        };
        rc = run();
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    CHECK(rc);
    if (gram_ms) *gram_ms = sum[0] / reps;
    if (factor_ms) *factor_ms = sum[1] / reps;
    if (forms_ms) *forms_ms = sum[2] / reps;
    return CSMP_OK;
}
