// host/analysis.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_colnorms (src/util.jl:2) and csmp_cumbabel (coherence / babel / cumbabel, src/util.jl:96-115) on the resident dictionary.
// ------------------------------------------------------------------------------------------ dictionary analysis
static int64_t analysis_strip_ld(int64_t N) { return (N + 15) / 16 * 16; }  // rows of the strip start on 128-byte boundaries

// The buffers of the context for the resident dictionary.  The norms alone serve csmp_colnorms; csmp_cumbabel needs all of them.
// Either way a failed allocation leaves NONE behind.
static int analysis_ensure(csmp_ctx* ctx, bool strip) {
    AnalysisBuf& t = ctx->analysis;
    if (t.N != ctx->N && t.N != 0) {
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        analysis_free(t);
    }
    if (t.norms && (!strip || t.strip)) return CSMP_OK;
    const size_t N = (size_t)ctx->N;
    AnalysisBuf n = t;  // (what exists is kept on success)
    auto all = [&]() -> int {
        if (!n.norms) CHECK(dmalloc(ctx, &n.norms, N));
        if (strip) {
            CHECK(dmalloc(ctx, &n.strip, (size_t)kGramQ * (size_t)analysis_strip_ld(ctx->N)));
            CHECK(dmalloc(ctx, &n.rowcum, (size_t)kGramQ * (size_t)kBabelCap));
            CHECK(dmalloc(ctx, &n.rowtop, (size_t)kGramQ));
            CHECK(dmalloc(ctx, &n.rowarg, (size_t)kGramQ));
            CHECK(dmalloc(ctx, &n.mu, (size_t)kBabelCap));
            CHECK(dmalloc(ctx, &n.best, (size_t)1));
        }
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        analysis_free(n);
        t = AnalysisBuf();
        return rc;
    }
    n.N = ctx->N;
    t = n;
    return CSMP_OK;
}

// s[j] = |a_j| (mode 0) or 1 / |a_j|, 0 for a zero column (mode 1): k_fr_colnorm2's sums of squares, then the root
static int analysis_launch_norms(csmp_ctx* ctx, int mode) {
    AnalysisBuf& t = ctx->analysis;
    const unsigned grid = (unsigned)((ctx->N + 3) / 4);
    if (ctx->dtype == CSMP_F32)
        hipLaunchKernelGGL(k_fr_colnorm2<float>, dim3(grid), dim3(256), 0, ctx->stream, (const float*)ctx->dA, ctx->ld, (int)ctx->M, ctx->N, t.norms);
    else
        hipLaunchKernelGGL(k_fr_colnorm2<double>, dim3(grid), dim3(256), 0, ctx->stream, (const double*)ctx->dA, ctx->ld, (int)ctx->M, ctx->N, t.norms);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_an_root, dim3((unsigned)((ctx->N + 255) / 256)), dim3(256), 0, ctx->stream, t.norms, ctx->N, mode);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

template <typename TA, bool VEC>
static hipError_t gram_strip_t(csmp_ctx* ctx, int64_t q0, const double* scale) {
    AnalysisBuf& t = ctx->analysis;
    auto kern = k_gram_strip<TA, VEC>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fr_rebuild_lds_bytes());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)((ctx->N + 127) / 128)), dim3(256), fr_rebuild_lds_bytes(), ctx->stream, (const TA*)ctx->dA, ctx->ld,
                       (int)ctx->M, ctx->N, q0, scale, t.strip, analysis_strip_ld(ctx->N));
    return hipGetLastError();
}
static int launch_gram_strip(csmp_ctx* ctx, int64_t q0, const double* scale) {
    // 16-byte loads of a column's rows need the column starts on 16-byte boundaries
    const size_t esz = ctx->dtype == CSMP_F32 ? 4 : 8;
    const bool vec = ((uintptr_t)ctx->dA % 16 == 0) && ((size_t)ctx->ld * esz) % 16 == 0;
    hipError_t e;
    if (ctx->dtype == CSMP_F32) e = vec ? gram_strip_t<float, true>(ctx, q0, scale) : gram_strip_t<float, false>(ctx, q0, scale);
    else e = vec ? gram_strip_t<double, true>(ctx, q0, scale) : gram_strip_t<double, false>(ctx, q0, scale);
    HIPCHECK(e);
    return CSMP_OK;
}

static int analysis_entry(csmp_ctx* ctx, const char* who) {
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, std::string(who) + ": a host-streamed dictionary is not served");
    return CSMP_OK;
}

extern "C" int csmp_colnorms(csmp_ctx* ctx, double* norms, int out_loc) {
    if (!ctx) return CSMP_EINVAL;
    if (!norms) return fail(ctx, CSMP_EINVAL, "colnorms: norms == NULL");
    if (out_loc != CSMP_HOST && out_loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "colnorms: out_loc must be CSMP_HOST or CSMP_DEVICE");
    CHECK(analysis_entry(ctx, "colnorms"));
    HIPCHECK(hipSetDevice(ctx->dev));
    {
        const int rc = analysis_ensure(ctx, false);
        if (rc == CSMP_EHIP) return fail(ctx, CSMP_ENOMEM, "colnorms: no device memory for the norms (" + ctx->err + ")");
        CHECK(rc);
    }
    CHECK(analysis_launch_norms(ctx, 0));
    HIPCHECK(hipMemcpyAsync(norms, ctx->analysis.norms, (size_t)ctx->N * sizeof(double),
                            out_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    return CSMP_OK;
}

extern "C" int csmp_cumbabel(csmp_ctx* ctx, int64_t k, int normalize, double* mu, int64_t* pair) {
    if (!ctx) return CSMP_EINVAL;
    if (!mu) return fail(ctx, CSMP_EINVAL, "cumbabel: mu == NULL");
    if (normalize != 0 && normalize != 1) return fail(ctx, CSMP_EINVAL, "cumbabel: normalize must be 0 or 1");
    CHECK(analysis_entry(ctx, "cumbabel"));
    if (k < 1 || k > std::min<int64_t>(ctx->N, CSMP_BABEL_KMAX))
        return fail(ctx, CSMP_ERANGE, "cumbabel: k has to lie in 1 .. min(size(A, 2), CSMP_BABEL_KMAX)");
    HIPCHECK(hipSetDevice(ctx->dev));
    {
        const int rc = analysis_ensure(ctx, true);
        if (rc == CSMP_EHIP) return fail(ctx, CSMP_ENOMEM, "cumbabel: no device memory for the strip (" + ctx->err + ")");
        CHECK(rc);
    }
    AnalysisBuf& t = ctx->analysis;
    struct Out {
        double mu[kBabelCap];
        BabelBest best;
    };
    void* pinned = nullptr;
    CHECK(pin_get(ctx, 1, sizeof(Out), &pinned));
    if (normalize) CHECK(analysis_launch_norms(ctx, 1));
    hipLaunchKernelGGL(k_babel_init, dim3(1), dim3(256), 0, ctx->stream, t.mu, t.best);
    HIPCHECK(hipGetLastError());
    const int64_t lds = analysis_strip_ld(ctx->N);
    for (int64_t q0 = 0; q0 < ctx->N; q0 += kGramQ) {
        const int nq = (int)std::min<int64_t>(kGramQ, ctx->N - q0);
        CHECK(launch_gram_strip(ctx, q0, normalize ? t.norms : nullptr));
        hipLaunchKernelGGL(k_babel_rows, dim3(nq), dim3(kBabelThreads), 0, ctx->stream, (const double*)t.strip, lds, ctx->N, q0, (int)k, t.rowcum,
                           t.rowtop, t.rowarg);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(k_babel_fold, dim3(1), dim3(256), 0, ctx->stream, (const double*)t.rowcum, (const double*)t.rowtop,
                           (const long long*)t.rowarg, nq, q0, (int)k, t.mu, t.best);
        HIPCHECK(hipGetLastError());
    }
    Out* out = (Out*)pinned;
    HIPCHECK(hipMemcpyAsync(out->mu, t.mu, sizeof(double) * kBabelCap, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipMemcpyAsync(&out->best, t.best, sizeof(BabelBest), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    memcpy(mu, out->mu, (size_t)k * sizeof(double));
    if (pair) {
        pair[0] = out->best.i;
        pair[1] = out->best.j;
    }
    return CSMP_OK;
}
