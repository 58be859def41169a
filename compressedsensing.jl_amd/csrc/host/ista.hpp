// host/ista.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_ista, the proximal-gradient driver (ista, src/basispursuit.jl:164-183, and FISTA on the same objective).
// ------------------------------------------------------------------------------------------ ista / fista
// segments of the list: at most kIstaMaxSegs, whole multiples of the update kernel's 256 atoms
static int64_t ista_seg_len(int64_t N) {
    const int64_t per = (N + kIstaMaxSegs - 1) / kIstaMaxSegs;
    return std::max<int64_t>(kIstaThreads, (per + kIstaThreads - 1) / kIstaThreads * kIstaThreads);
}
// row blocks of k_ista_axpy's grid, and its workgroups per row block: about two workgroups per CU in all
static int ista_row_blocks(const csmp_ctx* ctx) {
    const int vec = ctx->dtype == CSMP_F32 ? 4 : 2;
    const int per = (kIstaThreads / kWave) * kWave * kIstaL;  // vectors of a column one workgroup takes
    return (ctx->Mv / vec + per - 1) / per;
}
static int ista_parts_max(const csmp_ctx* ctx) { return std::max(1, 2 * ctx->prop.multiProcessorCount / ista_row_blocks(ctx)); }

// The buffers of the context for the resident dictionary: all of them, or none (a failed allocation leaves none behind).
static int ista_ensure(csmp_ctx* ctx) {
    IstaBuf& t = ctx->ista;
    const int P = ista_parts_max(ctx);
    if (t.x && t.N == ctx->N && t.Mv == ctx->Mv && t.P == P) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    ista_free(t);
    IstaBuf n;
    const size_t N = (size_t)ctx->N;
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.x, N));
        CHECK(dmalloc(ctx, &n.y, N));
        CHECK(dmalloc(ctx, &n.w, N));
        CHECK(dmalloc(ctx, &n.lidx, N));
        CHECK(dmalloc(ctx, &n.lval, N));
        CHECK(dmalloc(ctx, &n.seg_cnt, (size_t)kIstaMaxSegs));
        CHECK(dmalloc(ctx, &n.nnz, (size_t)1));
        CHECK(dmalloc(ctx, &n.part, (size_t)P * (size_t)ctx->Mv));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        ista_free(n);
        return rc;
    }
    n.N = ctx->N;
    n.Mv = ctx->Mv;
    n.P = P;
    t = n;
    return CSMP_OK;
}

static int ista_launch_update(csmp_ctx* ctx, int64_t nw, double alpha, double beta, int flags) {
    IstaBuf& t = ctx->ista;
    const int64_t seg_len = ista_seg_len(ctx->N);
    const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
    hipLaunchKernelGGL(k_ista_update, dim3(nseg), dim3(kIstaThreads), 0, ctx->stream, (const double*)ctx->s.cvec, (const double*)t.w, nw, t.x, t.y,
                       ctx->N, seg_len, alpha, beta, flags, t.lidx, t.lval, t.seg_cnt);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}

// r = b - A[:, list] * values: the axpy over the list the last update wrote, then the partials added in order
template <typename TA>
static int ista_launch_residual(csmp_ctx* ctx) {
    IstaBuf& t = ctx->ista;
    Solver& s = ctx->s;
    const int64_t seg_len = ista_seg_len(ctx->N);
    const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
    hipLaunchKernelGGL(k_ista_axpy<TA>, dim3(t.P, ista_row_blocks(ctx)), dim3(kIstaThreads), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld, ctx->Mv,
                       (const int*)t.seg_cnt, nseg, seg_len, (const int*)t.lidx, (const double*)t.lval, t.part, t.nnz);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ista_resum, dim3(((int)ctx->M + kWave - 1) / kWave), dim3(kIstaThreads), 0, ctx->stream, (const double*)t.part, ctx->Mv,
                       (int)ctx->M, (const unsigned*)t.nnz, t.P, (const double*)s.b, s.r);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}
static int ista_residual(csmp_ctx* ctx) { return ctx->dtype == CSMP_F32 ? ista_launch_residual<float>(ctx) : ista_launch_residual<double>(ctx); }

// exactly maxiter iterations from the x, y and weights in the context's buffers, no stopping rule (:177); nothing here waits for the
// device.  listed: the list (and r) belong to the current y -- false on entry only for x = y = 0, where r = b already.
static int ista_iterate(csmp_ctx* ctx, int64_t nw, int64_t maxiter, double stepsize, int accel, bool& listed) {
    Solver& s = ctx->s;
    double tk = 1.0;
    for (int64_t it = 1; it <= maxiter; ++it) {
        if (listed) CHECK(ista_residual(ctx));  // (the first iteration from x = 0: r = b already)
        CHECK(launch_sweep(ctx, s.r, 0.0, 0, 0));
        const double tn = (1.0 + std::sqrt(1.0 + 4.0 * tk * tk)) / 2.0;
        const double beta = accel ? (tk - 1.0) / tn : 0.0;
        tk = tn;
        CHECK(ista_launch_update(ctx, nw, stepsize, beta, (accel ? ISTA_ACCEL : 0) | (it == maxiter ? ISTA_LIST_X : 0)));
        listed = true;
    }
    return CSMP_OK;
}

// One solve on the active slot and the context's IstaBuf, b in place already (r = b, the residual of x = 0): the weights go up, then
// the warm start -- x0, a dense N-vector where x0_kind says (null: x = 0) --, maxiter iterations, ||b - A x|| (resnorm may be null) and
// x to the caller's vector at x_loc.  Returns with the stream drained.  csmp_ista and csmp_ista_batch's signal-by-signal path.
static int ista_solve(csmp_ctx* ctx, const double* w, int64_t nw, const double* x0, hipMemcpyKind x0_kind, int64_t maxiter, double stepsize,
                      int accel, double* x, int x_loc, double* resnorm) {
    IstaBuf& t = ctx->ista;
    HIPCHECK(hipMemcpyAsync(t.w, w, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    bool listed = false;  // the list (and r) belong to the current y
    if (x0) {
        HIPCHECK(hipMemcpyAsync(t.y, x0, (size_t)ctx->N * sizeof(double), x0_kind, ctx->stream));
        CHECK(ista_launch_update(ctx, nw, 0.0, 0.0, ISTA_INIT | ISTA_LIST_X));
        listed = true;
    } else {
        HIPCHECK(hipMemsetAsync(t.x, 0, (size_t)ctx->N * sizeof(double), ctx->stream));
        HIPCHECK(hipMemsetAsync(t.y, 0, (size_t)ctx->N * sizeof(double), ctx->stream));
    }
    CHECK(ista_iterate(ctx, nw, maxiter, stepsize, accel, listed));
    if (resnorm) {
        if (listed) CHECK(ista_residual(ctx));
        CHECK(residual_norm(ctx, resnorm));
    }
    HIPCHECK(hipMemcpyAsync(x, t.x, (size_t)ctx->N * sizeof(double), x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    return CSMP_OK;
}

extern "C" int csmp_ista(csmp_ctx* ctx, const void* b, int b_dtype, const double* w, int64_t nw, const int64_t* idx0, const double* val0,
                         int64_t nnz0, int64_t maxiter, double stepsize, int accel, double* x, int x_loc, double* resnorm) {
    if (!ctx) return CSMP_EINVAL;
    if (!b || !w || !x || nnz0 < 0 || (nnz0 > 0 && (!idx0 || !val0))) return fail(ctx, CSMP_EINVAL, "ista: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "ista: x_loc must be CSMP_HOST or CSMP_DEVICE");
    if (accel != 0 && accel != 1) return fail(ctx, CSMP_EINVAL, "ista: accel must be 0 (ISTA) or 1 (FISTA)");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, "ista: a host-streamed dictionary is not served");
    if (nw != 1 && nw != ctx->N) return fail(ctx, CSMP_EDIM, "ista: length(w) must be 1 or size(A, 2)");
    if (maxiter < 0) return fail(ctx, CSMP_EINVAL, "ista: maxiter has to be non-negative");
    if (!std::isfinite(stepsize) || !(stepsize > 0.0)) return fail(ctx, CSMP_EINVAL, "ista: stepsize has to be positive and finite");
    for (int64_t i = 0; i < nw; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(ctx, CSMP_EINVAL, "ista: the weights have to be non-negative and finite");
    std::vector<double> x0;  // the warm start, dense
    if (nnz0 > 0) {
        x0.assign((size_t)ctx->N, 0.0);
        std::vector<char> seen((size_t)ctx->N, 0);
        for (int64_t t = 0; t < nnz0; ++t) {
            if (idx0[t] < 0 || idx0[t] >= ctx->N) return fail(ctx, CSMP_EINVAL, "ista: warm-start index out of range");
            if (seen[(size_t)idx0[t]]) return fail(ctx, CSMP_EINVAL, "ista: warm-start index repeated");
            seen[(size_t)idx0[t]] = 1;
            x0[(size_t)idx0[t]] = val0[t];
        }
    }
    HIPCHECK(hipSetDevice(ctx->dev));
    {
        int rc = solver_ensure(ctx, 1, 1, false);
        if (rc == CSMP_OK) rc = ista_ensure(ctx);
        if (rc == CSMP_EHIP) return fail(ctx, CSMP_ENOMEM, "ista: no device memory for the iterates (" + ctx->err + ")");
        CHECK(rc);
    }
    ctx->s.begun = false;
    if (x_loc == CSMP_DEVICE)
        CHECK(b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)b) : init_from_device_t<double>(ctx, (const double*)b));
    else
        CHECK(upload_b(ctx, b, b_dtype));  // r = b: the residual of x = 0
    return ista_solve(ctx, w, nw, nnz0 > 0 ? x0.data() : nullptr, hipMemcpyHostToDevice, maxiter, stepsize, accel, x, x_loc, resnorm);
}
