// host/ista_joint.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_ista_joint -- ISTA / FISTA on ||B - A X||_F^2 + sum_j w_j ||X[j, :]||_2: ONE row support for all columns of B (kernels and the
// step: csmp_ista_joint.hpp).
// ------------------------------------------------------------------------------------------ ista_joint
// The columns live in the call's own arrays, released when the call returns: nsig is bounded by memory only,
//     8 (2 Mpad + 4 size(A,2)) + 64 bytes a column  (b and r of Mpad = size(A,1) rounded up to 256 rows; c, x, y and the list's values)
// beside what does not grow with nsig: the weights, the list's indices and ONE chunk's partials of the residual, 8 P Mv bytes for each
// of min(nsig, 8) columns (P = csmp_ista's workgroup count, 128 MiB at 4096 x 65536).  The residual runs CHUNK AFTER CHUNK on the
// stream -- k_jista_axpy and k_jista_resum for the columns [c0, c0 + 8), then the next eight -- so the partials never exceed one chunk's.
// The passes are csmp_somp's own (SompRun::passes): the shared pass over chunks of up to group_wide columns where the resident
// dictionary has one, else one launch_sweep per column.  One column is csmp_ista: it takes csmp_ista's launches on the context's
// IstaBuf.  Exactly maxiter iterations, no host decision between them: everything is enqueued on the context's stream and the host
// waits once, for the row count and the norms.
static int jista_nomem(csmp_ctx* ctx, int rc) {
    if (rc == CSMP_EHIP && ctx->err.find("hipMalloc") != std::string::npos)
        return fail(ctx, CSMP_ENOMEM, "ista_joint: no device memory for the iterates (" + ctx->err + ")");
    return rc;
}

struct JistaRun {
    csmp_ctx* ctx;
    SompRun pass;     // R, C and the passes' control blocks: csmp_somp's columns
    double *Bd;       // B promoted, R's layout
    double *X, *Y;    // column l from l * ldx
    int64_t ldx;
    double *w, *lval, *part;
    int *lidx, *seg_cnt;
    unsigned* nnz;
    int64_t nw;
    int P;

    int update(double alpha, double beta, int flags) const {
        const int64_t seg_len = ista_seg_len(ctx->N);
        const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
        hipLaunchKernelGGL(k_jista_update, dim3(nseg), dim3(kIstaThreads), 0, ctx->stream, (const double*)pass.g.C, pass.g.ldc, (const double*)w, nw,
                           X, Y, ldx, pass.g.nsig, ctx->N, seg_len, alpha, beta, flags, lidx, lval, seg_cnt);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    template <typename TA, int NS>
    int axpy(int c0, int size) const {
        const int64_t seg_len = ista_seg_len(ctx->N);
        const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
        const int per = (kIstaThreads / kWave) * kWave * JistaShape<TA, NS>::L;  // vectors of a column one workgroup takes
        const int rows = (ctx->Mv / Vec<TA>::n + per - 1) / per;
        hipLaunchKernelGGL((k_jista_axpy<TA, NS>), dim3(P, rows), dim3(kIstaThreads), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld, ctx->Mv,
                           (const int*)seg_cnt, nseg, seg_len, (const int*)lidx, (const double*)lval, pass.g.nsig, c0, size, part, nnz);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    // R = B - A Y over the list the last update wrote, chunk after chunk
    template <typename TA>
    int residual() const {
        const int M = (int)ctx->M, nsig = pass.g.nsig;
        for (int c0 = 0; c0 < nsig; c0 += kJistaChunk) {
            const int size = std::min(kJistaChunk, nsig - c0);
            CHECK((size > 4 ? axpy<TA, 8>(c0, size) : size > 2 ? axpy<TA, 4>(c0, size) : size > 1 ? axpy<TA, 2>(c0, size) : axpy<TA, 1>(c0, size)));
            hipLaunchKernelGGL(k_jista_resum, dim3((M + kWave - 1) / kWave, size), dim3(kIstaThreads), 0, ctx->stream, (const double*)part, ctx->Mv, M,
                               (const unsigned*)nnz, P, (const double*)Bd, pass.g.R, pass.g.ldr, c0);
            HIPCHECK(hipGetLastError());
        }
        return CSMP_OK;
    }
    // ista_iterate for the row-wise step
    template <typename TA>
    int iterate(int64_t maxiter, double stepsize, int accel, bool& listed) {
        double tk = 1.0;
        for (int64_t it = 1; it <= maxiter; ++it) {
            if (listed) CHECK(residual<TA>());  // (the first iteration from X = 0: R = B already)
            CHECK(pass.passes<TA>(0));
            const double tn = (1.0 + std::sqrt(1.0 + 4.0 * tk * tk)) / 2.0;
            const double beta = accel ? (tk - 1.0) / tn : 0.0;
            tk = tn;
            CHECK(update(stepsize, beta, (accel ? ISTA_ACCEL : 0) | (it == maxiter ? ISTA_LIST_X : 0)));
            listed = true;
        }
        return CSMP_OK;
    }
};

// the length of the list the last update wrote (X's: ISTA_LIST_X) from its segments' counts
static int64_t jista_rows(const std::vector<int>& cnt) {
    int64_t n = 0;
    for (int c : cnt) n += c;
    return n;
}

extern "C" int csmp_ista_joint(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, const double* w, int64_t nw,
                               const double* X0, int64_t ldX0, int64_t maxiter, double stepsize, int accel, double* X, int64_t ldX, int x_loc,
                               int64_t* nrows, double* resnorm) {
    if (!ctx) return CSMP_EINVAL;
    if (nsig < 0) return fail(ctx, CSMP_EINVAL, "ista_joint: nsig has to be non-negative");
    if (!w || (nsig > 0 && (!B || !X))) return fail(ctx, CSMP_EINVAL, "ista_joint: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if ((b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) || (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE))
        return fail(ctx, CSMP_EINVAL, "ista_joint: b_loc / x_loc must be CSMP_HOST or CSMP_DEVICE");
    if (accel != 0 && accel != 1) return fail(ctx, CSMP_EINVAL, "ista_joint: accel must be 0 (ISTA) or 1 (FISTA)");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, "ista_joint: a host-streamed dictionary is not served");
    if (ldB < ctx->M) return fail(ctx, CSMP_EDIM, "ista_joint: ldB < size(A, 1)");
    if (ldX < ctx->N) return fail(ctx, CSMP_EDIM, "ista_joint: ldX < size(A, 2)");
    if (X0 && ldX0 < ctx->N) return fail(ctx, CSMP_EDIM, "ista_joint: ldX0 < size(A, 2)");
    if (nw != 1 && nw != ctx->N) return fail(ctx, CSMP_EDIM, "ista_joint: length(w) must be 1 or size(A, 2)");
    if (maxiter < 0) return fail(ctx, CSMP_EINVAL, "ista_joint: maxiter has to be non-negative");
    if (!std::isfinite(stepsize) || !(stepsize > 0.0)) return fail(ctx, CSMP_EINVAL, "ista_joint: stepsize has to be positive and finite");
    for (int64_t i = 0; i < nw; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(ctx, CSMP_EINVAL, "ista_joint: the weights have to be non-negative and finite");
    if (nsig > ((int64_t)1 << 22)) return fail(ctx, CSMP_ERANGE, "ista_joint: nsig too large");  // (grids of nsig * ceil(size(A,1) / 256) workgroups)
    if (nsig == 0) return CSMP_OK;
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    {
        int rc = solver_ensure(ctx, 1, 1, false);
        if (rc == CSMP_OK && nsig == 1) rc = ista_ensure(ctx);
        CHECK(jista_nomem(ctx, rc));
    }
    Solver& s = ctx->s;
    s.begun = false;
    auto finish = [&](int rc) -> int {
        (void)hipStreamSynchronize(ctx->stream);  // (on every way out: the temporaries and the caller's buffers are at rest)
        return rc;
    };
    const size_t esz = b_dtype == CSMP_F32 ? 4 : 8;
    const int64_t seg_len = ista_seg_len(ctx->N);
    const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
    const hipMemcpyKind in_kind = x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    std::vector<int> cnt;  // the segments' counts of the final list

    DevTmp tB;  // a host caller's B on the device
    const void* dB = B;
    if (b_loc == CSMP_HOST) {
        const size_t bbytes = ((size_t)ldB * (size_t)(nsig - 1) + (size_t)ctx->M) * esz;  // (the last column ends at its last row)
        CHECK(jista_nomem(ctx, tB.alloc(ctx, bbytes)));
        HIPCHECK(hipMemcpy(tB.p, B, bbytes, hipMemcpyHostToDevice));
        dB = tB.p;
    }

    if (nsig == 1) {  // the problem IS csmp_ista's: its launches, its bits
        auto one = [&]() -> int {
            CHECK(b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)dB) : init_from_device_t<double>(ctx, (const double*)dB));
            CHECK(ista_solve(ctx, w, nw, X0, in_kind, maxiter, stepsize, accel, X, x_loc, resnorm));
            if (nrows) {
                *nrows = 0;
                if (X0 || maxiter > 0) {  // (the list is that of the result: ISTA_LIST_X)
                    cnt.assign((size_t)nseg, 0);
                    PinFetch f(ctx);
                    CHECK(f.begin((size_t)nseg * 4));
                    CHECK(f.add(cnt.data(), ctx->ista.seg_cnt, (size_t)nseg * 4));
                    CHECK(f.wait());
                    *nrows = jista_rows(cnt);
                }
            }
            return CSMP_OK;
        };
        return finish(one());
    }

    DevTmp tBd, tR, tC, tXY, tLv, tLi, tSeg, tNnz, tW, tPart, tSt, tPv, tPi, tNrm;
    JistaRun run{};
    run.ctx = ctx;
    run.nw = nw;
    run.P = ista_parts_max(ctx);
    run.ldx = (ctx->N + 1) / 2 * 2;
    SompRun& ps = run.pass;
    ps.ctx = ctx;
    ps.grouped = ctx->sweep_group >= 1;
    ps.pcap = ctx->prop.multiProcessorCount * 8 + 8;  // (what pipe_nblk allows a pass: solver_alloc's pval / pidx)
    SompCols& g = ps.g;
    g.nsig = (int)nsig;
    g.ldr = s.Mpad;
    g.ldc = run.ldx;
    const size_t ncol = (size_t)nsig, xbytes = ncol * (size_t)run.ldx * 8;
    auto allocate = [&]() -> int {
        CHECK(tBd.alloc(ctx, ncol * g.ldr * 8));
        CHECK(tR.alloc(ctx, ncol * g.ldr * 8));
        CHECK(tC.alloc(ctx, ncol * g.ldc * 8));
        CHECK(tXY.alloc(ctx, 2 * xbytes));
        CHECK(tLv.alloc(ctx, (size_t)ctx->N * ncol * 8));
        CHECK(tLi.alloc(ctx, (size_t)ctx->N * 4));
        CHECK(tSeg.alloc(ctx, (size_t)kIstaMaxSegs * 4));
        CHECK(tNnz.alloc(ctx, 4));
        CHECK(tW.alloc(ctx, (size_t)nw * 8));
        CHECK(tPart.alloc(ctx, (size_t)std::min<int64_t>(nsig, kJistaChunk) * (size_t)run.P * (size_t)ctx->Mv * 8));
        CHECK(tSt.alloc(ctx, ncol * sizeof(DevState)));
        CHECK(tPv.alloc(ctx, (size_t)kWideMax * ps.pcap * 8));
        CHECK(tPi.alloc(ctx, (size_t)kWideMax * ps.pcap * 4));
        if (resnorm) CHECK(tNrm.alloc(ctx, ncol * 8));
        return CSMP_OK;
    };
    CHECK(finish(jista_nomem(ctx, allocate())));
    run.Bd = (double*)tBd.p; g.R = (double*)tR.p; g.C = (double*)tC.p; g.st = (DevState*)tSt.p;
    run.X = (double*)tXY.p; run.Y = run.X + ncol * (size_t)run.ldx;
    run.lval = (double*)tLv.p; run.lidx = (int*)tLi.p; run.seg_cnt = (int*)tSeg.p; run.nnz = (unsigned*)tNnz.p;
    run.w = (double*)tW.p; run.part = (double*)tPart.p;
    ps.ppv = (double*)tPv.p; ps.ppi = (int*)tPi.p;

    auto solve = [&]() -> int {
        HIPCHECK(hipMemcpyAsync(run.w, w, (size_t)nw * 8, hipMemcpyHostToDevice, ctx->stream));
        // B promoted to Bd (rows past size(A,1) zero) and the passes' control blocks reset; R = B, the residual of X = 0
        SompCols gb = g;
        gb.R = run.Bd;
        const int iw = (int)(g.ldr / 256);
        const dim3 igrid((unsigned)((int64_t)iw * nsig));
        if (b_dtype == CSMP_F32)
            hipLaunchKernelGGL(k_somp_init<float>, igrid, dim3(256), 0, ctx->stream, (const float*)dB, ldB, (int)ctx->M, gb, iw);
        else
            hipLaunchKernelGGL(k_somp_init<double>, igrid, dim3(256), 0, ctx->stream, (const double*)dB, ldB, (int)ctx->M, gb, iw);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(g.R, run.Bd, ncol * g.ldr * 8, hipMemcpyDeviceToDevice, ctx->stream));
        bool listed = false;  // the list (and R) belong to the current Y
        if (X0) {
            HIPCHECK(hipMemcpy2DAsync(run.Y, (size_t)run.ldx * 8, X0, (size_t)ldX0 * 8, (size_t)ctx->N * 8, ncol, in_kind, ctx->stream));
            CHECK(run.update(0.0, 0.0, ISTA_INIT | ISTA_LIST_X));
            listed = true;
        } else {
            HIPCHECK(hipMemsetAsync(run.X, 0, 2 * xbytes, ctx->stream));  // (Y follows X)
        }
        CHECK(ctx->dtype == CSMP_F32 ? run.iterate<float>(maxiter, stepsize, accel, listed) : run.iterate<double>(maxiter, stepsize, accel, listed));
        if (resnorm) {
            if (listed) CHECK(ctx->dtype == CSMP_F32 ? run.residual<float>() : run.residual<double>());
            hipLaunchKernelGGL(k_jista_norm2, dim3((unsigned)nsig), dim3(256), 0, ctx->stream, (const double*)g.R, g.ldr, (int)ctx->M, (double*)tNrm.p);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipMemcpy2DAsync(X, (size_t)ldX * 8, run.X, (size_t)run.ldx * 8, (size_t)ctx->N * 8, ncol, out_kind, ctx->stream));
        if (resnorm) HIPCHECK(hipMemcpyAsync(resnorm, tNrm.p, ncol * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (listed) {
            cnt.assign((size_t)nseg, 0);
            PinFetch f(ctx);
            CHECK(f.begin((size_t)nseg * 4));
            CHECK(f.add(cnt.data(), run.seg_cnt, (size_t)nseg * 4));
            CHECK(f.wait());
        } else {
            HIPCHECK(hipStreamSynchronize(ctx->stream));
        }
        if (resnorm)
            for (int64_t l = 0; l < nsig; ++l) resnorm[l] = std::sqrt(resnorm[l]);
        if (nrows) *nrows = jista_rows(cnt);
        return CSMP_OK;
    };
    return finish(jista_nomem(ctx, solve()));
}
