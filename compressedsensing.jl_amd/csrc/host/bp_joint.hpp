// host/bp_joint.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_bp_joint -- row-sparse basis pursuit, min sum_j w_j ||X[j, :]||_2 subject to A X = B: ONE row support for all columns of B
// (kernels and the step: csmp_bp_joint.hpp).
// ------------------------------------------------------------------------------------------ bp_joint
// csmp_bp's ADMM with matrices in place of vectors.  The factor of A A' is bp_prepare's, kept with the dictionary.  The columns live
// in the call's own arrays, all allocated or none, released when the call returns: nsig is bounded by memory only,
//     8 (8 Mpad + 4 size(A,2)) + 64 bytes a column  (B, R, P, Q, E, V, Y, G Y of Mpad = size(A,1) rounded up to 256 rows; C, Z, U and the
//     list's values)
// beside what does not grow with nsig: the weights, the list's indices, the norms' partials and ONE chunk's partials of the residual
// (JistaRun::residual: CHUNK AFTER CHUNK on the stream, so the partials never exceed one chunk's).  An iteration, everything on the
// context's stream: three k_bp_gemm per chunk of up to eight columns (V, Y, G Y), csmp_somp's passes with Y as their residuals
// (SompRun::passes: the shared pass over chunks of up to group_wide columns where the resident dictionary has one, else one
// launch_sweep per column), k_jbp_update, the joint residual, k_jbp_pq.  Nothing is read back inside an interval of check_every
// iterations; at its end k_bp_fold adds the segments' partials and the host reads the two numbers through one PinFetch: ONE
// stopping rule for all columns.  One column is csmp_bp: it takes csmp_bp's own solve on the context's buffers.
static int jbp_nomem(csmp_ctx* ctx, int rc) {
    if (rc == CSMP_EHIP && ctx->err.find("hipMalloc") != std::string::npos)
        return fail(ctx, CSMP_ENOMEM, "bp_joint: no device memory for the iterates (" + ctx->err + ")");
    return rc;
}

struct JbpRun {
    csmp_ctx* ctx;
    SompRun pass;    // Y as the passes' "residuals", C and the passes' control blocks
    JistaRun res;    // R = B - A Z+ over the joint list: csmp_ista_joint's residual, its list and its partials
    double *P, *Q, *E, *V, *Y, *GY;  // column l from l * ldr (ldr = pass.g.ldr; rows past size(A,1) zero)
    double *Z, *U;                   // column l from l * ldx
    double *rpart, *fold;            // the norms' partials (k_bp_update's layout) and the two numbers the host reads
    double rho;

    int gemms() const {
        const BpBuf& t = ctx->bp;
        const int M = (int)ctx->M, np = t.np, npa = 2 * np, nsig = pass.g.nsig;
        const double* T = t.Gm + (size_t)np * npa;  // R^-T, lower
        const double* Ri = t.Gm + np;               // R^-1, upper
        const int64_t ldr = pass.g.ldr;
        for (int c0 = 0; c0 < nsig; c0 += kBpGemmMax) {
            const int L = std::min(kBpGemmMax, nsig - c0);
            BpGemm g1, g2, g3;
            for (int i = 0; i < kBpGemmMax; ++i) {
                const int64_t at = (int64_t)(c0 + std::min(i, L - 1)) * ldr;
                g1.x[i] = E + at; g1.out[i] = V + at;
                g2.x[i] = V + at; g2.out[i] = Y + at;
                g3.x[i] = Y + at; g3.out[i] = GY + at;
            }
            HIPCHECK(bp_gemm_launch(ctx, L, Ri, (int64_t)npa, M, (int)BP_UPPER, g1));
            HIPCHECK(bp_gemm_launch(ctx, L, T, (int64_t)npa, M, (int)BP_LOWER, g2));
            HIPCHECK(bp_gemm_launch(ctx, L, t.G, (int64_t)M, M, (int)BP_FULL, g3));
        }
        return CSMP_OK;
    }
    unsigned mgrid() const { return (unsigned)((int64_t)((ctx->M + 255) / 256) * pass.g.nsig); }
    int start() const {
        const int wgs = (int)((ctx->M + 255) / 256);
        hipLaunchKernelGGL(k_jbp_start, dim3(mgrid()), dim3(256), 0, ctx->stream, (const double*)res.Bd, pass.g.ldr, (int)ctx->M, pass.g.nsig, wgs, P, Q, E);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    int update() const {
        const int64_t seg_len = ista_seg_len(ctx->N);
        const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
        hipLaunchKernelGGL(k_jbp_update, dim3(nseg), dim3(kIstaThreads), 0, ctx->stream, (const double*)pass.g.C, pass.g.ldc, (const double*)res.w, res.nw,
                           rho, Z, U, res.ldx, pass.g.nsig, ctx->N, seg_len, res.lidx, res.lval, res.seg_cnt, rpart);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    int pq() const {
        const int wgs = (int)((ctx->M + 255) / 256);
        hipLaunchKernelGGL(k_jbp_pq, dim3(mgrid()), dim3(256), 0, ctx->stream, (const double*)res.Bd, (const double*)res.pass.g.R, (const double*)GY,
                           pass.g.ldr, (int)ctx->M, pass.g.nsig, wgs, P, Q, E);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
    // bp_iterate for all columns: one stopping rule
    template <typename TA>
    int iterate(int64_t maxiter, double tol, int64_t check_every, int64_t* iters, bool* converged) {
        const int64_t seg_len = ista_seg_len(ctx->N);
        const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
        *iters = 0;
        *converged = false;
        for (int64_t it = 1; it <= maxiter; ++it) {
            CHECK(gemms());
            CHECK(pass.passes<TA>(0));
            CHECK(update());
            CHECK(res.residual<TA>());
            CHECK(pq());
            *iters = it;
            if (it % check_every == 0) {
                hipLaunchKernelGGL(k_bp_fold, dim3(1), dim3(256), 0, ctx->stream, (const double*)rpart, nseg, fold);
                HIPCHECK(hipGetLastError());
                double r2[2];
                {
                    PinFetch f(ctx);
                    CHECK(f.begin(sizeof r2));
                    CHECK(f.add(r2, fold, sizeof r2));
                    CHECK(f.wait());
                }
                if (std::sqrt(r2[0]) < tol && rho * std::sqrt(r2[1]) < tol) {
                    *converged = true;
                    break;
                }
            }
        }
        return CSMP_OK;
    }
};

extern "C" int csmp_bp_joint(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, const double* w, int64_t nw,
                             double rho, int64_t maxiter, double tol, int64_t check_every, double* X, int64_t ldX, int x_loc,
                             int64_t* iterations, int64_t* nrows, double* resnorm, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (nsig < 0) return fail(ctx, CSMP_EINVAL, "bp_joint: nsig has to be non-negative");
    if (!w || (nsig > 0 && (!B || !X))) return fail(ctx, CSMP_EINVAL, "bp_joint: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if ((b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) || (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE))
        return fail(ctx, CSMP_EINVAL, "bp_joint: b_loc / x_loc must be CSMP_HOST or CSMP_DEVICE");
    CHECK(bp_entry(ctx, "bp_joint"));
    if (ldB < ctx->M) return fail(ctx, CSMP_EDIM, "bp_joint: ldB < size(A, 1)");
    if (ldX < ctx->N) return fail(ctx, CSMP_EDIM, "bp_joint: ldX < size(A, 2)");
    if (nw != 1 && nw != ctx->N) return fail(ctx, CSMP_EDIM, "bp_joint: length(w) must be 1 or size(A, 2)");
    CHECK(bp_check_knobs(ctx, "bp_joint", rho, maxiter, tol, check_every));
    for (int64_t i = 0; i < nw; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(ctx, CSMP_EINVAL, "bp_joint: the weights have to be non-negative and finite");
    if (nsig > ((int64_t)1 << 22)) return fail(ctx, CSMP_ERANGE, "bp_joint: nsig too large");  // (grids of nsig * ceil(size(A,1) / 256) workgroups)
    if (nsig == 0) return CSMP_OK;
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    bool did = false;
    CHECK(bp_prepare(ctx, &did));
    Solver& s = ctx->s;
    s.begun = false;
    auto finish = [&](int rc) -> int {
        (void)hipStreamSynchronize(ctx->stream);  // (on every way out: the temporaries and the caller's buffers are at rest)
        return rc;
    };
    const size_t esz = b_dtype == CSMP_F32 ? 4 : 8;
    const int64_t seg_len = ista_seg_len(ctx->N);
    const int nseg = (int)((ctx->N + seg_len - 1) / seg_len);
    const hipMemcpyKind out_kind = x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    std::vector<int> cnt;  // the segments' counts of the final list

    DevTmp tB;  // a host caller's B on the device
    const void* dB = B;
    if (b_loc == CSMP_HOST) {
        const size_t bbytes = ((size_t)ldB * (size_t)(nsig - 1) + (size_t)ctx->M) * esz;  // (the last column ends at its last row)
        CHECK(jbp_nomem(ctx, tB.alloc(ctx, bbytes)));
        HIPCHECK(hipMemcpy(tB.p, B, bbytes, hipMemcpyHostToDevice));
        dB = tB.p;
    }

    if (nsig == 1) {  // the problem IS csmp_bp's: its solve, its bits (csmp_bp_batch's lone signal)
        auto one = [&]() -> int {
            HIPCHECK(hipMemcpyAsync(ctx->ista.w, w, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            int64_t iters = 0;
            int conv = 0;
            BpBatchRun run{};
            run.ctx = ctx; run.dB = (const char*)dB; run.b_dtype = b_dtype; run.ldB = ldB; run.nw = nw; run.rho = rho; run.tol = tol;
            run.X = X; run.ldX = ldX; run.x_loc = x_loc; run.iterations = &iters; run.resnorm = resnorm; run.flags = &conv;
            run.maxiter = maxiter; run.check_every = check_every;
            CHECK(run.solve_one(0));
            int64_t rows = 0;
            if (nrows && iters > 0) {  // (the list is that of the result)
                cnt.assign((size_t)nseg, 0);
                PinFetch f(ctx);
                CHECK(f.begin((size_t)nseg * 4));
                CHECK(f.add(cnt.data(), ctx->ista.seg_cnt, (size_t)nseg * 4));
                CHECK(f.wait());
                rows = jista_rows(cnt);
            }
            if (iterations) *iterations = iters;
            if (nrows) *nrows = rows;
            if (flags) *flags = conv | (did ? CSMP_BP_FACTORED : 0);
            return CSMP_OK;
        };
        return finish(one());
    }

    DevTmp tVec, tC, tZU, tLv, tLi, tSeg, tNnz, tW, tPart, tRp, tSt, tPv, tPi, tNrm;
    JbpRun run{};
    run.ctx = ctx;
    run.rho = rho;
    JistaRun& rs = run.res;
    rs.ctx = ctx;
    rs.nw = nw;
    rs.P = ista_parts_max(ctx);
    rs.ldx = (ctx->N + 1) / 2 * 2;
    SompRun& ps = run.pass;
    ps.ctx = ctx;
    ps.grouped = ctx->sweep_group >= 1;
    ps.pcap = ctx->prop.multiProcessorCount * 8 + 8;  // (what pipe_nblk allows a pass: solver_alloc's pval / pidx)
    SompCols& g = ps.g;
    g.nsig = (int)nsig;
    g.ldr = s.Mpad;
    g.ldc = rs.ldx;
    const size_t ncol = (size_t)nsig, mat = ncol * (size_t)g.ldr, xbytes = ncol * (size_t)rs.ldx * 8;
    auto allocate = [&]() -> int {
        CHECK(tVec.alloc(ctx, 8 * mat * 8));
        CHECK(tC.alloc(ctx, ncol * g.ldc * 8));
        CHECK(tZU.alloc(ctx, 2 * xbytes));
        CHECK(tLv.alloc(ctx, (size_t)ctx->N * ncol * 8));
        CHECK(tLi.alloc(ctx, (size_t)ctx->N * 4));
        CHECK(tSeg.alloc(ctx, (size_t)kIstaMaxSegs * 4));
        CHECK(tNnz.alloc(ctx, 4));
        CHECK(tW.alloc(ctx, (size_t)nw * 8));
        CHECK(tPart.alloc(ctx, (size_t)std::min<int64_t>(nsig, kJistaChunk) * (size_t)rs.P * (size_t)ctx->Mv * 8));
        CHECK(tRp.alloc(ctx, ((size_t)2 * kIstaMaxSegs + 2) * 8));
        CHECK(tSt.alloc(ctx, ncol * sizeof(DevState)));
        CHECK(tPv.alloc(ctx, (size_t)kWideMax * ps.pcap * 8));
        CHECK(tPi.alloc(ctx, (size_t)kWideMax * ps.pcap * 4));
        if (resnorm) CHECK(tNrm.alloc(ctx, ncol * 8));
        return CSMP_OK;
    };
    CHECK(finish(jbp_nomem(ctx, allocate())));
    double* vec = (double*)tVec.p;
    rs.Bd = vec;
    rs.pass = ps;  // (the residual's columns: nsig and ldr; its passes are never run)
    rs.pass.g.R = vec + mat;
    run.P = vec + 2 * mat; run.Q = vec + 3 * mat; run.E = vec + 4 * mat; run.V = vec + 5 * mat; run.Y = vec + 6 * mat; run.GY = vec + 7 * mat;
    g.R = run.Y; g.C = (double*)tC.p; g.st = (DevState*)tSt.p;
    run.Z = (double*)tZU.p; run.U = run.Z + ncol * (size_t)rs.ldx;
    rs.X = run.Z; rs.Y = run.U;
    rs.lval = (double*)tLv.p; rs.lidx = (int*)tLi.p; rs.seg_cnt = (int*)tSeg.p; rs.nnz = (unsigned*)tNnz.p;
    rs.w = (double*)tW.p; rs.part = (double*)tPart.p;
    run.rpart = (double*)tRp.p; run.fold = run.rpart + (size_t)2 * kIstaMaxSegs;
    ps.ppv = (double*)tPv.p; ps.ppi = (int*)tPi.p;

    auto solve = [&]() -> int {
        HIPCHECK(hipMemcpyAsync(rs.w, w, (size_t)nw * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHECK(hipMemsetAsync(vec, 0, 8 * mat * 8, ctx->stream));  // (V, Y, G Y: the rows past size(A,1) stay zero -- the passes read Mpad rows)
        // B promoted (rows past size(A,1) zero) and the passes' control blocks reset; R = B, the residual of Z = 0
        SompCols gb = g;
        gb.R = rs.Bd;
        const int iw = (int)(g.ldr / 256);
        const dim3 igrid((unsigned)((int64_t)iw * nsig));
        if (b_dtype == CSMP_F32)
            hipLaunchKernelGGL(k_somp_init<float>, igrid, dim3(256), 0, ctx->stream, (const float*)dB, ldB, (int)ctx->M, gb, iw);
        else
            hipLaunchKernelGGL(k_somp_init<double>, igrid, dim3(256), 0, ctx->stream, (const double*)dB, ldB, (int)ctx->M, gb, iw);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(rs.pass.g.R, rs.Bd, mat * 8, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHECK(hipMemsetAsync(run.Z, 0, 2 * xbytes, ctx->stream));  // (U follows Z)
        CHECK(run.start());
        int64_t iters = 0;
        bool conv = false;
        CHECK(ctx->dtype == CSMP_F32 ? run.iterate<float>(maxiter, tol, check_every, &iters, &conv)
                                     : run.iterate<double>(maxiter, tol, check_every, &iters, &conv));
        if (resnorm) {  // R = B - A Z of the last iteration (R = B where there was none)
            hipLaunchKernelGGL(k_jbp_norm2, dim3((unsigned)nsig), dim3(256), 0, ctx->stream, (const double*)rs.pass.g.R, g.ldr, (int)ctx->M, (double*)tNrm.p);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipMemcpy2DAsync(X, (size_t)ldX * 8, run.Z, (size_t)rs.ldx * 8, (size_t)ctx->N * 8, ncol, out_kind, ctx->stream));
        if (resnorm) HIPCHECK(hipMemcpyAsync(resnorm, tNrm.p, ncol * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (iters > 0) {
            cnt.assign((size_t)nseg, 0);
            PinFetch f(ctx);
            CHECK(f.begin((size_t)nseg * 4));
            CHECK(f.add(cnt.data(), rs.seg_cnt, (size_t)nseg * 4));
            CHECK(f.wait());
        } else {
            HIPCHECK(hipStreamSynchronize(ctx->stream));
        }
        if (resnorm)
            for (int64_t l = 0; l < nsig; ++l) resnorm[l] = std::sqrt(resnorm[l]);
        if (iterations) *iterations = iters;
        if (nrows) *nrows = jista_rows(cnt);
        if (flags) *flags = (conv ? CSMP_BP_CONVERGED : 0) | (did ? CSMP_BP_FACTORED : 0);
        return CSMP_OK;
    };
    return finish(jbp_nomem(ctx, solve()));
}
