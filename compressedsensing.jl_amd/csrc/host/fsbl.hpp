// host/fsbl.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_fsbl and csmp_rmps (fsbl / rmps, src/sbl.jl:57-437, for a scalar noise variance).  One step is the N-pass k_fsbl_score and
// k_fsbl_pick, ONE host read -- the decision record -- and, where an action was decided, k_fsbl_col, k_bp_gemv (BP_FULL), k_fsbl_rank1
// and the product sweep; the S / Q update of the step rides in the next N-pass.  The buffers live in the context's FsblBuf, apart from
// SblBuf and from csmp_bp's and csmp_bpd's kept factors: no call here reads or invalidates them.
// ------------------------------------------------------------------------------------------ greedy sparse Bayesian learning
static bool fsbl_vec(const csmp_ctx* ctx) {
    // 16-byte loads of a column's rows need the column starts on 16-byte boundaries
    const size_t esz = ctx->dtype == CSMP_F32 ? 4 : 8;
    return ((uintptr_t)ctx->dA % 16 == 0) && ((size_t)ctx->ld * esz) % 16 == 0 && !ctx->tune_fsbl_scalar;
}
static int64_t fsbl_per(int64_t N) { return ((N + kFsblParts - 1) / kFsblParts + 255) / 256 * 256; }  // atoms of a workgroup of k_fsbl_score
static int fsbl_nparts(int64_t N) { return (int)((N + fsbl_per(N) - 1) / fsbl_per(N)); }

// The buffers of the context for the resident dictionary: all of them, or none.
static int fsbl_ensure(csmp_ctx* ctx) {
    FsblBuf& t = ctx->fsbl;
    if (t.Ci && t.M == (int)ctx->M && t.N == ctx->N) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    fsbl_free(t);
    FsblBuf n;
    const size_t M = (size_t)ctx->M, N = (size_t)ctx->N;
    n.Mp = (int)((M + 255) / 256 * 256);
    n.ldc = (int64_t)((M + 1) / 2 * 2);
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.Ci, (size_t)n.ldc * M));
        CHECK(dmalloc(ctx, &n.vec, (size_t)2 * n.Mp));
        CHECK(dmalloc(ctx, &n.alpha, N));
        CHECK(dmalloc(ctx, &n.S, N));
        CHECK(dmalloc(ctx, &n.Q, N));
        CHECK(dmalloc(ctx, &n.w, N));
        CHECK(dmalloc(ctx, &n.x, N));
        CHECK(dmalloc(ctx, &n.pval, (size_t)kFsblParts));
        CHECK(dmalloc(ctx, &n.pidx, (size_t)kFsblParts));
        CHECK(dmalloc(ctx, &n.rec, (size_t)1));
        // (the sweep reads v up to whole vectors, k_fsbl_rank1 up to ldc: zeros beyond M, which no kernel writes)
        HIPCHECK(hipMemsetAsync(n.vec, 0, (size_t)2 * n.Mp * sizeof(double), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        fsbl_free(n);
        return rc;
    }
    n.M = (int)ctx->M;
    n.N = ctx->N;
    t = n;
    return CSMP_OK;
}
static int fsbl_nomem(csmp_ctx* ctx, const char* who, int rc) {
    if (rc == CSMP_EHIP)
        return fail(ctx, CSMP_ENOMEM, std::string(who) + ": no device memory for C^-1, size(A,1)^2 doubles, and the vectors (" + ctx->err + ")");
    return rc;
}
static int fsbl_entry(csmp_ctx* ctx, const char* who) {
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
    if (ctx->streamed) return fail(ctx, CSMP_ESTATE, std::string(who) + ": a host-streamed dictionary is not served");
    if (ctx->M > kBpMaxRows) return fail(ctx, CSMP_ERANGE, std::string(who) + ": more than 2^19 rows");
    return CSMP_OK;
}

// the N-pass (the pending S / Q update, then the values of a mode) and the pick; vals: where every atom's value goes (NULL: nowhere)
static int fsbl_score(csmp_ctx* ctx, int mode, double* vals = nullptr) {
    FsblBuf& t = ctx->fsbl;
    const int np = fsbl_nparts(ctx->N);
    hipLaunchKernelGGL(k_fsbl_score, dim3(np), dim3(256), 0, ctx->stream, (const double*)t.alpha, t.S, t.Q, (const double*)t.w,
                       (const FsblRec*)t.rec, ctx->N, fsbl_per(ctx->N), mode, vals, t.pval, t.pidx);
    if (mode != FSBL_MODE_NONE)
        hipLaunchKernelGGL(k_fsbl_pick, dim3(1), dim3(256), 0, ctx->stream, (const double*)t.pval, (const long long*)t.pidx, np, mode, t.alpha,
                           (const double*)t.S, (const double*)t.Q, (long long)-1, 0.0, t.rec);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}
// the record of a rank-one step of atom i with the given gamma (alpha untouched)
static int fsbl_force(csmp_ctx* ctx, int64_t i, double gamma) {
    FsblBuf& t = ctx->fsbl;
    hipLaunchKernelGGL(k_fsbl_pick, dim3(1), dim3(256), 0, ctx->stream, (const double*)t.pval, (const long long*)t.pidx, 0, (int)FSBL_MODE_NONE, t.alpha,
                       (const double*)t.S, (const double*)t.Q, (long long)i, gamma, t.rec);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}
static int fsbl_col(csmp_ctx* ctx) {
    FsblBuf& t = ctx->fsbl;
    const int M = (int)ctx->M;
    const bool vec = fsbl_vec(ctx);
    const FsblRec* rec = t.rec;
    if (ctx->dtype == CSMP_F32) {
        const dim3 g((unsigned)((M + 1023) / 1024));
        if (vec) hipLaunchKernelGGL((k_fsbl_col<float, true>), g, dim3(256), 0, ctx->stream, (const float*)ctx->dA, ctx->ld, M, rec, t.vec);
        else hipLaunchKernelGGL((k_fsbl_col<float, false>), g, dim3(256), 0, ctx->stream, (const float*)ctx->dA, ctx->ld, M, rec, t.vec);
    } else {
        const dim3 g((unsigned)((M + 511) / 512));
        if (vec) hipLaunchKernelGGL((k_fsbl_col<double, true>), g, dim3(256), 0, ctx->stream, (const double*)ctx->dA, ctx->ld, M, rec, t.vec);
        else hipLaunchKernelGGL((k_fsbl_col<double, false>), g, dim3(256), 0, ctx->stream, (const double*)ctx->dA, ctx->ld, M, rec, t.vec);
    }
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}
static int fsbl_gemv(csmp_ctx* ctx) {
    FsblBuf& t = ctx->fsbl;
    const int M = (int)ctx->M;
    hipLaunchKernelGGL(k_bp_gemv, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, ctx->stream, (const double*)t.Ci, t.ldc, M, (int)BP_FULL,
                       (const double*)t.vec, t.vec + t.Mp);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}
static int fsbl_rank1(csmp_ctx* ctx) {
    FsblBuf& t = ctx->fsbl;
    hipLaunchKernelGGL(k_fsbl_rank1, dim3((unsigned)ctx->M, (unsigned)((t.ldc + 511) / 512)), dim3(256), 0, ctx->stream, t.Ci, t.ldc,
                       (const double*)(t.vec + t.Mp), (const FsblRec*)t.rec);
    HIPCHECK(hipGetLastError());
    return CSMP_OK;
}
static int fsbl_sweep(csmp_ctx* ctx) { return launch_sweep(ctx, ctx->fsbl.vec + ctx->fsbl.Mp, 0.0, 0, 0, ctx->fsbl.w); }
// sqc(i, gamma) of the record: C^-1 and w now, S and Q in the next N-pass.  No wait.
static int fsbl_step(csmp_ctx* ctx) {
    CHECK(fsbl_col(ctx));
    CHECK(fsbl_gemv(ctx));
    CHECK(fsbl_rank1(ctx));
    return fsbl_sweep(ctx);
}
static int fsbl_fetch(csmp_ctx* ctx, FsblRec* out) {
    PinFetch f(ctx);
    CHECK(f.begin(sizeof(FsblRec) + 16));
    CHECK(f.add(out, ctx->fsbl.rec, sizeof(FsblRec)));
    return f.wait();
}

// The checks both drivers share, the buffers, b, the state of alpha = +inf -- C^-1 = I / sigma2, S = |a_j|^2 / sigma2, Q = A'b / sigma2 --
// and the warm start: one sqc(j, 1 / alpha_j) per finite entry of alpha_in, in index order.  ha: the host's copy of alpha.
static int fsbl_begin(csmp_ctx* ctx, const char* who, const void* b, int b_dtype, double sigma2, double min_increase, const double* alpha_in, double* x,
                      int loc, std::vector<double>& ha) {
    const std::string w(who);
    if (!b || !x) return fail(ctx, CSMP_EINVAL, w + ": bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if (loc != CSMP_HOST && loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, w + ": loc must be CSMP_HOST or CSMP_DEVICE");
    if (!std::isfinite(sigma2) || !(sigma2 > 0.0)) return fail(ctx, CSMP_EINVAL, w + ": sigma2 has to be positive and finite");
    if (!(min_increase >= 0.0)) return fail(ctx, CSMP_EINVAL, w + ": min_increase has to be non-negative");
    CHECK(fsbl_entry(ctx, who));
    const int64_t N = ctx->N;
    const int M = (int)ctx->M;
    HIPCHECK(hipSetDevice(ctx->dev));
    ha.assign((size_t)N, HUGE_VAL);
    if (alpha_in) {
        if (loc == CSMP_HOST) {
            memcpy(ha.data(), alpha_in, (size_t)N * sizeof(double));
        } else {
            HIPCHECK(hipMemcpyAsync(ha.data(), alpha_in, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHECK(hipStreamSynchronize(ctx->stream));
        }
        for (int64_t j = 0; j < N; ++j)
            if (!(ha[(size_t)j] > 0.0)) return fail(ctx, CSMP_EINVAL, w + ": every entry of alpha has to be positive, or +inf for an inactive atom");
    }
    {
        int rc = solver_ensure(ctx, 1, 1, false);
        if (rc == CSMP_OK) rc = fsbl_ensure(ctx);
        CHECK(fsbl_nomem(ctx, who, rc));
    }
    FsblBuf& t = ctx->fsbl;
    Solver& s = ctx->s;
    s.begun = false;
    if (loc == CSMP_DEVICE)
        CHECK(b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)b) : init_from_device_t<double>(ctx, (const double*)b));
    else
        CHECK(upload_b(ctx, b, b_dtype));
    const unsigned gridN = (unsigned)((N + 255) / 256);
    HIPCHECK(hipMemsetAsync(t.rec, 0, sizeof(FsblRec), ctx->stream));
    hipLaunchKernelGGL(k_fsbl_eye, dim3((unsigned)((t.ldc * M + 255) / 256)), dim3(256), 0, ctx->stream, t.Ci, t.ldc, M, sigma2);
    if (ctx->dtype == CSMP_F32)
        hipLaunchKernelGGL(k_fr_colnorm2<float>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, (const float*)ctx->dA, ctx->ld, M, N, t.S);
    else
        hipLaunchKernelGGL(k_fr_colnorm2<double>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, (const double*)ctx->dA, ctx->ld, M, N, t.S);
    HIPCHECK(hipGetLastError());
    CHECK(launch_sweep(ctx, s.r, 0.0, 0, 0, t.Q));
    hipLaunchKernelGGL(k_fsbl_scale, dim3(gridN), dim3(256), 0, ctx->stream, t.S, t.Q, N, sigma2);
    HIPCHECK(hipGetLastError());
    if (alpha_in) {
        HIPCHECK(hipMemcpyAsync(t.alpha, alpha_in, (size_t)N * sizeof(double), loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                ctx->stream));
        for (int64_t j = 0; j < N; ++j) {
            if (!std::isfinite(ha[(size_t)j])) continue;
            CHECK(fsbl_score(ctx, FSBL_MODE_NONE));
            CHECK(fsbl_force(ctx, j, 1.0 / ha[(size_t)j]));
            CHECK(fsbl_step(ctx));
        }
    } else {
        hipLaunchKernelGGL(k_fsbl_fill, dim3(gridN), dim3(256), 0, ctx->stream, t.alpha, N, HUGE_VAL);
        HIPCHECK(hipGetLastError());
    }
    return CSMP_OK;
}
// one N-pass of a mode and its read; an applied action runs its rank-one step and joins the history
struct FsblRun {
    int64_t *history, cap, applied = 0;
};
static int fsbl_turn(csmp_ctx* ctx, const char* who, int mode, std::vector<double>& ha, FsblRun& run, FsblRec& r) {
    CHECK(fsbl_score(ctx, mode));
    CHECK(fsbl_fetch(ctx, &r));
    if (r.bad) return fail(ctx, CSMP_EINVAL, std::string(who) + ": a value of the marginal likelihood's change is not finite");
    if (r.action != FSBL_ACT_NONE) {
        CHECK(fsbl_step(ctx));
        ha[(size_t)r.i] = r.alpha_new;
        if (run.history && run.applied < run.cap) {
            run.history[2 * run.applied] = r.action;
            run.history[2 * run.applied + 1] = r.i;
        }
        run.applied += 1;
    }
    return CSMP_OK;
}
// the pending update, x = Q / alpha on the active atoms, and the results to where loc says
static int fsbl_finish(csmp_ctx* ctx, double* x, double* alpha_out, int loc) {
    FsblBuf& t = ctx->fsbl;
    const int64_t N = ctx->N;
    CHECK(fsbl_score(ctx, FSBL_MODE_NONE));
    HIPCHECK(hipMemsetAsync(t.rec, 0, sizeof(FsblRec), ctx->stream));
    hipLaunchKernelGGL(k_fsbl_x, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.alpha, (const double*)t.Q, N, t.x);
    HIPCHECK(hipGetLastError());
    const hipMemcpyKind out = loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHECK(hipMemcpyAsync(x, t.x, (size_t)N * sizeof(double), out, ctx->stream));
    if (alpha_out) HIPCHECK(hipMemcpyAsync(alpha_out, t.alpha, (size_t)N * sizeof(double), out, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    return CSMP_OK;
}

extern "C" int csmp_fsbl(csmp_ctx* ctx, const void* b, int b_dtype, double sigma2, int64_t maxiter, double min_increase, const double* alpha_in,
                         double* x, double* alpha_out, int loc, int64_t* history, int64_t history_cap, int64_t* iterations, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (maxiter < 1) return fail(ctx, CSMP_EINVAL, "fsbl: maxiter has to be at least 1");
    if (history && history_cap < 0) return fail(ctx, CSMP_EINVAL, "fsbl: history_cap has to be non-negative");
    std::vector<double> ha;
    CHECK(fsbl_begin(ctx, "fsbl", b, b_dtype, sigma2, min_increase, alpha_in, x, loc, ha));
    FsblRun run{history, history_cap};
    int64_t iters = 0;
    bool conv = false;
    for (int64_t it = 1; it <= maxiter; ++it) {
        FsblRec r;
        CHECK(fsbl_turn(ctx, "fsbl", FSBL_MODE_ALL, ha, run, r));
        iters = it;
        if (r.value < min_increase) {  // maximum(delta) < min_increase, after the pass (:158)
            conv = true;
            break;
        }
    }
    CHECK(fsbl_finish(ctx, x, alpha_out, loc));
    if (iterations) *iterations = iters;
    if (flags) *flags = conv ? CSMP_FSBL_CONVERGED : 0;
    return CSMP_OK;
}

extern "C" int csmp_rmps(csmp_ctx* ctx, const void* b, int b_dtype, double sigma2, int64_t maxiter, int64_t maxiter_acquisition,
                         int64_t maxiter_deletion, double min_increase, const double* alpha_in, double* x, double* alpha_out, int loc, int64_t* history,
                         int64_t history_cap, int64_t* iterations, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (maxiter < 1 || maxiter_acquisition < 1 || maxiter_deletion < 1)
        return fail(ctx, CSMP_EINVAL, "rmps: maxiter, maxiter_acquisition and maxiter_deletion have to be at least 1");
    if (history && history_cap < 0) return fail(ctx, CSMP_EINVAL, "rmps: history_cap has to be non-negative");
    std::vector<double> ha;
    CHECK(fsbl_begin(ctx, "rmps", b, b_dtype, sigma2, min_increase, alpha_in, x, loc, ha));
    FsblRun run{history, history_cap};
    std::vector<double> old = ha;
    // old != alpha as arrays of doubles: +inf equals +inf, and no entry is ever NaN
    auto unchanged = [&]() { return old == ha; };
    bool conv = false;
    for (int64_t it = 1; it <= maxiter; ++it) {
        FsblRec r;
        for (int64_t k = 0; k < maxiter_acquisition; ++k) {  // acquisition stage (:390-392)
            CHECK(fsbl_turn(ctx, "rmps", FSBL_MODE_ADD, ha, run, r));
            if (r.action == FSBL_ACT_NONE) break;
        }
        if (unchanged()) {
            conv = true;
            break;
        }
        old = ha;
        for (int64_t k = 0; k < maxiter_deletion; ++k) {  // deletion and update stage (:395-401)
            CHECK(fsbl_turn(ctx, "rmps", FSBL_MODE_RMP_DEL, ha, run, r));
            if (r.action != FSBL_ACT_NONE) continue;
            CHECK(fsbl_turn(ctx, "rmps", FSBL_MODE_UPD, ha, run, r));
            const double gain = r.action != FSBL_ACT_NONE ? r.value : 0.0;
            if (gain < min_increase) break;
        }
        if (unchanged()) {
            conv = true;
            break;
        }
        old = ha;
    }
    CHECK(fsbl_finish(ctx, x, alpha_out, loc));
    if (iterations) *iterations = run.applied;
    if (flags) *flags = conv ? CSMP_RMPS_CONVERGED : 0;
    return CSMP_OK;
}

// ------------------------------------------------------------------------------------------ measurement (include/csmp_internal.h)
extern "C" int csmp_fsbl_score(csmp_ctx* ctx, const double* alpha, const double* S, const double* Q, int mode, double* values, int64_t* pick,
                               double* value, int* action) {
    if (!ctx) return CSMP_EINVAL;
    if (!alpha || !S || !Q || !values) return fail(ctx, CSMP_EINVAL, "fsbl_score: bad arguments");
    if (mode < FSBL_MODE_ALL || mode > FSBL_MODE_UPD) return fail(ctx, CSMP_EINVAL, "fsbl_score: mode has to be 1 .. 4");
    CHECK(fsbl_entry(ctx, "fsbl_score"));
    HIPCHECK(hipSetDevice(ctx->dev));
    CHECK(fsbl_nomem(ctx, "fsbl_score", fsbl_ensure(ctx)));
    FsblBuf& t = ctx->fsbl;
    const size_t nbytes = (size_t)ctx->N * sizeof(double);
    HIPCHECK(hipMemcpyAsync(t.alpha, alpha, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipMemcpyAsync(t.S, S, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipMemcpyAsync(t.Q, Q, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipMemsetAsync(t.rec, 0, sizeof(FsblRec), ctx->stream));
    CHECK(fsbl_score(ctx, mode, t.x));
    FsblRec r;
    CHECK(fsbl_fetch(ctx, &r));
    HIPCHECK(hipMemcpyAsync(values, t.x, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipMemsetAsync(t.rec, 0, sizeof(FsblRec), ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    if (r.bad) return fail(ctx, CSMP_EINVAL, "fsbl_score: a value of the marginal likelihood's change is not finite");
    if (pick) *pick = r.i;
    if (value) *value = r.value;
    if (action) *action = r.action;
    return CSMP_OK;
}

extern "C" int csmp_fsbl_sqc(csmp_ctx* ctx, double* Cinv, double* S, double* Q, int64_t i, double gamma) {
    if (!ctx) return CSMP_EINVAL;
    if (!Cinv || !S || !Q) return fail(ctx, CSMP_EINVAL, "fsbl_sqc: bad arguments");
    CHECK(fsbl_entry(ctx, "fsbl_sqc"));
    if (i < 0 || i >= ctx->N) return fail(ctx, CSMP_EINVAL, "fsbl_sqc: i has to be a column of A");
    if (!std::isfinite(gamma) || gamma == 0.0) return fail(ctx, CSMP_EINVAL, "fsbl_sqc: gamma has to be finite and not zero");
    HIPCHECK(hipSetDevice(ctx->dev));
    {
        int rc = solver_ensure(ctx, 1, 1, false);
        if (rc == CSMP_OK) rc = fsbl_ensure(ctx);
        CHECK(fsbl_nomem(ctx, "fsbl_sqc", rc));
    }
    FsblBuf& t = ctx->fsbl;
    const size_t M = (size_t)ctx->M, nbytes = (size_t)ctx->N * sizeof(double);
    HIPCHECK(hipMemsetAsync(t.Ci, 0, (size_t)t.ldc * M * sizeof(double), ctx->stream));
    HIPCHECK(hipMemcpy2DAsync(t.Ci, (size_t)t.ldc * sizeof(double), Cinv, M * sizeof(double), M * sizeof(double), M, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipMemcpyAsync(t.S, S, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipMemcpyAsync(t.Q, Q, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(hipMemsetAsync(t.rec, 0, sizeof(FsblRec), ctx->stream));
    CHECK(fsbl_force(ctx, i, gamma));
    CHECK(fsbl_step(ctx));
    CHECK(fsbl_score(ctx, FSBL_MODE_NONE));
    HIPCHECK(hipMemsetAsync(t.rec, 0, sizeof(FsblRec), ctx->stream));
    HIPCHECK(hipMemcpy2DAsync(Cinv, M * sizeof(double), t.Ci, (size_t)t.ldc * sizeof(double), M * sizeof(double), M, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipMemcpyAsync(S, t.S, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipMemcpyAsync(Q, t.Q, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    return CSMP_OK;
}

extern "C" int csmp_bench_fsbl(csmp_ctx* ctx, int reps, double* score_ms, double* colgemv_ms, double* rank1_ms, double* sweep_ms) {
    if (!ctx || reps < 1) return CSMP_EINVAL;
    CHECK(fsbl_entry(ctx, "bench_fsbl"));
    FsblBuf& t = ctx->fsbl;
    if (!t.Ci || t.M != (int)ctx->M || t.N != ctx->N) return fail(ctx, CSMP_ESTATE, "bench_fsbl: no state (call csmp_fsbl first)");
    HIPCHECK(hipSetDevice(ctx->dev));
    hipEvent_t ev[5];
    for (auto& e : ev) HIPCHECK(hipEventCreate(&e));
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    int rc = CSMP_OK;
    for (int i = 0; i <= reps && rc == CSMP_OK; ++i) {  // (run 0 warms up)
        auto run = [&]() -> int {
            // every run adds the prior variance 1 to atom 0: a valid step on whatever state the last call left
            HIPCHECK(hipEventRecord(ev[0], ctx->stream));
            CHECK(fsbl_score(ctx, FSBL_MODE_ALL));
            CHECK(fsbl_force(ctx, 0, 1.0));
            HIPCHECK(hipEventRecord(ev[1], ctx->stream));
            CHECK(fsbl_col(ctx));
            CHECK(fsbl_gemv(ctx));
            HIPCHECK(hipEventRecord(ev[2], ctx->stream));
            CHECK(fsbl_rank1(ctx));
            HIPCHECK(hipEventRecord(ev[3], ctx->stream));
            CHECK(fsbl_sweep(ctx));
            HIPCHECK(hipEventRecord(ev[4], ctx->stream));
            HIPCHECK(hipStreamSynchronize(ctx->stream));
            for (int k = 0; k < 4; ++k) {
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
    if (score_ms) *score_ms = sum[0] / reps;
    if (colgemv_ms) *colgemv_ms = sum[1] / reps;
    if (rank1_ms) *rank1_ms = sum[2] / reps;
    if (sweep_ms) *sweep_ms = sum[3] / reps;
    return CSMP_OK;
}
