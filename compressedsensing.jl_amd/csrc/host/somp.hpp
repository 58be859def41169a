// host/somp.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_somp -- simultaneous OMP: ONE support for all columns of B (kernels and the step: csmp_somp.hpp).
// ------------------------------------------------------------------------------------------ somp
// The columns live in the call's own arrays (SompCols): nsig is bounded by memory only, 8 (size(A,1) + size(A,2) + k) bytes a column.
// The ONE factorisation is the solver slot's, grown by launch_append's safe chain (k_qr1 in mode 1 on the pick's partials, k_qr2,
// k_qr3) on a zero residual of its own.  A step's passes: the shared pass of the grouped scheduler (shared_pass_launch_of, host/omp.hpp)
// over chunks of up to group_wide columns where the resident dictionary has one, else one launch_sweep per column (the phased and
// the dynamic body, a host-streamed dictionary) -- the pick sees the same bits either way.  Everything is enqueued on the context's
// stream; the host looks at the control block every kPollSteps steps, as csmp_omp does, and once at the end.
static int somp_nomem(csmp_ctx* ctx, int rc) {
    if (rc == CSMP_EHIP && ctx->err.find("hipMalloc") != std::string::npos)
        return fail(ctx, CSMP_ENOMEM, "somp: no device memory for the columns, 8 (size(A,1) + size(A,2) + k) bytes each (" + ctx->err + ")");
    return rc;
}

struct SompRun {
    csmp_ctx* ctx;
    SompCols g;
    double* ppv;  // the passes' own arg-max partials (nobody reads them): one set per member of a pass
    int* ppi;
    int pcap;     // entries of a set
    int* nrun;
    int npick;    // workgroups of k_somp_pick
    bool grouped;
    int per_step;  // passes a step launches

    // c_l = A'r_l and ||r_l||^2 for every column
    template <typename TA>
    int passes(int skip) {
        if (!grouped) {
            Solver& s = ctx->s;
            DevState* const st0 = s.st;
            int rc = CSMP_OK;
            for (int l = 0; l < g.nsig && rc == CSMP_OK; ++l) {
                s.st = g.st + l;  // (the sweep writes ||r||^2 to the slot's control block and skips on its flags: this column's)
                rc = launch_sweep(ctx, g.R + (int64_t)l * g.ldr, 0.0, 0, skip, g.C + (int64_t)l * g.ldc);
            }
            s.st = st0;
            return rc;
        }
        const int W = ctx->group_wide;
        const int nblk = pipe_nblk(ctx, ctx->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid), nw = wide_nblk(ctx);
        const size_t excl = (size_t)(ctx->tune_pair_lds_kib > 0 ? ctx->tune_pair_lds_kib : kPairLdsKiB) * 1024;  // (one workgroup per CU, as the schedulers' passes)
        for (int off = 0; off < g.nsig; off += W) {
            const int size = std::min(W, g.nsig - off);
            CHECK(shared_pass_launch_of<TA>(ctx, size, 0.0, 0, skip, nblk, nw, excl, true, [&](int m) {
                const int64_t l = off + m;
                return PassMember{g.R + l * g.ldr, g.C + l * g.ldc, ppv + (size_t)m * pcap, ppi + (size_t)m * pcap, g.st + l};
            }));
        }
        return CSMP_OK;
    }

    int step(double eps, int check_eps, int p) {
        const int skip = STOP_EPS | STOP_STAG | STOP_FULL | STOP_REORTH;
        Solver& s = ctx->s;
        CHECK(ctx->dtype == CSMP_F32 ? passes<float>(skip) : passes<double>(skip));
        if (p == 1)
            hipLaunchKernelGGL(k_somp_pick<1>, dim3(npick), dim3(256), 0, ctx->stream, g, ctx->N, s.st, s.pval, s.pidx, eps, check_eps, skip, nrun);
        else
            hipLaunchKernelGGL(k_somp_pick<2>, dim3(npick), dim3(256), 0, ctx->stream, g, ctx->N, s.st, s.pval, s.pidx, eps, check_eps, skip, nrun);
        HIPCHECK(hipGetLastError());
        CHECK(launch_append(ctx, 1, 0, skip, false, 0.0, npick));
        hipLaunchKernelGGL(k_somp_project, dim3(g.nsig), dim3(256), 0, ctx->stream, g, (const DevState*)s.st, (const double*)s.Q, s.ldq);
        HIPCHECK(hipGetLastError());
        return CSMP_OK;
    }
};

extern "C" int csmp_somp(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k, double eps, int p,
                         int64_t* idx, double* val, int64_t ldval, int64_t* nnz, int64_t* order, double* resnorm, int64_t* passes,
                         int out_loc) {
    if (!ctx) return CSMP_EINVAL;
    if (!(eps >= 0.0)) return fail(ctx, CSMP_EINVAL, "somp: eps has to be non-negative");  // src/matchingpursuit.jl:74
    if (p != 1 && p != 2) return fail(ctx, CSMP_EINVAL, "somp: p has to be 1 or 2");
    if (nsig < 0 || k < 1) return fail(ctx, CSMP_EINVAL, "somp: nsig < 0 or k < 1");
    if (nsig > 0 && (!B || !idx || !val || !nnz)) return fail(ctx, CSMP_EINVAL, "somp: B, idx, val or nnz is NULL");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "somp: b_dtype must be CSMP_F32 or CSMP_F64");
    if ((b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) || (out_loc != CSMP_HOST && out_loc != CSMP_DEVICE))
        return fail(ctx, CSMP_EINVAL, "somp: b_loc / out_loc must be CSMP_HOST or CSMP_DEVICE");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "somp: no dictionary set (csmp_set_dictionary)");
    if (ldB < ctx->M || ldval < k) return fail(ctx, CSMP_EINVAL, "somp: ldB < size(A, 1) or ldval < k");
    if (k > ctx->M || k > ctx->N) return fail(ctx, CSMP_ERANGE, "somp: k exceeds min(size(A))");
    if (nsig > ((int64_t)1 << 22)) return fail(ctx, CSMP_ERANGE, "somp: nsig too large");  // (grids of nsig * ceil(size(A,1) / 256) workgroups)
    if (nsig == 0) return CSMP_OK;
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    auto finish = [&](int rc) -> int {
        (void)hipStreamSynchronize(ctx->stream);  // (on every way out: the temporaries and the caller's buffers are at rest)
        return rc;
    };
    const int kc = (int)k;
    CHECK(somp_nomem(ctx, solver_ensure(ctx, kc, 1)));
    Solver& s = ctx->s;
    s.begun = false;
    const int kcap = s.kcap;  // (the slot only grows: R_fac's leading dimension)
    const size_t esz = b_dtype == CSMP_F32 ? 4 : 8;
    const bool host_out = out_loc == CSMP_HOST;

    DevTmp tB, tR, tC, tZ, tSt, tPv, tPi, tRun, tIdx, tVal, tOrd, tRes, tNnz;
    SompRun run{};
    run.ctx = ctx;
    run.grouped = ctx->sweep_group >= 1 && !ctx->streamed;
    run.per_step = run.grouped ? (int)((nsig + ctx->group_wide - 1) / ctx->group_wide) : (int)nsig;
    run.pcap = ctx->prop.multiProcessorCount * 8 + 8;  // (what pipe_nblk allows a pass: solver_alloc's pval / pidx)
    run.npick = (int)std::max<int64_t>(1, std::min<int64_t>((ctx->N + 255) / 256, std::min(256, run.pcap)));
    SompCols& g = run.g;
    g.nsig = (int)nsig;
    g.ldr = s.Mpad;
    g.ldc = (ctx->N + 1) / 2 * 2;
    g.kcap = kcap;
    const void* dB = B;
    auto allocate = [&]() -> int {
        if (b_loc == CSMP_HOST) {
            const size_t bbytes = ((size_t)ldB * (size_t)(nsig - 1) + (size_t)ctx->M) * esz;  // (the last column ends at its last row)
            CHECK(tB.alloc(ctx, bbytes));
            HIPCHECK(hipMemcpy(tB.p, B, bbytes, hipMemcpyHostToDevice));
            dB = tB.p;
        }
        CHECK(tR.alloc(ctx, (size_t)nsig * g.ldr * 8));
        CHECK(tC.alloc(ctx, (size_t)nsig * g.ldc * 8));
        CHECK(tZ.alloc(ctx, (size_t)nsig * kcap * 8));
        CHECK(tSt.alloc(ctx, (size_t)nsig * sizeof(DevState)));
        CHECK(tPv.alloc(ctx, (size_t)kWideMax * run.pcap * 8));
        CHECK(tPi.alloc(ctx, (size_t)kWideMax * run.pcap * 4));
        CHECK(tRun.alloc(ctx, sizeof(int)));
        CHECK(tNnz.alloc(ctx, 8));
        if (host_out) {
            CHECK(tIdx.alloc(ctx, (size_t)k * 8));
            CHECK(tVal.alloc(ctx, (size_t)k * nsig * 8));
            if (order) CHECK(tOrd.alloc(ctx, (size_t)k * 8));
            if (resnorm) CHECK(tRes.alloc(ctx, (size_t)nsig * 8));
        }
        return CSMP_OK;
    };
    CHECK(finish(somp_nomem(ctx, allocate())));
    g.R = (double*)tR.p; g.C = (double*)tC.p; g.Z = (double*)tZ.p; g.st = (DevState*)tSt.p;
    run.ppv = (double*)tPv.p; run.ppi = (int*)tPi.p; run.nrun = (int*)tRun.p;
    int64_t* d_idx = host_out ? (int64_t*)tIdx.p : idx;
    double* d_val = host_out ? (double*)tVal.p : val;
    const int64_t d_ldval = host_out ? k : ldval;  // (a host caller's rows k .. ldval of val are not touched)
    int64_t* d_ord = host_out ? (int64_t*)tOrd.p : order;
    double* d_res = host_out ? (double*)tRes.p : resnorm;

    auto solve = [&]() -> int {
        // the slot: an empty factorisation, the control block reset (k_init through column 0), then a ZERO residual -- the chain
        // serves no column (csmp_somp.hpp)
        CHECK(b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)dB) : init_from_device_t<double>(ctx, (const double*)dB));
        HIPCHECK(hipMemsetAsync(s.r, 0, (size_t)s.Mpad * sizeof(double), ctx->stream));
        HIPCHECK(hipMemsetAsync(run.nrun, 0, sizeof(int), ctx->stream));
        HIPCHECK(hipMemsetAsync(g.Z, 0, (size_t)nsig * kcap * 8, ctx->stream));
        const int iw = (int)(g.ldr / 256);
        const dim3 igrid((unsigned)((int64_t)iw * nsig));
        if (b_dtype == CSMP_F32)
            hipLaunchKernelGGL(k_somp_init<float>, igrid, dim3(256), 0, ctx->stream, (const float*)dB, ldB, (int)ctx->M, g, iw);
        else
            hipLaunchKernelGGL(k_somp_init<double>, igrid, dim3(256), 0, ctx->stream, (const double*)dB, ldB, (int)ctx->M, g, iw);
        HIPCHECK(hipGetLastError());
        for (int64_t t = 0; t < k; ++t) {
            CHECK(run.step(eps, t > 0 ? 1 : 0, p));
            if ((t + 1) % kPollSteps == 0 && t + 1 < k) {
                bool stopped = false;
                CHECK(solver_poll(ctx, &stopped));
                if (stopped) break;
            }
        }
        hipLaunchKernelGGL(k_somp_solve, dim3((unsigned)nsig), dim3(256), 0, ctx->stream, g, (const DevState*)s.st, (const double*)s.R,
                           (const int*)s.sel, (int)ctx->M, d_idx, d_val, d_ldval, (int64_t*)tNnz.p, d_ord, d_res, kc);
        HIPCHECK(hipGetLastError());
        int64_t hn = 0;
        int hrun = 0;
        PinFetch f(ctx);
        CHECK(f.begin(64));
        CHECK(f.add(&hn, tNnz.p, 8));
        CHECK(f.add(&hrun, run.nrun, 4));
        CHECK(f.wait());
        if (host_out) {
            HIPCHECK(hipMemcpyAsync(idx, d_idx, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHECK(hipMemcpy2DAsync(val, (size_t)ldval * 8, d_val, (size_t)k * 8, (size_t)k * 8, (size_t)nsig, hipMemcpyDeviceToHost, ctx->stream));
            if (order) HIPCHECK(hipMemcpyAsync(order, d_ord, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (resnorm) HIPCHECK(hipMemcpyAsync(resnorm, d_res, (size_t)nsig * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        *nnz = hn;
        if (passes) *passes = (int64_t)hrun * run.per_step;
        return CSMP_OK;
    };
    return finish(somp_nomem(ctx, solve()));  // (a support beyond the LDS append kernels' range allocates their spill vectors)
}
