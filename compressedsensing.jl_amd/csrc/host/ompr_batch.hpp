// host/ompr_batch.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_ompr_batch -- csmp_ompr for every column of B, the members of a group taking their update! in lockstep on shared launches.
// ------------------------------------------------------------------------------------------ ompr batch
// An update! of OMP with replacement is one product sweep A'r, two thirds of its time, and five short launches on the member's own
// k x k state (csmp_swap.hpp).  The sweep's read of the dictionary is the same for every signal.  A GROUP of up to R members (R =
// group_wide where the batch has more signals than sweep_group and wide groups are on, else sweep_group) takes its update!s together.
// One TICK of the group is
//     the shared pass (csmp_mp_batch's groups)       c = A'r of every member that runs, c = A'b of every member that starts
//     k_ompr_pick_group                              every running member's arg-max over ITS partials, c on its support, the decision
//     k_swap_dots_group, k_swap_ufin_group,          the exchange of every member whose meta says so (the others leave each kernel at
//     k_swap_commit_res_group, k_swap_rsum_group     once: no host read in between)
//     k_swap_land_group, ONE wait                    every member's landing: sorted x, the shares of |r|^2, info, meta, the control block
// seven launches and one read whatever the number of members; a tick in which no member runs or starts launches nothing.  Every member
// has a small state machine on the host: START (b into the slot, r = b; it joins this tick's pass), ACQUIRE (OmprJob::acquire's exact
// branch on the member's slot behind the pass: the top k, least squares, the explicit inverse, H -- per member, with its own
// synchronisations, once per solve), RUN (one update! a tick: OmprJob::update's fast branch, the refresh every kSwapRefresh accepted
// exchanges, csmp_ompr's stop rule) and FINISH (the results out; the slot takes the next unsolved signal in ascending order in the
// same tick).  Member m lives in solver slot 3 m: its QR, explicit inverse, H, c, x, r, sel, the sorted list and the exchange buffers
// are that slot's, its support and norms an OmprJob of its own (bound to the slot by activating it around every call).  Only the fast
// path runs in groups.  A member whose landing shows a refused exchange, an arg-max inside the support or an acquisition short of k
// atoms LEAVES: its slot is freed and its signal solved from the start by csmp_ompr once the group's ticks have drained
// (CSMP_OMPR_SOLVED_ALONE).  Every member's arithmetic is csmp_ompr's: the pass gives the single sweep's bits per member, the arg-max
// does not depend on how the partials are cut, the group kernels call the single kernels' bodies on the member's own buffers, the
// host steps are OmprJob's: the results are the single calls' bit for bit.  One pipeline, on the context's own stream.
static_assert(kOmprGroupMax == kBpGroupMax, "one bound for the members of a lockstep group");

// The tick's pass over a list of L entries (bp_pass_members' scheme, host/bp_batch.hpp): entry i reads the residual res[i], writes its
// products to out[i] and leaves its arg-max partials and control block in solver slot 3 slots[i].  Up to kGroupMax entries the narrow
// pass's [0, n); more, the wide pass's halves -- launched exactly as mp_group_step launches it (host/mp_batch.hpp).
template <typename TA>
static int omprb_pass(csmp_ctx* ctx, const int* slots, const double* const* res, double* const* out, int L) {
    const bool wide = L > kGroupMax;
    MultiSweep<TA> p;
    p.A = (const TA*)ctx->dA; p.ld = ctx->ld; p.Mv = ctx->Mv; p.N = ctx->N;
    p.eps = 0.0; p.check_eps = 0; p.skipmask = 0; p.KP = ctx->sweep_KP;
    p.nblk = wide ? wide_nblk(ctx) : pipe_nblk(ctx, ctx->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid);
    p.n = wide ? (L + 1) / 2 : L;
    p.n1 = wide ? L / 2 : 0;
    for (int e = 0; e < kWideMax; ++e) {
        const int h = e / kGroupMax, i = e % kGroupMax;
        const int at = h == 0 || !wide ? std::min(i, p.n - 1) : p.n + std::min(i, p.n1 - 1);
        const Solver& s = *slot_ptr(ctx, 3 * slots[at]);
        p.r[e] = res[at]; p.cvec[e] = out[at]; p.pval[e] = s.pval; p.pidx[e] = s.pidx; p.st[e] = s.st;
    }
    const size_t excl = (size_t)(ctx->tune_pair_lds_kib > 0 ? ctx->tune_pair_lds_kib : kPairLdsKiB) * 1024;
    const size_t lds = std::max(sweep_multi_lds_bytes(p.KP, p.n), excl);
    const bool timed = prof_pick(ctx);  // (ONE sampled launch per shared pass, as shared_pass_launch)
    if (timed) CHECK(prof_mark(ctx));
    HIPCHECK(wide ? wide_launch<TA>(ctx, p, lds) : multi_launch<TA>(ctx, p, lds));
    if (timed) CHECK(prof_mark(ctx));
    return CSMP_OK;
}

struct OmprbState {
    enum Phase { FREE, ACQUIRE, RUN } phase = FREE;
    int64_t sig = 0, it = 0;
    double delta = 0.0;
};

struct OmprBatchRun {
    csmp_ctx* ctx;
    const char* dB;  // B on the device
    int b_dtype;
    int64_t ldB, nsig, k, maxiter;
    const double* delta;
    int64_t ndelta;
    int64_t *idx, *nnz, *iters;
    double* val;
    int* flags;
    std::vector<OmprJob> jobs;     // member m's OMPR object
    std::vector<int64_t> alone;    // the signals that left their group

    double delta_of(int64_t sig) const { return delta[ndelta == 1 ? 0 : sig]; }
    // f() with member m's slot active
    template <typename F>
    int on_slot(int m, F&& f) {
        activate_slot(ctx, 3 * m);
        const int rc = f();
        activate_slot(ctx, 0);
        return rc;
    }
    // signal sig into slot m, as OmprJob::begin starts a solve (the slot's buffers stand since the call began)
    int start(int m, int64_t sig, OmprbState& st) {
        const char* col = dB + (size_t)sig * (size_t)ldB * (b_dtype == CSMP_F32 ? 4 : 8);
        OmprJob& j = jobs[(size_t)m];
        CHECK(on_slot(m, [&]() -> int {
            CHECK(j.prepare(ctx, k));
            CHECK(b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)col) : init_from_device_t<double>(ctx, (const double*)col));
            j.reset();
            return CSMP_OK;
        }));
        st = OmprbState();
        st.sig = sig;
        st.delta = delta_of(sig);
        st.phase = OmprbState::ACQUIRE;
        return CSMP_OK;
    }
    // oblivious_acquisition! behind the pass that left c = A'b in the slot: OmprJob::acquire's exact branch from launch_topS on
    int acquire(int m) {
        OmprJob& j = jobs[(size_t)m];
        return on_slot(m, [&]() -> int {
            std::vector<int> top((size_t)k);
            CHECK(launch_topS(ctx, (int)k));
            HIPCHECK(hipMemcpyAsync(top.data(), ctx->s.cands, (size_t)k * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHECK(hipStreamSynchronize(ctx->stream));
            return j.acquire_fit(top);
        });
    }
    void copy_out(int m, const OmprbState& st) {
        const OmprJob& j = jobs[(size_t)m];
        for (size_t t = 0; t < j.xi.size(); ++t) {
            idx[st.sig * k + (int64_t)t] = j.xi[t];
            val[st.sig * k + (int64_t)t] = j.xv[t];
        }
        nnz[st.sig] = (int64_t)j.xi.size();
        if (iters) iters[st.sig] = st.it;
        if (flags) flags[st.sig] = 0;
    }
    // member i of the tick's group: slot 3 m and its exchange buffers (gram_begin_t's layout, held by the member's job)
    void member(OmprGroup& G, int i, int m) {
        const Solver& s = *slot_ptr(ctx, 3 * m);
        const OmprJob& j = jobs[(size_t)m];
        G.pval[i] = s.pval; G.pidx[i] = s.pidx; G.cvec[i] = s.cvec; G.st[i] = s.st;
        G.out_idx[i] = s.out_idx; G.out_val[i] = s.out_val; G.out_nnz[i] = s.out_nnz; G.coef[i] = s.coef; G.sel[i] = s.sel;
        G.x[i] = s.bwd_coef; G.b[i] = s.b; G.r[i] = s.r; G.H[i] = s.swapH; G.ldh[i] = s.kcap;
        G.g[i] = j.dG; G.upart[i] = j.dUpart; G.u[i] = j.dU; G.hp[i] = j.dHp; G.c[i] = j.dC; G.info[i] = j.dInfo; G.rpart[i] = j.dRpart;
        G.n2[i] = j.dN2; G.meta[i] = j.dMeta; G.counter[i] = j.dCounter;
    }

    // all signals on R slots (slot 0 active on entry and on return)
    template <typename TA>
    int run(int R) {
        const int kk = (int)k, M = (int)ctx->M;
        const int nchk = (kk + kSwapChunk - 1) / kSwapChunk, nchm = (kk + kResChunk - 1) / kResChunk, nshare = (M + 255) / 256;
        const int ncommit = (kk * kk + 255) / 256, nrb = (M + 255) / 256;
        const int lwords = swap_land_words(kk, nshare);
        jobs.assign((size_t)R, OmprJob());
        std::vector<OmprbState> st((size_t)R);
        int64_t next = 0, done = 0;
        while (done < nsig) {
            // the pass's entries: the members that run (their residual), then the members that start (b)
            int pslots[kOmprGroupMax], L = 0, runs[kOmprGroupMax], nrun = 0, starts[kOmprGroupMax], nstart = 0;
            const double* pres[kOmprGroupMax];
            double* pout[kOmprGroupMax];
            for (int m = 0; m < R; ++m)
                if (st[(size_t)m].phase == OmprbState::RUN) {
                    runs[nrun] = m;
                    nrun += 1;
                }
            for (int m = 0; m < R && next < nsig; ++m) {
                OmprbState& s = st[(size_t)m];
                if (s.phase != OmprbState::FREE) continue;
                CHECK(start(m, next, s));
                next += 1;
                starts[nstart] = m;
                nstart += 1;
            }
            if (nrun + nstart == 0) break;  // (what is left has left its group)
            for (int i = 0; i < nrun + nstart; ++i) {
                const int m = i < nrun ? runs[i] : starts[i - nrun];
                const Solver& s = *slot_ptr(ctx, 3 * m);
                pslots[L] = m; pres[L] = s.r; pout[L] = s.cvec;
                L += 1;
            }
            CHECK(omprb_pass<TA>(ctx, pslots, pres, pout, L));
            std::vector<unsigned long long> land;  // (the host's copy: a refresh below lands in the same page-locked slot)
            if (nrun > 0) {
                OmprGroup G{};
                G.n = nrun;
                G.k = kk;
                // (the partials per member: one per column stream of the pass this tick took)
                G.nblk = L > kGroupMax ? wide_nblk(ctx) / 2 : pipe_nblk(ctx, ctx->dtype == CSMP_F32 ? kGroupTickGrid : kPairTickGrid);
                for (int i = 0; i < kOmprGroupMax; ++i) member(G, i, runs[std::min(i, nrun - 1)]);
                const unsigned un = (unsigned)nrun;
                void* pv = nullptr;
                CHECK(pin_get(ctx, 1, (size_t)nrun * lwords * 8 + 64, &pv));
                hipLaunchKernelGGL(k_ompr_pick_group, dim3(1, 1, un), dim3(256), 0, ctx->stream, G);
                hipLaunchKernelGGL(k_swap_dots_group<TA>, dim3((unsigned)((kk + 2 + 3) / 4), 1, un), dim3(256), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld, M, G);
                hipLaunchKernelGGL(k_swap_ufin_group, dim3((unsigned)nchk, 1, un), dim3(256), (size_t)kk * sizeof(int), ctx->stream, G, nchk,
                                   ctx->tune_swap_refuse ? 2.0 : 1e-6);
                hipLaunchKernelGGL(k_swap_commit_res_group<TA>, dim3((unsigned)(ncommit + nrb * nchm), 1, un), dim3(256), 0, ctx->stream, (const TA*)ctx->dA,
                                   ctx->ld, M, G, ncommit, nrb);
                hipLaunchKernelGGL(k_swap_rsum_group, dim3((unsigned)nshare, 1, un), dim3(256), 0, ctx->stream, G, nchm, M);
                hipLaunchKernelGGL(k_swap_land_group, dim3((unsigned)std::max(1, std::min(64, (lwords + 255) / 256)), 1, un), dim3(256), 0, ctx->stream, G,
                                   nshare, lwords, (unsigned long long*)pv);
                HIPCHECK(hipGetLastError());
                HIPCHECK(hipStreamSynchronize(ctx->stream));  // the ONE read of the tick
                land.assign((const unsigned long long*)pv, (const unsigned long long*)pv + (size_t)nrun * lwords);
            }
            // every running member's landing: OmprJob::update's fast branch, the refresh, csmp_ompr's stop rule
            for (int i = 0; i < nrun; ++i) {
                const int m = runs[i];
                OmprbState& s = st[(size_t)m];
                OmprJob& j = jobs[(size_t)m];
                const unsigned long long* w = land.data() + (size_t)i * lwords;
                OmprJob::SwapLanding Ld;
                Ld.hi.resize((size_t)kk);
                Ld.hv.resize((size_t)kk);
                Ld.n2.resize((size_t)nshare);
                memcpy(Ld.hi.data(), w, (size_t)kk * 8);
                memcpy(Ld.hv.data(), w + kk, (size_t)kk * 8);
                memcpy(Ld.n2.data(), w + 2 * kk, (size_t)nshare * 8);
                memcpy(Ld.info, w + 2 * kk + nshare, 32);
                memcpy(Ld.meta, w + 2 * kk + nshare + 4, 16);
                // (the control block behind them -- the arg-max and its value -- serves a reader of the landing; the decision is in meta)
                const double oldnorm = j.resnorm;
                if (Ld.meta[0] == 2 || (Ld.meta[0] == 1 && Ld.info[2] != 0.0)) {
                    // off the fast path (the arg-max inside the support: the host's scan; a refused exchange: the QR path): alone, later
                    alone.push_back(s.sig);
                    s.phase = OmprbState::FREE;
                    done += 1;
                    continue;
                }
                if (Ld.meta[0] == 1) {
                    j.gram_accept(Ld);
                    CHECK(on_slot(m, [&]() -> int { return j.gram_refresh_if_due(); }));
                }
                s.it += 1;
                if (j.resnorm <= s.delta || oldnorm <= j.resnorm || s.it == maxiter) {
                    copy_out(m, s);
                    s.phase = OmprbState::FREE;
                    done += 1;
                }
            }
            // the members that started: their acquisition behind the pass
            for (int i = 0; i < nstart; ++i) {
                const int m = starts[i];
                OmprbState& s = st[(size_t)m];
                OmprJob& j = jobs[(size_t)m];
                CHECK(acquire(m));
                if ((int64_t)j.xi.size() != k || !j.gram) {  // (a support short of k atoms: the QR path's)
                    alone.push_back(s.sig);
                    s.phase = OmprbState::FREE;
                    done += 1;
                } else if (maxiter == 0) {
                    copy_out(m, s);
                    s.phase = OmprbState::FREE;
                    done += 1;
                } else {
                    s.phase = OmprbState::RUN;
                }
            }
        }
        return CSMP_OK;
    }
};

// a failed device allocation (dmalloc's report) is the call's CSMP_ENOMEM, any other failure of the runtime stays what it is
static int omprb_nomem(csmp_ctx* ctx, int rc) {
    if (rc == CSMP_EHIP && ctx->err.find("hipMalloc") != std::string::npos)
        return fail(ctx, CSMP_ENOMEM, "ompr_batch: no device memory for the members' buffers, per member the factorisation, its inverse and H (" + ctx->err + ")");
    return rc;
}

extern "C" int csmp_ompr_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, int64_t k, const double* delta,
                               int64_t ndelta, int64_t maxiter, int64_t* idx, double* val, int64_t* nnz, int64_t* iters, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    if (nsig < 0) return fail(ctx, CSMP_EINVAL, "ompr_batch: nsig has to be non-negative");
    if (k < 1) return fail(ctx, CSMP_EINVAL, "ompr_batch: k < 1");
    if (!delta || (nsig > 0 && (!B || !idx || !val || !nnz))) return fail(ctx, CSMP_EINVAL, "ompr_batch: bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "ompr_batch: b_dtype must be CSMP_F32 or CSMP_F64");
    if (b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) return fail(ctx, CSMP_EINVAL, "ompr_batch: b_loc must be CSMP_HOST or CSMP_DEVICE");
    if (ndelta != 1 && ndelta != nsig) return fail(ctx, CSMP_EINVAL, "ompr_batch: ndelta has to be 1 or nsig");
    for (int64_t s = 0; s < ndelta; ++s)
        if (delta[s] != delta[s]) return fail(ctx, CSMP_EINVAL, "ompr_batch: delta is NaN");
    if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "ompr_batch: no dictionary set (csmp_set_dictionary)");
    if (ldB < ctx->M) return fail(ctx, CSMP_EDIM, "ompr_batch: ldB < size(A, 1)");
    if (k > ctx->N || k > ctx->M) return fail(ctx, CSMP_ERANGE, "ompr_batch: k exceeds size(A)");
    if (nsig == 0) return CSMP_OK;
    if (maxiter < 0) maxiter = ctx->M;
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    const size_t esz = b_dtype == CSMP_F32 ? 4 : 8;
    const size_t cbytes = (size_t)ctx->M * esz;
    const size_t bbytes = (size_t)ldB * (size_t)(nsig - 1) * esz + cbytes;  // (the last column ends at its last row)
    auto finish = [&](int rc) -> int {
        activate_slot(ctx, 0);
        (void)hipStreamSynchronize(ctx->stream);  // (on every way out: the temporaries and the caller's buffers are at rest)
        return rc;
    };
    // signal s by the single call (b where csmp_ompr wants it: on the host)
    std::vector<char> hcol;
    auto solve_alone = [&](const char* hB, const char* dB, int64_t s, int flag) -> int {
        const void* b = hB ? hB + (size_t)s * (size_t)ldB * esz : nullptr;
        if (!b) {
            hcol.resize(cbytes);
            HIPCHECK(hipMemcpy(hcol.data(), dB + (size_t)s * (size_t)ldB * esz, cbytes, hipMemcpyDeviceToHost));
            b = hcol.data();
        }
        const int rc = csmp_ompr(ctx, b, b_dtype, k, delta[ndelta == 1 ? 0 : s], maxiter, idx + s * k, val + s * k, nnz + s, iters ? iters + s : nullptr);
        if (rc != CSMP_OK) ctx->err = "ompr_batch: " + ctx->err + " (signal " + std::to_string(s) + ")";
        else if (flags) flags[s] = flag;
        return rc;
    };
    // The shared pass where the resident dictionary has one and the sweeps are exact, on the inverse Gram matrix's range of k; a lone
    // signal keeps csmp_ompr's launches.
    const bool grouped = ctx->pipeline && ctx->sweep_group >= 1 && !screened_on(ctx) && !ctx->streamed && nsig >= 2 && k <= kTMaxCols;
    if (!grouped) {
        const char* hB = b_loc == CSMP_HOST ? (const char*)B : nullptr;
        int rc = CSMP_OK;
        for (int64_t s = 0; s < nsig && rc == CSMP_OK; ++s) rc = solve_alone(hB, (const char*)B, s, 0);
        return finish(rc);
    }
    OmprBatchRun run{};
    run.ctx = ctx; run.dB = (const char*)B; run.b_dtype = b_dtype; run.ldB = ldB; run.nsig = nsig; run.k = k; run.maxiter = maxiter;
    run.delta = delta; run.ndelta = ndelta; run.idx = idx; run.val = val; run.nnz = nnz; run.iters = iters; run.flags = flags;
    // a slot ready for a member: what OmprJob::begin makes, and the exchange buffers
    auto ensure = [&](csmp_ctx* c) -> int {
        OmprJob j;
        CHECK(j.prepare(c, k));
        return j.gram_ensure();
    };
    CHECK(omprb_nomem(ctx, ensure(ctx)));
    DevTmp tB;  // a host caller's B on the device
    if (b_loc == CSMP_HOST) {
        CHECK(omprb_nomem(ctx, tB.alloc(ctx, bbytes)));
        HIPCHECK(hipMemcpy(tB.p, B, bbytes, hipMemcpyHostToDevice));
        run.dB = (const char*)tB.p;
    }
    const int wide_members = ctx->group_wide > ctx->sweep_group && nsig > ctx->sweep_group && !ctx->wide_refused ? ctx->group_wide : 0;
    int ticks_rc = CSMP_OK;  // (the ticks' own status)
    auto enqueue = [&](csmp_ctx*, bool granted) -> int {
        const int R = (int)std::min<int64_t>(granted ? wide_members : ctx->sweep_group, nsig);
        ticks_rc = ctx->dtype == CSMP_F32 ? run.run<float>(R) : run.run<double>(R);
        return CSMP_OK;
    };
    int rc = omprb_nomem(ctx, batch_pipelines(ctx, false, ctx->sweep_group, wide_members, 3, ensure, enqueue));
    if (rc == CSMP_OK) rc = omprb_nomem(ctx, ticks_rc);  // (a member's first acquisition allocates the least-squares panels of its slot)
    if (rc == CSMP_OK && !run.alone.empty()) {
        // the signals that left their groups, from the start, by the single call on slot 0
        activate_slot(ctx, 0);
        HIPCHECK(hipStreamSynchronize(ctx->stream));
        std::sort(run.alone.begin(), run.alone.end());
        const char* hB = b_loc == CSMP_HOST ? (const char*)B : nullptr;
        for (size_t q = 0; q < run.alone.size() && rc == CSMP_OK; ++q) rc = solve_alone(hB, run.dB, run.alone[q], CSMP_OMPR_SOLVED_ALONE);
    }
    return finish(rc);
}
