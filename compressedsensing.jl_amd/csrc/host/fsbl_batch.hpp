// host/fsbl_batch.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// csmp_fsbl_batch / csmp_rmps_batch -- csmp_fsbl / csmp_rmps for every column of B, the members of a group in lockstep on shared launches.
// ------------------------------------------------------------------------------------------ fsbl batch
// A greedy step reads the whole dictionary once, for w = A'v, and that read is the same for every signal.  A GROUP of up to R members
// (R = group_wide where the batch has more signals than sweep_group and wide groups are on, else sweep_group) takes its steps
// together.  One TICK of the group is
//     k_fsbl_score_group, k_fsbl_pick_group          the N-pass (with the pending S / Q update) and the decision of every member
//     k_fsbl_col_group, k_fsbl_gemv_group,           a_i, v = C^-1 a_i and C^-1 -= v v' / den of every member whose device record holds an
//     k_fsbl_rank1_group                             action (the others leave at once: no host read in between)
//     ONE PinFetch of the group's decision records   (R x 64 bytes; skipped where no member waits for a decision)
//     the shared pass (csmp_mp_batch's groups)       w = A'v of the members that acted, and Q = A'b of the members that start
// five launches, one read and one pass whatever the number of members; a tick in which nobody acts or starts launches no pass.
// Every member has a small state machine on the host (FsblbState): START (C^-1 = I / sigma2, alpha, the record; it joins the tick's
// pass with b as its residual and Q as the output, then k_fsbl_scale), REPLAY (the warm start: one forced record a tick), RUN (csmp_fsbl's
// loop, or csmp_rmps's stages, one turn a tick) and FINISH (the pending update in the next tick's N-pass, k_fsbl_x, the copies); a
// freed slot takes the next unsolved signal in ascending order, in the same tick.  Member m lives in solver slot 3 m (b and the pass's
// partials and control block) and in its share of FsblBatchBuf.  Every member's arithmetic is csmp_fsbl's: the pass gives the single
// sweep's bits per member, the group kernels call the single kernels' bodies on the member's own buffers, the squared column norms
// are k_fr_colnorm2's (taken once per call instead of once per solve), a member starts as fsbl_begin does: the results are the single
// calls' bit for bit.  One pipeline, on the context's own stream; csmp_fsbl's FsblBuf is left alone.
static int fsblb_ensure(csmp_ctx* ctx, int R) {
    FsblBatchBuf& t = ctx->fsblb;
    if (t.Ci && t.R >= R && t.M == (int)ctx->M && t.N == ctx->N) return CSMP_OK;
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    fsblb_free(t);
    FsblBatchBuf n;
    const size_t M = (size_t)ctx->M, N = (size_t)ctx->N, Rr = (size_t)R;
    n.Mp = (int)((M + 255) / 256 * 256);
    n.ldc = (int64_t)((M + 1) / 2 * 2);
    auto all = [&]() -> int {
        CHECK(dmalloc(ctx, &n.Ci, (size_t)n.ldc * M * Rr));
        CHECK(dmalloc(ctx, &n.vec, (size_t)2 * n.Mp * Rr));
        CHECK(dmalloc(ctx, &n.alpha, N * Rr));
        CHECK(dmalloc(ctx, &n.S, N * Rr));
        CHECK(dmalloc(ctx, &n.Q, N * Rr));
        CHECK(dmalloc(ctx, &n.w, N * Rr));
        CHECK(dmalloc(ctx, &n.x, N * Rr));
        CHECK(dmalloc(ctx, &n.pval, (size_t)kFsblParts * Rr));
        CHECK(dmalloc(ctx, &n.pidx, (size_t)kFsblParts * Rr));
        CHECK(dmalloc(ctx, &n.rec, Rr));
        CHECK(dmalloc(ctx, &n.norms, N));
        // (the pass reads v up to whole vectors, k_fsbl_rank1_group up to ldc: zeros beyond M, which no kernel writes)
        HIPCHECK(hipMemsetAsync(n.vec, 0, (size_t)2 * n.Mp * Rr * sizeof(double), ctx->stream));
        HIPCHECK(hipMemsetAsync(n.rec, 0, Rr * sizeof(FsblRec), ctx->stream));
        return CSMP_OK;
    };
    const int rc = all();
    if (rc != CSMP_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        fsblb_free(n);
        return rc;
    }
    n.R = R;
    n.M = (int)ctx->M;
    n.N = ctx->N;
    t = n;
    return CSMP_OK;
}

// member m's pointers
struct FsblbMember {
    double *Ci, *col, *v, *alpha, *S, *Q, *w, *x, *pval;
    long long* pidx;
    FsblRec* rec;
};
static FsblbMember fsblb_member(const csmp_ctx* ctx, int m) {
    const FsblBatchBuf& t = ctx->fsblb;
    const size_t N = (size_t)t.N, mm = (size_t)m;
    FsblbMember r;
    r.Ci = t.Ci + (size_t)t.ldc * (size_t)t.M * mm;
    r.col = t.vec + (size_t)2 * t.Mp * mm;
    r.v = r.col + t.Mp;
    r.alpha = t.alpha + N * mm;
    r.S = t.S + N * mm;
    r.Q = t.Q + N * mm;
    r.w = t.w + N * mm;
    r.x = t.x + N * mm;
    r.pval = t.pval + (size_t)kFsblParts * mm;
    r.pidx = t.pidx + (size_t)kFsblParts * mm;
    r.rec = t.rec + mm;
    return r;
}

// bp_pass_members' scheme (host/bp_batch.hpp) over a list of L entries: entry i reads the residual res[i], writes its products to
// out[i] and borrows the partials and the control block of solver slot 3 slots[i].  Up to kGroupMax entries the narrow pass's [0, n);
// more, the wide pass's halves.
template <typename TA>
static int fsblb_pass(csmp_ctx* ctx, const int* slots, const double* const* res, double* const* out, int L) {
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
    HIPCHECK(wide ? wide_launch<TA>(ctx, p, lds) : multi_launch<TA>(ctx, p, lds));
    return CSMP_OK;
}

// a member's state machine
struct FsblbState {
    enum Phase { FREE, REPLAY, RUN, FINISH } phase = FREE;
    enum Stage { ACQ, DEL, UPD } stage = ACQ;  // csmp_rmps's stages
    int64_t sig = 0;
    double sigma2 = 0.0;
    std::vector<double> ha, old;   // the host's copy of alpha, and what it was at the last "unchanged" test (csmp_rmps)
    std::vector<int64_t> replay;   // the finite entries of the warm start, in index order
    size_t rp = 0;
    int64_t it = 1, k = 0, iters = 0, applied = 0;
    bool conv = false;
};

// The arguments of one call and the group's ticks
struct FsblBatchRun {
    csmp_ctx* ctx;
    bool rmps;
    const char* who;
    const char* dB;  // B on the device
    int b_dtype;
    int64_t ldB, nsig;
    const double* sigma2;
    int64_t nsigma2, maxiter, max_acq, max_del;
    double min_increase;
    const double* alpha_in;  // where x_loc says, or NULL
    int64_t ld_ain;
    const double* ha_in;     // the host's dense copy of alpha_in (leading dimension N), or NULL
    double* X;
    int64_t ldX;
    double* alpha_out;
    int64_t ld_aout;
    int x_loc;
    int64_t *history, history_cap, *iterations;
    int* flags;

    hipMemcpyKind out_kind() const { return x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost; }
    hipMemcpyKind in_kind() const { return x_loc == CSMP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }
    double sigma2_of(int64_t sig) const { return sigma2[nsigma2 == 1 ? 0 : sig]; }
    int bad_value(int64_t sig) const {
        return fail(ctx, CSMP_EINVAL, std::string(who) + ": a value of the marginal likelihood's change is not finite (signal " + std::to_string(sig) + ")");
    }

    // signal sig into slot m, as fsbl_begin starts a solve; the member joins this tick's pass with b, and k_fsbl_scale follows the pass
    int start(int m, int64_t sig, FsblbState& st) {
        const FsblbMember b = fsblb_member(ctx, m);
        const FsblBatchBuf& t = ctx->fsblb;
        const int64_t N = ctx->N;
        const int M = (int)ctx->M;
        const char* col = dB + (size_t)sig * (size_t)ldB * (b_dtype == CSMP_F32 ? 4 : 8);
        activate_slot(ctx, 3 * m);
        ctx->s.begun = false;
        const int rc = b_dtype == CSMP_F32 ? init_from_device_t<float>(ctx, (const float*)col) : init_from_device_t<double>(ctx, (const double*)col);
        activate_slot(ctx, 0);
        CHECK(rc);
        st = FsblbState();
        st.sig = sig;
        st.sigma2 = sigma2_of(sig);
        HIPCHECK(hipMemsetAsync(b.rec, 0, sizeof(FsblRec), ctx->stream));
        hipLaunchKernelGGL(k_fsbl_eye, dim3((unsigned)((t.ldc * M + 255) / 256)), dim3(256), 0, ctx->stream, b.Ci, t.ldc, M, st.sigma2);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(b.S, t.norms, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        if (alpha_in) {
            HIPCHECK(hipMemcpyAsync(b.alpha, alpha_in + sig * ld_ain, (size_t)N * sizeof(double), in_kind(), ctx->stream));
            const double* h = ha_in + (size_t)sig * (size_t)N;
            st.ha.assign(h, h + N);
            for (int64_t j = 0; j < N; ++j)
                if (std::isfinite(h[j])) st.replay.push_back(j);
        } else {
            hipLaunchKernelGGL(k_fsbl_fill, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, b.alpha, N, HUGE_VAL);
            HIPCHECK(hipGetLastError());
            st.ha.assign((size_t)N, HUGE_VAL);
        }
        if (rmps) st.old = st.ha;
        st.phase = st.replay.empty() ? FsblbState::RUN : FsblbState::REPLAY;
        return CSMP_OK;
    }
    int mode_of(const FsblbState& st) const {
        if (st.phase != FsblbState::RUN) return FSBL_MODE_NONE;
        if (!rmps) return FSBL_MODE_ALL;
        return st.stage == FsblbState::ACQ ? FSBL_MODE_ADD : st.stage == FsblbState::DEL ? FSBL_MODE_RMP_DEL : FSBL_MODE_UPD;
    }
    // the record of a RUN member's turn: fsbl_turn's bookkeeping, then csmp_fsbl's loop or csmp_rmps's stages, one turn on
    void took_turn(FsblbState& st, const FsblRec& r) const {
        if (r.action != FSBL_ACT_NONE) {
            st.ha[(size_t)r.i] = r.alpha_new;
            int64_t* h = history ? history + 2 * history_cap * st.sig : nullptr;
            if (h && st.applied < history_cap) {
                h[2 * st.applied] = r.action;
                h[2 * st.applied + 1] = r.i;
            }
            st.applied += 1;
        }
        auto finish = [&](bool conv) {
            st.conv = conv;
            st.phase = FsblbState::FINISH;
        };
        if (!rmps) {
            st.iters = st.it;
            if (r.value < min_increase) finish(true);  // maximum(delta) < min_increase, after the pass
            else if (st.it == maxiter) finish(false);
            else st.it += 1;
            return;
        }
        // (old != alpha as arrays of doubles: +inf equals +inf, and no entry is ever NaN)
        auto end_stage = [&](bool deletion) {
            if (st.old == st.ha) return finish(true);
            st.old = st.ha;
            st.k = 0;
            if (!deletion) {
                st.stage = FsblbState::DEL;
                return;
            }
            if (st.it == maxiter) return finish(false);
            st.it += 1;
            st.stage = FsblbState::ACQ;
        };
        if (st.stage == FsblbState::ACQ) {  // acquisition stage
            st.k += 1;
            if (r.action == FSBL_ACT_NONE || st.k == max_acq) end_stage(false);
        } else if (st.stage == FsblbState::DEL) {  // deletion and update stage: a deletion, else the update's turn
            if (r.action != FSBL_ACT_NONE) {
                st.k += 1;
                if (st.k == max_del) end_stage(true);
            } else {
                st.stage = FsblbState::UPD;
            }
        } else {
            const double gain = r.action != FSBL_ACT_NONE ? r.value : 0.0;
            st.k += 1;
            if (gain < min_increase || st.k == max_del) end_stage(true);
            else st.stage = FsblbState::DEL;
        }
    }
    // a finished member's results: x = Q / alpha on the active atoms (the pending update went with this tick's N-pass), the copies
    int retire(int m, const FsblbState& st) const {
        const FsblbMember b = fsblb_member(ctx, m);
        const int64_t N = ctx->N;
        hipLaunchKernelGGL(k_fsbl_x, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)b.alpha, (const double*)b.Q, N, b.x);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(X + st.sig * ldX, b.x, (size_t)N * sizeof(double), out_kind(), ctx->stream));
        if (alpha_out) HIPCHECK(hipMemcpyAsync(alpha_out + st.sig * ld_aout, b.alpha, (size_t)N * sizeof(double), out_kind(), ctx->stream));
        if (iterations) iterations[st.sig] = rmps ? st.applied : st.iters;
        if (flags) flags[st.sig] = st.conv ? CSMP_FSBL_CONVERGED : 0;
        return CSMP_OK;
    }

    // all signals on R slots (slot 0 active on entry and on return)
    template <typename TA>
    int run(int R) {
        const FsblBatchBuf& t = ctx->fsblb;
        const int64_t N = ctx->N;
        const int M = (int)ctx->M;
        const int np = fsbl_nparts(N);
        const bool vec = fsbl_vec(ctx);
        constexpr int PERV = 16 / (int)sizeof(TA);
        // |a_j|^2, the same for every signal: one read of A per call
        hipLaunchKernelGGL(k_fr_colnorm2<TA>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld, M, N, t.norms);
        HIPCHECK(hipGetLastError());
        std::vector<FsblbState> st((size_t)R);
        int64_t next = 0, done = 0;
        while (done < nsig) {
            // the members that take part in the N-pass: REPLAY and RUN take a turn, FINISH the pending update alone
            FsblGroup G{};
            int slots[kBpGroupMax], n = 0, turns = 0;
            bool decide = false;
            for (int m = 0; m < R; ++m) {
                const FsblbState& s = st[(size_t)m];
                if (s.phase == FsblbState::FREE) continue;
                slots[n] = m;
                n += 1;
            }
            for (int i = 0; i < kBpGroupMax && n > 0; ++i) {
                const int m = slots[std::min(i, n - 1)];
                const FsblbState& s = st[(size_t)m];
                const FsblbMember b = fsblb_member(ctx, m);
                G.mode[i] = mode_of(s);
                G.turn[i] = s.phase != FsblbState::FINISH;
                G.force_i[i] = -1;
                G.force_gamma[i] = 0.0;
                if (s.phase == FsblbState::REPLAY) {
                    G.force_i[i] = s.replay[s.rp];
                    G.force_gamma[i] = 1.0 / s.ha[(size_t)s.replay[s.rp]];
                }
                G.alpha[i] = b.alpha; G.S[i] = b.S; G.Q[i] = b.Q; G.w[i] = b.w; G.pval[i] = b.pval; G.pidx[i] = b.pidx; G.rec[i] = b.rec;
                G.Ci[i] = b.Ci; G.col[i] = b.col; G.v[i] = b.v;
                if (i < n) {
                    turns += G.turn[i];
                    decide = decide || s.phase == FsblbState::RUN;
                }
            }
            G.n = n;
            if (n > 0) {
                const unsigned un = (unsigned)n;
                hipLaunchKernelGGL(k_fsbl_score_group, dim3(np, 1, un), dim3(256), 0, ctx->stream, G, N, fsbl_per(N));
                HIPCHECK(hipGetLastError());
                if (turns > 0) {
                    hipLaunchKernelGGL(k_fsbl_pick_group, dim3(1, 1, un), dim3(256), 0, ctx->stream, G, np);
                    const dim3 gc((unsigned)((M + 256 * PERV - 1) / (256 * PERV)), 1, un);
                    if (vec) hipLaunchKernelGGL((k_fsbl_col_group<TA, true>), gc, dim3(256), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld, M, G);
                    else hipLaunchKernelGGL((k_fsbl_col_group<TA, false>), gc, dim3(256), 0, ctx->stream, (const TA*)ctx->dA, ctx->ld, M, G);
                    hipLaunchKernelGGL(k_fsbl_gemv_group, dim3((unsigned)((M + 3) / 4), 1, un), dim3(256), 0, ctx->stream, t.ldc, M, G);
                    hipLaunchKernelGGL(k_fsbl_rank1_group, dim3((unsigned)M, (unsigned)((t.ldc + 511) / 512), un), dim3(256), 0, ctx->stream, t.ldc, G);
                    HIPCHECK(hipGetLastError());
                }
            }
            // the ONE read of the tick: every member's decision record
            FsblRec recs[kBpGroupMax];
            if (decide) {
                PinFetch f(ctx);
                CHECK(f.begin(sizeof recs + 16));
                CHECK(f.add(recs, t.rec, (size_t)R * sizeof(FsblRec)));
                CHECK(f.wait());
            }
            // the pass's entries: the members that acted, then the members that start
            int pslots[kBpGroupMax], L = 0, starts[kBpGroupMax], nstart = 0;
            const double* pres[kBpGroupMax];
            double* pout[kBpGroupMax];
            for (int i = 0; i < n; ++i) {
                const int m = slots[i];
                FsblbState& s = st[(size_t)m];
                const FsblbMember b = fsblb_member(ctx, m);
                bool acted = false;
                if (s.phase == FsblbState::FINISH) {
                    CHECK(retire(m, s));
                    s.phase = FsblbState::FREE;
                    done += 1;
                } else if (s.phase == FsblbState::REPLAY) {
                    acted = true;
                    s.rp += 1;
                    if (s.rp == s.replay.size()) s.phase = FsblbState::RUN;
                } else {
                    const FsblRec& r = recs[m];
                    if (r.bad) return bad_value(s.sig);
                    acted = r.action != FSBL_ACT_NONE;
                    took_turn(s, r);
                }
                if (acted) {
                    pslots[L] = m; pres[L] = b.v; pout[L] = b.w;
                    L += 1;
                }
            }
            for (int m = 0; m < R && next < nsig; ++m) {
                FsblbState& s = st[(size_t)m];
                if (s.phase != FsblbState::FREE) continue;
                CHECK(start(m, next, s));
                next += 1;
                pslots[L] = m; pres[L] = slot_ptr(ctx, 3 * m)->r; pout[L] = fsblb_member(ctx, m).Q;
                L += 1;
                starts[nstart] = m;
                nstart += 1;
            }
            if (L > 0) CHECK(fsblb_pass<TA>(ctx, pslots, pres, pout, L));
            for (int i = 0; i < nstart; ++i) {
                const FsblbMember b = fsblb_member(ctx, starts[i]);
                hipLaunchKernelGGL(k_fsbl_scale, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, b.S, b.Q, N, st[(size_t)starts[i]].sigma2);
                HIPCHECK(hipGetLastError());
            }
        }
        return CSMP_OK;
    }
};

static int fsblb_nomem(csmp_ctx* ctx, const char* who, int rc) {
    if (rc == CSMP_EHIP)
        return fail(ctx, CSMP_ENOMEM, std::string(who) + ": no device memory for the members' buffers, R x size(A,1)^2 doubles and the vectors (" + ctx->err + ")");
    return rc;
}

// the body of both entries (rmps: csmp_rmps_batch, whose two further caps csmp_fsbl_batch does not have)
static int fsbl_batch_impl(csmp_ctx* ctx, const char* who, bool rmps, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc,
                           const double* sigma2, int64_t nsigma2, int64_t maxiter, int64_t max_acq, int64_t max_del, double min_increase,
                           const double* alpha_in, int64_t ld_ain, double* X, int64_t ldX, double* alpha_out, int64_t ld_aout, int x_loc,
                           int64_t* history, int64_t history_cap, int64_t* iterations, int* flags) {
    const std::string w(who);
    if (nsig < 0) return fail(ctx, CSMP_EINVAL, w + ": nsig has to be non-negative");
    if (!sigma2 || (nsig > 0 && (!B || !X))) return fail(ctx, CSMP_EINVAL, w + ": bad arguments");
    if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
    if ((b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) || (x_loc != CSMP_HOST && x_loc != CSMP_DEVICE))
        return fail(ctx, CSMP_EINVAL, w + ": b_loc / x_loc must be CSMP_HOST or CSMP_DEVICE");
    if (nsigma2 != 1 && nsigma2 != nsig) return fail(ctx, CSMP_EINVAL, w + ": nsigma2 has to be 1 or nsig");
    for (int64_t s = 0; s < nsigma2; ++s)
        if (!std::isfinite(sigma2[s]) || !(sigma2[s] > 0.0)) return fail(ctx, CSMP_EINVAL, w + ": sigma2 has to be positive and finite");
    if (!(min_increase >= 0.0)) return fail(ctx, CSMP_EINVAL, w + ": min_increase has to be non-negative");
    if (maxiter < 1 || (rmps && (max_acq < 1 || max_del < 1)))
        return fail(ctx, CSMP_EINVAL, rmps ? w + ": maxiter, maxiter_acquisition and maxiter_deletion have to be at least 1" : w + ": maxiter has to be at least 1");
    if (history_cap < 0) return fail(ctx, CSMP_EINVAL, w + ": history_cap has to be non-negative");
    CHECK(fsbl_entry(ctx, who));
    if (ldB < ctx->M) return fail(ctx, CSMP_EDIM, w + ": ldB < size(A, 1)");
    if (ldX < ctx->N) return fail(ctx, CSMP_EDIM, w + ": ldX < size(A, 2)");
    if (alpha_in && ld_ain < ctx->N) return fail(ctx, CSMP_EDIM, w + ": ld_alpha_in < size(A, 2)");
    if (alpha_out && ld_aout < ctx->N) return fail(ctx, CSMP_EDIM, w + ": ld_alpha_out < size(A, 2)");
    if (nsig == 0) return CSMP_OK;
    HIPCHECK(hipSetDevice(ctx->dev));
    activate_slot(ctx, 0);
    const int64_t N = ctx->N;
    std::vector<double> ha;  // every signal's warm start on the host, checked before any device work
    if (alpha_in) {
        ha.resize((size_t)N * (size_t)nsig);
        if (x_loc == CSMP_HOST) {
            for (int64_t s = 0; s < nsig; ++s) memcpy(ha.data() + (size_t)s * N, alpha_in + s * ld_ain, (size_t)N * sizeof(double));
        } else {
            HIPCHECK(hipMemcpy2DAsync(ha.data(), (size_t)N * sizeof(double), alpha_in, (size_t)ld_ain * sizeof(double), (size_t)N * sizeof(double),
                                      (size_t)nsig, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHECK(hipStreamSynchronize(ctx->stream));
        }
        for (double a : ha)
            if (!(a > 0.0)) return fail(ctx, CSMP_EINVAL, w + ": every entry of alpha has to be positive, or +inf for an inactive atom");
    }
    const size_t esz = b_dtype == CSMP_F32 ? 4 : 8;
    const size_t bbytes = (size_t)ldB * (size_t)(nsig - 1) * esz + (size_t)ctx->M * esz;  // (the last column ends at its last row)
    auto finish = [&](int rc) -> int {
        activate_slot(ctx, 0);
        (void)hipStreamSynchronize(ctx->stream);  // (on every way out: the temporaries and the caller's buffers are at rest)
        return rc;
    };
    // The shared pass where the resident dictionary has one and the sweeps are exact; a lone signal keeps csmp_fsbl's launches.
    const bool grouped = ctx->pipeline && ctx->sweep_group >= 1 && !screened_on(ctx) && nsig >= 2;
    if (!grouped) {
        // the loop over the single calls, B brought to where x lives (the single calls take one location for b, x and alpha)
        DevTmp tB;
        std::vector<char> hB;
        const char* Bx = (const char*)B;
        if (b_loc == CSMP_HOST && x_loc == CSMP_DEVICE) {
            CHECK(fsblb_nomem(ctx, who, tB.alloc(ctx, bbytes)));
            HIPCHECK(hipMemcpy(tB.p, B, bbytes, hipMemcpyHostToDevice));
            Bx = (const char*)tB.p;
        } else if (b_loc == CSMP_DEVICE && x_loc == CSMP_HOST) {
            hB.resize(bbytes);
            HIPCHECK(hipMemcpy(hB.data(), B, bbytes, hipMemcpyDeviceToHost));
            Bx = hB.data();
        }
        int rc = CSMP_OK;
        for (int64_t s = 0; s < nsig && rc == CSMP_OK; ++s) {
            const void* b = Bx + (size_t)s * (size_t)ldB * esz;
            const double s2 = sigma2[nsigma2 == 1 ? 0 : s];
            const double* ai = alpha_in ? alpha_in + s * ld_ain : nullptr;
            double* ao = alpha_out ? alpha_out + s * ld_aout : nullptr;
            int64_t* h = history ? history + 2 * history_cap * s : nullptr;
            int64_t* it = iterations ? iterations + s : nullptr;
            int* fl = flags ? flags + s : nullptr;
            rc = rmps ? csmp_rmps(ctx, b, b_dtype, s2, maxiter, max_acq, max_del, min_increase, ai, X + s * ldX, ao, x_loc, h, history_cap, it, fl)
                      : csmp_fsbl(ctx, b, b_dtype, s2, maxiter, min_increase, ai, X + s * ldX, ao, x_loc, h, history_cap, it, fl);
            if (rc == CSMP_EINVAL) ctx->err += " (signal " + std::to_string(s) + ")";
        }
        return finish(rc);
    }
    CHECK(fsblb_nomem(ctx, who, solver_ensure(ctx, 1, 1, false)));
    FsblBatchRun run{};
    run.ctx = ctx; run.rmps = rmps; run.who = who; run.dB = (const char*)B; run.b_dtype = b_dtype; run.ldB = ldB; run.nsig = nsig;
    run.sigma2 = sigma2; run.nsigma2 = nsigma2; run.maxiter = maxiter; run.max_acq = max_acq; run.max_del = max_del;
    run.min_increase = min_increase; run.alpha_in = alpha_in; run.ld_ain = ld_ain; run.ha_in = alpha_in ? ha.data() : nullptr;
    run.X = X; run.ldX = ldX; run.alpha_out = alpha_out; run.ld_aout = ld_aout; run.x_loc = x_loc;
    run.history = history; run.history_cap = history_cap; run.iterations = iterations; run.flags = flags;
    DevTmp tB;  // a host caller's B on the device
    if (b_loc == CSMP_HOST) {
        CHECK(fsblb_nomem(ctx, who, tB.alloc(ctx, bbytes)));
        HIPCHECK(hipMemcpy(tB.p, B, bbytes, hipMemcpyHostToDevice));
        run.dB = (const char*)tB.p;
    }
    const int wide_members = ctx->group_wide > ctx->sweep_group && nsig > ctx->sweep_group && !ctx->wide_refused ? ctx->group_wide : 0;
    auto ensure = [&](csmp_ctx* c) -> int {
        const int rc = solver_ensure(c, 1, 1, false);
        c->s.begun = false;
        return rc;
    };
    int ticks_rc = CSMP_OK;  // (the ticks' own status: only a failed allocation is reported as CSMP_ENOMEM)
    auto enqueue = [&](csmp_ctx*, bool granted) -> int {
        const int R = (int)std::min<int64_t>(granted ? wide_members : ctx->sweep_group, nsig);
        CHECK(fsblb_ensure(ctx, R));
        ticks_rc = ctx->dtype == CSMP_F32 ? run.run<float>(R) : run.run<double>(R);
        return CSMP_OK;
    };
    const int rc = fsblb_nomem(ctx, who, batch_pipelines(ctx, false, ctx->sweep_group, wide_members, 3, ensure, enqueue));
    return finish(rc != CSMP_OK ? rc : ticks_rc);
}

extern "C" int csmp_fsbl_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, const double* sigma2, int64_t nsigma2,
                               int64_t maxiter, double min_increase, const double* alpha_in, int64_t ld_alpha_in, double* X, int64_t ldX,
                               double* alpha_out, int64_t ld_alpha_out, int x_loc, int64_t* history, int64_t history_cap, int64_t* iterations,
                               int* flags) {
    if (!ctx) return CSMP_EINVAL;
    return fsbl_batch_impl(ctx, "fsbl_batch", false, B, b_dtype, ldB, nsig, b_loc, sigma2, nsigma2, maxiter, 0, 0, min_increase, alpha_in, ld_alpha_in,
                           X, ldX, alpha_out, ld_alpha_out, x_loc, history, history_cap, iterations, flags);
}

extern "C" int csmp_rmps_batch(csmp_ctx* ctx, const void* B, int b_dtype, int64_t ldB, int64_t nsig, int b_loc, const double* sigma2, int64_t nsigma2,
                               int64_t maxiter, int64_t maxiter_acquisition, int64_t maxiter_deletion, double min_increase, const double* alpha_in,
                               int64_t ld_alpha_in, double* X, int64_t ldX, double* alpha_out, int64_t ld_alpha_out, int x_loc, int64_t* history,
                               int64_t history_cap, int64_t* iterations, int* flags) {
    if (!ctx) return CSMP_EINVAL;
    return fsbl_batch_impl(ctx, "rmps_batch", true, B, b_dtype, ldB, nsig, b_loc, sigma2, nsigma2, maxiter, maxiter_acquisition, maxiter_deletion,
                           min_increase, alpha_in, ld_alpha_in, X, ldX, alpha_out, ld_alpha_out, x_loc, history, history_cap, iterations, flags);
}
