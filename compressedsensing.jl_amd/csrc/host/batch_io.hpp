// host/batch_io.hpp -- part of the host side of libcsmp.so (included by csmp.hip, in order; ONE translation unit):
// the front end of the batch drivers (csmp_omp_batch, csmp_fr_batch, csmp_gomp_batch, csmp_sp_batch, csmp_omp_batch_mfma): the
// checks they share, B and the outputs of a host caller on the device, the staggered schedule of whole solves on several
// contexts, the re-solve of one signal, and the two-pipeline scaffold of the omp, fr and mp batches (batch_pipelines: the twin, the
// solver slots of both contexts, the wide groups' all-or-none slots, the fork and join of the two streams, the drain of a failure).
// ------------------------------------------------------------------------------------------ batch front end
// The arguments of one batch call (B: ldB x nsig column-major, idx / val: k x nsig, nnz: nsig) and the device copies a host
// caller's B and outputs need.  Every temporary is freed on every return path.
struct BatchIO {
    csmp_ctx* ctx;
    const void* B;
    int b_dtype;
    int64_t ldB, nsig;
    int b_loc;
    int64_t k;
    int64_t* idx;
    double* val;
    int64_t* nnz;
    int out_loc;
    const char* dB;  // B where the solvers read it: on the device once stage() has run
    int64_t *d_idx, *d_nnz;  // the outputs on the device
    double* d_val;
    int* d_flag = nullptr;  // per-signal stop flags: stage(true)
    DevTmp tB, tIdx, tVal, tNnz, tFlag;

    BatchIO(csmp_ctx* c, const void* B_, int b_dtype_, int64_t ldB_, int64_t nsig_, int b_loc_, int64_t k_, int64_t* idx_, double* val_,
            int64_t* nnz_, int out_loc_)
        : ctx(c), B(B_), b_dtype(b_dtype_), ldB(ldB_), nsig(nsig_), b_loc(b_loc_), k(k_), idx(idx_), val(val_), nnz(nnz_), out_loc(out_loc_),
          dB((const char*)B_), d_idx(idx_), d_nnz(nnz_), d_val(val_) {}
    BatchIO(const BatchIO&) = delete;
    BatchIO& operator=(const BatchIO&) = delete;

    size_t es() const { return b_dtype == CSMP_F32 ? 4 : 8; }
    // signals off .. off+n of this call, unstaged (csmp_omp_batch_mfma's chunks)
    BatchIO part(int64_t off, int64_t n) const {
        return BatchIO(ctx, (const char*)B + (size_t)off * (size_t)ldB * es(), b_dtype, ldB, n, b_loc, k, idx + off * k, val + off * k,
                       nnz + off, out_loc);
    }
    // The checks every batch entry shares.  An entry makes its own (eps, l, NaN tolerances, ...) before these, so that a bad
    // argument is reported ahead of a missing dictionary, and those that depend on the dictionary's shape (2k > M) after them.
    int check() const {
        if ((b_loc != CSMP_HOST && b_loc != CSMP_DEVICE) || (out_loc != CSMP_HOST && out_loc != CSMP_DEVICE))
            return fail(ctx, CSMP_EINVAL, "b_loc / out_loc must be CSMP_HOST or CSMP_DEVICE");
        if (!B || nsig < 0 || k < 1 || ldB < ctx->M || (nsig > 0 && (!idx || !val || !nnz))) return fail(ctx, CSMP_EINVAL, "batch: bad arguments");
        if (b_dtype != CSMP_F32 && b_dtype != CSMP_F64) return fail(ctx, CSMP_EINVAL, "b_dtype must be CSMP_F32 or CSMP_F64");
        if (!ctx->dA) return fail(ctx, CSMP_ESTATE, "no dictionary set (csmp_set_dictionary)");
        return CSMP_OK;
    }
    // a host B to the device, device outputs for a host caller, and (flags) a stop-flag word per signal
    int stage(bool flags) {
        if (b_loc == CSMP_HOST) {
            CHECK(tB.alloc(ctx, (size_t)ldB * (size_t)nsig * es()));
            HIPCHECK(hipMemcpy(tB.p, B, (size_t)ldB * (size_t)nsig * es(), hipMemcpyHostToDevice));
            dB = (const char*)tB.p;
        }
        if (out_loc == CSMP_HOST) {
            CHECK(tIdx.alloc(ctx, (size_t)k * nsig * 8));
            CHECK(tVal.alloc(ctx, (size_t)k * nsig * 8));
            CHECK(tNnz.alloc(ctx, (size_t)nsig * 8));
            d_idx = (int64_t*)tIdx.p;
            d_val = (double*)tVal.p;
            d_nnz = (int64_t*)tNnz.p;
        }
        if (flags) {
            CHECK(tFlag.alloc(ctx, (size_t)nsig * sizeof(int)));
            d_flag = (int*)tFlag.p;
        }
        return CSMP_OK;
    }
    const void* col(int64_t s) const { return dB + (size_t)s * (size_t)ldB * es(); }
    int* flag(int64_t s) const { return d_flag + s; }
    // signal s into c's active slot
    int init(csmp_ctx* c, int64_t s) const {
        return b_dtype == CSMP_F32 ? init_from_device_t<float>(c, (const float*)col(s)) : init_from_device_t<double>(c, (const double*)col(s));
    }
    // c's solution into signal s's outputs (sflag: its stop flags, or null)
    int emit(csmp_ctx* c, int64_t s, int* sflag) const { return launch_finish(c, d_idx + s * k, d_val + s * k, d_nnz + s, nullptr, (int)k, sflag); }
    // emit's arguments for solver sv as a member of a round's finish launch (launch_finish_group)
    FinishMember member(const Solver& sv, int64_t s, int* sflag) const { return finish_member(sv, d_idx + s * k, d_val + s * k, d_nnz + s, sflag); }
    // the end of the call: a host caller's outputs come back (after a success only), and this context's stream is drained
    int done(int rc) {
        if (out_loc == CSMP_HOST) {
            if (rc == CSMP_OK) {
                HIPCHECK(hipMemcpyAsync(idx, d_idx, (size_t)k * nsig * 8, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHECK(hipMemcpyAsync(val, d_val, (size_t)k * nsig * 8, hipMemcpyDeviceToHost, ctx->stream));
                HIPCHECK(hipMemcpyAsync(nnz, d_nnz, (size_t)nsig * 8, hipMemcpyDeviceToHost, ctx->stream));
            }
            HIPCHECK(hipStreamSynchronize(ctx->stream));
        }
        return rc;
    }
};

// Signal s solved on c's active slot: its column in, step(t) for t = 0 .. k-1, the solution out
template <typename Step>
static int batch_solve(csmp_ctx* c, const BatchIO& io, int64_t s, int* flag, Step&& step) {
    int rc = io.init(c, s);
    for (int64_t t = 0; t < io.k && rc == CSMP_OK; ++t) rc = step(t);
    return rc == CSMP_OK ? io.emit(c, s, flag) : rc;
}
// The exact re-solve of a signal some faster path flagged: omp with the full append chain
static int omp_solve_exact(csmp_ctx* c, const BatchIO& io, int64_t s, double eps, int* flag) {
    return batch_solve(c, io, s, flag, [&](int64_t t) { return omp_step(c, eps, t > 0, false); });
}

// The staggered schedule: T whole solves in flight on cc[0 .. T) -- a context and T - 1 twins, each on its own stream -- with
// signal s on cc[s % T], everything enqueued up front.  enqueue(c, s, ev) enqueues signal s's solve on c and, when ev is not null,
// records ev behind the solve's first sweep; the next twin's first solve waits for it.  The chains then run OUT of phase: one
// signal's short stages fall under another's sweep (in phase they would fall on each other).  Returns once the twins' streams
// are done; on a failure every stream is drained before the return.
template <typename Enqueue>
static int batch_stagger(csmp_ctx* const* cc, int T, int64_t nsig, Enqueue&& enqueue) {
    csmp_ctx* ctx = cc[0];
    auto run = [&]() -> int {
        HIPCHECK(hipStreamSynchronize(ctx->stream));  // (the caller's buffers and our temporaries are ready before any stream starts)
        for (int q = 0; q + 1 < T; ++q)
            if (!cc[q]->ev_twin) HIPCHECK(hipEventCreateWithFlags(&cc[q]->ev_twin, hipEventDisableTiming));
        for (int64_t s = 0; s < nsig; ++s) {
            const int q = (int)(s % T);
            csmp_ctx* c = cc[q];
            if (s > 0 && s < T) HIPCHECK(hipStreamWaitEvent(c->stream, cc[q - 1]->ev_twin, 0));  // a twin starts one sweep behind
            const int rc = enqueue(c, s, s + 1 < T ? c->ev_twin : nullptr);
            if (rc != CSMP_OK) {
                if (c != ctx) ctx->err = c->err;
                return rc;
            }
        }
        for (int w = 1; w < T; ++w) HIPCHECK(hipStreamSynchronize(cc[w]->stream));
        return CSMP_OK;
    };
    const int rc = run();
    if (rc != CSMP_OK)
        for (int w = 0; w < T; ++w) (void)hipStreamSynchronize(cc[w]->stream);
    return rc;
}

// ------------------------------------------------------------------------------------------ two pipelines
// The scaffold of csmp_omp_batch / csmp_fr_batch (batch_impl, host/forward.hpp) and csmp_mp_batch (host/mp_batch.hpp): a batch on
// the caller's context and, where wanted, on a twin -- a clone on its own stream -- beside it.
// Two pipelines: csmp_tune(CSMP_TUNE_PIPELINES, 1) keeps one, 2 and 3 take two whatever the size; automatic where a sweep is long
// enough for its tail to matter: dictionaries of kPairMinBytes and more (measured: tools/probes/pair_sizes.py)
static bool batch_two_pipelines(const csmp_ctx* ctx) {
    constexpr size_t kPairMinBytes = (size_t)4 << 20;  // two pipelines: 1 MiB -10 %, 8 MiB +35 %, 32 MiB +40 %, 64 MiB ... 1 GiB +5 ... +16 %
    const size_t dict_bytes = (size_t)ctx->Mv * (size_t)ctx->N * (ctx->dtype == CSMP_F32 ? 4 : 8);
    return ctx->tune_pipelines != 1 && (ctx->tune_pipelines >= 2 || dict_bytes >= kPairMinBytes);
}
// the status of a step made on c, the caller's context or its twin: a twin's failure is reported on the caller's context
static int twin_rc(csmp_ctx* ctx, csmp_ctx* c, int rc) {
    if (rc != CSMP_OK && c != ctx) ctx->err = c->err;
    return rc;
}
// The solver slots of both contexts made ready, the twin's stream forked behind the caller's, the rounds enqueued, the streams
// joined.  The slots are q * stride: q < narrow the set the batch cannot run without (slot 0 of the caller's context is the
// driver's, ready before the call's staging buffers), narrow <= q < wide the wide groups' extension (wide <= narrow: none), with or
// without a twin.  ensure(c) makes c's active slot ready.  enqueue(tw, granted) enqueues the rounds: tw is the twin or null, granted
// says whether the extension is there.
// Device allocations come in this order: the caller's narrow slots, the twin and its narrow slots, then the extension, the caller's
// before the twin's.  A failure in the extension is not a failure of the call; any other returns its status on the caller's
// context, both streams drained, the contexts usable.
template <typename Ensure, typename Enqueue>
static int batch_pipelines(csmp_ctx* ctx, bool twin, int narrow, int wide, int stride, Ensure&& ensure, Enqueue&& enqueue) {
    csmp_ctx* tw = nullptr;  // pipeline B's context
    auto ensure_slots = [&](csmp_ctx* c, int from, int to) -> int {
        int rc = CSMP_OK;
        for (int q = from; q < to && rc == CSMP_OK; ++q) {
            activate_slot(c, q * stride);
            rc = ensure(c);
        }
        activate_slot(c, 0);
        return twin_rc(ctx, c, rc);
    };
    auto run = [&]() -> int {  // (every way out of here passes what follows it below: slot 0 active again on both contexts -- enqueue may
                               // return with another slot active --, and once the twin exists the drain)
        CHECK(ensure_slots(ctx, 1, narrow));
        if (twin) {
            CHECK(twins_ensure(ctx, 1));
            tw = ctx->twins[0];
            tw->prof = ctx->prof;  // (csmp_profile_*: the second pipeline's launches are sampled like the first's)
            tw->prof_every = ctx->prof_every;
            CHECK(ensure_slots(tw, 0, narrow));
        }
        csmp_ctx* cs[2] = {ctx, tw};
        bool granted = false;
        if (wide > narrow) {
            // the slots beyond the narrow groups': all of them on both contexts, or none -- a device that cannot hold them runs the
            // groups of sweep_group members it has the slots for (the failure's text, which ensure_slots leaves on the caller's
            // context, is cleared with the slots)
            int r3 = CSMP_OK;
            for (csmp_ctx* c : cs) {
                if (!c || r3 != CSMP_OK) continue;
                c->tune_fail_alloc = ctx->tune_fail_alloc;  // (the test hook counts on through the twin's allocations)
                r3 = ensure_slots(c, narrow, wide);
                ctx->tune_fail_alloc = c->tune_fail_alloc;
                if (c != ctx) c->tune_fail_alloc = 0;
            }
            granted = r3 == CSMP_OK;
            if (!granted) {
                ctx->wide_refused = true;  // (not tried again batch after batch: about a thousand allocations and two drains)
                for (csmp_ctx* c : cs) {
                    if (!c) continue;
                    (void)hipStreamSynchronize(c->stream);
                    for (int q = narrow; q < wide; ++q) {
                        activate_slot(c, q * stride);
                        solver_free(c->s);
                    }
                    activate_slot(c, 0);
                    c->err.clear();
                }
                (void)hipGetLastError();
            }
        }
        if (tw) {
            if (!ctx->ev_twin) HIPCHECK(hipEventCreateWithFlags(&ctx->ev_twin, hipEventDisableTiming));
            if (!tw->ev_twin) HIPCHECK(hipEventCreateWithFlags(&tw->ev_twin, hipEventDisableTiming));
            // (the twin starts behind everything this context's stream holds: the caller's buffers, the slots' allocation)
            HIPCHECK(hipEventRecord(ctx->ev_twin, ctx->stream));
            HIPCHECK(hipStreamWaitEvent(tw->stream, ctx->ev_twin, 0));
        }
        CHECK(enqueue(tw, granted));
        if (tw) {  // this context's stream goes on behind the twin's last launch
            HIPCHECK(hipEventRecord(tw->ev_twin, tw->stream));
            HIPCHECK(hipStreamWaitEvent(ctx->stream, tw->ev_twin, 0));
        }
        return CSMP_OK;
    };
    const int rc = run();
    activate_slot(ctx, 0);
    if (tw) activate_slot(tw, 0);
    if (rc != CSMP_OK && tw) {  // (a failed enqueue: both streams drained before anything is released)
        (void)hipStreamSynchronize(tw->stream);
        (void)hipStreamSynchronize(ctx->stream);
    }
    return rc;
}

static int omp_batch_screened(csmp_ctx* ctx, BatchIO& io, double eps);  // host/screened.hpp
