"""GPU tests (pytest -m gpu) of csmp_bpd_batch: basis pursuit denoising for every column of B, the signals of a group in lockstep on
shared launches.  Every member keeps csmp_bpd's arithmetic -- k_bp_gemm repeats k_bp_gemv's operations per right-hand side, the shared
pass gives the single sweep's bits per member, the group kernels (k_bpd_pq_group and k_bpd_ball_group among them) call the single
kernels' bodies on the member's own buffers and radius, a refilled slot starts as bpd_start does -- so a batch must return the BITS of
a caller's loop over csmp_bpd: X, iterations, converged and resnorm, whatever the batch size, the group sizes, the radii and the
iterations at which the members leave."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as btw  # noqa: E402
import bpd_twin as tw  # noqa: E402
from test_gpu_bp_batch import signals, torch_dictionary, same, cut  # noqa: E402

pytestmark = pytest.mark.gpu

NSIGS = (1, 2, 3, 5, 8, 9, 13)
SHAPES = [(32, 48, np.float64, False), (100, 257, np.float32, True), (130, 1000, np.float32, False), (257, 300, np.float32, False),
          (48, 32, np.float64, False)]
RHO = tw.RHO


@pytest.fixture
def D(cs):
    """dictionaries of ONE test, closed when it ends"""
    made = []

    def make(A, **kw):
        d = cs.Dictionary(A, **kw)
        made.append(d)
        return d
    yield make
    for d in made:
        d.close()


def noisy(A, nsig):
    """test_gpu_bp_batch.py's signals plus noise of norm δ_s = 1e-2 √M (1 + s mod 3) per column; the zero, single-atom and copied
    columns are set after the noise is added, δ_3 = δ_0.  Returns (B, δ)."""
    M, N = A.shape
    clean = signals(A, nsig)
    delta = np.array([1e-2 * np.sqrt(M) * (1 + s % 3) for s in range(nsig)])
    noise = np.random.default_rng(M + N).standard_normal((M, nsig))
    B = clean + noise * (delta / np.linalg.norm(noise, axis=0))
    if nsig > 1:
        B[:, 1] = clean[:, 1]
    if nsig > 2:
        B[:, 2] = clean[:, 2]
    if nsig > 3:
        B[:, 3] = B[:, 0]
        delta[3] = delta[0]
    return np.asfortranarray(B), delta


def problem(M, N, dtype, weighted, nsig=max(NSIGS)):
    A = btw.data(M, N, 3, M + N, dtype)[0]
    w = 0.5 + np.random.default_rng(N).random(N) if weighted else 1.0
    B, delta = noisy(A, nsig)
    return A, B, delta, w


def deltas(delta, nsig):
    delta = np.atleast_1d(np.asarray(delta, dtype=np.float64))
    return np.full(nsig, delta[0]) if len(delta) == 1 else delta[:nsig]


def loop(d, B, delta, w=1.0, **kw):
    """what a caller without the batch form writes: csmp_bpd column by column on the same Dictionary"""
    nsig = B.shape[1]
    kw.setdefault("rho", RHO)
    dl = deltas(delta, nsig)
    X = np.zeros((d.shape[1], nsig), np.float64, order="F")
    it, conv, rn = np.zeros(nsig, np.int64), np.zeros(nsig, bool), np.zeros(nsig, np.float64)
    for s in range(nsig):
        X[:, s], info = d.ctx.bpd(np.ascontiguousarray(B[:, s]), float(dl[s]), w, **kw)
        it[s], conv[s], rn[s] = info["iterations"], info["converged"], info["resnorm"]
    return X, it, conv, rn


def flat(res):
    X, info = res
    return X, info["iterations"], info["converged"], info["resnorm"]


def batch(d, B, delta, w=1.0, tunes=None, **kw):
    tunes = tunes or {}
    kw.setdefault("rho", RHO)
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return flat(d.ctx.bpd_batch(B, delta, w, **kw))
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


# ------------------------------------------------------------------------------------------ 1. bits of the loop
@pytest.mark.parametrize("M,N,dtype,weighted", SHAPES, ids=[f"{m}x{n}" for m, n, _, _ in SHAPES])
def test_bits_of_the_loop(cs, D, M, N, dtype, weighted):
    A, Ball, dall, w = problem(M, N, dtype, weighted)
    d = D(A)
    for mode, delta in (("per column", dall), ("shared", float(dall[0]))):
        ref = loop(d, Ball, delta, w, maxiter=2000)
        print(f"{M} x {N}, {mode} delta: loop iterations {ref[1].tolist()}, converged {ref[2].astype(int).tolist()}")
        assert len(set(ref[1].tolist())) >= 3                 # the precondition: the slots are refilled at different times
        assert np.all(ref[0][:, 1] == 0.0) and ref[1][1] == 32   # the zero column
        assert np.array_equal(ref[0][:, 3], ref[0][:, 0]) and ref[1][3] == ref[1][0]   # the copy of column 0
        for nsig in NSIGS:
            dl = delta if np.isscalar(delta) else delta[:nsig]
            got = batch(d, np.asfortranarray(Ball[:, :nsig]), dl, w, maxiter=2000)
            assert same(got, cut(ref, nsig)), (mode, nsig, got[1], ref[1][:nsig])
    # the public function, against the public bpd
    ref = loop(d, Ball, dall, w, maxiter=2000)
    xs, info = cs.bpd_batch(d, Ball[:, :9], dall[:9], None if not weighted else w, maxiter=2000, return_info=True)
    assert len(xs) == 9 and not info["factored"] and np.array_equal(info["iterations"], ref[1][:9])
    for s, x in enumerate(xs):
        one, oi = cs.bpd(d, Ball[:, s], float(dall[s]), None if not weighted else w, maxiter=2000, return_info=True)
        assert np.array_equal(x.nzind, one.nzind) and np.array_equal(x.nzval, one.nzval), s
        assert oi["iterations"] == info["iterations"][s]
        assert np.array_equal(x.to_dense(), ref[0][:, s])


# ------------------------------------------------------------------------------------------ 2. a cap inside an interval
def test_a_cap_inside_an_interval(cs, D):
    A, Ball, dall, w = problem(130, 1000, np.float32, False)
    B, delta = np.asfortranarray(Ball[:, :9]), dall[:9]
    d = D(A)
    ref = loop(d, B, delta, maxiter=300, check_every=32)
    print(f"maxiter 300: loop iterations {ref[1].tolist()}, converged {ref[2].astype(int).tolist()}")
    assert ref[2].any() and any(i == 300 and not c for i, c in zip(ref[1], ref[2]))   # the precondition
    assert same(batch(d, B, delta, maxiter=300, check_every=32), ref)
    for ce in (1, 7):
        ref = loop(d, B, delta, maxiter=50, check_every=ce)
        assert same(batch(d, B, delta, maxiter=50, check_every=ce), ref), ce
    got = batch(d, B, delta, maxiter=0)
    assert same(got, loop(d, B, delta, maxiter=0))
    assert np.all(got[0] == 0.0) and np.all(got[1] == 0) and not got[2].any()
    assert np.allclose(got[3], np.linalg.norm(B.astype(np.float64), axis=0), rtol=1e-14)


# ------------------------------------------------------------------------------------------ 3. every pass instantiation
@pytest.mark.parametrize("M,N,dtype,group,wide", [(4096, 4200, np.float32, 4, 8), (3000, 3100, np.float32, 4, 8), (1024, 1500, np.float64, 4, 4)],
                         ids=["whole_units_wide", "clamped_loads", "f64_four_waves"])
def test_every_pass_instantiation(cs, D, M, N, dtype, group, wide):
    At, A = torch_dictionary(M, N, dtype, 7 + N)
    d = D(At)
    cfg = d.ctx.sweep_config()
    assert cfg["group_max"] == group and cfg["group_wide"] == wide
    B, delta = noisy(A, 9)
    ref = loop(d, B, delta, maxiter=96)
    print(f"{M} x {N}: loop iterations {ref[1].tolist()}, converged {ref[2].astype(int).tolist()}")
    assert len(set(ref[1].tolist())) >= 2                 # members leave at different times: passes of fewer members follow
    assert same(batch(d, B, delta, maxiter=96), ref)


# ------------------------------------------------------------------------------------------ 4. schedule switches
def test_schedule_switches(cs, D):
    A, Ball, dall, w = problem(130, 1000, np.float32, False)
    B, delta = np.asfortranarray(Ball[:, :9]), dall[:9]
    d = D(A)
    ref = loop(d, B, delta, maxiter=2000)
    assert len(set(ref[1].tolist())) >= 3
    assert same(batch(d, B, delta, maxiter=2000), ref)
    for tunes in ({"group_max": 1}, {"group_max": 2}, {"group_max": 3}, {"group_max": 4}, {"group_wide": 1}):
        assert same(batch(d, B, delta, maxiter=2000, tunes=tunes), ref), tunes
    d.ctx.tune("sweep_dyn", 1)  # no shared pass: the batch takes the loop
    try:
        assert d.ctx.sweep_config()["group_max"] == 0
        ref_dyn = loop(d, B, delta, maxiter=2000)
        assert same(batch(d, B, delta, maxiter=2000), ref_dyn)
    finally:
        d.ctx.tune("sweep_dyn", 0)
    d.ctx.set_option("screened_sweep", 1)  # the screened sweeps: signal by signal, the loop's bits under the same option
    try:
        assert same(batch(d, B, delta, maxiter=2000), loop(d, B, delta, maxiter=2000))
    finally:
        d.ctx.set_option("screened_sweep", 0)
    assert same(batch(d, B, delta, maxiter=2000), ref)


# ------------------------------------------------------------------------------------------ 5. twin parity
def test_parity_with_the_twin(cs, D):
    A, Ball, dall, w = problem(100, 257, np.float32, False)
    d = D(A)
    X, it, conv, rn = batch(d, Ball, dall, maxiter=2000)
    picked = [s for s in range(Ball.shape[1]) if conv[s] and s not in (1, 3)][:5]
    assert len(picked) == 5
    for s in picked:
        zt, info = tw.bpd(A, Ball[:, s].astype(np.float64), float(dall[s]), maxiter=2000)
        assert info["converged"]
        err = float(np.max(np.abs(X[:, s] - zt)))
        print(f"signal {s}: iterations {it[s]} (twin {info['iterations']}), max|z - twin| = {err:.3e}")
        assert np.array_equal(np.flatnonzero(X[:, s]), np.flatnonzero(zt)), s
        assert err <= tw.RTOL * np.max(np.abs(zt)), s


# ------------------------------------------------------------------------------------------ 6. the factor and interleaving
def test_the_factor_and_interleaving(cs, D):
    A, Ball, dall, w = problem(64, 256, np.float32, False)
    B, delta = np.asfortranarray(Ball[:, :5]), dall[:5]
    b0 = np.ascontiguousarray(B[:, 0])
    d = D(A)
    X, info = d.ctx.bpd_batch(B, delta, maxiter=64)
    assert info["factored"] and info["iterations"].shape == (5,) and info["converged"].dtype == bool
    assert not d.ctx.bpd(b0, float(delta[0]), maxiter=64)[1]["factored"]
    assert not d.ctx.bpd_batch(B, delta, maxiter=64)[1]["factored"]
    d1 = D(A)
    assert d1.ctx.bpd(b0, float(delta[0]), maxiter=64)[1]["factored"]
    assert not d1.ctx.bpd_batch(B, delta, maxiter=64)[1]["factored"]   # not after a prior bpd
    d2 = D(A)

    def others(ctx):
        xi, rni = ctx.ista(b0, 0.05, maxiter=20)
        xb, ib = ctx.bp(b0, maxiter=64)
        xd, idn = ctx.bpd(b0, float(delta[0]), maxiter=64)
        Xb, ibb = ctx.bp_batch(B, maxiter=64)
        mp = ctx.mp_batch(B, 6)
        return (xi, np.float64(rni), xb, np.array([ib["iterations"], ib["converged"], ib["resnorm"]]), xd,
                np.array([idn["iterations"], idn["converged"], idn["resnorm"]]), Xb, ibb["iterations"], ibb["converged"], ibb["resnorm"]) + tuple(mp)

    before = others(d2.ctx)
    got = flat(d2.ctx.bpd_batch(B, delta, maxiter=64))
    assert same(got, flat((X, info)))
    assert same(others(d2.ctx), before)
    assert same(flat(d2.ctx.bpd_batch(B, delta, maxiter=64)), got)


# ------------------------------------------------------------------------------------------ 7. device pointers
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["B_f32", "B_f64"])
def test_device_pointers(cs, D, dtype):
    import torch
    A, Ball, dall, w = problem(100, 257, np.float32, True)
    M, N = A.shape
    nsig, ldB, ldX = 9, M + 3, N + 5
    Bh, delta = np.asfortranarray(Ball[:, :nsig].astype(dtype)), dall[:nsig]
    d = D(A)
    d.ctx.bpd_batch(Bh, delta, w, maxiter=0)  # (the call that factorises)
    want = d.ctx.bpd_batch(Bh, delta, w, maxiter=256)
    buf = torch.full((nsig, ldB), 3.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    buf[:, :M] = torch.from_numpy(np.ascontiguousarray(Bh.T)).cuda()
    xbuf = torch.full((nsig, ldX), 7.0, dtype=torch.float64, device="cuda")
    Bt, Xt = buf.T[:M], xbuf.T[:N]
    assert Bt.stride() == (1, ldB) and Xt.stride() == (1, ldX)
    info = d.ctx.bpd_batch_device(Bt, delta, w, Xt, maxiter=256)
    assert same((Xt.cpu().numpy(),) + flat((None, info))[1:], flat(want)) and not info["factored"]
    assert np.all(xbuf[:, N:].cpu().numpy() == 7.0)      # the padding rows of X are untouched
    assert np.all(buf[:, M:].cpu().numpy() == 3.0)


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(cs):
    L = cs._lib
    A, Ball, dall, w = problem(32, 48, np.float64, False)
    M, N = A.shape
    nsig = 3
    B, delta = np.asfortranarray(Ball[:, :nsig]), np.ascontiguousarray(dall[:nsig])
    d = cs.Dictionary(A)
    bare = L.Context(0)
    want = flat(d.ctx.bpd_batch(B, delta))

    def call(ctx, **over):
        a = dict(B=B, dtype=L.F64, ldB=M, nsig=nsig, b_loc=L.HOST, delta=delta, w=np.ones(1), rho=RHO, maxiter=64, tol=1e-8, ce=32, ldX=N,
                 x_loc=L.HOST)
        a.update(over)
        X = np.full((N, nsig), 5.0, order="F")
        it, rn, fl = np.full(nsig, 5, np.int64), np.full(nsig, 5.0), np.full(nsig, 5, np.int32)
        C = L.C
        rc = L.lib().csmp_bpd_batch(ctx._h, None if a["B"] is None else L.ptr(a["B"]), a["dtype"], L.i64(a["ldB"]), L.i64(a["nsig"]), a["b_loc"],
                                    None if a["delta"] is None else L.ptr(a["delta"]), L.i64(0 if a["delta"] is None else len(a["delta"])),
                                    None if a["w"] is None else L.ptr(a["w"]), L.i64(0 if a["w"] is None else len(a["w"])), C.c_double(a["rho"]),
                                    L.i64(a["maxiter"]), C.c_double(a["tol"]), L.i64(a["ce"]), L.ptr(X), L.i64(a["ldX"]), a["x_loc"],
                                    it.ctypes.data_as(C.POINTER(L.i64)), rn.ctypes.data_as(C.POINTER(C.c_double)), fl.ctypes.data_as(C.POINTER(C.c_int)))
        untouched = np.all(X == 5.0) and np.all(it == 5) and np.all(rn == 5.0) and np.all(fl == 5)
        return rc, untouched

    try:
        cases = [("ldB < M", dict(ldB=M - 1), L.EDIM), ("ldX < N", dict(ldX=N - 1), L.EDIM), ("nsig < 0", dict(nsig=-1), L.EINVAL),
                 ("nsig == 0", dict(nsig=0, delta=np.ones(1)), L.OK), ("length(w)", dict(w=np.ones(N - 1)), L.EDIM),
                 ("length(delta)", dict(delta=np.ones(2)), L.EDIM), ("length(delta) > nsig", dict(delta=np.ones(4)), L.EDIM),
                 ("negative delta", dict(delta=np.array([0.1, -0.1, 0.1])), L.EINVAL), ("nan delta", dict(delta=np.array([np.nan])), L.EINVAL),
                 ("inf delta", dict(delta=np.array([0.1, 0.1, np.inf])), L.EINVAL), ("null delta", dict(delta=None), L.EINVAL),
                 ("negative weight", dict(w=-np.ones(N)), L.EINVAL), ("null w", dict(w=None), L.EINVAL), ("null B", dict(B=None), L.EINVAL),
                 ("dtype", dict(dtype=5), L.EINVAL), ("b_loc", dict(b_loc=7), L.EINVAL), ("x_loc", dict(x_loc=-1), L.EINVAL),
                 ("rho", dict(rho=0.0), L.EINVAL), ("tol", dict(tol=float("nan")), L.EINVAL), ("maxiter", dict(maxiter=-1), L.EINVAL),
                 ("check_every", dict(ce=0), L.EINVAL)]
        for name, over, code in cases:
            rc, untouched = call(d.ctx, **over)
            assert rc == code and untouched, (name, rc)
            assert same(flat(d.ctx.bpd_batch(B, delta)), want), name  # the context still solves
        rc, untouched = call(d.ctx)
        assert rc == L.OK and not untouched                   # (the harness itself: a served call writes)
        assert call(bare, nsig=nsig) == (L.ESTATE, True)      # no dictionary
        # more rows than columns and a repeated row are SERVED, as csmp_bpd serves them: the loop's bits
        R = np.array(A)
        R[5] = R[3]
        Bt = np.asfortranarray(np.random.default_rng(5).standard_normal((N, 3)))
        for other, Bo, do in ((np.asfortranarray(A.T), Bt, 0.5), (np.asfortranarray(R), B, delta)):
            o = cs.Dictionary(other)
            try:
                X, info = o.ctx.bpd_batch(Bo, do, maxiter=64)
                assert info["factored"] and same(flat((X, info)), loop(o, Bo, do, maxiter=64))
            finally:
                o.close()
        d.ctx.set_dictionary(np.asfortranarray(R))            # a new dictionary: the factor and the group's buffers are made afresh
        d.ctx.set_dictionary(A)
        X, info = d.ctx.bpd_batch(B, delta)
        assert info["factored"] and same(flat((X, info)), want)
    finally:
        d.close()
        bare.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        with pytest.raises(cs.CsmpError) as e:
            S.ctx.bpd_batch(B, delta)
        assert e.value.code == L.ESTATE
    finally:
        S.close()


# ------------------------------------------------------------------------------------------ 9. allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_bpd.py's pattern: every device allocation of a bpd_batch call fails in turn with CSMP_ENOMEM, the same context
    then returns the clean context's bits, and the library holds what it held before.  Least failures: csmp_bpd's 18 (the iterates,
    the factor and the M-vectors, A A' and k_rowgram's partials), the staged B, BpdBatchBuf's 11 -- 30 -- and the three further solver
    slots of a group of four come on top.  (A Float64 dictionary: no wide groups, whose slots may fail without failing the call.)"""
    L = cs._lib
    A, Ball, dall, w = problem(32, 48, np.float64, False)
    B, delta = np.asfortranarray(Ball[:, :5]), dall[:5]
    gc.collect()
    base = L.live_resources()
    clean = cs.Dictionary(A)
    assert clean.ctx.sweep_config()["group_wide"] == clean.ctx.sweep_config()["group_max"] == 4
    want = flat(clean.ctx.bpd_batch(B, delta))
    assert same(want, loop(clean, B, delta))
    clean.close()
    n, seen_ok, failed = 0, 0, 0
    while seen_ok < 2 and n < 600:
        n += 1
        d = cs.Dictionary(A)
        d.ctx.tune("fail_alloc", n)
        try:
            got = flat(d.ctx.bpd_batch(B, delta))
            assert same(got, want), n
            seen_ok += 1
        except cs.CsmpError as e:
            seen_ok = 0
            failed += 1
            assert e.code == L.ENOMEM, (n, e.code, str(e))
        d.ctx.tune("fail_alloc", 0)
        assert same(flat(d.ctx.bpd_batch(B, delta)), want), (n, "after the failed call")
        d.close()
    print(f"bpd_batch: {failed} allocations failed in turn")
    assert n < 600 and failed >= 30
    gc.collect()
    assert L.live_resources() == base
