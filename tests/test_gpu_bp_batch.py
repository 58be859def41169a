"""GPU tests (pytest -m gpu) of csmp_bp_batch: basis pursuit for every column of B, the signals of a group in lockstep on shared
launches.  Every member keeps csmp_bp's arithmetic -- k_bp_gemm repeats k_bp_gemv's operations per right-hand side, the shared pass
gives the single sweep's bits per member, the group kernels call the single kernels' bodies, a refilled slot starts as bp_start does --
so a batch must return the BITS of a caller's loop over csmp_bp: X, iterations, converged and resnorm, whatever the batch size, the
group sizes and the iterations at which the members leave.  k_bp_gemm has no measurement hook of its own: the comparisons with the loop
below carry it for every L = 1 .. 8 and the three modes (a step of L live members runs the three products at that L)."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu

NSIGS = (1, 2, 3, 5, 8, 9, 13)
SHAPES = [(32, 48, np.float64, False), (100, 257, np.float32, True), (130, 1000, np.float32, False), (64, 256, np.float32, False)]


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


def signals(A, nsig):
    """signal s: 1 + (3 s) mod max(2, M // 6) atoms with values N(0, 1) + sign; column 1 zero, column 2 the atom N // 3, column 3 a copy
    of column 0"""
    M, N = A.shape
    A64 = np.asarray(A, dtype=np.float64)
    rng = np.random.default_rng(M * N)
    cols = []
    for s in range(nsig):
        k = 1 + (3 * s) % max(2, M // 6)
        sup = rng.choice(N, k, replace=False)
        val = rng.standard_normal(k) + np.sign(rng.standard_normal(k))
        cols.append(A64[:, sup] @ val)
    if nsig > 1:
        cols[1] = np.zeros(M)
    if nsig > 2:
        cols[2] = A64[:, N // 3].copy()
    if nsig > 3:
        cols[3] = cols[0].copy()
    return np.asfortranarray(np.stack(cols, axis=1))


def problem(M, N, dtype, weighted, nsig=max(NSIGS)):
    A = tw.data(M, N, 3, M + N, dtype)[0]
    w = 0.5 + np.random.default_rng(N).random(N) if weighted else 1.0
    return A, signals(A, nsig), w


def loop(d, B, w=1.0, **kw):
    """what a caller without the batch form writes: csmp_bp column by column on the same Dictionary"""
    nsig = B.shape[1]
    X = np.zeros((d.shape[1], nsig), np.float64, order="F")
    it, conv, rn = np.zeros(nsig, np.int64), np.zeros(nsig, bool), np.zeros(nsig, np.float64)
    for s in range(nsig):
        X[:, s], info = d.ctx.bp(np.ascontiguousarray(B[:, s]), w, **kw)
        it[s], conv[s], rn[s] = info["iterations"], info["converged"], info["resnorm"]
    return X, it, conv, rn


def flat(res):
    X, info = res
    return X, info["iterations"], info["converged"], info["resnorm"]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def cut(ref, n):
    return (np.asfortranarray(ref[0][:, :n]),) + tuple(r[:n] for r in ref[1:])


def batch(d, B, w=1.0, tunes=None, **kw):
    tunes = tunes or {}
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return flat(d.ctx.bp_batch(B, w, **kw))
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


def torch_dictionary(M, N, dtype, seed):
    """tests/test_gpu_mp_batch.py's dictionaries: made on the device"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    At = torch.randn((N, M), generator=g, device="cuda", dtype=torch.float64)
    At /= At.norm(dim=1, keepdim=True)
    At = At.to(torch.float32 if dtype == np.float32 else torch.float64)
    return At, np.asfortranarray(At.cpu().numpy().T)


# ------------------------------------------------------------------------------------------ 1. bits of the loop
@pytest.mark.parametrize("M,N,dtype,weighted", SHAPES, ids=[f"{m}x{n}" for m, n, _, _ in SHAPES])
def test_bits_of_the_loop(cs, D, M, N, dtype, weighted):
    A, Ball, w = problem(M, N, dtype, weighted)
    d = D(A)
    ref = loop(d, Ball, w, maxiter=2000)
    print(f"{M} x {N}: loop iterations {ref[1].tolist()}, converged {ref[2].astype(int).tolist()}")
    assert len(set(ref[1].tolist())) >= 3                 # the precondition: the slots are refilled at different times
    assert np.all(ref[0][:, 1] == 0.0) and ref[1][1] == 32 and ref[3][1] == 0.0   # the zero column
    assert np.array_equal(ref[0][:, 3], ref[0][:, 0]) and ref[1][3] == ref[1][0]   # the copy of column 0
    for nsig in NSIGS:
        got = batch(d, np.asfortranarray(Ball[:, :nsig]), w, maxiter=2000)
        assert same(got, cut(ref, nsig)), (nsig, got[1], ref[1][:nsig])
    # the public function, against the public bp
    xs, info = cs.bp_batch(d, Ball[:, :9], None if not weighted else w, maxiter=2000, return_info=True)
    assert len(xs) == 9 and not info["factored"] and np.array_equal(info["iterations"], ref[1][:9])
    for s, x in enumerate(xs):
        one = cs.bp(d, Ball[:, s], None if not weighted else w, maxiter=2000)
        assert np.array_equal(x.nzind, one.nzind) and np.array_equal(x.nzval, one.nzval), s
        assert np.array_equal(x.to_dense(), ref[0][:, s])


# ------------------------------------------------------------------------------------------ 2. a cap inside an interval
def test_a_cap_inside_an_interval(cs, D):
    A, Ball, w = problem(130, 1000, np.float32, False)
    B = np.asfortranarray(Ball[:, :9])
    d = D(A)
    ref = loop(d, B, maxiter=100, check_every=32)
    print(f"maxiter 100: loop iterations {ref[1].tolist()}, converged {ref[2].astype(int).tolist()}")
    assert ref[2].any() and any(i == 100 and not c for i, c in zip(ref[1], ref[2]))   # the precondition
    assert same(batch(d, B, maxiter=100, check_every=32), ref)
    for ce in (1, 7):
        ref = loop(d, B, maxiter=50, check_every=ce)
        assert same(batch(d, B, maxiter=50, check_every=ce), ref), ce
        assert len(set(ref[1].tolist())) >= 2, (ce, ref[1])
    got = batch(d, B, maxiter=0)
    assert same(got, loop(d, B, maxiter=0))
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
    B = signals(A, 9)
    ref = loop(d, B, maxiter=96)
    print(f"{M} x {N}: loop iterations {ref[1].tolist()}, converged {ref[2].astype(int).tolist()}")
    assert len(set(ref[1].tolist())) >= 2                 # members leave at different times: passes of fewer members follow
    assert same(batch(d, B, maxiter=96), ref)


# ------------------------------------------------------------------------------------------ 4. schedule switches
def test_schedule_switches(cs, D):
    A, Ball, w = problem(130, 1000, np.float32, False)
    B = np.asfortranarray(Ball[:, :9])
    d = D(A)
    ref = loop(d, B, maxiter=2000)
    assert len(set(ref[1].tolist())) >= 3
    assert same(batch(d, B, maxiter=2000), ref)
    for tunes in ({"group_max": 1}, {"group_max": 2}, {"group_max": 3}, {"group_max": 4}, {"group_wide": 1}):
        assert same(batch(d, B, maxiter=2000, tunes=tunes), ref), tunes
    d.ctx.tune("sweep_dyn", 1)  # no shared pass: the batch takes the loop
    try:
        assert d.ctx.sweep_config()["group_max"] == 0
        ref_dyn = loop(d, B, maxiter=2000)
        assert same(flat(d.ctx.bp_batch(B, maxiter=2000)), ref_dyn)
    finally:
        d.ctx.tune("sweep_dyn", 0)
    d.ctx.set_option("screened_sweep", 1)  # the screened sweeps: signal by signal, the loop's bits under the same option
    try:
        assert same(flat(d.ctx.bp_batch(B, maxiter=2000)), loop(d, B, maxiter=2000))
    finally:
        d.ctx.set_option("screened_sweep", 0)
    assert same(batch(d, B, maxiter=2000), ref)


# ------------------------------------------------------------------------------------------ 6. twin parity
def test_parity_with_the_twin(cs, D):
    A, Ball, w = problem(100, 257, np.float32, False)
    d = D(A)
    X, it, conv, rn = batch(d, Ball, maxiter=2000)
    picked = [s for s in range(Ball.shape[1]) if conv[s] and s not in (1, 3)][:5]
    assert len(picked) == 5
    for s in picked:
        zt, info = tw.bp(A, Ball[:, s].astype(np.float64), maxiter=2000)
        assert info["converged"]
        err = float(np.max(np.abs(X[:, s] - zt)))
        print(f"signal {s}: iterations {it[s]} (twin {info['iterations']}), max|z - twin| = {err:.3e}")
        assert np.array_equal(np.flatnonzero(X[:, s]), np.flatnonzero(zt)), s
        assert err <= tw.RTOL * np.max(np.abs(zt)), s


# ------------------------------------------------------------------------------------------ 7. the factor and interleaving
def test_the_factor_and_interleaving(cs, D):
    A, Ball, w = problem(64, 256, np.float32, False)
    B = np.asfortranarray(Ball[:, :5])
    d = D(A)
    X, info = d.ctx.bp_batch(B, maxiter=64)
    assert info["factored"] and info["iterations"].shape == (5,) and info["converged"].dtype == bool
    assert not d.ctx.bp(np.ascontiguousarray(B[:, 0]), maxiter=64)[1]["factored"]
    assert not d.ctx.bp_batch(B, maxiter=64)[1]["factored"]
    d2 = D(A)
    b0 = np.ascontiguousarray(B[:, 0])

    def others(ctx):
        xi, rni = ctx.ista(b0, 0.05, maxiter=20)
        xb, ib = ctx.bp(b0, maxiter=64)
        mp = ctx.mp_batch(B, 6)
        return (xi, np.float64(rni), xb, np.array([ib["iterations"], ib["converged"], ib["resnorm"]])) + tuple(mp)

    before = others(d2.ctx)
    got = flat(d2.ctx.bp_batch(B, maxiter=64))
    assert same(got, flat((X, info)))
    assert same(others(d2.ctx), before)
    assert same(flat(d2.ctx.bp_batch(B, maxiter=64)), got)


# ------------------------------------------------------------------------------------------ 8. device pointers
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["B_f32", "B_f64"])
def test_device_pointers(cs, D, dtype):
    import torch
    A, Ball, w = problem(100, 257, np.float32, True)
    M, N = A.shape
    nsig, ldB, ldX = 9, M + 3, N + 5
    Bh = np.asfortranarray(Ball[:, :nsig].astype(dtype))
    d = D(A)
    d.ctx.bp_batch(Bh, w, maxiter=0)  # (the call that factorises)
    want = d.ctx.bp_batch(Bh, w, maxiter=256)
    buf = torch.full((nsig, ldB), 3.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    buf[:, :M] = torch.from_numpy(np.ascontiguousarray(Bh.T)).cuda()
    xbuf = torch.full((nsig, ldX), 7.0, dtype=torch.float64, device="cuda")
    Bt, Xt = buf.T[:M], xbuf.T[:N]
    assert Bt.stride() == (1, ldB) and Xt.stride() == (1, ldX)
    info = d.ctx.bp_batch_device(Bt, w, Xt, maxiter=256)
    assert same((Xt.cpu().numpy(),) + flat((None, info))[1:], flat(want)) and not info["factored"]
    assert np.all(xbuf[:, N:].cpu().numpy() == 7.0)      # the padding rows of X are untouched
    assert np.all(buf[:, M:].cpu().numpy() == 3.0)


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(cs):
    L = cs._lib
    A, Ball, w = problem(32, 48, np.float64, False)
    M, N = A.shape
    nsig = 3
    B = np.asfortranarray(Ball[:, :nsig])
    d = cs.Dictionary(A)
    bare = L.Context(0)
    want = flat(d.ctx.bp_batch(B))

    def call(ctx, **over):
        a = dict(B=B, dtype=L.F64, ldB=M, nsig=nsig, b_loc=L.HOST, w=np.ones(1), rho=1.0, maxiter=64, tol=1e-8, ce=32, ldX=N, x_loc=L.HOST)
        a.update(over)
        X = np.full((N, nsig), 5.0, order="F")
        it, rn, fl = np.full(nsig, 5, np.int64), np.full(nsig, 5.0), np.full(nsig, 5, np.int32)
        C = L.C
        rc = L.lib().csmp_bp_batch(ctx._h, None if a["B"] is None else L.ptr(a["B"]), a["dtype"], L.i64(a["ldB"]), L.i64(a["nsig"]), a["b_loc"],
                                   None if a["w"] is None else L.ptr(a["w"]), L.i64(0 if a["w"] is None else len(a["w"])), C.c_double(a["rho"]),
                                   L.i64(a["maxiter"]), C.c_double(a["tol"]), L.i64(a["ce"]), L.ptr(X), L.i64(a["ldX"]), a["x_loc"],
                                   it.ctypes.data_as(C.POINTER(L.i64)), rn.ctypes.data_as(C.POINTER(C.c_double)), fl.ctypes.data_as(C.POINTER(C.c_int)))
        untouched = np.all(X == 5.0) and np.all(it == 5) and np.all(rn == 5.0) and np.all(fl == 5)
        return rc, untouched

    try:
        cases = [("ldB < M", dict(ldB=M - 1), L.EDIM), ("ldX < N", dict(ldX=N - 1), L.EDIM), ("nsig < 0", dict(nsig=-1), L.EINVAL),
                 ("nsig == 0", dict(nsig=0), L.OK), ("length(w)", dict(w=np.ones(N - 1)), L.EDIM), ("negative weight", dict(w=-np.ones(N)), L.EINVAL),
                 ("null w", dict(w=None), L.EINVAL), ("null B", dict(B=None), L.EINVAL), ("dtype", dict(dtype=5), L.EINVAL),
                 ("b_loc", dict(b_loc=7), L.EINVAL), ("x_loc", dict(x_loc=-1), L.EINVAL), ("rho", dict(rho=0.0), L.EINVAL),
                 ("tol", dict(tol=float("nan")), L.EINVAL), ("maxiter", dict(maxiter=-1), L.EINVAL), ("check_every", dict(ce=0), L.EINVAL)]
        for name, over, code in cases:
            rc, untouched = call(d.ctx, **over)
            assert rc == code and untouched, (name, rc)
            assert same(flat(d.ctx.bp_batch(B)), want), name  # the context still solves
        assert call(bare, nsig=nsig)[0] == L.ESTATE          # no dictionary
        # more rows than columns: CSMP_EDIM, as csmp_bp (more than 2^19 rows, CSMP_ERANGE, needs 2^38 entries: bp_entry's check is shared)
        d.ctx.set_dictionary(np.asfortranarray(A.T))
        with pytest.raises(cs.CsmpError) as e:
            d.ctx.bp_batch(np.ones((N, 2)))
        assert e.value.code == L.EDIM
        # a repeated row: A A' is singular
        R = np.array(A)
        R[5] = R[3]
        d.ctx.set_dictionary(np.asfortranarray(R))
        for _ in range(2):
            with pytest.raises(cs.CsmpError) as e:
                d.ctx.bp_batch(np.asfortranarray(R @ np.eye(N)[:, :2]))
            assert e.value.code == L.EINVAL and "not positive definite to working precision" in str(e.value)
        with pytest.raises(ValueError):
            cs.bp_batch(d, np.asfortranarray(R @ np.eye(N)[:, :2]))
        d.ctx.set_dictionary(A)
        X, info = d.ctx.bp_batch(B)
        assert info["factored"] and same(flat((X, info)), want)
    finally:
        d.close()
        bare.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        with pytest.raises(cs.CsmpError) as e:
            S.ctx.bp_batch(B)
        assert e.value.code == L.ESTATE
    finally:
        S.close()


# ------------------------------------------------------------------------------------------ 10. allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_bp.py's pattern: every device allocation of a bp_batch call fails in turn with CSMP_ENOMEM, the same context then
    returns the clean context's bits, and the library holds what it held before.  Least failures: csmp_bp's 17 (the iterates, G and its
    factor, k_rowgram's partials), the staged B, BpBatchBuf's 10 -- 28 -- and the three further solver slots of a group of four come
    on top.  (A Float64 dictionary: no wide groups, whose slots may fail without failing the call.)"""
    L = cs._lib
    A, Ball, w = problem(32, 48, np.float64, False)
    B = np.asfortranarray(Ball[:, :5])
    gc.collect()
    base = L.live_resources()
    clean = cs.Dictionary(A)
    assert clean.ctx.sweep_config()["group_wide"] == clean.ctx.sweep_config()["group_max"] == 4
    want = flat(clean.ctx.bp_batch(B))
    assert same(want, loop(clean, B))
    clean.close()
    n, seen_ok, failed = 0, 0, 0
    while seen_ok < 2 and n < 600:
        n += 1
        d = cs.Dictionary(A)
        d.ctx.tune("fail_alloc", n)
        try:
            got = flat(d.ctx.bp_batch(B))
            assert same(got, want), n
            seen_ok += 1
        except cs.CsmpError as e:
            seen_ok = 0
            failed += 1
            assert e.code == L.ENOMEM, (n, e.code, str(e))
        d.ctx.tune("fail_alloc", 0)
        assert same(flat(d.ctx.bp_batch(B)), want), (n, "after the failed call")
        d.close()
    print(f"bp_batch: {failed} allocations failed in turn")
    assert n < 600 and failed >= 28
    gc.collect()
    assert L.live_resources() == base
