"""GPU tests (pytest -m gpu) of csmp_ista_batch: ista / fista for every column of B, the signals of a group on shared launches.  Every
member keeps csmp_ista's arithmetic -- the shared pass gives the single sweep's bits per member, the group kernels call the single
kernels' bodies on the member's own buffers, the FISTA coefficient is the same Float64 recurrence, a member starts as csmp_ista does --
so a batch must return the BITS of a caller's loop over csmp_ista: X and resnorm, whatever the batch size, the group sizes, the
weights' form and the warm start."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_twin  # noqa: E402
import ista_twin  # noqa: E402
from test_gpu_bp_batch import cut, same, signals, torch_dictionary  # noqa: E402

pytestmark = pytest.mark.gpu

NSIGS = (1, 2, 3, 5, 8, 9, 13)
SHAPES = [(32, 48, np.float64), (100, 257, np.float32), (130, 1000, np.float32), (257, 300, np.float32)]
LAMBDAS = (1e-3, 0.2)
_problems = {}


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


def problem(M, N, dtype):
    """(A, B, stepsize): bp_twin's dictionary, 13 noisy signals with column 1 zero; made once per shape, never changed"""
    key = (M, N, np.dtype(dtype).name)
    if key not in _problems:
        A = bp_twin.data(M, N, 3, M + N, dtype)[0]
        B = signals(A, max(NSIGS)) + 5e-3 * np.random.default_rng(M + N).standard_normal((M, max(NSIGS)))
        B[:, 1] = 0.0
        B = np.asfortranarray(B)
        _problems[key] = (A, B, float(ista_twin.stepsize(A)))
    return _problems[key]


def column_weights(cs, w, N, nsig, s):
    """signal s's weights as csmp_ista takes them"""
    arr, nw, ldw = cs._lib.ista_batch_weights(w, N, nsig)
    if ldw == 0:
        return arr
    return arr[s:s + 1] if nw == 1 else np.ascontiguousarray(arr[:, s])


def loop(cs, d, B, w, X0=None, **kw):
    """what a caller without the batch form writes: csmp_ista column by column on the same Dictionary"""
    N, nsig = d.shape[1], B.shape[1]
    X = np.zeros((N, nsig), np.float64, order="F")
    rn = np.zeros(nsig, np.float64)
    for s in range(nsig):
        i0 = v0 = None
        if X0 is not None:
            i0 = np.flatnonzero(X0[:, s])
            v0 = X0[i0, s]
        X[:, s], rn[s] = d.ctx.ista(np.ascontiguousarray(B[:, s]), column_weights(cs, w, N, nsig, s), i0, v0, **kw)
    return X, rn


def batch(d, B, w, X0=None, tunes=None, **kw):
    tunes = tunes or {}
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return d.ctx.ista_batch(B, w, X0, **kw)
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


# ------------------------------------------------------------------------------------------ 1. bits of the loop
@pytest.mark.parametrize("M,N,dtype", SHAPES, ids=[f"{m}x{n}" for m, n, _ in SHAPES])
def test_bits_of_the_loop(cs, D, M, N, dtype):
    A, Ball, alpha = problem(M, N, dtype)
    d = D(A)
    for accel in (False, True):
        for maxiter in (1, 2, 40):
            for lam in LAMBDAS:
                kw = dict(maxiter=maxiter, stepsize=alpha, accel=accel)
                ref = loop(cs, d, Ball, lam, **kw)
                nnz = np.count_nonzero(ref[0], axis=0)
                if maxiter == 40 and not accel:   # the preconditions: a trivial input cannot pass
                    print(f"{M} x {N} lambda {lam}: non-zeros of the loop's columns {nnz.tolist()}")
                    if lam == 0.2:
                        assert len(set(nnz.tolist()) - {0}) >= 3
                    else:
                        assert all(n > N / 2 for s, n in enumerate(nnz) if s != 1)
                assert nnz[1] == 0 and ref[1][1] == 0.0                   # the zero column: an empty list
                for nsig in NSIGS:
                    got = batch(d, np.asfortranarray(Ball[:, :nsig]), lam, **kw)
                    assert same(got, cut(ref, nsig)), (accel, maxiter, lam, nsig)
    # the public functions, against the public ista / fista
    for fb, f1 in ((cs.ista_batch, cs.ista), (cs.fista_batch, cs.fista)):
        xs = fb(d, Ball[:, :9], 0.2, maxiter=40, stepsize=alpha)
        assert len(xs) == 9
        for s, x in enumerate(xs):
            one = f1(d, Ball[:, s], 0.2, maxiter=40, stepsize=alpha)
            assert x.n == N and np.array_equal(x.nzind, one.nzind) and np.array_equal(x.nzval, one.nzval), s


# ------------------------------------------------------------------------------------------ 2. weights
@pytest.mark.parametrize("accel", [False, True], ids=["ista", "fista"])
def test_weights(cs, D, accel):
    M, N, dtype = SHAPES[1]
    A, Ball, alpha = problem(M, N, dtype)
    nsig = 9
    B = np.asfortranarray(Ball[:, :nsig])
    d = D(A)
    rng = np.random.default_rng(N)
    kw = dict(maxiter=20, stepsize=alpha, accel=accel)
    shared = 0.5 * (0.5 + rng.random(N))
    per_signal = np.array([0.2, 0.05, 0.2, 0.0, 1e-3, 0.4, 0.05, 0.1, 0.3])       # a repeated lambda and a zero
    matrix = np.asfortranarray(0.2 * rng.random((N, nsig)))
    for name, w in (("shared vector", shared), ("a lambda per signal", per_signal), ("matrix", matrix)):
        ref = loop(cs, d, B, w, **kw)
        assert same(batch(d, B, w, **kw), ref), name
        assert len({np.count_nonzero(ref[0][:, s]) for s in range(nsig)}) >= 3, name
    assert not same(loop(cs, d, B, per_signal, **kw), loop(cs, d, B, 0.2, **kw))   # (the weights do reach the columns)
    # the path: one b under 8 lambdas
    path = np.asfortranarray(np.repeat(Ball[:, :1], 8, axis=1))
    lams = np.array([0.8, 0.4, 0.2, 0.1, 0.05, 0.02, 1e-2, 1e-3])
    ref = loop(cs, d, path, lams, **kw)
    counts = np.count_nonzero(ref[0], axis=0)
    print(f"path: non-zeros {counts.tolist()}")
    assert len(set(counts.tolist())) >= 4
    assert same(batch(d, path, lams, **kw), ref)


# ------------------------------------------------------------------------------------------ 3. warm starts
@pytest.mark.parametrize("accel", [False, True], ids=["ista", "fista"])
def test_warm_starts(cs, D, accel):
    import torch
    M, N, dtype = SHAPES[2]
    A, Ball, alpha = problem(M, N, dtype)
    nsig = 9
    B = np.asfortranarray(Ball[:, :nsig])
    d = D(A)
    rng = np.random.default_rng(7)
    X0 = np.zeros((N, nsig), np.float64, order="F")
    for s in range(nsig):                                                       # 0, 1 and N / 4 non-zeros, in turn
        k = (0, 1, N // 4)[s % 3]
        X0[rng.choice(N, k, replace=False), s] = rng.standard_normal(k)
    kw = dict(stepsize=alpha, accel=accel)
    for maxiter in (0, 1, 20):
        ref = loop(cs, d, B, 0.05, X0, maxiter=maxiter, **kw)
        got = batch(d, B, 0.05, X0, maxiter=maxiter, **kw)
        assert same(got, ref), maxiter
    got = batch(d, B, 0.05, X0, maxiter=0, **kw)
    assert np.array_equal(got[0], X0)                                           # maxiter = 0 returns the warm start
    A64 = np.asarray(A, np.float64)
    for s in range(nsig):
        # a residual entry is a sum of at most N / 4 + 1 products: its error is below 251 eps (|b_i| + sum_j |a_ij| |x0_j|) < 1e-12 (...)
        tol = 1e-12 * (np.linalg.norm(B[:, s]) + np.linalg.norm(np.abs(A64) @ np.abs(X0[:, s])))
        assert abs(got[1][s] - np.linalg.norm(B[:, s] - A64 @ X0[:, s])) <= tol, s
    zero = batch(d, B, 0.05, maxiter=0, **kw)                                   # ... and zeros, with ||b||, from no start
    assert np.all(zero[0] == 0.0) and same(zero, loop(cs, d, B, 0.05, maxiter=0, **kw))
    assert np.allclose(zero[1], np.linalg.norm(B, axis=0), rtol=1e-14)
    # continuing in place: two calls of 20 against two looped calls of 20
    first = loop(cs, d, B, 0.05, maxiter=20, **kw)
    second = loop(cs, d, B, 0.05, first[0], maxiter=20, **kw)
    assert not np.array_equal(first[0], second[0])
    Bt = torch.from_numpy(np.ascontiguousarray(B.T)).cuda().T
    Xt = torch.zeros((nsig, N), dtype=torch.float64, device="cuda").T
    rn1 = d.ctx.ista_batch_device(Bt, 0.05, Xt, maxiter=20, **kw)
    assert same((Xt.cpu().numpy(), rn1), first)
    rn2 = d.ctx.ista_batch_device(Bt, 0.05, Xt, X0=Xt, maxiter=20, **kw)
    assert same((Xt.cpu().numpy(), rn2), second)
    h1 = batch(d, B, 0.05, maxiter=20, **kw)
    assert same(batch(d, B, 0.05, h1[0], maxiter=20, **kw), second)
    # the public functions take the warm starts as SparseVectors or as a dense matrix
    fb = cs.fista_batch if accel else cs.ista_batch
    ref = loop(cs, d, B, 0.05, X0, maxiter=20, **kw)
    sparse = [cs.SparseVector(N, np.flatnonzero(X0[:, s]), X0[np.flatnonzero(X0[:, s]), s]) for s in range(nsig)]
    for start in (sparse, X0):
        xs = fb(d, B, 0.05, start, maxiter=20, stepsize=alpha)
        assert all(np.array_equal(x.to_dense(), ref[0][:, s]) for s, x in enumerate(xs))


# ------------------------------------------------------------------------------------------ 4. every pass instantiation
@pytest.mark.parametrize("M,N,dtype,group,wide", [(4096, 4200, np.float32, 4, 8), (3000, 3100, np.float32, 4, 8), (1024, 1500, np.float64, 4, 4),
                                                  (256, 4096, np.float32, None, None)],
                         ids=["whole_units_wide", "clamped_loads", "f64_four_waves", "short_columns"])
def test_every_pass_instantiation(cs, D, M, N, dtype, group, wide):
    At, A = torch_dictionary(M, N, dtype, 7 + N)
    d = D(At)
    cfg = d.ctx.sweep_config()
    print(f"{M} x {N}: group_max {cfg['group_max']}, group_wide {cfg['group_wide']}")
    if group is not None:
        assert cfg["group_max"] == group and cfg["group_wide"] == wide
    B = signals(A, 9)
    # the 2-norm of these dictionaries costs an SVD of seconds; for unit Gaussian columns it is about 1 + sqrt(N / M), and three
    # iterations compare bits, not convergence
    alpha = 0.45 / (1.0 + np.sqrt(N / M)) ** 2
    for accel in (False, True):
        kw = dict(maxiter=3, stepsize=alpha, accel=accel)
        ref = loop(cs, d, B, 0.05, **kw)
        counts = np.count_nonzero(ref[0], axis=0)
        assert counts[1] == 0 and np.count_nonzero(counts) == 8                 # every signal but the zero column has a list
        assert same(batch(d, B, 0.05, **kw), ref), accel


# ------------------------------------------------------------------------------------------ 5. schedule switches
def test_schedule_switches(cs, D):
    M, N, dtype = SHAPES[2]
    A, Ball, alpha = problem(M, N, dtype)
    B = np.asfortranarray(Ball[:, :9])
    d = D(A)
    kw = dict(maxiter=12, stepsize=alpha, accel=True)
    ref = loop(cs, d, B, 0.05, **kw)
    assert same(batch(d, B, 0.05, **kw), ref)
    for tunes in ({"group_max": 1}, {"group_max": 2}, {"group_max": 3}, {"group_max": 4}, {"group_wide": 1}):
        assert same(batch(d, B, 0.05, tunes=tunes, **kw), ref), tunes
    d.ctx.tune("sweep_dyn", 1)  # no shared pass: the batch takes the loop
    try:
        assert d.ctx.sweep_config()["group_max"] == 0
        assert same(d.ctx.ista_batch(B, 0.05, **kw), loop(cs, d, B, 0.05, **kw))
    finally:
        d.ctx.tune("sweep_dyn", 0)
    d.ctx.set_option("screened_sweep", 1)  # the screened sweeps: signal by signal, the loop's bits under the same option
    try:
        assert same(d.ctx.ista_batch(B, 0.05, **kw), loop(cs, d, B, 0.05, **kw))
    finally:
        d.ctx.set_option("screened_sweep", 0)
    assert same(batch(d, B, 0.05, **kw), ref)


# ------------------------------------------------------------------------------------------ 6. device pointers
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["B_f32", "B_f64"])
def test_device_pointers(cs, D, dtype):
    import torch
    M, N, adtype = SHAPES[1]
    A, Ball, alpha = problem(M, N, adtype)
    nsig, ldB, ldX, ldX0 = 9, M + 3, N + 5, N + 2
    Bh = np.asfortranarray(Ball[:, :nsig].astype(dtype))
    rng = np.random.default_rng(3)
    X0 = np.asfortranarray(rng.standard_normal((N, nsig)) * (rng.random((N, nsig)) < 0.1))
    w = 0.1 * (0.5 + rng.random(N))
    d = D(A)
    kw = dict(maxiter=20, stepsize=alpha, accel=True)
    want = d.ctx.ista_batch(Bh, w, X0, **kw)
    assert same(want, loop(cs, d, Bh, w, X0, **kw))
    buf = torch.full((nsig, ldB), 3.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    buf[:, :M] = torch.from_numpy(np.ascontiguousarray(Bh.T)).cuda()
    xbuf = torch.full((nsig, ldX), 7.0, dtype=torch.float64, device="cuda")
    x0buf = torch.full((nsig, ldX0), 9.0, dtype=torch.float64, device="cuda")
    x0buf[:, :N] = torch.from_numpy(np.ascontiguousarray(X0.T)).cuda()
    Bt, Xt, X0t = buf.T[:M], xbuf.T[:N], x0buf.T[:N]
    assert Bt.stride() == (1, ldB) and Xt.stride() == (1, ldX) and X0t.stride() == (1, ldX0)
    for _ in range(2):                                       # two runs: the same bits
        rn = d.ctx.ista_batch_device(Bt, w, Xt, X0=X0t, **kw)
        assert same((Xt.cpu().numpy(), rn), want)
    assert np.all(xbuf[:, N:].cpu().numpy() == 7.0)          # the padding rows of X are untouched
    assert np.all(buf[:, M:].cpu().numpy() == 3.0)
    assert np.array_equal(x0buf[:, :N].cpu().numpy().T, X0) and np.all(x0buf[:, N:].cpu().numpy() == 9.0)   # X0 is read only


def test_other_solvers_are_undisturbed(cs, D):
    M, N, dtype = SHAPES[1]
    A, Ball, alpha = problem(M, N, dtype)
    B = np.asfortranarray(Ball[:, :5])
    d = D(A)
    b0 = np.ascontiguousarray(B[:, 0])

    def others(ctx):
        xi, rni = ctx.ista(b0, 0.05, maxiter=20, stepsize=alpha)
        xb, ib = ctx.bp_batch(B, maxiter=64)
        mp = ctx.mp_batch(B, 6)
        return (xi, np.float64(rni), xb, ib["iterations"], ib["resnorm"]) + tuple(mp)

    kw = dict(maxiter=20, stepsize=alpha)
    before = others(d.ctx)
    got = d.ctx.ista_batch(B, 0.05, **kw)
    assert same(got, loop(cs, d, B, 0.05, **kw))
    assert same(others(d.ctx), before)
    assert same(d.ctx.ista_batch(B, 0.05, **kw), got)


# ------------------------------------------------------------------------------------------ 7. twin parity
@pytest.mark.parametrize("method,lam", [("ista", 1e-3), ("ista", 0.2), ("fista", 2e-2), ("fista", 0.2)],
                         ids=["ista-1e-3", "ista-0.2", "fista-2e-2", "fista-0.2"])
def test_parity_with_the_twin(cs, D, method, lam):
    M, N, dtype = SHAPES[1]
    A, Ball, alpha = problem(M, N, dtype)
    d = D(A)
    X, rn = d.ctx.ista_batch(Ball, lam, maxiter=40, stepsize=alpha, accel=method == "fista")
    A64 = np.asarray(A, np.float64)
    for s in (0, 2, 5, 12):
        xt = getattr(ista_twin, method)(A64, Ball[:, s], lam, None, 40, alpha)
        ista_twin.compare(X[:, s], xt)
        rt = np.linalg.norm(Ball[:, s] - A64 @ xt)
        assert abs(rn[s] - rt) <= ista_twin.RTOL * max(rt, np.linalg.norm(Ball[:, s])), s


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(cs):
    L = cs._lib
    M, N, dtype = SHAPES[0]
    A, Ball, alpha = problem(M, N, dtype)
    nsig = 3
    B = np.asfortranarray(Ball[:, :nsig])
    d = cs.Dictionary(A)
    bare = L.Context(0)
    want = d.ctx.ista_batch(B, 0.05, maxiter=8, stepsize=alpha)
    X0 = np.zeros((N, nsig), order="F")

    def call(ctx, **over):
        a = dict(B=B, dtype=L.F64, ldB=M, nsig=nsig, b_loc=L.HOST, w=np.full(1, 0.05), nw=1, ldw=0, X0=None, ldX0=N, maxiter=8, stepsize=alpha,
                 accel=0, ldX=N, x_loc=L.HOST)
        a.update(over)
        X = np.full((N, nsig), 5.0, order="F")
        rn = np.full(nsig, 5.0)
        C = L.C
        rc = L.lib().csmp_ista_batch(ctx._h, None if a["B"] is None else L.ptr(a["B"]), a["dtype"], L.i64(a["ldB"]), L.i64(a["nsig"]), a["b_loc"],
                                     None if a["w"] is None else L.ptr(a["w"]), L.i64(a["nw"]), L.i64(a["ldw"]),
                                     None if a["X0"] is None else L.ptr(a["X0"]), L.i64(a["ldX0"]), L.i64(a["maxiter"]), C.c_double(a["stepsize"]),
                                     a["accel"], L.ptr(X), L.i64(a["ldX"]), a["x_loc"], rn.ctypes.data_as(C.POINTER(C.c_double)))
        return rc, bool(np.all(X == 5.0) and np.all(rn == 5.0))

    try:
        per = np.full(nsig, 0.05)
        cases = [("ldB < M", dict(ldB=M - 1), L.EDIM), ("ldX < N", dict(ldX=N - 1), L.EDIM), ("ldX0 < N", dict(X0=X0, ldX0=N - 1), L.EDIM),
                 ("nsig < 0", dict(nsig=-1), L.EINVAL), ("nsig == 0", dict(nsig=0), L.OK),
                 ("nw", dict(w=np.ones(N - 1), nw=N - 1), L.EDIM), ("nw 2", dict(w=np.ones(2), nw=2), L.EDIM),
                 ("negative weight", dict(w=-np.ones(N), nw=N), L.EINVAL), ("nan weight", dict(w=np.full(1, np.nan)), L.EINVAL),
                 ("infinite weight", dict(w=np.full(1, np.inf)), L.EINVAL),
                 ("a negative weight in the last column", dict(w=np.array([0.05, 0.05, -0.05]), ldw=1), L.EINVAL),
                 ("ldw < 0", dict(w=per, ldw=-1), L.EINVAL), ("0 < ldw < nw", dict(w=np.ones(N * nsig), nw=N, ldw=N - 1), L.EINVAL),
                 ("null w", dict(w=None), L.EINVAL), ("null B", dict(B=None), L.EINVAL), ("dtype", dict(dtype=5), L.EINVAL),
                 ("b_loc", dict(b_loc=7), L.EINVAL), ("x_loc", dict(x_loc=-1), L.EINVAL), ("accel", dict(accel=2), L.EINVAL),
                 ("maxiter", dict(maxiter=-1), L.EINVAL), ("stepsize 0", dict(stepsize=0.0), L.EINVAL),
                 ("stepsize nan", dict(stepsize=float("nan")), L.EINVAL), ("stepsize inf", dict(stepsize=float("inf")), L.EINVAL)]
        for name, over, code in cases:
            rc, untouched = call(d.ctx, **over)
            assert rc == code and untouched, (name, rc, untouched)
            assert same(d.ctx.ista_batch(B, 0.05, maxiter=8, stepsize=alpha), want), name  # the context still solves
        rc, untouched = call(d.ctx, w=per, ldw=1)            # (the harness itself: an accepted call does write)
        assert rc == L.OK and not untouched
        rc, untouched = call(bare)
        assert rc == L.ESTATE and untouched                  # no dictionary
        null_x = L.lib().csmp_ista_batch(d.ctx._h, L.ptr(B), L.F64, L.i64(M), L.i64(nsig), L.HOST, L.ptr(per), L.i64(1), L.i64(0), None, L.i64(N),
                                         L.i64(8), L.C.c_double(alpha), 0, None, L.i64(N), L.HOST, None)
        assert null_x == L.EINVAL
    finally:
        d.close()
        bare.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        with pytest.raises(cs.CsmpError) as e:
            S.ctx.ista_batch(B, 0.05)
        assert e.value.code == L.ESTATE
    finally:
        S.close()


# ------------------------------------------------------------------------------------------ 9. allocations
def test_every_allocation_may_fail_and_nothing_leaks(cs):
    """tests/test_gpu_bp_batch.py's pattern: every device allocation of an ista_batch call fails in turn with CSMP_ENOMEM, the same
    context then returns the clean context's bits, and the library holds what it held before.  Least failures: the staged B,
    IstaBatchBuf's 8 and one or more for each of the four solver slots of a group -- 13.  (A Float64 dictionary: no wide groups, whose
    slots may fail without failing the call.)"""
    L = cs._lib
    M, N, dtype = SHAPES[0]
    A, Ball, alpha = problem(M, N, dtype)
    B = np.asfortranarray(Ball[:, :5])
    kw = dict(maxiter=8, stepsize=alpha, accel=True)
    gc.collect()
    base = L.live_resources()
    clean = cs.Dictionary(A)
    assert clean.ctx.sweep_config()["group_wide"] == clean.ctx.sweep_config()["group_max"] == 4
    want = clean.ctx.ista_batch(B, 0.05, **kw)
    assert same(want, loop(cs, clean, B, 0.05, **kw))
    clean.close()
    n, seen_ok, failed = 0, 0, 0
    while seen_ok < 2 and n < 600:
        n += 1
        d = cs.Dictionary(A)
        d.ctx.tune("fail_alloc", n)
        try:
            got = d.ctx.ista_batch(B, 0.05, **kw)
            assert same(got, want), n
            seen_ok += 1
        except cs.CsmpError as e:
            seen_ok = 0
            failed += 1
            assert e.code == L.ENOMEM, (n, e.code, str(e))
        d.ctx.tune("fail_alloc", 0)
        assert same(d.ctx.ista_batch(B, 0.05, **kw), want), (n, "after the failed call")
        d.close()
    print(f"ista_batch: {failed} allocations failed in turn")
    assert n < 600 and failed >= 13
    gc.collect()
    assert L.live_resources() == base
