"""GPU tests (pytest -m gpu) of csmp_bp_joint: row-sparse basis pursuit, min Σ_j w_j ‖X[j, :]‖₂ subject to A X = B, ONE support and ONE
stopping rule for all columns of B.  The reference is the numpy twin (tests/bp_joint_twin.py, checked on the CPU by
tests/test_bp_joint_static.py) under ista_joint_twin's parity rule per row.  Beside the parity: the joint recovery where one column
fails; bit for bit, one column against csmp_bp, zero weights against bp column by column (the new driver and update against the single
solve), the same bits under every chunking and on every run, equal columns; check_every, maxiter and the trivial cases; the refusals at
the ABI and failed allocations."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bp_joint_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-6
TOL = tw.TWIN_TOL
CHECK_EVERY = 32


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


def weights(w):
    return 1.0 if w is None else w


def run(d, B, w, **kw):
    tunes = {k: kw.pop(k) for k in list(kw) if k in ("group_max", "group_wide")}
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return d.ctx.bp_joint(B, w, **kw)
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


def same(a, b):
    return (np.array_equal(a[0], b[0]) and a[1]["iterations"] == b[1]["iterations"] and a[1]["converged"] == b[1]["converged"]
            and a[1]["rows"] == b[1]["rows"] and np.array_equal(a[1]["resnorm"], b[1]["resnorm"]))


def check(got, case, A, B):
    X, info = got
    Zt, it = tw.case_twin(case)
    print(tw.case_id(case), "iterations", info["iterations"], "/ twin", it["iterations"], "converged", info["converged"], "/", it["converged"])
    tw.compare(X, Zt)
    assert info["converged"] == it["converged"]
    assert info["iterations"] <= it["iterations"] + 2 * CHECK_EVERY       # (the check may fall on the other side of tol)
    if not it["converged"]:
        assert info["iterations"] == it["iterations"] == 64
    B64 = np.asarray(B, np.float64)
    rn = np.linalg.norm(B64 - np.asarray(A, np.float64) @ X, axis=0)
    bn = np.linalg.norm(B64, axis=0)
    print("resnorm err", float(np.max(np.abs(info["resnorm"] - rn) / bn)), "rows", info["rows"])
    assert np.all(np.abs(info["resnorm"] - rn) <= RTOL * bn)
    assert info["rows"] == int(np.any(X != 0, axis=1).sum())


# ------------------------------------------------------------------------------------------ parity with the twin
@pytest.mark.parametrize("shape", list(tw.SHAPES))
def test_parity_with_the_twin(cs, D, shape):
    A = tw.shape_data(shape)[0]
    d = D(A)
    cfg = d.ctx.sweep_config()
    assert cfg["group_max"] == 4 and cfg["group_wide"] == (8 if A.dtype == np.float32 else 4)
    cases = [c for c in tw.parity_cases() if c.shape == shape]
    assert cases
    for c in cases:
        _, B, w, maxiter = tw.case_args(c)
        got = d.ctx.bp_joint(B, weights(w), maxiter=maxiter, tol=TOL, check_every=CHECK_EVERY)
        check(got, c, A, B)


def test_joint_recovery_where_one_column_fails(cs, D):
    A, Xp, Ball, _, _ = tw.shape_data("vertex_32x64_f64")
    planted = np.flatnonzero(np.any(Xp != 0, axis=1))
    d = D(A)
    x, info = d.ctx.bp(np.ascontiguousarray(Ball[:, 0]), tol=TOL)
    print("bp on column 0:", info["iterations"], "iterations,", np.count_nonzero(x), "non-zeros")
    assert info["converged"] and np.count_nonzero(x) > 12
    xs, info = cs.bp_joint(d, Ball[:, :8], tol=TOL, return_info=True)
    err = max(float(np.max(np.abs(z.nzval - Xp[planted, s]))) for s, z in enumerate(xs))
    print("bp_joint on 8 columns:", info["iterations"], "iterations,", info["rows"], "rows, max|Z − X| =", err)
    assert info["converged"] and info["rows"] == 12 and len(xs) == 8
    assert all(np.array_equal(z.nzind, planted) for z in xs) and err <= 1e-8


# ------------------------------------------------------------------------------------------ bit-level checks
@pytest.mark.parametrize("shape", ["weighted_100x257_f32", "32x48_f64"])
def test_one_column_is_bp(cs, D, shape):
    A, _, Ball, w, _ = tw.shape_data(shape)
    d = D(A)
    b = np.ascontiguousarray(Ball[:, 0])
    for wt, kw in ((weights(w), dict(tol=TOL)), (1.0, dict(maxiter=50, check_every=7)), (0.5, dict(maxiter=0))):
        x, one = d.ctx.bp(b, wt, **kw)
        X, info = d.ctx.bp_joint(b[:, None], wt, **kw)
        assert np.array_equal(X[:, 0], x) and info["iterations"] == one["iterations"] and info["converged"] == one["converged"]
        assert info["resnorm"][0] == one["resnorm"] and info["rows"] == np.count_nonzero(x) and not info["factored"]


@pytest.mark.parametrize("shape", ["wide_130x1000_f32", "32x48_f64"])
def test_zero_weights_pin_the_driver_to_the_single_solve(cs, D, shape):
    """w = 0: nothing is shrunk (1 − 0/n = 1 exactly, U = 0) and every list is all of 0..N; maxiter = 20 < check_every = 32: both sides run
    exactly 20 iterations.  Column s is then bp(A, B[:, s], 0.0)'s bit for bit -- which holds only if the chunked products, the passes on
    Y, k_jbp_update, the joint residual and k_jbp_pq repeat csmp_bp's arithmetic column by column"""
    A, _, Ball, _, _ = tw.shape_data(shape)
    d = D(A)
    for nsig in (3, 9):
        B = np.asfortranarray(Ball[:, :nsig])
        X, info = d.ctx.bp_joint(B, 0.0, maxiter=20)
        assert np.all(X != 0.0) and info["rows"] == A.shape[1] and info["iterations"] == 20 and not info["converged"]   # the lists do coincide
        for s in range(nsig):
            x, one = d.ctx.bp(np.ascontiguousarray(B[:, s]), 0.0, maxiter=20)
            assert one["iterations"] == 20
            assert np.array_equal(X[:, s], x), (nsig, s, float(np.max(np.abs(X[:, s] - x))))
            assert info["resnorm"][s] == one["resnorm"], (nsig, s)


def test_same_bits_under_every_chunking_and_on_every_run(cs, D):
    A, _, Ball, _, _ = tw.shape_data("wide_130x1000_f32")
    d = D(A)
    for nsig in (9, 17):
        B = np.asfortranarray(Ball[:, :nsig])
        first = d.ctx.bp_joint(B, 1.0, tol=TOL)
        assert first[1]["converged"]
        assert same(d.ctx.bp_joint(B, 1.0, tol=TOL), first)
        for tunes in ({"group_max": 1}, {"group_max": 2}, {"group_wide": 1}):
            assert same(run(d, B, 1.0, tol=TOL, **tunes), first), tunes
        assert same(d.ctx.bp_joint(B, 1.0, tol=TOL), first)


def test_equal_columns_stay_equal(cs, D):
    A, _, Ball, _, _ = tw.shape_data("wide_130x1000_f32")
    d = D(A)
    B = np.asfortranarray(Ball[:, [0, 1, 0, 2, 3, 4, 5, 6, 7, 0, 1]])    # copies in one chunk and across two
    X, info = d.ctx.bp_joint(B, 1.0, tol=TOL)
    assert info["converged"]
    for a, b in ((0, 2), (0, 9), (1, 10)):
        assert np.array_equal(X[:, a], X[:, b]) and info["resnorm"][a] == info["resnorm"][b], (a, b)
    assert not np.array_equal(X[:, 0], X[:, 1])


def test_check_every_and_maxiter(cs, D):
    A, _, Ball, _, _ = tw.shape_data("wide_130x1000_f32")
    d = D(A)
    B = np.asfortranarray(Ball[:, :5])
    bn = np.linalg.norm(np.asarray(B, np.float64), axis=0)
    for ce in (1, 7):
        for tol in (0.1, 1e-3):     # (the twin: tol = 0.1 stops at 45 and at 49, tol = 1e-3 runs all 50)
            X, info = d.ctx.bp_joint(B, 1.0, maxiter=50, tol=tol, check_every=ce)
            twin = tw.bp_joint(A, B, None, maxiter=50, tol=tol, check_every=ce)[1]
            print("check_every", ce, "tol", tol, "iterations", info["iterations"], "converged", info["converged"], "/ twin", twin["iterations"])
            assert info["iterations"] == 50 or (info["converged"] and info["iterations"] % ce == 0 and 0 < info["iterations"] < 50)
            assert info["converged"] or info["iterations"] == 50
            assert info["iterations"] <= twin["iterations"] + 2 * ce
    X, info = d.ctx.bp_joint(B, 1.0, maxiter=50, tol=1e-300, check_every=7)   # never below tol: all 50
    assert info["iterations"] == 50 and not info["converged"]
    X, info = d.ctx.bp_joint(B, 1.0, maxiter=0)
    assert not X.any() and info["iterations"] == 0 and not info["converged"] and info["rows"] == 0
    assert np.all(np.abs(info["resnorm"] - bn) <= 1e-12 * bn)


def test_trivial_cases(cs, D):
    A, Xp, Ball, _, _ = tw.shape_data("wide_130x1000_f32")
    M, N = A.shape
    d = D(A)
    empty = d.ctx.bp_joint(np.zeros((M, 0), np.float32, order="F"))
    assert empty[0].shape == (N, 0) and empty[1]["rows"] == 0 and len(empty[1]["resnorm"]) == 0 and empty[1]["iterations"] == 0
    assert cs.bp_joint(d, np.zeros((M, 0))) == []
    X, info = d.ctx.bp_joint(np.zeros((M, 5), order="F"))                 # B = 0: zero rows, converged at the first check
    assert not X.any() and info["rows"] == 0 and info["converged"] and info["iterations"] == CHECK_EVERY and not info["resnorm"].any()
    # a weight vector with zeros: four planted and four other rows are free (never shrunk)
    planted = np.flatnonzero(np.any(Xp != 0, axis=1))
    w = np.ones(N)
    w[planted[:4]] = 0.0
    w[[5, 250, 500, 750]] = 0.0
    B = np.asfortranarray(Ball[:, :5])
    Zt, it = tw.bp_joint(A, B, w, tol=TOL)
    X, info = d.ctx.bp_joint(B, w, tol=TOL)
    print("zero weights in w: iterations", info["iterations"], "/ twin", it["iterations"], "rows", info["rows"])
    tw.compare(X, Zt)
    assert info["converged"] and it["converged"] and info["iterations"] <= it["iterations"] + 2 * CHECK_EVERY
    assert np.all(np.any(X[planted] != 0, axis=1))


def test_other_solvers_are_undisturbed(cs, D):
    A, _, Ball, _, _ = tw.shape_data("wide_130x1000_f32")
    d = D(A)
    B = np.asfortranarray(Ball[:, :5])
    b0 = np.ascontiguousarray(B[:, 0])

    def others(ctx):
        xb, ib = ctx.bp(b0, maxiter=96)
        Xb, iB = ctx.bp_batch(B, maxiter=64)
        Xj, ij = ctx.ista_joint(B, 0.05, maxiter=20, stepsize=0.05)
        so = ctx.somp(B, 6, 0.0, 1)
        return (xb, np.float64(ib["resnorm"]), np.int64(ib["iterations"]), Xb, iB["iterations"], iB["resnorm"], Xj, ij["resnorm"], so[0], so[1],
                so[2]["resnorm"])

    before = others(d.ctx)
    got = d.ctx.bp_joint(B, 1.0, tol=TOL)
    assert not got[1]["factored"]                                         # (bp above formed the factor)
    after = others(d.ctx)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert same(d.ctx.bp_joint(B, 1.0, tol=TOL), got)
    d2 = D(A)                                                             # the first call on a dictionary factorises, the second does not
    first = d2.ctx.bp_joint(B, 1.0, tol=TOL)
    second = d2.ctx.bp_joint(B, 1.0, tol=TOL)
    assert first[1]["factored"] and not second[1]["factored"] and same(first, got) and same(second, got)
    assert all(np.array_equal(a, b) for a, b in zip(before, others(d2.ctx)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["B_f32", "B_f64"])
def test_device_pointers(cs, D, dtype):
    import torch
    A, _, Ball, w, _ = tw.shape_data("weighted_100x257_f32")
    M, N = A.shape
    nsig, ldB, ldX = 9, M + 3, N + 5
    Bh = np.asfortranarray(Ball[:, :nsig].astype(dtype))
    d = D(A)
    want = d.ctx.bp_joint(Bh, w, tol=TOL)
    buf = torch.full((nsig, ldB), 3.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    buf[:, :M] = torch.from_numpy(np.ascontiguousarray(Bh.T)).cuda()
    xbuf = torch.full((nsig, ldX), 7.0, dtype=torch.float64, device="cuda")
    Bt, Xt = buf.T[:M], xbuf.T[:N]
    assert Bt.stride() == (1, ldB) and Xt.stride() == (1, ldX)
    info = d.ctx.bp_joint_device(Bt, w, Xt, tol=TOL)
    assert same((Xt.cpu().numpy(), info), want) and not info["factored"]
    assert np.all(xbuf[:, N:].cpu().numpy() == 7.0)      # the padding rows of X are untouched
    assert np.all(buf[:, M:].cpu().numpy() == 3.0)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(cs):
    L = cs._lib
    A, _, Ball, _, _ = tw.shape_data("32x48_f64")
    M, N = A.shape
    nsig = 3
    B = np.asfortranarray(Ball[:, :nsig])
    d = cs.Dictionary(A)
    bare = L.Context(0)
    want = d.ctx.bp_joint(B, 1.0, maxiter=64)
    C = L.C

    def call(ctx, **over):
        a = dict(B=B, dtype=L.F64, ldB=M, nsig=nsig, b_loc=L.HOST, w=np.ones(1), nw=None, rho=1.0, maxiter=64, tol=1e-8, ce=32, ldX=N, x_loc=L.HOST)
        a.update(over)
        X = np.full((N, nsig), 5.0, order="F")
        rn = np.full(nsig, 5.0)
        it, rows, fl = L.i64(5), L.i64(5), C.c_int(5)
        nw = a["nw"] if a["nw"] is not None else (0 if a["w"] is None else len(a["w"]))
        rc = L.lib().csmp_bp_joint(ctx._h, None if a["B"] is None else L.ptr(a["B"]), a["dtype"], L.i64(a["ldB"]), L.i64(a["nsig"]), a["b_loc"],
                                   None if a["w"] is None else L.ptr(a["w"]), L.i64(nw), C.c_double(a["rho"]), L.i64(a["maxiter"]),
                                   C.c_double(a["tol"]), L.i64(a["ce"]), L.ptr(X), L.i64(a["ldX"]), a["x_loc"], C.byref(it), C.byref(rows),
                                   rn.ctypes.data_as(C.POINTER(C.c_double)), C.byref(fl))
        untouched = bool(np.all(X == 5.0) and np.all(rn == 5.0) and it.value == 5 and rows.value == 5 and fl.value == 5)
        info = {"iterations": it.value, "converged": bool(fl.value & 1), "rows": rows.value, "resnorm": rn}
        return rc, untouched, (X, info)

    try:
        nan, inf = float("nan"), float("inf")
        cases = [("ldB < M", dict(ldB=M - 1), L.EDIM), ("ldX < N", dict(ldX=N - 1), L.EDIM), ("nsig < 0", dict(nsig=-1), L.EINVAL),
                 ("nsig == 0", dict(nsig=0), L.OK), ("nw", dict(w=np.ones(N - 1)), L.EDIM), ("nw 2", dict(w=np.ones(2)), L.EDIM),
                 ("nw = nsig", dict(w=np.ones(nsig)), L.EDIM), ("nw = 0", dict(nw=0), L.EDIM),
                 ("negative weight", dict(w=-np.ones(N)), L.EINVAL), ("nan weight", dict(w=np.full(1, nan)), L.EINVAL),
                 ("infinite weight", dict(w=np.full(1, inf)), L.EINVAL),
                 ("a negative weight in the last row", dict(w=np.r_[np.ones(N - 1), -1.0]), L.EINVAL),
                 ("null w", dict(w=None, nw=1), L.EINVAL), ("null B", dict(B=None), L.EINVAL), ("dtype", dict(dtype=5), L.EINVAL),
                 ("b_loc", dict(b_loc=7), L.EINVAL), ("x_loc", dict(x_loc=-1), L.EINVAL),
                 ("rho 0", dict(rho=0.0), L.EINVAL), ("rho < 0", dict(rho=-1.0), L.EINVAL), ("rho nan", dict(rho=nan), L.EINVAL),
                 ("rho inf", dict(rho=inf), L.EINVAL), ("tol 0", dict(tol=0.0), L.EINVAL), ("tol nan", dict(tol=nan), L.EINVAL),
                 ("tol inf", dict(tol=inf), L.EINVAL), ("maxiter", dict(maxiter=-1), L.EINVAL), ("check_every", dict(ce=0), L.EINVAL)]
        for name, over, code in cases:
            rc, untouched, _ = call(d.ctx, **over)
            assert rc == code and untouched, (name, rc, untouched)
            assert same(d.ctx.bp_joint(B, 1.0, maxiter=64), want), name   # the context still solves
        rc, untouched, got = call(d.ctx)                                  # (the harness itself: an accepted call does write)
        assert rc == L.OK and not untouched and same(got, want)
        rc, untouched, _ = call(bare)
        assert rc == L.ESTATE and untouched                               # no dictionary
        null_x = L.lib().csmp_bp_joint(d.ctx._h, L.ptr(B), L.F64, L.i64(M), L.i64(nsig), L.HOST, L.ptr(np.ones(1)), L.i64(1), C.c_double(1.0),
                                       L.i64(64), C.c_double(1e-8), L.i64(32), None, L.i64(N), L.HOST, None, None, None, None)
        assert null_x == L.EINVAL
        X = np.zeros((N, nsig), order="F")                                # iterations, nrows, resnorm and flags may be NULL
        rc = L.lib().csmp_bp_joint(d.ctx._h, L.ptr(B), L.F64, L.i64(M), L.i64(nsig), L.HOST, L.ptr(np.ones(1)), L.i64(1), C.c_double(1.0), L.i64(64),
                                   C.c_double(1e-8), L.i64(32), L.ptr(X), L.i64(N), L.HOST, None, None, None, None)
        assert rc == L.OK and np.array_equal(X, want[0])
        # more rows than columns: CSMP_EDIM, as csmp_bp (more than 2^19 rows, CSMP_ERANGE, needs 2^38 entries: bp_entry's check is shared)
        d.ctx.set_dictionary(np.asfortranarray(A.T))
        with pytest.raises(cs.CsmpError) as e:
            d.ctx.bp_joint(np.ones((N, 2)))
        assert e.value.code == L.EDIM
        # a repeated row: A A' is singular
        R = np.array(A)
        R[5] = R[3]
        d.ctx.set_dictionary(np.asfortranarray(R))
        for _ in range(2):
            with pytest.raises(cs.CsmpError) as e:
                d.ctx.bp_joint(np.asfortranarray(R @ np.eye(N)[:, :2]))
            assert e.value.code == L.EINVAL and "not positive definite to working precision" in str(e.value)
        with pytest.raises(ValueError):
            cs.bp_joint(d, np.asfortranarray(R @ np.eye(N)[:, :2]))
        d.ctx.set_dictionary(A)
        got = d.ctx.bp_joint(B, 1.0, maxiter=64)
        assert got[1]["factored"] and same(got, want)
    finally:
        d.close()
        bare.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        with pytest.raises(cs.CsmpError) as e:
            S.ctx.bp_joint(B)
        assert e.value.code == L.ESTATE
    finally:
        S.close()


def test_every_allocation_may_fail(cs):
    """fail_alloc = n makes the n-th device allocation from now fail for real (the hook of tests/test_gpu_mp_batch.py).  For every n
    until the call goes through twice in a row: a failing call returns CSMP_ENOMEM, and the same context then returns the clean bits.
    Least failures: csmp_bp's 17 (the iterates, G and its factor, k_rowgram's partials), the staged B and the call's fourteen arrays."""
    L = cs._lib
    A, _, Ball, _, _ = tw.shape_data("wide_130x1000_f32")
    B = np.asfortranarray(Ball[:, :9])
    kw = dict(maxiter=40, check_every=8)
    gc.collect()
    base = L.live_resources()
    clean = cs.Dictionary(A)
    assert clean.ctx.sweep_config()["group_wide"] == 8
    want = clean.ctx.bp_joint(B, 1.0, **kw)
    clean.close()
    n, seen_ok, failed = 0, 0, 0
    while seen_ok < 2 and n < 500:
        n += 1
        d = cs.Dictionary(A)
        d.ctx.tune("fail_alloc", n)
        try:
            got = d.ctx.bp_joint(B, 1.0, **kw)
            assert same(got, want), (n, "the call went through with a result of its own")
            seen_ok += 1
        except cs.CsmpError as e:
            seen_ok = 0
            failed += 1
            assert e.code == L.ENOMEM, (n, e.code, str(e))
        d.ctx.tune("fail_alloc", 0)
        assert same(d.ctx.bp_joint(B, 1.0, **kw), want), (n, "after the failed call")
        d.close()
    print(f"bp_joint: {failed} allocations failed in turn")
    assert n < 500 and failed >= 32, (n, failed)
    gc.collect()
    assert L.live_resources() == base
