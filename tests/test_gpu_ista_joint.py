"""GPU tests (pytest -m gpu) of csmp_ista_joint: ISTA / FISTA on the row-sparse objective ‖B − A X‖_F² + Σ_j w_j ‖X[j, :]‖₂, ONE support for
all columns of B.  The reference is the numpy twin (tests/ista_joint_twin.py, checked on the CPU by tests/test_ista_joint_static.py)
under ista_twin's parity rule per row.  Beside the parity, bit for bit: one column against csmp_ista, zero weights against ista column
by column (the joint residual kernel against the single one), the same bits under every chunking and on every run, equal columns, a
run continued in place, the trivial cases; the refusals at the ABI and failed allocations."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ista_joint_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = tw.RTOL


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


def run(d, B, w, X0=None, **kw):
    tunes = {k: kw.pop(k) for k in list(kw) if k in ("group_max", "group_wide", "pipelines")}
    for key, v in tunes.items():
        d.ctx.tune(key, v)
    try:
        return d.ctx.ista_joint(B, w, X0, **kw)
    finally:
        for key in tunes:
            d.ctx.tune(key, 0)


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1]["rows"] == b[1]["rows"] and np.array_equal(a[1]["resnorm"], b[1]["resnorm"])


def check(got, case, A, B):
    X, info = got
    Xt = tw.case_twin(case)
    print(tw.case_id(case))
    tw.compare(X, Xt)
    rt = np.linalg.norm(np.asarray(B, np.float64) - np.asarray(A, np.float64) @ Xt, axis=0)
    scale = np.maximum(rt, np.linalg.norm(np.asarray(B, np.float64), axis=0))
    print("resnorm err", float(np.max(np.abs(info["resnorm"] - rt) / scale)), "rows", info["rows"])
    assert np.all(np.abs(info["resnorm"] - rt) <= RTOL * scale)
    assert info["rows"] == int(np.any(X != 0, axis=1).sum())


# ------------------------------------------------------------------------------------------ parity with the twin
@pytest.mark.parametrize("shape", list(tw.SHAPES))
def test_parity_with_the_twin(cs, D, shape):
    A = tw.shape_data(shape)[0]
    d = D(A)
    cfg = d.ctx.sweep_config()
    if shape.startswith("long"):
        assert cfg["group_max"] == 0          # no shared pass: one sweep per column
    else:
        assert cfg["group_max"] == 4 and cfg["group_wide"] == (8 if A.dtype == np.float32 else 4)
    cases = [c for c in tw.parity_cases() if c.shape == shape]
    assert cases
    for c in cases:
        _, B, w, X0, maxiter, alpha = tw.case_args(c)
        got = d.ctx.ista_joint(B, w, X0, maxiter=maxiter, stepsize=alpha, accel=c.method == "fista")
        check(got, c, A, B)


def test_the_public_functions(cs, D):
    c = tw.Case("fista", "256x1024_f32", 9, 0.2, None)
    A, B, w, _, maxiter, alpha = tw.case_args(c)
    d = D(A)
    ref = d.ctx.ista_joint(B, w, maxiter=maxiter, stepsize=alpha, accel=True)
    xs, info = cs.fista_joint(d, B, w, maxiter=maxiter, stepsize=alpha, return_info=True)
    rows = np.flatnonzero(np.any(ref[0] != 0, axis=1))
    assert len(xs) == 9 and info["rows"] == len(rows) and np.array_equal(info["resnorm"], ref[1]["resnorm"])
    assert all(np.array_equal(x.nzind, rows) and np.array_equal(x.nzval, ref[0][rows, s]) for s, x in enumerate(xs))
    xi = cs.ista_joint(d, B, w, xs, maxiter=3, stepsize=alpha)            # a list of SparseVectors as the warm start
    want = d.ctx.ista_joint(B, w, ref[0], maxiter=3, stepsize=alpha)
    wrows = np.flatnonzero(np.any(want[0] != 0, axis=1))
    assert all(np.array_equal(x.nzind, wrows) and np.array_equal(x.nzval, want[0][wrows, s]) for s, x in enumerate(xi))


# ------------------------------------------------------------------------------------------ bit-level checks
@pytest.mark.parametrize("shape", ["256x1024_f32", "ragged_1000x3000_f64"])
def test_one_column_is_ista(cs, D, shape):
    A, _, Ball, alpha, _ = tw.shape_data(shape)
    d = D(A)
    b = np.ascontiguousarray(Ball[:, 0])
    rng = np.random.default_rng(1)
    x0 = rng.standard_normal(A.shape[1]) * (rng.random(A.shape[1]) < 0.05)
    nz = np.flatnonzero(x0)
    for accel in (False, True):
        for w in (0.02, 0.1 * rng.random(A.shape[1])):
            x, rn = d.ctx.ista(b, w, maxiter=16, stepsize=alpha, accel=accel)
            X, info = d.ctx.ista_joint(b[:, None], w, maxiter=16, stepsize=alpha, accel=accel)
            assert np.array_equal(X[:, 0], x) and info["resnorm"][0] == rn and info["rows"] == np.count_nonzero(x)
        x, rn = d.ctx.ista(b, 0.02, nz, x0[nz], maxiter=16, stepsize=alpha, accel=accel)
        X, info = d.ctx.ista_joint(b[:, None], 0.02, x0[:, None], maxiter=16, stepsize=alpha, accel=accel)
        assert np.array_equal(X[:, 0], x) and info["resnorm"][0] == rn and info["rows"] == np.count_nonzero(x)


@pytest.mark.parametrize("shape", ["256x1024_f32", "ragged_1000x3000_f64"])
def test_zero_weights_pin_the_joint_residual_to_the_single_one(cs, D, shape):
    """w = 0: nothing is shrunk (1 − 0/n = 1 exactly) and every list is all of 0..N, so column s is ista(A, B[:, s], 0.0)'s bit for bit
    -- which holds only if k_jista_axpy adds each column's terms in k_ista_axpy's order and split"""
    A, _, Ball, alpha, _ = tw.shape_data(shape)
    d = D(A)
    B = np.asfortranarray(Ball[:, :9])
    for accel in (False, True):
        X, info = d.ctx.ista_joint(B, 0.0, maxiter=8, stepsize=alpha, accel=accel)
        assert np.all(X != 0.0) and info["rows"] == A.shape[1]      # the lists do coincide
        for s in range(9):
            x, rn = d.ctx.ista(np.ascontiguousarray(B[:, s]), 0.0, maxiter=8, stepsize=alpha, accel=accel)
            assert np.array_equal(X[:, s], x), (accel, s, float(np.max(np.abs(X[:, s] - x))))
            assert abs(info["resnorm"][s] - rn) <= 1e-12 * rn, (accel, s)


def test_same_bits_under_every_chunking_and_on_every_run(cs, D):
    import torch
    A, _, Ball, alpha, _ = tw.shape_data("256x1024_f32")
    d = D(A)
    for nsig, lam, accel in ((17, 2e-2, False), (9, 0.2, True)):
        B = np.asfortranarray(Ball[:, :nsig])
        kw = dict(maxiter=24, stepsize=alpha, accel=accel)
        first = d.ctx.ista_joint(B, lam, **kw)
        assert same(d.ctx.ista_joint(B, lam, **kw), first)
        for tunes in ({"group_max": 1}, {"group_max": 2}, {"group_wide": 1}, {"pipelines": 1}):
            assert same(run(d, B, lam, **kw, **tunes), first), tunes
        assert same(d.ctx.ista_joint(B, lam, **kw), first)
        # a column's numbers do not depend on the columns beside it in a chunk of the residual: the first 3 columns alone share the
        # list only when the list is everything, so w = 0 there
        free = d.ctx.ista_joint(B, 0.0, maxiter=6, stepsize=alpha, accel=accel)[0]
        assert np.array_equal(d.ctx.ista_joint(np.asfortranarray(B[:, 5:8]), 0.0, maxiter=6, stepsize=alpha, accel=accel)[0], free[:, 5:8])
        # device pointers, padded leading dimensions, X0 == X in place
        M, N = A.shape
        bbuf = torch.full((nsig, M + 3), 3.0, dtype=torch.float32, device="cuda")
        bbuf[:, :M] = torch.from_numpy(np.ascontiguousarray(B.T)).cuda()
        xbuf = torch.full((nsig, N + 5), 7.0, dtype=torch.float64, device="cuda")
        info = d.ctx.ista_joint_device(bbuf.T[:M], lam, xbuf.T[:N], **kw)
        assert same((xbuf.T[:N].cpu().numpy(), info), first)
        assert np.all(xbuf[:, N:].cpu().numpy() == 7.0) and np.all(bbuf[:, M:].cpu().numpy() == 3.0)


def test_equal_columns_stay_equal(cs, D):
    A, _, Ball, alpha, _ = tw.shape_data("256x1024_f32")
    d = D(A)
    B = np.asfortranarray(Ball[:, [0, 1, 0, 2, 3, 4, 5, 6, 7, 0, 1]])    # copies in one chunk of the residual and across two
    for accel in (False, True):
        X, info = d.ctx.ista_joint(B, 2e-2, maxiter=24, stepsize=alpha, accel=accel)
        for a, b in ((0, 2), (0, 9), (1, 10)):
            assert np.array_equal(X[:, a], X[:, b]) and info["resnorm"][a] == info["resnorm"][b], (accel, a, b)
        assert not np.array_equal(X[:, 0], X[:, 1])


@pytest.mark.parametrize("shape,nsig", [("256x1024_f32", 9), ("32x48_f64", 5)])
def test_a_run_continued_in_place(cs, D, shape, nsig):
    import torch
    A, _, Ball, alpha, _ = tw.shape_data(shape)
    d = D(A)
    B = np.asfortranarray(Ball[:, :nsig])
    whole = d.ctx.ista_joint(B, 2e-2, maxiter=32, stepsize=alpha)
    half = d.ctx.ista_joint(B, 2e-2, maxiter=16, stepsize=alpha)
    assert same(d.ctx.ista_joint(B, 2e-2, half[0], maxiter=16, stepsize=alpha), whole)
    Bt = torch.from_numpy(np.ascontiguousarray(B.T)).cuda().T
    Xt = torch.zeros((nsig, A.shape[1]), dtype=torch.float64, device="cuda").T
    d.ctx.ista_joint_device(Bt, 2e-2, Xt, maxiter=16, stepsize=alpha)
    info = d.ctx.ista_joint_device(Bt, 2e-2, Xt, X0=Xt, maxiter=16, stepsize=alpha)      # X0 == X
    assert same((Xt.cpu().numpy(), info), whole)


def test_trivial_cases(cs, D):
    A, _, Ball, alpha, _ = tw.shape_data("256x1024_f32")
    A64 = np.asarray(A, np.float64)
    d = D(A)
    B = np.asfortranarray(Ball[:, :9])
    B64 = np.asarray(B, np.float64)
    bn = np.linalg.norm(B64, axis=0)
    rng = np.random.default_rng(2)
    X0 = np.zeros((A.shape[1], 9), order="F")
    rows = rng.choice(A.shape[1], 20, replace=False)
    X0[rows] = rng.standard_normal((20, 9))
    X0[rows[0], 1:] = 0.0                                               # a row with one non-zero entry is a non-zero row
    for accel in (False, True):
        X, info = d.ctx.ista_joint(B, 0.05, X0, maxiter=0, stepsize=alpha, accel=accel)   # maxiter = 0: the warm start
        want = np.linalg.norm(B64 - A64 @ X0, axis=0)
        assert np.array_equal(X, X0) and info["rows"] == 20 and np.all(np.abs(info["resnorm"] - want) <= 1e-12 * bn)
        X, info = d.ctx.ista_joint(B, 0.05, maxiter=0, stepsize=alpha, accel=accel)       # ... without one: zeros and ‖b_l‖
        assert not X.any() and info["rows"] == 0 and np.all(np.abs(info["resnorm"] - bn) <= 1e-12 * bn)
        X, info = d.ctx.ista_joint(B, 1e6, X0, maxiter=3, stepsize=alpha, accel=accel)    # a λ that kills every row
        assert not X.any() and info["rows"] == 0 and np.all(np.abs(info["resnorm"] - bn) <= 1e-12 * bn)
    empty = d.ctx.ista_joint(np.zeros((A.shape[0], 0), np.float32, order="F"), 0.05)
    assert empty[0].shape == (A.shape[1], 0) and empty[1]["rows"] == 0 and len(empty[1]["resnorm"]) == 0


def test_other_solvers_are_undisturbed(cs, D):
    A, _, Ball, alpha, _ = tw.shape_data("256x1024_f32")
    d = D(A)
    B = np.asfortranarray(Ball[:, :5])
    b0 = np.ascontiguousarray(B[:, 0])

    def others(ctx):
        xi, rni = ctx.ista(b0, 0.05, maxiter=20, stepsize=alpha)
        xb, rnb = ctx.ista_batch(B, 0.05, maxiter=10, stepsize=alpha)
        so = ctx.somp(B, 6, 0.0, 1)
        return xi, np.float64(rni), xb, rnb, so[0], so[1], so[2]["resnorm"]

    before = others(d.ctx)
    got = d.ctx.ista_joint(B, 0.05, maxiter=20, stepsize=alpha)
    after = others(d.ctx)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert same(d.ctx.ista_joint(B, 0.05, maxiter=20, stepsize=alpha), got)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(cs):
    L = cs._lib
    A, _, Ball, alpha, _ = tw.shape_data("32x48_f64")
    M, N = A.shape
    nsig = 3
    B = np.asfortranarray(Ball[:, :nsig])
    d = cs.Dictionary(A)
    bare = L.Context(0)
    want = d.ctx.ista_joint(B, 0.05, maxiter=8, stepsize=alpha)
    X0 = np.zeros((N, nsig), order="F")

    def call(ctx, **over):
        a = dict(B=B, dtype=L.F64, ldB=M, nsig=nsig, b_loc=L.HOST, w=np.full(1, 0.05), nw=1, X0=None, ldX0=N, maxiter=8, stepsize=alpha, accel=0,
                 ldX=N, x_loc=L.HOST)
        a.update(over)
        X = np.full((N, nsig), 5.0, order="F")
        rn = np.full(nsig, 5.0)
        rows = L.i64(5)
        C = L.C
        rc = L.lib().csmp_ista_joint(ctx._h, None if a["B"] is None else L.ptr(a["B"]), a["dtype"], L.i64(a["ldB"]), L.i64(a["nsig"]), a["b_loc"],
                                     None if a["w"] is None else L.ptr(a["w"]), L.i64(a["nw"]), None if a["X0"] is None else L.ptr(a["X0"]),
                                     L.i64(a["ldX0"]), L.i64(a["maxiter"]), C.c_double(a["stepsize"]), a["accel"], L.ptr(X), L.i64(a["ldX"]),
                                     a["x_loc"], C.byref(rows), rn.ctypes.data_as(C.POINTER(C.c_double)))
        return rc, bool(np.all(X == 5.0) and np.all(rn == 5.0) and rows.value == 5), (X, {"rows": rows.value, "resnorm": rn})

    try:
        cases = [("ldB < M", dict(ldB=M - 1), L.EDIM), ("ldX < N", dict(ldX=N - 1), L.EDIM), ("ldX0 < N", dict(X0=X0, ldX0=N - 1), L.EDIM),
                 ("nsig < 0", dict(nsig=-1), L.EINVAL), ("nsig == 0", dict(nsig=0), L.OK),
                 ("nw", dict(w=np.ones(N - 1), nw=N - 1), L.EDIM), ("nw 2", dict(w=np.ones(2), nw=2), L.EDIM),
                 ("nw = nsig", dict(w=np.ones(nsig), nw=nsig), L.EDIM),
                 ("negative weight", dict(w=-np.ones(N), nw=N), L.EINVAL), ("nan weight", dict(w=np.full(1, np.nan)), L.EINVAL),
                 ("infinite weight", dict(w=np.full(1, np.inf)), L.EINVAL),
                 ("a negative weight in the last row", dict(w=np.r_[np.ones(N - 1), -1.0], nw=N), L.EINVAL),
                 ("null w", dict(w=None), L.EINVAL), ("null B", dict(B=None), L.EINVAL), ("dtype", dict(dtype=5), L.EINVAL),
                 ("b_loc", dict(b_loc=7), L.EINVAL), ("x_loc", dict(x_loc=-1), L.EINVAL), ("accel", dict(accel=2), L.EINVAL),
                 ("maxiter", dict(maxiter=-1), L.EINVAL), ("stepsize 0", dict(stepsize=0.0), L.EINVAL),
                 ("stepsize nan", dict(stepsize=float("nan")), L.EINVAL), ("stepsize inf", dict(stepsize=float("inf")), L.EINVAL)]
        for name, over, code in cases:
            rc, untouched, _ = call(d.ctx, **over)
            assert rc == code and untouched, (name, rc, untouched)
            assert same(d.ctx.ista_joint(B, 0.05, maxiter=8, stepsize=alpha), want), name  # the context still solves
        rc, untouched, got = call(d.ctx)                          # (the harness itself: an accepted call does write)
        assert rc == L.OK and not untouched and same(got, want)
        rc, untouched, _ = call(bare)
        assert rc == L.ESTATE and untouched                       # no dictionary
        C = L.C
        null_x = L.lib().csmp_ista_joint(d.ctx._h, L.ptr(B), L.F64, L.i64(M), L.i64(nsig), L.HOST, L.ptr(np.full(1, 0.05)), L.i64(1), None, L.i64(N),
                                         L.i64(8), C.c_double(alpha), 0, None, L.i64(N), L.HOST, None, None)
        assert null_x == L.EINVAL
        X = np.zeros((N, nsig), order="F")                        # nrows and resnorm may be NULL
        rc = L.lib().csmp_ista_joint(d.ctx._h, L.ptr(B), L.F64, L.i64(M), L.i64(nsig), L.HOST, L.ptr(np.full(1, 0.05)), L.i64(1), None, L.i64(N),
                                     L.i64(8), C.c_double(alpha), 0, L.ptr(X), L.i64(N), L.HOST, None, None)
        assert rc == L.OK and np.array_equal(X, want[0])
    finally:
        d.close()
        bare.close()
    S = cs.Dictionary(A, streamed=True)
    try:
        with pytest.raises(cs.CsmpError) as e:
            S.ctx.ista_joint(B, 0.05)
        assert e.value.code == L.ESTATE
    finally:
        S.close()


def test_every_allocation_may_fail(cs):
    """fail_alloc = n makes the n-th device allocation from now fail for real (the hook of tests/test_gpu_mp_batch.py).  For every n
    until the call goes through twice in a row: a failing call returns CSMP_ENOMEM, and the same context then returns the clean bits.
    Least failures: the staged B and the call's fourteen arrays, beside the solver slot's."""
    L = cs._lib
    A, _, Ball, alpha, _ = tw.shape_data("256x1024_f32")
    B = np.asfortranarray(Ball[:, :9])
    kw = dict(maxiter=8, stepsize=alpha, accel=True)
    gc.collect()
    base = L.live_resources()
    clean = cs.Dictionary(A)
    assert clean.ctx.sweep_config()["group_wide"] == 8
    want = clean.ctx.ista_joint(B, 2e-2, **kw)
    clean.close()
    n, seen_ok, failed = 0, 0, 0
    while seen_ok < 2 and n < 500:
        n += 1
        d = cs.Dictionary(A)
        d.ctx.tune("fail_alloc", n)
        try:
            got = d.ctx.ista_joint(B, 2e-2, **kw)
            assert same(got, want), (n, "the call went through with a result of its own")
            seen_ok += 1
        except cs.CsmpError as e:
            seen_ok = 0
            failed += 1
            assert e.code == L.ENOMEM, (n, e.code, str(e))
        d.ctx.tune("fail_alloc", 0)
        assert same(d.ctx.ista_joint(B, 2e-2, **kw), want), (n, "after the failed call")
        d.close()
    print(f"ista_joint: {failed} allocations failed in turn")
    assert n < 500 and failed >= 15, (n, failed)
    gc.collect()
    assert L.live_resources() == base
